"""The jobs and drivers of tests/test_sharded_consumers.py: batches made the two ways several GPUs make them -- range sharding
(sqg_set_range_mode, sqg_batch_sample_range or sqg_skip_reads, sqg_batch_run_begin / _end) and worker sharding (worker_lo / worker_hi, a
worker[] array) -- and what the consumer calls of include/sqg_*.h must produce on them: the numpy references of the single-context test
files, fed with the reads of the oracle's single-process run that a rank holds.  Not collected."""
import numpy as np
import torch  # noqa: F401  (before the library is loaded: the HIP runtime torch brings is the one the library then uses)

import align_ref as AL
import call_ref as CL
import chunks_ref as R
import collapse_ref as CO
import detect_ref as DT
import detect_vec as DVEC
import events_ref as EV
import events_vec as VEC
import orc
import pileup_ref as PR
import scale_ref as SCL
import segments_ref as SR
import sites_ref as S
import targets_ref as T
from squigulator_amd import api, model, profiles, shard
from test_range_sharding import MFREQ_DENSE, Hip, _ranges
from test_sampler import NCOV, SEQUIN, _contigs

SEED = 42
CHUNK = (512, 256, 128)                                     # chunk_len, stride, max_label
CHUNK_SETTINGS = (("f16", "medmad"), ("f32", "pa"))
SITE_GEOMETRIES = ((256, 128), (64, 32))                    # (win_len, before); the focus is (k + 1) // 2
EVENT_SETTINGS = (("pa", False), ("medmad", False), ("pa", True), ("medmad", True))
DETECT_B = (3, 6, 4.0, 3.0, 0.2)                            # "detect B": thresholds under which both detectors record
ALIGN_TRUTH = (256, 1024, 16384)                            # "align truth": the cfg of tests/test_align.py
ALIGN_DEFAULT = (4096, 4096, 65536)                         # SQG_ALIGN_DEFAULT, typed out: "align detected" passes no cfg
EVENT_INDICES = ("true_ev", "al_ev")                        # the columns that hold batch-wide event indices: restrict() renumbers them
# (of the scale, collapse and call groups only "align scaled" has such a column, al_ev: the collapse groups' rows ARE the events, in the
# rank's own order; site_pos counts bases within the read and site_key is absolute: neither is renumbered)
CALL_OBSERVED = (CL.NEIGH_READ, 256 * 50, 0, 2)             # "call observed": (neigh, term_cap, llr_min, min_obs)
CALL_ROWS = tuple(n for n in CL.OUTPUTS if n != "site_read")
KEY_BASE = (1 << 40) + 12345                                # the caller's origin of the staged jobs: keys past 32 bits
METH_LETTERS = b"ACGTM" + b"ACGTM" + b"ACGTM" + b"mN"

# name -> the job.  kind: the driver; empty: the (batch, rank) pairs that hold no read on purpose; short: (batch, read, bases) of the reads cut
# to less than a k-mer -- the drawn lengths (40 ... 873 bases) hold none: batch 0 (ranges [0, 5) and [5, 11)) has one as the first and one as
# the last read of either rank, batch 1 (ranges [0, 3) and [3, 6)) one as the last read of rank 0 and one as the first of rank 1.
# expect: what the oracle and sites_ref give on the CPU (test_the_jobs_hold_what_can_go_wrong asserts it): per batch
# (sites, sites with label 1, dropped candidates, sites per rank, positions keyed by reads of two different ranks)
JOBS = {
    "r9_meth_g3": dict(kind="range_sampled", profile="dna-r9-prom", meth=True, fasta=NCOV, rlen=900, T=1, G=3, batches=[9, 2], empty={(1, 0)},
                       strands=["-+-++----", None], expect=[(124, 17, 2, [75, 10, 39], 454), (29, None, None, [0, 15, 14], None)]),
    "r9_meth_t2_g3": dict(kind="range_sampled", profile="dna-r9-prom", meth=True, fasta=NCOV, rlen=900, T=2, G=3, batches=[12],
                          expect=[(157, 20, 2, None, 748)]),
    "r10_g2": dict(kind="range_sampled", profile="dna-r10-prom", fasta=NCOV, rlen=700, T=1, G=2, batches=[10], expect=[(118, 0, 4, None, 349)]),
    "r10_g2_meth": dict(kind="range_sampled", profile="dna-r10-prom", meth=True, fasta=NCOV, rlen=700, T=1, G=2, batches=[10],
                        expect=[(118, 13, 4, None, 349)]),
    # (with batches [8, 9] no transcript position is keyed by reads of both ranks, nor with a second batch of up to 20 reads: 22 is the first
    # size that has one -- 4393 positions; the first batch has none)
    "rna004_prefix_g2": dict(kind="range_sampled", profile="rna004-prom", flags=profiles.SQ_PREFIX, fasta=SEQUIN, rlen=10000, sample=api.SAMPLE_RNA,
                             T=1, G=2, batches=[8, 22], exact=True, shared=[0, 4393]),
    "staged_t2_g2": dict(kind="range_staged", profile="dna-r9-prom", k=6, T=2, G=2, letters=b"ACGT", sizes=(11, 6), lengths=(5, 900), reads_seed=3, shared=[128, 177], short=((0, 0, 1), (0, 4, 5), (0, 5, 3), (0, 10, 2), (1, 2, 4), (1, 3, 5))),
    "staged_t2_g2_meth": dict(kind="range_staged", profile="dna-r9-prom", k=6, meth=True, T=2, G=2, letters=METH_LETTERS, sizes=(11, 6),
                              lengths=(5, 900), reads_seed=3, shared=[128, 177], short=((0, 0, 1), (0, 4, 5), (0, 5, 3), (0, 10, 2), (1, 2, 4), (1, 3, 5))),
    # one context in range mode, four batches of as many reads: tests/test_sharded_consumers.py's lifetime test
    "lifetime_g1": dict(kind="range_staged", profile="dna-r9-prom", k=6, meth=True, T=1, G=1, letters=METH_LETTERS, sizes=(5, 5, 5, 5), lengths=(500, 900), reads_seed=17),
    "workers_t4_g2": dict(kind="worker_staged", profile="dna-r9-prom", T=4, G=2, letters=b"ACGT", sizes=(24, 24, 24), lengths=(300, 2500), reads_seed=31),
    "workers_t6_g3": dict(kind="worker_staged", profile="dna-r10-prom", T=6, G=3, letters=b"ACGT", sizes=(18, 18, 18), lengths=(300, 2500), reads_seed=31),
    "workers_t4_g2_sampled": dict(kind="worker_sampled", profile="dna-r9-prom", fasta=NCOV, rlen=1200, T=4, G=2, batches=[24, 24, 24]),
    "workers_t6_g3_sampled": dict(kind="worker_sampled", profile="dna-r10-prom", fasta=NCOV, rlen=1200, T=6, G=3, batches=[18, 18, 18]),
}


# what the consumer calls of a setup are asked for: an attribute of the setup each, these being the defaults (the jobs of JOBS run under them)
CFGS = dict(
    chunk=CHUNK, chunk_settings=CHUNK_SETTINGS,
    site_geometries=SITE_GEOMETRIES, focus=None, site_ctx=(21, 10),     # focus None: (k + 1) // 2; site_ctx: (ctx_len, ctx_before)
    event_settings=EVENT_SETTINGS,                          # the first one is the table the aligner's references read: ("pa", False)
    detect_b=DETECT_B,
    align_detected=None,                                    # None: the call passes no cfg and the reference takes ALIGN_DEFAULT
    align_rows=("detect A",),                               # the detectors whose rows are aligned: "align detected", "align detected B"
    align_truth=ALIGN_TRUTH,
    pile_kmer=False,                                        # True: pile_cfgs has a by="kmer" pileup without a prefix too
    call_observed=CALL_OBSERVED,                            # "align scaled" takes the cfg of align_detected; "call true" the binding's defaults
    # added to "align scaled"'s al_ev before collapse and pileup_rows take it.  The banded aligner assigns every row to an event of its
    # own read, so under 0 no row is ever dropped; under another value the rows at one end of a read point past it -- into the
    # neighbouring read's events or past the batch's -- and are (sqg_collapse.h: not an event of the row's own read)
    collapse_shift=0,
)


class Setup:
    """what a job's contexts are created with, and what the references need to know of them"""

    def __init__(self, name, extra_flags=0):
        j = JOBS[name]
        prof, fl = profiles.get_profile(j["profile"])
        flags = fl | j.get("flags", 0) | (profiles.SQ_METH if j.get("meth") else 0) | extra_flags
        self._set(name, j, prof, flags, j.get("k") or profiles.default_kmer_size(flags), 0, {})

    @classmethod
    def of(cls, name, prof, flags, k, salt, T, batches, amp_noise=1.0, seed=SEED, **cfgs):
        """a setup from explicit values instead of a JOBS name: one plain context (G = 1) of T workers over the profile object prof, the
        whole flag word (the profile's own bits and SQ_METH included), k-mers of k bases, the synthetic model of that salt, the staged
        reads `batches` (a list of lists of bytes), and any of CFGS by keyword"""
        su = cls.__new__(cls)
        su._set(name, dict(kind="staged", T=T, G=1, reads_seed=seed), prof, flags, k, salt, cfgs)
        su.batches, su.amp_noise, su.seed = [list(bt) for bt in batches], amp_noise, seed
        return su

    def _set(self, name, j, prof, flags, k, salt, cfgs):
        self.name, self.job = name, j
        self.prof, self.flags, self.k = prof, flags, k
        self.meth = bool(flags & profiles.SQ_METH)
        self.mean, self.stdv = model.synthetic_model(self.k, salt=salt, meth=self.meth)
        self.rna, self.prefix = bool(self.flags & profiles.SQ_RNA), bool(self.flags & profiles.SQ_PREFIX)
        self.sps = int(self.prof.dwell_mean)
        self.T, self.G = j["T"], j["G"]
        self.sampled = j["kind"] in ("range_sampled", "worker_sampled")
        self.by_worker = j["kind"] in ("worker_staged", "worker_sampled")
        self.sites = not self.rna and not self.prefix
        self.calls = self.meth and self.sites               # the contexts include/sqg_call.h takes; the others are refused under ...
        self.call_flag = "SQG_RNA" if self.rna else "SQG_PREFIX" if self.prefix else "SQG_METH"       # ... this flag's name
        self.n_rows = self.T * len(self.mean)
        self.contigs = self.names = None
        self.batches, self.amp_noise, self.seed = None, 1.0, SEED
        self._chains = {}                                   # id of a job's batch's reads -> job_chain()'s entry
        assert set(cfgs) <= set(CFGS), sorted(set(cfgs) - set(CFGS))
        for key, default in CFGS.items():
            setattr(self, key, cfgs.get(key, default))
        if self.focus is None:
            self.focus = (self.k + 1) // 2
        assert tuple(self.event_settings[0]) == ("pa", False) and set(self.align_rows) <= {"detect A", "detect B"}

    def generator(self, mode=api.MODE_CERTIFIED, worker_lo=0, worker_hi=None):
        g = api.SignalGenerator(self.prof, self.flags, self.k, self.mean, self.stdv, self.seed, num_workers=self.T, amp_noise=self.amp_noise, mode=mode,
                                worker_lo=worker_lo, worker_hi=worker_hi)
        if self.sampled:
            self.oracle_job()                               # (the contigs as the oracle loaded them)
            g.load_genome(self.contigs, self.job["rlen"], self.job.get("sample", api.SAMPLE_DNA))
            if self.meth:
                g.set_meth(self.contigs, self.names, MFREQ_DENSE)
        return g

    # ---- the job on the CPU
    def staged_reads(self):
        j = self.job
        if self.batches is not None:                        # a setup made by Setup.of: the reads it was given
            return self.batches
        rng = np.random.default_rng(j["reads_seed"])
        out = [[bytes(rng.choice(list(j["letters"]), int(m)).astype(np.uint8)) for m in rng.integers(*j["lengths"], nb)] for nb in j["sizes"]]
        for bi, i, m in j.get("short", ()):                 # reads shorter than a k-mer: the first m bases of the read drawn at that place
            assert 1 <= m < self.k
            out[bi][i] = out[bi][i][:m]
        return out

    def workers_of(self, n):
        """the worker of every read of a batch of n: the reference's static partition"""
        return shard.batch_workers(n, self.T)

    def oracle_job(self):
        """the oracle's single-process run of the whole job -> per batch dict(reads [dict(sig, ss, seq, offset)], key0, step, lens, strand)"""
        if (self.name, self.flags) in _ORACLE:
            self.contigs, self.names = _ORACLE[(self.name, self.flags)][1:]
            return _ORACLE[(self.name, self.flags)][0]
        j = self.job
        orac = orc.Oracle(self.prof, self.flags, self.k, self.mean, self.stdv, self.seed, num_workers=self.T, rlen=j.get("rlen", 10000), amp_noise=self.amp_noise)
        out = []
        if self.sampled:
            ref = orac.load_ref(j["fasta"], None, MFREQ_DENSE if self.meth else None)
            self.contigs, self.names = _contigs(ref), [ref.names[i].decode() for i in range(ref.num_ref)]
            off = np.concatenate(([0], np.cumsum([len(c) for c in self.contigs])))
            for nb in j["batches"]:
                rs = orac.run_batch(nb)
                strand = "".join(r.strand for r in rs).encode()
                key0, step = PR.sampler_origin(off, [r.ref_idx for r in rs], [r.ref_pos_st for r in rs], [r.rlen for r in rs], strand, self.k)
                out.append(dict(reads=[dict(sig=r.sig, ss=r.ss, seq=r.seq, offset=r.offset) for r in rs], key0=key0, step=step, strand=strand.decode()))
        else:
            rng = np.random.default_rng(j["reads_seed"] + 1000)
            for bt in self.staged_reads():
                rs = orac.run_batch_assigned(bt, self.workers_of(len(bt)))
                n = len(bt)
                # the caller's origin: every read laid somewhere on a span of 2000 keys, so that reads of different ranks meet; the steps go
                # round -1, 0, +1 from a drawn start, so that every rank that holds three reads or more has all three values
                step = ((np.arange(n) + int(rng.integers(0, 3))) % 3 - 1).astype(np.int8)
                key0 = KEY_BASE + rng.integers(0, 2000, n).astype(np.int64)
                out.append(dict(reads=[dict(sig=r.sig, ss=r.ss, seq=s, offset=r.offset) for r, s in zip(rs, bt)], key0=key0, step=step, strand=None))
        for o in out:
            o["lens"] = np.array([len(r["seq"]) for r in o["reads"]], np.int64)
        orac.close()
        _ORACLE[(self.name, self.flags)] = (out, self.contigs, self.names)
        return out

    def rank_reads(self, n, g):
        """the indices in a batch of n reads of the reads rank g holds"""
        if self.by_worker:
            return shard.shard_batch(n, self.T, g, self.G)[0]
        lo, hi = _ranges(n, self.G)[g]
        return np.arange(lo, hi)

    def window(self):
        """[lo, hi) of the job's by-position keys: the loaded genome, or the span the caller's origin lays the staged reads on"""
        if self.sampled:
            self.oracle_job()
            return 0, sum(len(c) for c in self.contigs)
        return KEY_BASE - 3000, KEY_BASE + 5000

    def pile_cfgs(self):
        """name -> (new_pileup's keywords, norm, trim): the configurations of the pileups that must add up"""
        out = {}
        lo, hi = self.window()
        out["ref_split"] = (dict(by="ref", split=("strand", "meth") if self.meth else ("strand",), lo=lo, hi=hi), "pa", False)
        keys = np.sort(np.concatenate([self.keys(o, np.arange(len(o["reads"]))) for o in self.oracle_job()]))
        if len(keys):                                       # (a job of JOBS always has some; a drawn one may hold nothing but reads without a step)
            lo = int(keys[len(keys) // 4]) + 1
            out["ref_window"] = (dict(by="ref", lo=lo, hi=max(int(keys[3 * len(keys) // 4]), lo + 1)), "medmad", False)
        if self.prefix:
            out["kmer_segs"] = (dict(by="kmer", segs=(0, 1, 2, 3)), "medmad", True)
        elif self.pile_kmer:
            out["kmer"] = (dict(by="kmer"), "medmad", True)
        return out

    def keys(self, o, idx):
        """the by-position keys of the events of reads idx of the oracle's batch o that count"""
        ev_off = np.concatenate(([0], np.cumsum([len(o["reads"][i]["ss"]) for i in idx]))).astype(np.int64)
        ev = dict(ev_read=np.repeat(np.arange(len(idx)), np.diff(ev_off)))
        ok, key, _ = PR.eligible_and_key(ev, ev_off, o["key0"][idx], o["step"][idx], o["lens"][idx], self.k, self.rna, self.prefix)
        return key[ok]

    def detect_settings(self, threaded=False):
        """name -> (cfg, the preset's name or the cfg as Batch.detect takes it, norm, trim)"""
        preset = "rna" if self.rna else "dna"
        out = {"detect A": (DT.RNA if self.rna else DT.DNA, preset, "pa", False)}
        if not threaded:
            out["detect B"] = (self.detect_b, self.detect_b, "medmad", True)
        return out

    def align_settings(self, threaded=False):
        """the detector's name -> (the align group of its rows, the cfg the call is given, the cfg the reference takes)"""
        cfg = self.align_detected
        names = {"detect A": "align detected", "detect B": "align detected B"}
        return {d: (names[d], cfg, ALIGN_DEFAULT if cfg is None else cfg) for d in self.detect_settings(threaded) if d in self.align_rows}

    def expected_detect_align(self, reads, ev, threaded=False, seen=None, plain=False, align=True):
        """the groups of sqg_batch_detect and sqg_batch_align: detect_ref and align_ref over the reads and over ev, events_ref's table of
        them ("pa", untrimmed).  seen: a dict that gets detect_ref's info of every detect group.  The two references walk every row in
        Python, some seconds for a job's rows, so what walks here is their second statement each -- detect_vec.batch_rows_of_reads (the
        boundaries stay detect_ref's) and the oracle's compiled banded recurrence; plain=True takes detect_ref.batch_rows and
        align_ref.banded themselves: tests/test_sharded_consumers.py and tests/test_align.py hold the two ways to each other bit for bit"""
        p, k, rna, prefix, sps = self.prof, self.k, self.rna, self.prefix, self.sps
        rows_of = DT.batch_rows if plain else DVEC.batch_rows_of_reads
        banded = AL.banded if plain else orc.align_banded
        out, det = {}, {}
        for name, (cfg, _, norm, trim) in self.detect_settings(threaded).items():
            info = {}
            w = det[name] = rows_of(reads, cfg, k, rna, prefix, sps, norm, trim, p.range, p.digitisation, info)
            if seen is not None:
                seen[name] = info
            out[name] = dict(off=w["det_off"], read=w["dt_read"], rows={key: w[key] for key in DT.PER_ROW if key != "dt_read"},
                             per_read=dict(med2=w["med2"], mad4=w["mad4"]))
        if not align:                                       # (the detect groups alone: what job_chain() starts from)
            return out
        ev_off = ev["ev_off"]
        for d, (name, _, cfg) in self.align_settings(threaded).items():
            w = det[d]
            a = AL.batch(w["det_off"], w["sum"], w["dt_len"], ev_off, ev["level_raw"], rna, cfg, one=banded)
            out[name] = dict(off=w["det_off"], read=w["dt_read"], rows=dict(al_ev=a["al_ev"]), per_read=dict(al_cost=a["al_cost"], al_edge=a["al_edge"]))
        if not threaded:
            def both(q, lv, cfg):                           # a read of at most 32 events: the full matrix as well, what is compared is held to both
                js, cost, edge = banded(q, lv, cfg)
                if len(lv) <= 32:
                    fj, fc, fe = AL.full(q, lv, cfg)
                    assert fj.tolist() == js.tolist() and (fc, fe) == (cost, edge), "align_ref's two statements differ"
                return js, cost, edge
            idx = stored_order(ev_off, rna)
            a = AL.batch(ev_off, ev["sum"][idx], ev["ev_len"][idx], ev_off, ev["level_raw"], rna, self.align_truth, one=both)
            out["align truth"] = dict(off=ev_off, read=ev["ev_read"], rows=dict(al_ev=a["al_ev"]), per_read=dict(al_cost=a["al_cost"], al_edge=a["al_edge"]))
        return out

    # ---- the references, as groups: name -> dict(off [n_reads + 1], read [rows], rows {key: [rows, ...]}, per_read {key: [n_reads]})
    def collapse_settings(self, threaded=False):
        """(norm, trim) of the "collapse" groups"""
        return [("pa", False)] + ([] if threaded else [("medmad", self.prefix)])

    def event_table(self, reads, norm, trim, tables=None):
        """events_ref's table of the reads under (norm, trim); tables: those at hand, {(norm, trim): table}, added to"""
        key = (norm, bool(trim))
        if tables is None or key not in tables:
            p = self.prof
            w = EV.batch_events(reads, self.mean, self.k, self.rna, self.meth, self.prefix, self.sps, norm, trim, p.range, p.digitisation)
            if tables is None:
                return w
            tables[key] = w
        return tables[key]

    def collapse_of(self, reads, inner, norm, trim, tables=None):
        """collapse_ref over the rows the "collapse" groups take -- detect A's, assigned by "align scaled"'s al_ev --, the reads'
        constants from events_ref's table under (norm, trim)"""
        p = self.prof
        if norm == "pa":
            consts = dict(offset=[r["offset"] for r in reads], rng=p.range, dig=p.digitisation)
        elif (tables is None or (norm, bool(trim)) not in tables) and not trim and not self.prefix:
            st = [R.stats(np.asarray(r["sig"], np.int16)) for r in reads]       # (the whole read's statistics: what pileup_table takes too)
            consts = dict(med2=np.array([s[0] for s in st], np.int32), mad4=np.array([s[1] for s in st], np.int32))
        else:
            t = self.event_table(reads, norm, trim, tables)
            consts = dict(med2=t["med2"], mad4=t["mad4"])
        d = inner["det"]
        return CO.collapse(d["off"], inner["rows_ev"], d["rows"]["sum"], d["rows"]["sumsq"], d["rows"]["dt_len"], inner["ev_off"], norm, **consts)

    def expected_chain(self, reads, groups, tables, origin=None, threaded=False):
        """the groups of sqg_batch_scale, sqg_batch_align_scaled, sqg_batch_collapse and sqg_batch_call, chained reference to reference
        from the oracle's reads: detect A's rows (groups["detect A"]) -> scale_ref (moments) -> the scaled aligner -> scale_ref (fit) and
        collapse_ref -> call_ref on the collapsed rows under the fitted scaling; and call_ref on the true table.  tables: events_ref's,
        {(norm, trim): table}, ("pa", False) among them.  origin: (key0, step) of the reads; without one the call groups have no
        site_key.  -> (the groups, what expected_pileup_rows and the cases' facts take of the chain).  A call group has "stat" as well,
        "call observed" under the job's window, and "freq": what it adds to the context's frequency table"""
        p, k = self.prof, self.k
        ev = tables[("pa", False)]
        ev_off = ev["ev_off"]
        d = groups["detect A"]
        off, read, s1, ln = d["off"], d["read"], d["rows"]["sum"], d["rows"]["dt_len"]
        cfg = ALIGN_DEFAULT if self.align_detected is None else self.align_detected
        out = {}
        mom = SCL.vectorised(off, s1, ln, ev_off, ev["level_raw"], SCL.MOMENTS)
        out["scale moments"] = dict(off=off, read=read, rows={}, per_read=mom)
        a = SCL.align_scaled(off, s1, ln, ev_off, ev["level_raw"], self.rna, cfg, mom["gain"], mom["shift"], one=orc.align_banded)
        out["align scaled"] = dict(off=off, read=read, rows=dict(al_ev=a["al_ev"]), per_read=dict(al_cost=a["al_cost"], al_edge=a["al_edge"]))
        fit = SCL.vectorised(off, s1, ln, ev_off, ev["level_raw"], SCL.FIT, ev=a["al_ev"])
        out["scale fit"] = dict(off=off, read=read, rows={}, per_read=fit)
        inner = dict(det=d, rows_ev=a["al_ev"] + self.collapse_shift, ev_off=ev_off, ev=ev, mom=mom, fit=fit, ob={})
        for norm, trim in self.collapse_settings(threaded):
            ob = inner["ob"][(norm, bool(trim))] = self.collapse_of(reads, inner, norm, trim, tables)
            out[f"collapse {norm} {int(trim)}"] = dict(off=ev_off, read=ev["ev_read"], rows={key: ob[key] for key in CO.OUTPUTS if key != "rd_dropped"},
                                                      per_read=dict(rd_dropped=ob["rd_dropped"]))
        if self.calls:
            ob = inner["ob"][("pa", False)]
            model_ = CL.call_model(self.stdv, p.range, p.digitisation)
            args = lambda cfg, s, n: ([r["seq"] for r in reads], k, cfg, s, n, ev_off, np.asarray(self.mean, np.float32), [r["offset"] for r in reads],      # noqa: E731
                                      p.range, p.digitisation, *model_)
            inner["call true args"] = (args(CL.DEFAULT, ev["sum"], ev["ev_len"]), dict(origin=origin))
            inner["call observed args"] = (args(self.call_observed, ob["ob_sum"], ob["ob_len"]),
                                           dict(scale=(fit["gain"], fit["shift"]), origin=origin, window=self.window() if origin is not None else None))
            for name in ("call true", "call observed"):
                w = inner[name] = CL.vectorised(*inner[f"{name} args"][0], **inner[f"{name} args"][1])
                out[name] = dict(off=w["site_off"], read=w["site_read"], rows={key: w[key] for key in CALL_ROWS if key in w}, per_read={}, stat=w["stat"], freq=w.get("freq"),
                                 args=inner[f"{name} args"])
        return out, inner

    def job_chain(self):
        """per batch of the oracle's job: (the chain's groups, its inner values, the event tables) of the whole batch"""
        out = []
        for o in self.oracle_job():
            if id(o["reads"]) not in self._chains:          # (expected() of the whole batch under the job's own origin leaves it there)
                tables = {}
                ev = self.event_table(o["reads"], "pa", False, tables)
                groups, inner = self.expected_chain(o["reads"], self.expected_detect_align(o["reads"], ev, threaded=True, align=False), tables, (o["key0"], o["step"]))
                self._chains[id(o["reads"])] = (groups, inner, tables)
            out.append(self._chains[id(o["reads"])])
        return out

    def expected_pileup_rows(self, kw, norm, trim):
        """collapse_ref.pileup_rows over the whole job, batch after batch into the same sums -> (the six arrays, the four statistics)"""
        by = PR.BY_KMER if kw["by"] == "kmer" else PR.BY_REF
        split = sum({"strand": PR.SPLIT_STRAND, "meth": PR.SPLIT_METH}[s] for s in kw.get("split", ()))
        segs = sum(1 << q for q in kw.get("segs", ()))
        lo, hi = (kw["lo"], kw["hi"]) if by == PR.BY_REF else (0, len(self.mean))
        into, stats = None, [0, 0, 0, 0]
        for o, (_, inner, tables) in zip(self.oracle_job(), self.job_chain()):
            ob = self.collapse_of(o["reads"], inner, norm, trim, tables)
            ev = tables[("pa", False)]                      # (ev_read, kmer and seg are the same under every norm and trim)
            into, *st = CO.pileup_rows(ob, ev, inner["ev_off"], o["key0"], o["step"], o["lens"], self.k, self.rna, self.prefix, by, split, segs, lo, hi, into)
            stats = [a + b for a, b in zip(stats, st)]
        return into, tuple(stats)

    def expected_call_freq(self):
        """what "call observed" adds to a frequency table over window() in the whole job: the reference's freq, summed"""
        lo, hi = self.window()
        total = {n: np.zeros(hi - lo, np.uint32) for n in CL.FREQ}
        for _, inner, _ in self.job_chain():
            for n in CL.FREQ:
                total[n] += inner["call observed"]["freq"][n]
        return total

    def expected(self, reads, threaded=False, seen=None, origin=None):
        """seen: as in expected_detect_align; origin: as in expected_chain"""
        p, k, rna, meth, prefix, sps, mean = self.prof, self.k, self.rna, self.meth, self.prefix, self.sps, self.mean
        L, St, W = self.chunk
        n = len(reads)
        out, tables = {}, {}
        for dtype, norm in self.chunk_settings[:1] if threaded else self.chunk_settings:
            fdt = np.float16 if dtype == "f16" else np.float32
            if n == 0:
                w = dict(signal=np.zeros((0, L), fdt), labels=np.zeros((0, W), np.uint8), label_len=np.zeros(0, np.int32), chunk_start=np.zeros(0, np.int64),
                         chunk_read=np.zeros(0, np.int32), med2=np.zeros(0, np.int32), mad4=np.zeros(0, np.int32), chunk_off=np.zeros(1, np.int64))
                t = dict(clean=np.zeros((0, L), fdt), clean_raw=np.zeros((0, L), np.int16), moves=np.zeros((0, L), np.uint8), kmer=np.zeros((0, L), np.uint32))
            elif prefix:
                w = SR.batch_chunks_trimmed(reads, k, rna, meth, prefix, sps, L, St, W, dtype, norm, p.range, p.digitisation)
                t = None if threaded else SR.batch_targets_trimmed(reads, mean, k, rna, meth, prefix, sps, L, St, dtype, norm, p.range, p.digitisation)
            else:
                w = R.batch_chunks(reads, k, rna, meth, L, St, W, dtype, norm, p.range, p.digitisation)
                t = None if threaded else T.batch_targets(reads, mean, k, rna, meth, L, St, dtype, norm, p.range, p.digitisation)
            out[f"chunks {dtype} {norm}"] = dict(off=w["chunk_off"], read=w["chunk_read"], rows={key: w[key] for key in ("signal", "labels", "label_len", "chunk_start")},
                                                 per_read=dict(med2=w["med2"], mad4=w["mad4"]))
            if t is not None:
                assert n == 0 or np.array_equal(t["chunk_off"], w["chunk_off"])
                out[f"targets {dtype} {norm}"] = dict(off=w["chunk_off"], read=w["chunk_read"], rows={key: t[key] for key in ("clean", "clean_raw", "moves", "kmer")}, per_read={})
        if self.sites:
            for Lw, before in self.site_geometries[:1] if threaded else self.site_geometries:
                w = S.batch_sites(reads, k, meth, S.Cfg(Lw, before, self.focus, *self.site_ctx, "f16", "medmad"), p.range, p.digitisation)
                out[f"sites {Lw}"] = dict(off=w["site_off"], read=w["site_read"], rows={key: w[key] for key in S.KEYS if key != "site_read"},
                                          per_read=dict(med2=w["med2"], mad4=w["mad4"]))
        for norm, trim in self.event_settings[:1] if threaded else self.event_settings:
            w = self.event_table(reads, norm, trim, tables)
            out[f"events {norm} {int(trim)}"] = dict(off=w["ev_off"], read=w["ev_read"], rows={key: w[key] for key in EV.PER_EVENT if key != "ev_read"},
                                                    per_read=dict(med2=w["med2"], mad4=w["mad4"]))
            if (norm, trim) == tuple(self.event_settings[0]):
                out.update(self.expected_detect_align(reads, w, threaded, seen))
        groups, inner = self.expected_chain(reads, out, tables, origin, threaded)
        if not threaded and origin is not None and any(reads is o["reads"] and origin[0] is o["key0"] and origin[1] is o["step"] for o in self.oracle_job()):
            self._chains[id(reads)] = (groups, inner, tables)   # a whole batch of the job under the job's origin: what job_chain() takes
        out.update(groups)
        if prefix and not threaded:
            seg, shift = SR.batch_segments(reads, k, rna, prefix, sps)
            out["segments"] = dict(off=np.arange(n + 1, dtype=np.int64), read=np.arange(n, dtype=np.int32), rows=dict(seg=seg, shift=shift), per_read={})
        return out

    def expected_sites(self, reads):
        """sites_ref at the first geometry: window 256, 128 samples in front of the anchor event"""
        Lw, before = self.site_geometries[0]
        return S.batch_sites(reads, self.k, self.meth, S.Cfg(Lw, before, self.focus, *self.site_ctx, "f16", "medmad"), self.prof.range, self.prof.digitisation)

    def pileup_table(self, reads, norm, trim, need_kmer):
        """the per-event columns pileup_ref takes: events_ref's, or -- where neither the key nor a split needs k-mer and segment -- the
        vectorised rows that tests/test_event_grids.py pins to it"""
        p = self.prof
        if need_kmer or trim or self.prefix:
            return EV.batch_events(reads, self.mean, self.k, self.rna, self.meth, self.prefix, self.sps, norm, trim, p.range, p.digitisation)
        sig = np.concatenate([r["sig"] for r in reads]) if reads else np.zeros(0, np.int16)
        dw = np.concatenate([np.asarray(r["ss"]) for r in reads]) if reads else np.zeros(0, np.int64)
        sig_off = np.concatenate(([0], np.cumsum([len(r["sig"]) for r in reads]))).astype(np.int64)
        ev_off = np.concatenate(([0], np.cumsum([len(r["ss"]) for r in reads]))).astype(np.int64)
        w = VEC.batch_rows(sig, sig_off, dw, ev_off, [r["offset"] for r in reads], self.rna, norm, p.range, p.digitisation,
                           stats=[R.stats(np.asarray(r["sig"], np.int16)) for r in reads] if norm != "pa" else None)
        w["ev_off"] = ev_off
        return w

    def expected_pileup(self, kw, norm, trim):
        """pileup_ref over the whole job, batch after batch into the same sums -> (the six arrays, counted, outside)"""
        by = PR.BY_KMER if kw["by"] == "kmer" else PR.BY_REF
        split = sum({"strand": PR.SPLIT_STRAND, "meth": PR.SPLIT_METH}[s] for s in kw.get("split", ()))
        segs = sum(1 << q for q in kw.get("segs", ()))
        lo, hi = (kw["lo"], kw["hi"]) if by == PR.BY_REF else (0, len(self.mean))
        into, counted, outside = None, 0, 0
        for o in self.oracle_job():
            ev = self.pileup_table(o["reads"], norm, trim, by == PR.BY_KMER or bool(split & PR.SPLIT_METH))
            into, c, x = PR.pileup(ev, ev["ev_off"], o["key0"], o["step"], o["lens"], self.k, self.rna, self.prefix, by, split, segs, lo, hi, into)
            counted += c; outside += x
        return into, counted, outside

    # ---- the consumer calls of a batch, as the same groups
    def consume(self, b, threaded=False, order=None, extra=(), origin=None, freq=None, want=None, kept=None):
        """extra: further steps (callables that take the dict of groups), behind the listed ones; one given as (label, step) runs behind
        the listed step of that label (a group's name).  order: a permutation of range(len(self.consume_steps(b, threaded)) + len(extra))
        -- the steps run in that order instead of the listed one.  A call that takes another call's tensors as they are -- the aligner
        the detector's, the collapse the scaled aligner's, the caller the collapse's and the fit's -- names the steps that must have run:
        if its step comes first, those run there, in front of it, and not again.  What is returned does not depend on the order.
        origin, freq, want, kept: as in consume_steps"""
        steps = self.consume_steps(b, threaded, origin, freq, want, kept)
        at = {step.label: i for i, (_, step) in enumerate(steps)}
        steps += [((at[step[0]],), step[1]) if isinstance(step, tuple) else (None, step) for step in extra]
        out, ran = {}, set()

        def run(i):
            if i in ran:
                return
            ran.add(i)
            need = steps[i][0]
            for j in () if need is None else (need,) if isinstance(need, int) else need:
                run(j)
            steps[i][1](out)
        for i in range(len(steps)) if order is None else order:
            run(int(i))
        assert len(ran) == len(steps)
        return out

    def consume_steps(self, b, threaded=False, origin=None, freq=None, want=None, kept=None):
        """the calls of consume() on batch b in the listed order: [(the steps that must have run before -- None, an index or a tuple of
        them --, the step)]; a step takes the dict of groups and adds its own, and has its group's name as .label.  origin: what
        Batch.call takes as origin= (Setup.origin); freq: the CallFreq "call observed" adds to; want: the expected groups -- the call
        steps assert their stat against them; kept: a dict that gets the tensors the steps hand on ("rows": what collapse takes)"""
        L, St, W = self.chunk
        trim = self.prefix
        cpu = _host
        steps, kept = [], {} if kept is None else kept

        def chunks(dtype, norm):
            def step(out):
                ch = b.chunks(L, St, W, dtype=dtype, norm=norm, trim=trim)
                plan, nc = b.chunk_plan(L, St, trim=trim)
                assert nc == ch.n_chunks == len(ch.chunk_read) and plan[-1] == nc
                out[f"chunks {dtype} {norm}"] = dict(off=ch.chunk_off, plan=plan, read=cpu(ch.chunk_read), rows={key: cpu(getattr(ch, key)) for key in ("signal", "labels", "label_len", "chunk_start")},
                                                     per_read=dict(med2=cpu(ch.med2), mad4=cpu(ch.mad4)))
                if not threaded:
                    tg = b.chunk_targets(L, St, dtype=dtype, norm=norm, clean=True, clean_raw=True, moves=True, kmer=True, trim=trim)
                    assert tg.n_chunks == nc
                    out[f"targets {dtype} {norm}"] = dict(off=tg.chunk_off, read=cpu(ch.chunk_read), rows={key: cpu(getattr(tg, key), key) for key in ("clean", "clean_raw", "moves", "kmer")}, per_read={})
            return step

        def sites(Lw, before):
            def step(out):
                st = b.sites(Lw, before, self.focus, *self.site_ctx, dtype="f16", norm="medmad")
                plan, ns = b.site_plan(Lw, before, self.focus)
                assert ns == st.n_sites
                out[f"sites {Lw}"] = dict(off=st.site_off, plan=plan, read=cpu(st.site_read), rows={key: cpu(getattr(st, key)) for key in S.KEYS if key != "site_read"},
                                          per_read=dict(med2=cpu(st.med2), mad4=cpu(st.mad4)))
            return step

        def events(norm, tr):
            def step(out):
                ev = b.events(norm, tr)
                assert ev.n_events == b.n_events
                out[f"events {norm} {int(tr)}"] = dict(off=b.ev_off, read=cpu(ev.ev_read), rows={key: cpu(getattr(ev, key), key) for key in EV.PER_EVENT if key != "ev_read"},
                                                      per_read=dict(med2=cpu(ev.med2), mad4=cpu(ev.mad4)))
            return step

        def detect(name, cfg, norm, tr):
            def step(out):
                dt = kept[name] = b.detect(cfg, norm, tr)
                plan, nr = b.detect_plan(cfg)
                assert nr == dt.n_rows == len(dt.dt_read) and plan[-1] == nr
                out[name] = dict(off=dt.det_off, plan=plan, read=cpu(dt.dt_read), rows={key: cpu(getattr(dt, key)) for key in DT.PER_ROW if key != "dt_read"},
                                 per_read=dict(med2=cpu(dt.med2), mad4=cpu(dt.mad4)))
            return step

        def align_detected(name, group, cfg):               # the tensors handed on as they are; cfg None: under SQG_ALIGN_DEFAULT
            def step(out):
                dt = kept[name]
                al = b.align(dt.det_off, dt.sum, dt.dt_len) if cfg is None else b.align(dt.det_off, dt.sum, dt.dt_len, cfg)
                assert al.n_rows == dt.n_rows
                out[group] = dict(off=al.row_off, read=cpu(dt.dt_read), rows=dict(al_ev=cpu(al.al_ev)), per_read=dict(al_cost=cpu(al.al_cost), al_edge=cpu(al.al_edge)))
            return step

        def align_truth(out):                               # the true table's own rows in stored-sample order: row_off is ev_off
            ev = b.events(outputs=("ev_read", "sum", "ev_len"))
            idx = torch.from_numpy(stored_order(b.ev_off, self.rna)).to(ev.sum.device)
            al = b.align(b.ev_off, ev.sum[idx].contiguous(), ev.ev_len[idx].contiguous(), self.align_truth)
            out["align truth"] = dict(off=al.row_off, read=cpu(ev.ev_read), rows=dict(al_ev=cpu(al.al_ev)), per_read=dict(al_cost=cpu(al.al_cost), al_edge=cpu(al.al_edge)))

        def segments(out):
            seg, shift = b.segments()
            out["segments"] = dict(off=np.arange(b.n_reads + 1, dtype=np.int64), read=np.arange(b.n_reads, dtype=np.int32), rows=dict(seg=cpu(seg), shift=cpu(shift)), per_read={})

        def scale(name, mode):                              # detect A's rows; mode "fit": assigned by "align scaled"'s al_ev
            def step(out):
                dt = kept["detect A"]
                sc = kept[name] = b.scale(dt.det_off, dt.sum, dt.dt_len, ev=kept["align scaled"].al_ev if mode == "fit" else None, mode=mode)
                assert sc.n_rows == dt.n_rows
                out[name] = dict(off=sc.row_off, read=cpu(dt.dt_read), rows={}, per_read={key: cpu(getattr(sc, key)) for key in SCL.OUTPUTS})
            return step

        def align_scaled(out):                              # under the moments estimate and the cfg of "align detected"
            dt, sc, cfg = kept["detect A"], kept["scale moments"], self.align_detected
            al = kept["align scaled"] = b.align(dt.det_off, dt.sum, dt.dt_len, scale=(sc.gain, sc.shift)) if cfg is None else b.align(dt.det_off, dt.sum, dt.dt_len, cfg, scale=(sc.gain, sc.shift))
            assert al.n_rows == dt.n_rows
            kept["rows"] = (dt.det_off, al.al_ev + self.collapse_shift if self.collapse_shift else al.al_ev, dt.sum, dt.sumsq, dt.dt_len)
            out["align scaled"] = dict(off=al.row_off, read=cpu(dt.dt_read), rows=dict(al_ev=cpu(al.al_ev)), per_read=dict(al_cost=cpu(al.al_cost), al_edge=cpu(al.al_edge)))

        def collapse(name, norm, tr):
            def step(out):
                co = kept[name] = b.collapse(*kept["rows"], norm=norm, trim=tr)
                ev = b.events(outputs=("ev_read",))
                assert co.n_events == b.n_events and co.n_rows == kept["detect A"].n_rows
                out[name] = dict(off=b.ev_off, read=cpu(ev.ev_read), rows={key: cpu(getattr(co, key), key) for key in CO.OUTPUTS if key != "rd_dropped"},
                                 per_read=dict(rd_dropped=cpu(co.rd_dropped)))
            return step

        def call(name, rows, scaled=False, **kw):
            def step(out):
                scale_ = (kept["scale fit"].gain, kept["scale fit"].shift) if scaled else None
                ch = b.call(*rows(), scale=scale_, origin=origin, **kw)
                plan, ns = b.call_plan()
                assert ns == ch.n_sites == ch.stat[0] == len(ch.site_read) and plan[-1] == ns
                if want is not None:                        # (without a frequency table the call counts nothing as outside)
                    ws = want[name]["stat"]
                    assert ch.stat == (ws if kw.get("freq") is not None else (ws[0], 0) + ws[2:]), f"{name}: stat {ch.stat}, expected {ws}"
                out[name] = dict(off=ch.site_off, plan=plan, read=cpu(ch.site_read), rows={key: cpu(getattr(ch, key)) for key in CALL_ROWS if getattr(ch, key) is not None},
                                 per_read={})
            return step

        def call_true():
            ev = b.events(outputs=("sum", "ev_len"))
            return ev.sum, ev.ev_len

        def call_observed():                                # the collapsed rows: int64 lengths, events without a row among them
            return kept["collapse pa 0"].ob_sum, kept["collapse pa 0"].ob_len

        def call_refused(out):
            try:
                b.call_plan()
            except api.SqgError as e:
                assert e.code == -1 and self.call_flag in str(e), str(e)
            else:
                raise AssertionError(f"sqg_call_plan did not refuse a context with {self.call_flag}")

        def add(need, step, label):
            step.label = label
            steps.append((need, step))
            return len(steps) - 1

        for dtype, norm in self.chunk_settings[:1] if threaded else self.chunk_settings:
            add(None, chunks(dtype, norm), f"chunks {dtype} {norm}")
        if self.sites:
            for Lw, before in self.site_geometries[:1] if threaded else self.site_geometries:
                add(None, sites(Lw, before), f"sites {Lw}")
        for norm, tr in self.event_settings[:1] if threaded else self.event_settings:
            add(None, events(norm, tr), f"events {norm} {int(tr)}")
        aligned = self.align_settings(threaded)
        for name, (_, cfg, norm, tr) in self.detect_settings(threaded).items():
            at = add(None, detect(name, cfg, norm, tr), name)
            if name in aligned:
                add(at, align_detected(name, aligned[name][0], aligned[name][1]), aligned[name][0])
            if name == "detect A":                          # the chain: every call takes the tensors of the ones before it as they are
                mom = add(at, scale("scale moments", "moments"), "scale moments")
                als = add(mom, align_scaled, "align scaled")
                fit = add(als, scale("scale fit", "fit"), "scale fit")
                cos = [add(als, collapse(f"collapse {norm} {int(tr)}", norm, tr), f"collapse {norm} {int(tr)}") for norm, tr in self.collapse_settings(threaded)]
        if not threaded:
            add(None, align_truth, "align truth")
        if self.prefix and not threaded:
            add(None, segments, "segments")
        if self.calls:
            add(None, call("call true", call_true), "call true")
            neigh, term_cap, llr_min, min_obs = self.call_observed
            add((cos[0], fit), call("call observed", call_observed, scaled=True, freq=freq, neigh=neigh, term_cap=term_cap, llr_min=llr_min, min_obs=min_obs), "call observed")
        else:
            add(None, call_refused, "call refused")
        return steps

    def origin(self, o, idx):
        """what Batch.pileup takes as origin= for reads idx of the oracle's batch o: nothing for a sampled batch -- the rank derives the keys
        from its own range of the sampler's records --, the slice of the caller's origin for a staged one"""
        return None if self.sampled else (o["key0"][idx], o["step"][idx])


_ORACLE = {}                                                # (job name, flags) -> the oracle's run


def stored_order(ev_off, rna):
    """a batch's event indices, every read's in stored-sample order: an RNA read's events are stored last to first"""
    idx = np.arange(int(ev_off[-1]), dtype=np.int64)
    if rna:
        for r in range(len(ev_off) - 1):
            idx[int(ev_off[r]):int(ev_off[r + 1])] = idx[int(ev_off[r]):int(ev_off[r + 1])][::-1]
    return idx


def _host(t, key=None):
    """a tensor on the host; the k-mer columns and collapse's row counts as the uint32 they are"""
    a = t.cpu().numpy()
    return a.view(np.uint32) if key in ("kmer", "ob_rows") else a


def assert_groups(got, want, what):
    """every group of `got` against `want`, bit for bit (floats as integers)"""
    assert set(got) == set(want), f"{what}: {sorted(got)} vs {sorted(want)}"
    for name, g in got.items():
        w = want[name]
        np.testing.assert_array_equal(g["off"], w["off"], err_msg=f"{what}: {name}: the rows' offsets")
        if "plan" in g:
            np.testing.assert_array_equal(g["plan"], w["off"], err_msg=f"{what}: {name}: the plan call")
        assert set(g["rows"]) == set(w["rows"]) and set(g["per_read"]) == set(w["per_read"]), f"{what}: {name}: {sorted(g['rows'])} {sorted(g['per_read'])}"
        cols = [("read", g["read"], w["read"])] + [(key, g["rows"][key], w["rows"][key]) for key in w["rows"]] + [(key, g["per_read"][key], w["per_read"][key]) for key in w["per_read"]]
        for key, a, e in cols:
            assert a.shape == e.shape and a.dtype == e.dtype, f"{what}: {name}: {key} {a.shape} {a.dtype} vs {e.shape} {e.dtype}"
            np.testing.assert_array_equal(R.bits(a), R.bits(e), err_msg=f"{what}: {name}: {key}")


def restrict(groups, idx):
    """the groups of a whole batch restricted to the reads idx (increasing) and renumbered: what the rank that holds them must produce.
    The rows' reads are renumbered, and so are the batch-wide event indices of EVENT_INDICES: the event at place j of read idx[i] of the
    whole batch is the event at place j of read i of the rank's (-1, no event, stays)"""
    idx = np.asarray(idx, np.int64)
    ev_whole = np.asarray(groups[f"events {EVENT_SETTINGS[0][0]} {int(EVENT_SETTINGS[0][1])}"]["off"], np.int64)
    ev_rank = np.concatenate(([0], np.cumsum(ev_whole[idx + 1] - ev_whole[idx]))).astype(np.int64)
    out = {}
    for name, g in groups.items():
        off = np.asarray(g["off"], np.int64)
        rows = np.concatenate([np.arange(off[i], off[i + 1]) for i in idx]) if len(idx) else np.zeros(0, np.int64)
        counts = off[idx + 1] - off[idx]
        out[name] = dict(off=np.concatenate(([0], np.cumsum(counts))).astype(np.int64),
                         read=np.repeat(np.arange(len(idx)), counts).astype(g["read"].dtype),
                         rows={key: a[rows] for key, a in g["rows"].items()}, per_read={key: a[idx] for key, a in g["per_read"].items()})
        assert np.array_equal(g["read"][rows], np.repeat(idx, counts))
        shift = np.repeat(ev_rank[:-1] - ev_whole[idx], counts)      # per row: its read's first event in the rank's numbering less that in the batch's
        for key in EVENT_INDICES:
            if key in out[name]["rows"]:
                v = out[name]["rows"][key]
                out[name]["rows"][key] = np.where(v < 0, v, v + shift).astype(v.dtype)
    return out


def pile_arrays(p):
    """the six arrays of a Pileup on the host (n as the uint32 it is)"""
    return {n: (lambda a: a.view(np.uint32) if n == "n" else a)(getattr(p, n).cpu().numpy()) for n in api.PILEUP_OUTPUTS}


def freq_arrays(f):
    """the four arrays of a CallFreq on the host, as the uint32 they are"""
    return {n: getattr(f, n).cpu().numpy().view(np.uint32) for n in api.CALL_FREQ}


# ---------------------------------------------------------------------------------------------------------- drivers (GPU)
class RangeRanks:
    """G contexts in range mode on one GPU; the one exchange step -- the per-stream sample counts -- goes through the host"""

    def __init__(self, su, mode=api.MODE_CERTIFIED):
        self.su, self.hip = su, Hip()
        self.gens = [su.generator(mode) for _ in range(su.G)]
        for g in self.gens:
            g.set_range_mode(True)

    def sample(self, nb):
        return [self.gens[g].sample(nb, lo=lo, hi=hi) for g, (lo, hi) in enumerate(_ranges(nb, self.su.G))]

    def stage(self, bt):
        """reads staged from the host: every rank calls sqg_skip_reads for the reads in front of and behind its range"""
        n = len(bt)
        wk = np.array([self.gens[0].L.sqg_worker_of(i, n, self.su.T) for i in range(n)], np.int32)
        assert np.array_equal(wk, self.su.workers_of(n))
        lens = np.array([len(r) for r in bt], np.int64)
        bs = []
        for g, (lo, hi) in enumerate(_ranges(n, self.su.G)):
            self.gens[g].skip_reads(lens[:lo], wk[:lo])
            bs.append(self.gens[g].stage(bt[lo:hi], wk[lo:hi]))
            self.gens[g].skip_reads(lens[hi:], wk[hi:])
        return bs

    def begin(self, bs):
        return [self.hip.to_host(b.run_begin(), self.su.n_rows).astype(np.uint64) for b in bs]

    def end(self, bs, counts):
        zero = np.zeros(self.su.n_rows, np.uint64)
        for g, b in enumerate(bs):
            pb, pa = self.hip.to_device(sum(counts[:g], zero)), self.hip.to_device(sum(counts[g + 1:], zero))
            b.run_end(pb, pa).wait()
            self.hip.free(pb); self.hip.free(pa)

    def close(self):
        for g in self.gens:
            g.close()


def range_sampled(su, mode=api.MODE_CERTIFIED):
    """yields (batch index, rank, the run batch, the indices of its reads in the job's batch): sample(nb, lo=, hi=), run_begin, the counts
    exchanged, run_end"""
    rk = RangeRanks(su, mode)
    try:
        for bi, nb in enumerate(su.job["batches"]):
            bs = rk.sample(nb)
            rk.end(bs, rk.begin(bs))
            for g, b in enumerate(bs):
                yield bi, g, b, su.rank_reads(nb, g)
            for b in bs:
                b.free()
    finally:
        rk.close()


def range_staged(su, mode=api.MODE_CERTIFIED):
    rk = RangeRanks(su, mode)
    try:
        for bi, bt in enumerate(su.staged_reads()):
            bs = rk.stage(bt)
            rk.end(bs, rk.begin(bs))
            for g, b in enumerate(bs):
                yield bi, g, b, su.rank_reads(len(bt), g)
            for b in bs:
                b.free()
    finally:
        rk.close()


def worker_contexts(su, mode=api.MODE_CERTIFIED):
    return [su.generator(mode, *shard.worker_range(g, su.G, su.T)) for g in range(su.G)]


def worker_batch(su, gen, g, n, bt=None):
    """rank g's part of a batch of n reads, staged (bt: the batch's reads) or sampled: (the staged batch, the indices of its reads)"""
    idx, wk = shard.shard_batch(n, su.T, g, su.G)
    return (gen.stage([bt[i] for i in idx], wk) if bt is not None else gen.sample(len(idx), workers=wk)), idx


def worker_sharded(su, mode=api.MODE_CERTIFIED):
    """one context per block of workers, driven one after the other; staged reads, or the sampler's for a sampled job"""
    gens = worker_contexts(su, mode)
    try:
        batches = [(nb, None) for nb in su.job["batches"]] if su.sampled else [(len(bt), bt) for bt in su.staged_reads()]
        for bi, (n, bt) in enumerate(batches):
            for g, gen in enumerate(gens):
                b, idx = worker_batch(su, gen, g, n, bt)
                b.run().wait()
                yield bi, g, b, idx
                b.free()
    finally:
        for gen in gens:
            gen.close()


def single(su, mode=api.MODE_CERTIFIED):
    """the same job on one plain context that owns every worker: yields (batch index, the run batch)"""
    gen = su.generator(mode)
    try:
        batches = [(nb, None) for nb in su.job["batches"]] if su.sampled else [(len(bt), bt) for bt in su.staged_reads()]
        for bi, (n, bt) in enumerate(batches):
            b = (gen.sample(n) if bt is None else gen.stage(bt, su.workers_of(n))).run().wait()
            yield bi, b
            b.free()
    finally:
        gen.close()


DRIVERS = dict(range_sampled=range_sampled, range_staged=range_staged, worker_staged=worker_sharded, worker_sampled=worker_sharded)
