"""include/sqg_pileup.h: per-site event statistics summed across reads on the device (sqg_batch_pileup), against the numpy statement of
the header's rules (pileup_ref.py) fed with the batch's own event table, with events_ref's table, and with plain np.add.at / np.bincount
over the table's columns.  Every comparison is bit for bit: the sums are integers."""
import ctypes as C
import gzip
import os
import re
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (before the library is loaded: the HIP runtime torch brings is the one the library then uses)

import events_ref as EV
import inject
import pileup_ref as PR
import segments_ref as G
import signal_cases
import targets_ref as T
from chunk_support import _context, _declared, _fixture_reads
from refcases import CASES as REF_CASES
from refvec_cases import REFVEC_CASES
from squigulator_amd import api, build, model, options, profiles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_LIB = os.path.join(ROOT, "oracle", "libsqg_cpu.so")
INPUTS = os.path.join(ROOT, "tests", "golden", "inputs")
NCOV = os.path.join(INPUTS, "nCoV-2019.reference.fasta")
SEQUIN = os.path.join(INPUTS, "rnasequin_sequences_2.4.fa")
MFREQ_DENSE = os.path.join(INPUTS, "mfreq_dense.tsv")
OUT = api.PILEUP_OUTPUTS
LANE_MAX = 64       # k_events_table.h's EVT_LANE_MAX


def _fasta(path):
    names, seqs = [], []
    for ln in open(path, "rb"):
        if ln.startswith(b">"):
            names.append(ln[1:].split()[0].decode()); seqs.append([])
        else:
            seqs[-1].append(ln.strip())
    return [b"".join(s) for s in seqs], names


# ---------------------------------------------------------------------------------------------------------- no GPU
def _struct_fields(hdr, struct):
    body = hdr[:hdr.index("} " + struct)]
    body = body[body.rindex("typedef struct"):]
    body = body[body.index("{") + 1:]
    return [re.sub(r"[\s*]", "", name) for decl in body.split(";") if decl.strip() for name in re.sub(r"^\s*(const\s+)?\w+\s", "", decl.strip()).split(",")]


def test_header_declares_the_pileup_export_and_the_libraries_have_it():
    assert _declared("sqg_pileup.h") == set(api.EXPORTS_PILEUP) == {"sqg_batch_pileup"}
    others = set(api.EXPORTS) | set(api.EXPORTS_CHUNKS) | set(api.EXPORTS_TARGETS) | set(api.EXPORTS_SEGMENTS) | set(api.EXPORTS_SITES) | set(api.EXPORTS_EVENTS)
    assert not set(api.EXPORTS_PILEUP) & others
    assert _declared("sqg_events.h") == set(api.EXPORTS_EVENTS) and _declared("sqg_sites.h") == set(api.EXPORTS_SITES)      # the other headers: unchanged
    assert _declared("sqg_segments.h") == set(api.EXPORTS_SEGMENTS) and _declared("sqg_targets.h") == set(api.EXPORTS_TARGETS)
    assert _declared("sqg_chunks.h") == set(api.EXPORTS_CHUNKS) and _declared("sqg.h") == set(api.EXPORTS)
    build.build()
    for lib in (build.LIB, build.LIB_DEV):
        L = api.load_library(lib)
        for n in api.EXPORTS_PILEUP:
            assert hasattr(L, n), f"{n} not exported by {lib}"
    assert os.path.join(ROOT, "include", "sqg_pileup.h") in build.headers()
    for h in ("k_pileup.h", "h_pileup.h"):
        assert os.path.join(ROOT, "squigulator_amd", "csrc", h) in build.headers()
    raw = open(os.path.join(ROOT, "include", "sqg_pileup.h")).read()
    assert '#include "sqg_events.h"' in raw and "SQG_ABI_VERSION is unchanged" in raw and "wrap modulo 2^64" in raw
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for struct, ctype in (("sqg_pileup_cfg_t", api.CPileupCfg), ("sqg_pileup_origin_t", api.COrigin),
                          ("sqg_pileup_out_t", api.CPileupOut), ("sqg_pileup_stat_t", api.CPileupStat)):
        assert _struct_fields(hdr, struct) == [f[0] for f in ctype._fields_], struct
    assert [f[0] for f in api.CPileupCfg._fields_] == ["by", "split", "norm", "trim", "segs", "lo", "hi"]
    assert tuple(f[0] for f in api.CPileupOut._fields_) == OUT == PR.OUTPUTS
    assert C.sizeof(api.CPileupCfg) == 40 and C.sizeof(api.CPileupStat) == 16
    defs = dict(re.findall(r"#define\s+(SQG_PILEUP_\w+)\s+(\d+)u", hdr))
    assert {k: int(v) for k, v in defs.items()} == dict(SQG_PILEUP_BY_REF=api.PILEUP_BY_REF, SQG_PILEUP_BY_KMER=api.PILEUP_BY_KMER,
                                                         SQG_PILEUP_SPLIT_STRAND=api.PILEUP_SPLIT_STRAND, SQG_PILEUP_SPLIT_METH=api.PILEUP_SPLIT_METH)
    assert (PR.BY_REF, PR.BY_KMER, PR.SPLIT_STRAND, PR.SPLIT_METH) == (api.PILEUP_BY_REF, api.PILEUP_BY_KMER, api.PILEUP_SPLIT_STRAND, api.PILEUP_SPLIT_METH)


def test_the_cpu_backend_has_no_pileup_and_says_so():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "libsqg_cpu.so"])
    prof, fl = profiles.get_profile("dna-r9-prom")
    mean, stdv = model.synthetic_model(6)
    gen = api.SignalGenerator(prof, fl, 6, mean, stdv, 42, lib_path=CPU_LIB)
    for n in api.EXPORTS_PILEUP:
        assert not hasattr(gen.L, n)
    b = gen.submit([b"ACGTACGTACGTTTGACA" * 40])
    with pytest.raises(api.SqgError) as e:
        gen.new_pileup(by="kmer")
    assert e.value.code == -1 and "sqg_batch_pileup" in str(e.value)
    with pytest.raises(api.SqgError) as e:
        b.pileup(None)
    assert e.value.code == -1 and "sqg_batch_pileup" in str(e.value)
    b.free(); gen.close()


def test_a_hand_worked_pileup():
    """k = 6, every dwell 4.  Read 0: '+', 12 bases from reference position 10: 7 k-mers at 10 .. 16.  Read 1: '-', 10 bases over [14, 24): its
    base 0 is the complement of position 23, so its 5 k-mers lie at 18, 17, 16, 15, 14 in read order.  Window [8, 20)"""
    k, d = 6, 4
    key0, step = PR.sampler_origin([0], [0, 0], [10, 14], [12, 10], b"+-", k)
    assert key0.tolist() == [10, 18] and step.tolist() == [1, -1]
    mean = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0] + [10.0, 20.0, 30.0, 40.0, 0.5 + 1 / 8192], np.float32)
    ev = dict(ev_read=np.array([0] * 7 + [1] * 5), ev_len=np.full(12, d), mean=mean, sd=np.full(12, 0.25, np.float32))
    got, counted, outside = PR.pileup(ev, [0, 7, 12], key0, step, [12, 10], k, False, False, lo=8, hi=20)
    #                 8  9 10 11 12 13 14 15 16 17 18 19
    assert got["n"].tolist() == [[0, 0, 1, 1, 1, 1, 2, 2, 2, 1, 1, 0]] and (counted, outside) == (12, 0)
    assert got["dwell"].tolist() == [[d * v for v in got["n"][0]]] and got["dwell_sq"].tolist() == [[d * d * v for v in got["n"][0]]]
    #   position 14: read 0's fifth k-mer (5.0) and read 1's last (0.5 + 2^-13: q = 2048.5, the tie goes to the even 2048)
    assert got["mean_sum"][0].tolist() == [0, 0] + [4096 * v for v in (1, 2, 3, 4)] + [4096 * 5 + 2048, 4096 * (6 + 40), 4096 * (7 + 30), 4096 * 20, 4096 * 10, 0]
    assert got["mean_sq"][0][6] == (4096 * 5) ** 2 + 2048 ** 2 and got["sd_sum"][0].tolist() == [1024 * v for v in got["n"][0]]
    # the window cut to [12, 16): 4 events of read 0 and 2 of read 1 inside, the other 6 outside; a plane per strand
    got, counted, outside = PR.pileup(ev, [0, 7, 12], key0, step, [12, 10], k, False, False, split=PR.SPLIT_STRAND, lo=12, hi=16)
    assert got["n"].tolist() == [[1, 1, 1, 1], [0, 0, 1, 1]] and (counted, outside) == (6, 6)
    # a step of 0 takes a read out; wrapping: a sum that passes 2^63 comes back negative
    got, counted, outside = PR.pileup(ev, [0, 7, 12], key0, [1, 0], [12, 10], k, False, False, lo=8, hi=20,
                                      into=dict(mean_sq=np.full((1, 12), np.iinfo(np.int64).max)))
    assert counted == 7 and got["n"].sum() == 7 and got["mean_sq"][0][2] == np.iinfo(np.int64).min + 4096 ** 2 - 1


def test_the_key_rule_gives_the_target_interval_of_the_reference_paf():
    """every record of the reference's --paf-ref output: the keys of the read's eligible events span exactly [t_st, t_end)"""
    cmd = next(c for _, c, outs in REF_CASES if outs.get("paf") == "dna_r10_paf-ref.paf.exp")
    k = options.parse_args(cmd).kmer_size_default
    recs = gzip.open(os.path.join(ROOT, "tests", "golden", "ref_exp", "dna_r10_paf-ref.paf.exp.gz"), "rt").read().splitlines()
    assert len(recs) >= 2
    for rec in recs:
        f = rec.split("\t")
        _, _, st, end, strand = f[0].split("!")
        st, end = int(st), int(end)
        rlen = end - st
        key0, step = PR.sampler_origin([0], [0], [st], [rlen], strand.encode(), k)
        ev = dict(ev_read=np.zeros(rlen - k + 1, np.int64))
        ok, key, _ = PR.eligible_and_key(ev, [0, rlen - k + 1], key0, step, [rlen], k, False, False)
        assert ok.all() and f[4] == strand
        assert (int(key.min()), int(key.max()) + 1) == (int(f[7]), int(f[8])), rec[:80]
        assert key[0] == (int(f[7]) if strand == "+" else int(f[8]) - 1)


def test_the_last_events_of_an_rna_insert_with_a_prefix_are_not_counted():
    """rna004, k = 9, SQG_PREFIX: chain 0 is insert + poly-A + adaptor, and segments_ref calls the first `length` events insert; the last
    k - 1 of them have k-mers that run into the poly-A and are left out, like everything behind them and chain 1"""
    k, sps = 9, 20
    for length in (400, k, k - 1, 3):
        ne0, ne1 = length + 237 - k + 1, 30 - k + 1
        ss = np.full(ne0 + ne1, sps)
        lo, hi = G.segments(ss, length, k, True, True, sps)["events"][3]
        assert (lo, hi) == (0, length)
        ev = dict(ev_read=np.zeros(ne0 + ne1, np.int64))
        ok, key, _ = PR.eligible_and_key(ev, [0, ne0 + ne1], [1000], [1], [length], k, True, True)
        assert np.flatnonzero(ok).tolist() == list(range(lo, max(hi - (k - 1), 0)))
        assert key[ok].tolist() == list(range(1000, 1000 + max(length - k + 1, 0)))
    # DNA with a prefix: the insert's events are the last ones, all of them whole; a stand-in read has none
    ok, key, _ = PR.eligible_and_key(dict(ev_read=np.zeros(85 + 50 - 6 + 1, np.int64)), [0, 130], [7], [-1], [50], 6, False, True)
    assert np.flatnonzero(ok).tolist() == list(range(85, 130)) and key[ok].tolist() == list(range(7, 7 - 45, -1))
    ok, _, _ = PR.eligible_and_key(dict(ev_read=np.zeros(5, np.int64)), [0, 5], [7], [1], [4], 6, False, False)
    assert not ok.any()


# ---------------------------------------------------------------------------------------------------------- GPU
EV_COLS = ("ev_read", "ev_len", "kmer", "seg", "mean", "sd")


def _table(b, norm, trim=False):
    """the columns of the batch's own event table pileup_ref takes"""
    ev = b.events(norm, trim, outputs=EV_COLS)
    out = {n: getattr(ev, n).cpu().numpy() for n in EV_COLS}
    out["kmer"] = out["kmer"].view(np.uint32)
    return out


def _got(p):
    out = {}
    for n in OUT:
        t = getattr(p, n)
        out[n] = None if t is None else (t.cpu().numpy().view(np.uint32) if n == "n" else t.cpu().numpy())
    return out


def _want(b, p, key0, step, lens, rna, prefix, into=None, ev=None):
    norm = "pa" if p.cfg.norm == api.CHUNK_PA else "medmad"
    ev = _table(b, norm, bool(p.cfg.trim)) if ev is None else ev
    return PR.pileup(ev, b.ev_off, key0, step, lens, b.gen.kmer_size, rna, prefix, p.cfg.by, p.cfg.split, p.cfg.segs, p.cfg.lo, p.cfg.hi, into)


def _assert_pile(p, want, what):
    got = _got(p)
    for n in OUT:
        if got[n] is None:
            continue
        assert got[n].shape == want[n].shape and got[n].dtype == want[n].dtype, f"{what}: {n} {got[n].shape} {got[n].dtype}"
        np.testing.assert_array_equal(got[n], want[n], err_msg=f"{what}: {n}")


def _sampler_origin(gen_contigs, b, k):
    s = b.sampled
    off = np.concatenate(([0], np.cumsum([len(c) for c in gen_contigs])))
    return PR.sampler_origin(off, s["ref_idx"], s["ref_pos"], s["rlen"], s["strand"], k)


def _own_reads(b, seqs):
    sig, dw = b.signal(), b.dwell()
    return [dict(sig=sig[b.sig_off[i]:b.sig_off[i + 1]], ss=dw[b.ev_off[i]:b.ev_off[i + 1]], seq=s, offset=float(b.offset[i])) for i, s in enumerate(seqs)]


class _Dna:
    """one sampled batch of the nCoV genome (dna-r9-prom, k = 6, 48 reads of about 1500 bases over 3 workers) and what the tests share of it"""
    made = None

    @classmethod
    def get(cls):
        if cls.made is None:
            prof, fl = profiles.get_profile("dna-r9-prom")
            k = 6
            mean, stdv = model.synthetic_model(k)
            gen = api.SignalGenerator(prof, fl, k, mean, stdv, 42, num_workers=3, mode=api.MODE_CERTIFIED)
            contigs, _ = _fasta(NCOV)
            gen.load_genome(contigs, 1500)
            b = gen.sample(48).run().wait()
            key0, step = _sampler_origin(contigs, b, k)
            cls.made = dict(gen=gen, b=b, k=k, level=mean, prof=prof, contigs=contigs, key0=key0, step=step, lens=b.sampled["rlen"].astype(np.int64),
                            glen=sum(len(c) for c in contigs), tables={})
        return cls.made

    @classmethod
    def table(cls, norm):
        d = cls.get()
        if norm not in d["tables"]:
            d["tables"][norm] = _table(d["b"], norm)
        return d["tables"][norm]


@pytest.mark.gpu
def test_sampled_dna_reads_of_both_strands():
    """the whole-genome window, all six outputs, both norms: against pileup_ref fed with Batch.events(), and with events_ref's table built
    from the reads, the signal and the dwells the batch hands back"""
    d = _Dna.get()
    gen, b, k = d["gen"], d["b"], d["k"]
    assert set(b.sampled["strand"]) == set(b"+-")
    own = _own_reads(b, b.reads())
    eligible = int(np.maximum(d["lens"] - k + 1, 0).sum())
    for norm in ("pa", "medmad"):
        p = gen.new_pileup(norm=norm)
        assert p.planes == 1 and (p.cfg.lo, p.cfg.hi) == (0, d["glen"]) and all(tuple(getattr(p, n).shape) == (1, d["glen"]) for n in OUT)
        counted, outside = b.pileup(p)
        want, wc, wo = _want(b, p, d["key0"], d["step"], d["lens"], False, False, ev=_Dna.table(norm))
        _assert_pile(p, want, f"sampled {norm}")
        assert (counted, outside) == (wc, wo) == (eligible, 0)
        ref = EV.batch_events(own, d["level"], k, False, False, False, int(d["prof"].dwell_mean), norm, False, d["prof"].range, d["prof"].digitisation)
        want2, _, _ = PR.pileup(ref, b.ev_off, d["key0"], d["step"], d["lens"], k, False, False, lo=0, hi=d["glen"])
        _assert_pile(p, want2, f"sampled {norm}, events_ref")
        n = _got(p)["n"]
        assert n.max() >= 2 and int(n.sum()) == counted                     # reads do collide
        assert _got(p)["dwell"].sum() == b.dwell().sum()                     # without a prefix every sample belongs to a counted event


@pytest.mark.gpu
def test_a_window_that_cuts_reads_and_guarded_outputs():
    """[lo, hi) through reads at both ends; every output inside a guarded buffer; any subset of the outputs may be NULL"""
    d = _Dna.get()
    gen, b, k = d["gen"], d["b"], d["k"]
    left = np.where(d["step"] > 0, d["key0"], d["key0"] - (d["lens"] - k))     # leftmost k-mer of every read
    order = np.argsort(left)
    lo, hi = int(left[order[5]]) + 123, int(left[order[-5]]) + 777
    assert lo < hi and ((left < lo) & (left + d["lens"] - k >= lo)).any() and ((left < hi) & (left + d["lens"] - k >= hi)).any()
    width, guard = hi - lo, 37
    dev = torch.device("cuda", gen.device)
    for names in (OUT, ("n",), ("mean_sq", "sd_sum"), ("dwell", "dwell_sq", "mean_sum"), ()):
        p = gen.new_pileup(norm="medmad", lo=lo, hi=hi, outputs=())
        bufs = {}
        for n in names:
            dt = torch.int32 if n == "n" else torch.int64
            bufs[n] = torch.full((width + 2 * guard,), -0x5a5a5a5b, dtype=dt, device=dev)
            bufs[n][guard:guard + width] = 0
            setattr(p, n, bufs[n][guard:guard + width].view(1, width))
            assert getattr(p, n).data_ptr() == bufs[n].data_ptr() + guard * bufs[n].element_size()
        counted, outside = b.pileup(p)
        want, wc, wo = _want(b, p, d["key0"], d["step"], d["lens"], False, False, ev=_Dna.table("medmad"))
        assert (counted, outside) == (wc, wo) and counted > 0 and outside > 0 and counted + outside == int(np.maximum(d["lens"] - k + 1, 0).sum())
        _assert_pile(p, want, f"window {names}")
        for n in names:
            g = bufs[n].cpu().numpy()
            assert (g[:guard] == -0x5a5a5a5b).all() and (g[guard + width:] == -0x5a5a5a5b).all(), f"{n}: a guard element was written"


@pytest.mark.gpu
def test_sums_are_added_to_and_two_calls_give_the_same_bytes():
    d = _Dna.get()
    gen, b, k = d["gen"], d["b"], d["k"]
    lo, hi = 3000, 21000
    fresh = gen.new_pileup(lo=lo, hi=hi)
    again = gen.new_pileup(lo=lo, hi=hi)
    st = b.pileup(fresh)
    assert b.pileup(again) == st
    for n in OUT:
        assert torch.equal(getattr(fresh, n), getattr(again, n)), n
    # arrays that hold something are added to
    rng = np.random.default_rng(3)
    into = {n: (rng.integers(0, 1 << 32, (1, hi - lo), dtype=np.uint32) if n == "n" else rng.integers(-1 << 63, (1 << 63) - 1, (1, hi - lo), dtype=np.int64)) for n in OUT}
    p = gen.new_pileup(lo=lo, hi=hi)
    for n in OUT:
        getattr(p, n).copy_(torch.from_numpy(into[n].view(np.int32) if n == "n" else into[n]))
    b.pileup(p)
    want, _, _ = _want(b, p, d["key0"], d["step"], d["lens"], False, False, into=into, ev=_Dna.table("pa"))
    _assert_pile(p, want, "pre-filled")
    with np.errstate(over="ignore"):
        for n in OUT:
            np.testing.assert_array_equal(_got(p)[n], into[n] + _got(fresh)[n], err_msg=n)
    # a second batch -- of a context of its own: the shared batch keeps its device results -- into the same pileup: the element-wise sum
    # of two separate pileups
    g2 = api.SignalGenerator(d["prof"], gen.flags, k, d["level"], model.synthetic_model(k)[1], 43, num_workers=2, mode=api.MODE_CERTIFIED)
    g2.load_genome(d["contigs"], 1500)
    b2 = g2.sample(20).run().wait()
    alone = gen.new_pileup(lo=lo, hi=hi)
    st2 = b2.pileup(alone)
    assert b2.pileup(fresh) == st2 and st2[0] > 0
    with np.errstate(over="ignore"):
        for n in OUT:
            np.testing.assert_array_equal(_got(fresh)[n], _got(again)[n] + _got(alone)[n], err_msg=n)
    assert int(_got(fresh)["n"].sum()) == st[0] + st2[0]
    b2.free(); g2.close()


@pytest.mark.gpu
def test_no_update_is_lost_when_every_read_hits_the_same_keys():
    """256 copies of one 300-base read over 8 workers (drawn dwells: every copy has its own signal), a caller's origin that lays all of them
    on one span -- half of them forwards, half backwards -- and 8 more reads with step 0.  A workgroup takes 256 events and a read has 295, so
    the adds to one key come from 256 different workgroups: n is 256 at every key"""
    prof, fl = profiles.get_profile("dna-r9-prom")
    k = 6
    mean, stdv = model.synthetic_model(k)
    gen = api.SignalGenerator(prof, fl, k, mean, stdv, 9, num_workers=8, mode=api.MODE_CERTIFIED)
    read = inject.seqs_for([300])[0]
    n_reads, span = 264, 300 - k + 1
    b = gen.stage([read] * n_reads, workers=np.arange(n_reads) % 8).run().wait()
    step = np.array([1, -1] * 128 + [0] * 8, np.int8)
    key0 = np.where(step < 0, 1000 + span - 1, 1000).astype(np.int64)
    lens = np.full(n_reads, 300)
    assert len(set(b.dwell()[:span].tolist())) > 5 and not np.array_equal(b.dwell()[:span], b.dwell()[span:2 * span])
    for norm in ("pa", "medmad"):
        p = gen.new_pileup(norm=norm, lo=1000, hi=1000 + span)
        counted, outside = b.pileup(p, origin=(key0, step))
        assert (counted, outside) == (256 * span, 0)
        assert (_got(p)["n"] == 256).all()
        want, _, _ = _want(b, p, key0, step, lens, False, False)
        _assert_pile(p, want, f"contended {norm}")
        assert _got(p)["dwell"].sum() == b.dwell()[:256 * span].sum()
    p = gen.new_pileup(lo=1000, hi=1000 + span)                # only the reads that are not counted
    assert b.pileup(p, origin=(key0, np.where(step == 0, 1, 0).astype(np.int8))) == (8 * span, 0) and (_got(p)["n"] == 8).all()
    p = gen.new_pileup(lo=1000, hi=1000 + span)
    assert b.pileup(p, origin=(key0, np.zeros(n_reads, np.int8))) == (0, 0) and all(not _got(p)[n].any() for n in OUT)
    b.free(); gen.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dwell", [1, LANE_MAX, LANE_MAX + 1, 5000])
def test_constant_dwell_with_injected_signals(dwell):
    """every dwell 1, 64 (the last a lane takes alone), 65 (the first its wavefront takes) and 5000; the samples overwritten with the cases of
    signal_cases.py, the ends of int16 among them.  Reads of 3, 1, 70 and 2 events laid over each other, one of them backwards; mean_sq
    starts just below 2^63 and wraps"""
    prof, fl = profiles.get_profile("dna-r9-prom")
    prof = prof.replace(dwell_mean=float(dwell), dwell_std=0.0)
    fl |= profiles.SQ_IDEAL_TIME
    k = profiles.default_kmer_size(fl)
    mean, stdv = model.synthetic_model(k)
    gen = api.SignalGenerator(prof, fl, k, mean, stdv, inject.SEED, num_workers=1, mode=api.MODE_CERTIFIED)
    events = [3, 1, 70, 2]
    seqs = inject.seqs_for(inject.bases_for([e * dwell for e in events], k, dwell))
    b = inject.run_geometry(gen, seqs)
    assert b.n_events == 76 and b.n_samples == 76 * dwell
    lens = np.array([len(s) for s in seqs])
    key0, step = np.array([0, 1, 69, 3], np.int64), np.array([1, 1, -1, 1], np.int8)
    top = np.iinfo(np.int64).max
    for name in ("svb_wrap", "all_equal", "uniform", "svb_classes"):
        inject.inject(b, signal_cases.CASES[name](b.sig_off))
        for norm, trim in (("pa", False), ("medmad", True)):
            p = gen.new_pileup(norm=norm, trim=trim, lo=0, hi=70)
            p.mean_sq.fill_(top)
            assert b.pileup(p, origin=(key0, step)) == (76, 0)
            want, _, _ = _want(b, p, key0, step, lens, False, False, into=dict(mean_sq=np.full((1, 70), top)))
            _assert_pile(p, want, f"dwell {dwell} {name} {norm}")
            g = _got(p)
            assert g["n"][0].tolist() == [2, 3, 2, 2, 2] + [1] * 65 and (g["dwell"] == dwell * g["n"]).all() and (g["dwell_sq"] == dwell * dwell * g["n"].astype(np.int64)).all()
            if name == "uniform" and norm == "pa":
                assert (g["mean_sq"] < 0).all()                                                     # 2^63 - 1 plus a square: wrapped
    b.free(); gen.close()


KMER_CASES = {  # name -> (profile, extra flags, letters)
    "dna": ("dna-r9-prom", 0, b"ACGT"),
    "meth": ("dna-r9-prom", profiles.SQ_METH, b"ACGTM"),
    "rna004_prefix": ("rna004-prom", profiles.SQ_PREFIX, b"ACGU"),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(KMER_CASES))
def test_by_kmer(name):
    """keyed by pore-table row, no origin: against np.bincount / np.add.at over events().kmer and .seg; the insert only, all four segments,
    the stall only; a window over a subrange of the rows; a read shorter than a k-mer counts with its stand-in events"""
    pname, extra, letters = KMER_CASES[name]
    prof, fl = profiles.get_profile(pname)
    fl |= extra
    k = profiles.default_kmer_size(fl)
    meth, rna, prefix = bool(fl & profiles.SQ_METH), bool(fl & profiles.SQ_RNA), bool(fl & profiles.SQ_PREFIX)
    rows = 5 ** k if meth else 4 ** k
    assert (k, rows) == ((9, 262144) if name == "rna004_prefix" else (6, 15625 if meth else 4096))
    level, stdv = model.synthetic_model(k, meth=meth)
    gen = api.SignalGenerator(prof, fl, k, level, stdv, 5, num_workers=2, mode=api.MODE_CERTIFIED)
    rng = np.random.default_rng(8)
    seqs = [bytes(rng.choice(list(letters), m).astype(np.uint8)) for m in (700, 2, 1300, k, 90)]
    b = gen.submit(seqs)
    ev = _table(b, "pa")
    q_mean, q_sd, ln = PR.q(ev["mean"]), PR.q(ev["sd"]), ev["ev_len"].astype(np.int64)
    assert set(ev["seg"].tolist()) == ({0, 1, 2, 3} if prefix else {3})
    for segs, lo, hi in (((3,), None, None), ((0, 1, 2, 3), None, None), ((0,), None, None), (None, rows // 3, rows // 3 + rows // 2)):
        p = gen.new_pileup(by="kmer", segs=segs, lo=lo, hi=hi)
        lo, hi = p.cfg.lo, p.cfg.hi
        assert (lo, hi) == (0, rows) or segs is None
        counted, outside = b.pileup(p)
        sel = np.isin(ev["seg"], list(segs or (3,)))
        inside = sel & (ev["kmer"] >= lo) & (ev["kmer"] < hi)
        assert (counted, outside) == (int(inside.sum()), int((sel & ~inside).sum())) and (counted > 0 or (segs == (0,) and not prefix))
        g = _got(p)
        at = ev["kmer"][inside].astype(np.int64) - lo
        np.testing.assert_array_equal(g["n"][0], np.bincount(at, minlength=hi - lo).astype(np.uint32))
        assert int(g["n"].sum()) == counted
        for n, col in (("dwell", ln), ("dwell_sq", ln * ln), ("mean_sum", q_mean), ("mean_sq", q_mean * q_mean), ("sd_sum", q_sd)):
            w = np.zeros(hi - lo, np.int64)
            np.add.at(w, at, col[inside])
            np.testing.assert_array_equal(g[n][0], w, err_msg=f"{name} segs {segs} {n}")
    if not prefix:                                            # the stand-in events of the read of 2 bases are counted by row
        short = slice(int(b.ev_off[1]), int(b.ev_off[2]))
        assert (ev["kmer"][short] == T.kmer_ranks(G.SHORT_HACK[:5 + k - 1], k, meth)).all() and (ev["seg"][short] == 3).all()
    b.free(); gen.close()


@pytest.mark.gpu
def test_planes_by_strand_and_by_methylation():
    """sampled methylated reads of both strands: a plane per strand, per methylation state, and both; the planes add up to the unsplit
    pileup, and the 'M' plane holds exactly the keys of the k-mers of Batch.reads() that carry an 'M'"""
    prof, fl = profiles.get_profile("dna-r9-prom")
    fl |= profiles.SQ_METH
    k, rlen = 6, 1500
    mean, stdv = model.synthetic_model(k, meth=True)
    contigs, names = _fasta(NCOV)
    gen = api.SignalGenerator(prof, fl, k, mean, stdv, 42, num_workers=3, mode=api.MODE_CERTIFIED)
    gen.load_genome(contigs, rlen)
    gen.set_meth(contigs, names, MFREQ_DENSE)
    b = gen.sample(24).run().wait()
    seqs = b.reads()
    assert set(b.sampled["strand"]) == set(b"+-") and all(any(b"M" in s for s, sd in zip(seqs, b.sampled["strand"]) if sd == c) for c in b"+-")
    key0, step = _sampler_origin(contigs, b, k)
    lens = b.sampled["rlen"].astype(np.int64)
    ev = _table(b, "pa")
    flat = gen.new_pileup()
    st = b.pileup(flat)
    _assert_pile(flat, _want(b, flat, key0, step, lens, False, False, ev=ev)[0], "unsplit")
    for split in (("meth",), ("strand",), ("strand", "meth")):
        p = gen.new_pileup(split=split)
        assert p.planes == 2 ** len(split) and b.pileup(p) == st
        _assert_pile(p, _want(b, p, key0, step, lens, False, False, ev=ev)[0], f"split {split}")
        g = _got(p)
        assert all(g["n"][q].any() for q in range(p.planes)), f"{split}: an empty plane"
        with np.errstate(over="ignore"):
            for n in OUT:
                np.testing.assert_array_equal(g[n].sum(axis=0, dtype=g[n].dtype), _got(flat)[n][0], err_msg=f"{split} {n}")
    meth_keys = {(int(key0[i]) + int(step[i]) * j, int(step[i] < 0)) for i, s in enumerate(seqs) for j in range(len(s) - k + 1) if b"M" in s[j:j + k]}
    g = _got(p)["n"]                                            # (strand, meth): planes 2 and 3 are the 'M' k-mers of '+' and '-'
    assert {(int(x), s) for s in (0, 1) for x in np.flatnonzero(g[2 + s])} == meth_keys and len(meth_keys) > 50
    with pytest.raises(api.SqgError) as e:                      # a context without the 5-letter table has no 'M' plane
        d = _Dna.get()
        d["b"].pileup(d["gen"].new_pileup(split=("meth",)))
    assert e.value.code == -1 and "SQG_METH" in str(e.value)
    b.free(); gen.close()


@pytest.mark.gpu
@pytest.mark.parametrize("prefix,trunc", [(False, False), (True, False), (True, True)], ids=["plain", "prefix", "prefix_trunc"])
def test_sampled_rna_reads(prefix, trunc):
    """sequin transcripts, rna004 (k = 9): only whole insert k-mers are counted -- no stall, adaptor or poly-A event, and with a prefix
    not the last k - 1 insert events; SQG_SAMPLE_TRUNC starts reads inside the transcripts"""
    prof, fl = profiles.get_profile("rna004-prom")
    fl |= profiles.SQ_PREFIX if prefix else 0
    k = profiles.default_kmer_size(fl)
    mean, stdv = model.synthetic_model(k)
    contigs, _ = _fasta(SEQUIN)
    gen = api.SignalGenerator(prof, fl, k, mean, stdv, 42, num_workers=3, mode=api.MODE_CERTIFIED)
    gen.load_genome(contigs, 1500, api.SAMPLE_RNA | (api.SAMPLE_TRUNC if trunc else 0))
    b = gen.sample(9).run().wait()
    key0, step = _sampler_origin(contigs, b, k)
    lens = b.sampled["rlen"].astype(np.int64)
    assert (b.sampled["ref_pos"] > 0).any() == trunc and (step == 1).all()
    ev = _table(b, "medmad", True)
    p = gen.new_pileup(norm="medmad", trim=True)
    counted, outside = b.pileup(p)
    want, wc, wo = _want(b, p, key0, step, lens, True, prefix, ev=ev)
    _assert_pile(p, want, "rna")
    assert (counted, outside) == (wc, wo) == (int((lens - k + 1).sum()), 0)
    ok, key, _ = PR.eligible_and_key(ev, b.ev_off, key0, step, lens, k, True, prefix)
    assert (ev["seg"][ok] == 3).all()
    insert = np.bincount(ev["ev_read"][ev["seg"] == 3], minlength=b.n_reads)
    np.testing.assert_array_equal(np.bincount(ev["ev_read"][ok], minlength=b.n_reads), insert - (k - 1 if prefix else 0))
    if prefix:
        assert set(ev["seg"].tolist()) == {0, 1, 2, 3}
    # every counted key lies inside the read's transcript
    off = np.concatenate(([0], np.cumsum([len(c) for c in contigs])))
    r = ev["ev_read"][ok]
    assert (key[ok] >= off[b.sampled["ref_idx"]][r]).all() and (key[ok] + k <= off[b.sampled["ref_idx"] + 1][r]).all()
    # the reads as the sampler returned them are the genome at the keys
    seqs = b.reads()
    genome = b"".join(contigs).upper().replace(b"T", b"U")
    assert all(seqs[i].upper().replace(b"T", b"U")[:k] == genome[int(key0[i]):int(key0[i]) + k] for i in range(b.n_reads))
    b.free()
    if not prefix:                                            # a staged read shorter than a k-mer adds nothing by position
        b = gen.submit([b"ACGUACG", inject.seqs_for([40])[0]])
        p = gen.new_pileup(lo=0, hi=100)
        assert b.pileup(p, origin=(np.array([0, 50]), np.array([1, 1]))) == (40 - k + 1, 0)
        assert not _got(p)["n"][0][:50].any() and (_got(p)["n"][0][50:50 + 40 - k + 1] == 1).all()
        b.free()
    gen.close()


def _raw(gen, b, cfg, origin, out, stat=None):
    return gen.L.sqg_batch_pileup(gen.ctx, b.handle if b is not None else None, C.byref(cfg) if cfg is not None else None,
                                  C.byref(origin) if origin is not None else None, C.byref(out) if out is not None else None,
                                  C.byref(stat) if stat is not None else None)


@pytest.mark.gpu
def test_errors():
    d = _Dna.get()
    gen, b = d["gen"], d["b"]
    Lb, none = gen.L, api.CPileupOut()
    err = lambda: Lb.sqg_last_error(gen.ctx)                # noqa: E731
    good = dict(by=0, split=0, norm=api.CHUNK_PA, trim=0, segs=0, lo=0, hi=100)
    cfg = api.CPileupCfg(**good)
    st = api.CPileupStat(-1, -1)
    assert _raw(gen, b, cfg, None, none, st) == 0 and st.counted >= 0 and st.counted + st.outside == int((d["lens"] - d["k"] + 1).sum())   # nothing wanted: only counted
    assert _raw(gen, b, cfg, None, none) == 0                                                # ... and stat may be NULL
    assert Lb.sqg_batch_pileup(None, None, None, None, None, None) == -1 and Lb.sqg_batch_pileup(None, b.handle, C.byref(cfg), None, C.byref(none), None) == -1
    assert _raw(gen, None, cfg, None, none) == -1 and b"sqg_batch_pileup" in err() and b"batch" in err()
    assert _raw(gen, b, None, None, none) == -1 and b"sqg_batch_pileup" in err() and b"cfg" in err()
    assert _raw(gen, b, cfg, None, None) == -1 and b"sqg_batch_pileup" in err() and b"out" in err()
    for bad, what in ((dict(by=2), b"by"), (dict(split=4), b"split"), (dict(split=8 | 1), b"split"), (dict(norm=2), b"norm"), (dict(trim=2), b"trim"), (dict(trim=-1), b"trim"),
                      (dict(segs=16), b"segs"), (dict(by=1, segs=0x80000000), b"segs"), (dict(lo=5, hi=4), b"hi"), (dict(split=2), b"SQG_METH")):
        assert _raw(gen, b, api.CPileupCfg(**dict(good, **bad)), None, none) == -1 and b"sqg_batch_pileup" in err() and what in err(), bad
    n = b.n_reads
    key0, step = np.zeros(n, np.int64), np.ones(n, np.int8)
    kp, sp = key0.ctypes.data_as(C.POINTER(C.c_int64)), step.ctypes.data_as(C.POINTER(C.c_int8))
    assert _raw(gen, b, cfg, api.COrigin(kp, sp), none) == 0
    assert _raw(gen, b, cfg, api.COrigin(None, sp), none) == -1 and b"origin" in err()
    assert _raw(gen, b, cfg, api.COrigin(kp, None), none) == -1 and b"origin" in err()
    for v in (2, -2, 127, -128):
        step[n // 2] = v
        assert _raw(gen, b, cfg, api.COrigin(kp, sp), none) == -1 and b"step" in err(), v
    for bad in (dict(by="row"), dict(norm="z"), dict(split=("colour",)), dict(outputs=("n", "median")), dict(lo=9, hi=3)):
        with pytest.raises(api.SqgError) as e:
            gen.new_pileup(**bad)
        assert e.value.code == -1, bad
    with pytest.raises(api.SqgError) as e:
        b.pileup(gen.new_pileup(), origin=(key0[:-1], step[:-1]))
    assert e.value.code == -1
    p = gen.new_pileup(lo=77, hi=77)                          # an empty window: nothing is added, every event is outside
    assert b.pileup(p) == (0, int((d["lens"] - d["k"] + 1).sum())) and all(tuple(getattr(p, n).shape) == (1, 0) for n in OUT)
    # a staged batch: no sampler origin; by position and per strand need one, by row does not; and it has to be run
    prof, fl = profiles.get_profile("dna-r9-prom")
    mean, stdv = model.synthetic_model(6)
    g2 = api.SignalGenerator(prof, fl, 6, mean, stdv, 1, mode=api.MODE_CERTIFIED)
    with pytest.raises(api.SqgError) as e:
        g2.new_pileup()                                         # no genome: no default window
    assert e.value.code == -1
    s = g2.stage(inject.seqs_for([50, 60]))
    for kw in (dict(by="kmer"), dict(by="ref", lo=0, hi=100)):
        with pytest.raises(api.SqgError) as e:                  # staged, not run: an error, not a hang
            s.pileup(g2.new_pileup(**kw), origin=(np.zeros(2, np.int64), np.ones(2, np.int8)))
        assert e.value.code == -4 and "sqg_batch_pileup" in str(e.value) and "not been run" in str(e.value)
    s.run().wait()
    for kw in (dict(by="ref", lo=0, hi=100), dict(by="kmer", split=("strand",))):
        with pytest.raises(api.SqgError) as e:
            s.pileup(g2.new_pileup(**kw))
        assert e.value.code == -1 and "origin" in str(e.value) and "sampled" in str(e.value), kw
    assert s.pileup(g2.new_pileup(by="kmer")) == (50 + 60 - 2 * 5, 0)
    assert s.pileup(g2.new_pileup(by="kmer", split=("strand",)), origin=(np.zeros(2, np.int64), np.array([1, -1], np.int8))) == (50 + 60 - 2 * 5, 0)
    e0 = g2.submit([])                                          # an empty batch succeeds and adds nothing
    p = g2.new_pileup(by="kmer")
    assert e0.pileup(p) == (0, 0) and not _got(p)["n"].any()
    e0.free(); s.free(); g2.close()


@pytest.mark.gpu
def test_lifetime_and_a_pileup_while_the_generator_runs_ahead():
    """a batch keeps what the pileup needs until two more batches have been run; taken while two later batches are staged and one is
    running it is what it was when the generator was quiet"""
    o, k, rna, meth, prefix, sps, level = (lambda o: (o, o.kmer_size_default, True, False, bool(o.flags & profiles.SQ_PREFIX), int(o.profile.dwell_mean), None))(
        options.parse_args(dict(REFVEC_CASES)["rna004_tk4"]))
    reads = _fixture_reads("rna004_tk4")
    _, _, gen = _context(dict(REFVEC_CASES)["rna004_tk4"], api.MODE_EXACT)
    parts = [[r["seq"] for r in reads[0:4]], [r["seq"] for r in reads[4:8]], [r["seq"] for r in reads[0:4]], [r["seq"] for r in reads[4:8]]]
    lens = np.array([len(s) for s in parts[0]])
    key0, step = np.arange(4, dtype=np.int64) * 100, np.ones(4, np.int8)
    hi = int((key0 + lens).max())
    new = lambda: gen.new_pileup(norm="medmad", trim=True, lo=0, hi=hi)      # noqa: E731
    b0 = gen.stage(parts[0]).run().wait()
    quiet = new()
    st = b0.pileup(quiet, origin=(key0, step))
    _assert_pile(quiet, _want(b0, quiet, key0, step, lens, rna, prefix)[0], "quiet")
    assert st == (int(np.maximum(lens - k + 1, 0).sum()), 0) and st[0] > 0
    b1, b2, b3 = (gen.stage(p) for p in parts[1:])
    b1.run()                                                # one running, two staged
    busy = new()
    assert b0.pileup(busy, origin=(key0, step)) == st
    b1.wait()
    again = new()                                           # after one more batch has run: the same
    assert b0.pileup(again, origin=(key0, step)) == st
    for n in OUT:
        assert torch.equal(getattr(busy, n), getattr(quiet, n)) and torch.equal(getattr(again, n), getattr(quiet, n)), n
    b2.run().wait()
    with pytest.raises(api.SqgError) as e:                  # two more batches: slabs and dwells are batch 2's
        b0.pileup(new(), origin=(key0, step))
    assert e.value.code == -4 and "sqg_batch_pileup" in str(e.value)
    lens1 = np.array([len(s) for s in parts[1]])
    p = gen.new_pileup(lo=0, hi=int(lens1.max()))
    assert b1.pileup(p, origin=(np.zeros(4, np.int64), step))[0] == int(np.maximum(lens1 - k + 1, 0).sum())
    _assert_pile(p, _want(b1, p, np.zeros(4, np.int64), step, lens1, rna, prefix)[0], "batch 1 after batch 2")
    for b in (b0, b1, b2, b3):
        b.free()
    gen.close()
