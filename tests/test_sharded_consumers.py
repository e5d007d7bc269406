"""The consumer calls -- sqg_batch_chunks / sqg_chunk_plan, sqg_batch_chunk_targets, sqg_batch_segments and the *_trimmed calls,
sqg_site_plan / sqg_batch_sites, sqg_batch_events, sqg_batch_pileup, sqg_detect_plan / sqg_batch_detect, sqg_batch_align, sqg_batch_scale,
sqg_batch_align_scaled, sqg_batch_collapse, sqg_batch_pileup_rows, sqg_call_plan / sqg_batch_call -- on batches
made the way several GPUs make them: range-sharded contexts (sqg_batch_run_begin / _end), worker-sharded contexts, and contexts on host
threads of their own (tests/shard_cases.py has the jobs and the drivers).  What a rank that holds reads idx of the job must produce is
the numpy reference of the call's header over [reads[i] for i in idx], the reads being those of the oracle's single-process run of the
whole job; and the same job on one plain context, restricted to the rank's reads and renumbered, gives the same rows.  Every comparison
is bit for bit (floats as integers)."""
import ctypes as C
import threading
import time
import warnings

import numpy as np
import pytest
import torch  # noqa: F401  (before the library is loaded: the HIP runtime torch brings is the one the library then uses)

import chunks_ref as R
import events_ref as EV
import pileup_ref as PR
import segments_ref as SR
import shard_cases as SC
from squigulator_amd import api, profiles, shard

SHARDED = [n for n in SC.JOBS if SC.JOBS[n]["G"] > 1]
RUNS = [(n, api.MODE_CERTIFIED) for n in SHARDED] + [(n, api.MODE_EXACT) for n in SHARDED if SC.JOBS[n].get("exact")]
RUN_IDS = [f"{n}-{'exact' if m == api.MODE_EXACT else 'certified'}" for n, m in RUNS]
OUT = api.PILEUP_OUTPUTS


# ---------------------------------------------------------------------------------------------------------- no GPU
def _detect_align_hold(su, reads, what):
    """what the detect and align groups need of a rank's reads, asserted of detect_ref, align_ref and events_ref alone -> the detected
    rows under either setting.  Both settings detect rows; under setting B both detectors record; the alignment of the detected rows is
    neither the detector's own answer nor lost (true_ev is the event under a row's first sample, al_ev the event the row is aligned to);
    RNA with a prefix has a read whose path runs along the band's rim; the staged range jobs hold a read that the full matrix covers"""
    p = su.prof
    ev = EV.batch_events(reads, su.mean, su.k, su.rna, su.meth, su.prefix, su.sps, "pa", False, p.range, p.digitisation)
    seen = {}
    w = su.expected_detect_align(reads, ev, seen=seen)
    rows = {name: len(w[name]["read"]) for name in ("detect A", "detect B")}
    assert min(rows.values()) > len(reads), f"{what}: detected rows {rows}"
    assert seen["detect B"]["short"] >= 1 and seen["detect B"]["long"] >= 1, f"{what}: under setting B the detectors recorded {seen['detect B']}"
    assert np.array_equal(w["align detected"]["off"], w["detect A"]["off"]) and np.array_equal(w["align truth"]["off"], ev["ev_off"])
    share = float((w["align detected"]["rows"]["al_ev"] == w["detect A"]["rows"]["true_ev"]).mean())
    edge = int((w["align detected"]["per_read"]["al_edge"] > 0).sum())
    few = int((np.diff(ev["ev_off"]) <= 32).sum())
    print(f"{what}: {share:.3f} of the detected rows aligned to the event under their first sample, {edge} reads with al_edge > 0, {few} reads of at most 32 events")
    assert 0.5 < share < 1, f"{what}: {share} of the detected rows are aligned to the event under their first sample"
    if su.name == "rna004_prefix_g2":
        assert edge > 0, f"{what}: no read with al_edge > 0"
    if "short" in su.job:
        assert few > 0, f"{what}: no read of at most 32 events"
        short = [i for i, r in enumerate(reads) if len(r["seq"]) < su.k]            # these are among them: five stand-in events each
        print(f"{what}: the reads shorter than a k-mer have {[int(w['detect A']['off'][i + 1] - w['detect A']['off'][i]) for i in short]} detected rows")
        assert short and all(ev["ev_off"][i + 1] - ev["ev_off"][i] == 5 for i in short)
    return rows


def _chain_holds(su, job):
    """what the scale, collapse and call groups need of a job, asserted of the chained references over the whole job (Setup.job_chain):
    in every rank that holds a read the fit gives a gain other than 65536 and a shift other than 0, an event has no row and another
    one two or more (the reads shorter than a k-mer of the staged range jobs, the first or last of their ranks, are among the reads
    scaled: test_the_jobs_hold_what_can_go_wrong asserts where they lie); and under SQG_METH every rank that holds a read holds a CpG
    site, the site counts differ from rank to rank, a staged job has sites that the frequency table does not take (reads without a
    step), all three call values occur, and a frequency key is added to by sites of two different ranks"""
    name = su.name
    chain = su.job_chain()
    lo, hi = su.window()
    rank_keys = [set() for _ in range(su.G)]
    calls, outside = set(), 0
    for bi, (o, (groups, inner, _)) in enumerate(zip(job, chain)):
        n = len(o["reads"])
        fit, co = groups["scale fit"]["per_read"], groups["collapse pa 0"]
        ev_off = co["off"]
        sites = []
        for g in range(su.G):
            idx = su.rank_reads(n, g)
            if not len(idx):
                continue
            ev = np.concatenate([np.arange(ev_off[i], ev_off[i + 1]) for i in idx])
            row = dict(gains=int((fit["gain"][idx] != 65536).sum()), shifts=int((fit["shift"][idx] != 0).sum()), fallbacks=int((fit["n"][idx] < 2).sum()),
                       unseen=int((co["rows"]["ob_rows"][ev] == 0).sum()), summed=int((co["rows"]["ob_rows"][ev] >= 2).sum()), dropped=int(co["per_read"]["rd_dropped"][idx].sum()))
            assert row["gains"] and row["shifts"] and row["unseen"] and row["summed"], f"{name} batch {bi} rank {g}: {row}"
            if su.calls:
                c = groups["call observed"]
                mine = np.isin(c["read"], idx)
                key = c["rows"]["site_key"][mine]
                row.update(sites=int(mine.sum()), unobserved=int((c["rows"]["n_obs"][mine] == 0).sum()), called=int((c["rows"]["call"][mine] != 0).sum()))
                rank_keys[g] |= set(key[(key >= lo) & (key < hi)].tolist())
                calls |= set(c["rows"]["call"][mine].tolist())
                sites.append(row["sites"])
            print(f"{name} batch {bi} rank {g}: " + ", ".join(f"{v} {key}" for key, v in row.items()))
        if su.calls:
            outside += groups["call observed"]["stat"][1]
            assert min(sites) > 0 and len(set(sites)) == len(sites), f"{name} batch {bi}: call sites per rank {sites}"
    if su.calls:
        both = set().union(*[rank_keys[a] & rank_keys[b] for a in range(su.G) for b in range(a + 1, su.G)])
        print(f"{name}: {len(both)} frequency keys added to by sites of two different ranks, {outside} sites outside, call values {sorted(calls)}")
        assert both and calls == {0, 1, 2} and (outside > 0 or su.sampled)


@pytest.mark.parametrize("name", SHARDED)
def test_the_jobs_hold_what_can_go_wrong(name):
    """from the oracle and the numpy references alone: every rank but the designated empty one holds a read; a sampled DNA job holds both
    strands; a job with sites holds a site in every rank that has a read, a dropped candidate and under SQG_METH both labels; a job
    piled up by position has a key that reads of two different ranks add to; a staged job's steps take all three values in every rank;
    every rank of the staged range jobs holds a read shorter than a k-mer, as its first or last read among others; the chunk, site,
    event and detected-row counts of a batch's ranks are above zero and differ from rank to rank; and every rank that holds a read holds
    what the detect and align groups need (_detect_align_hold) and what the scale, collapse and call groups need (_chain_holds)"""
    su = SC.Setup(name)
    j = su.job
    job = su.oracle_job()
    L, St, _ = SC.CHUNK
    shared_job, labels, dropped, strands, edges = 0, set(), 0, set(), set()
    for bi, o in enumerate(job):
        n = len(o["reads"])
        counts, keys = [], []
        for g in range(su.G):
            idx = su.rank_reads(n, g)
            reads = [o["reads"][i] for i in idx]
            assert (len(idx) == 0) == ((bi, g) in j.get("empty", ())), f"{name} batch {bi} rank {g}: {len(idx)} reads"
            short = sum(len(r["seq"]) < su.k for r in reads)
            assert (short > 0) == ("short" in j), f"{name} batch {bi} rank {g}: {short} reads shorter than a k-mer"
            if short:
                edges |= ({"first"} if len(reads[0]["seq"]) < su.k else set()) | ({"last"} if len(reads[-1]["seq"]) < su.k else set())
            row = dict(reads=len(idx), short=short, events=sum(len(r["ss"]) for r in reads),
                       chunks=sum(R.n_chunks_of(len(r["sig"]), L, St) for r in reads if len(r["seq"]) >= su.k))
            if su.sites:
                w = su.expected_sites(reads)
                row.update(sites=int(w["site_off"][-1]), label1=int(w["label"].sum()), dropped=int(w["dropped"].sum()))
                labels |= set(w["label"].tolist()); dropped += row["dropped"]
            if len(idx):
                row.update(_detect_align_hold(su, reads, f"{name} batch {bi} rank {g}"))
            if not su.sampled and len(idx):
                assert set(o["step"][idx].tolist()) == {-1, 0, 1}, f"{name} batch {bi} rank {g}: steps {o['step'][idx]}"
            keys.append(set(su.keys(o, idx).tolist()))
            counts.append(row)
            print(f"{name} batch {bi} rank {g}: " + ", ".join(f"{v} {key}" for key, v in row.items()))
        shared = set().union(*[keys[a] & keys[b] for a in range(su.G) for b in range(a + 1, su.G)])
        shared_job += len(shared)
        print(f"{name} batch {bi}: strands {o['strand']}, {len(shared)} positions keyed by reads of two different ranks")
        strands |= set(o["strand"] or "")
        full = [c for c in counts if c["reads"]]
        for what in ("events", "chunks", "detect A", "detect B") + (("sites",) if su.sites else ()):
            vals = [c[what] for c in full]
            assert min(vals) > 0 and len(set(vals)) == len(vals), f"{name} batch {bi}: {what} per rank {vals}"
        if "expect" in j:                                   # the figures of the case table
            sites, label1, drop, per_rank, both = j["expect"][bi]
            assert sum(c["sites"] for c in counts) == sites
            assert label1 is None or sum(c["label1"] for c in counts) == label1
            assert drop is None or sum(c["dropped"] for c in counts) == drop
            assert per_rank is None or [c["sites"] for c in counts] == per_rank
            assert both is None or len(shared) == both
        if j.get("strands") and j["strands"][bi]:
            assert o["strand"] == j["strands"][bi]
        if "shared" in j:
            assert len(shared) == j["shared"][bi]
        if "short" in j:                                    # the table's reads and no others; the oracle gives each its five stand-in events
            at = sorted(i for b, i, _ in j["short"] if b == bi)
            assert at == [i for i, r in enumerate(o["reads"]) if len(r["seq"]) < su.k] and all(len(o["reads"][i]["ss"]) == 5 for i in at)
    if "short" in j:
        assert edges == {"first", "last"}, f"{name}: a read shorter than a k-mer is a rank's {sorted(edges)} read only"
    if su.sampled and not su.rna:
        assert strands == {"+", "-"}
    if su.sites:
        assert dropped > 0 and labels == ({0, 1} if su.meth else {0})
    assert shared_job > 0
    _chain_holds(su, job)
    kw = su.pile_cfgs()["ref_window"][0]
    allk = np.concatenate([su.keys(o, np.arange(len(o["reads"]))) for o in job])
    assert kw["lo"] < kw["hi"] and (allk < kw["lo"]).any() and (allk >= kw["hi"]).any()          # the window cuts reads


@pytest.mark.parametrize("name", ["staged_t2_g2_meth", "rna004_prefix_g2", "r10_g2"])
def test_the_fast_statements_are_the_plain_references(name):
    """the groups as the GPU tests take them -- detect_vec.batch_rows_of_reads and the oracle's compiled banded recurrence -- against
    detect_ref.batch_rows and align_ref.banded themselves, bit for bit, on every rank of a job's first batch: reads shorter than a k-mer
    and SQG_METH; RNA with a prefix, trimmed statistics and paths on the band's rim; R10's nine-base k-mers"""
    su = SC.Setup(name)
    p = su.prof
    o = su.oracle_job()[0]
    for g in range(su.G):
        reads = [o["reads"][i] for i in su.rank_reads(len(o["reads"]), g)]
        ev = EV.batch_events(reads, su.mean, su.k, su.rna, su.meth, su.prefix, su.sps, "pa", False, p.range, p.digitisation)
        fast, plain = {}, {}
        SC.assert_groups(su.expected_detect_align(reads, ev, seen=fast), su.expected_detect_align(reads, ev, seen=plain, plain=True), f"{name} rank {g}")
        assert fast == plain and fast["detect B"]["long"] >= 1


@pytest.mark.parametrize("name", ["staged_t2_g2", "rna004_prefix_g2", "workers_t6_g3"])
def test_restrict_renumbers_the_event_indices(name):
    """the references alone: the detect and align groups of a whole batch, restricted to a rank's reads, are the groups of those reads --
    true_ev and al_ev in the rank's own numbering of the events, as absolute indices; for every rank but the first they differ from the
    whole batch's"""
    su = SC.Setup(name)
    p = su.prof
    o = su.oracle_job()[0]
    table = lambda reads: EV.batch_events(reads, su.mean, su.k, su.rna, su.meth, su.prefix, su.sps, "pa", False, p.range, p.digitisation)      # noqa: E731
    ev = table(o["reads"])
    whole = su.expected_detect_align(o["reads"], ev)
    whole["events pa 0"] = dict(off=ev["ev_off"], read=ev["ev_read"], rows={}, per_read={})
    moved = 0
    for g in range(su.G):
        idx = su.rank_reads(len(o["reads"]), g)
        reads = [o["reads"][i] for i in idx]
        evr = table(reads)
        want = su.expected_detect_align(reads, evr)
        want["events pa 0"] = dict(off=evr["ev_off"], read=evr["ev_read"], rows={}, per_read={})
        got = SC.restrict(whole, idx)
        SC.assert_groups(got, want, f"{name} rank {g}")
        for gname, key in (("detect A", "true_ev"), ("detect B", "true_ev"), ("align detected", "al_ev"), ("align truth", "al_ev")):
            v = got[gname]["rows"][key]
            assert len(v) and (v >= 0).all() and (v < evr["ev_off"][-1]).all()
            rows = np.concatenate([np.arange(whole[gname]["off"][i], whole[gname]["off"][i + 1]) for i in idx])
            moved += int((whole[gname]["rows"][key][rows] != v).any())
    assert moved >= 4 * (su.G - 1)


# ---------------------------------------------------------------------------------------------------------- GPU
def _pile_sum(parts):
    out = {n: parts[0][n].copy() for n in OUT}
    with np.errstate(over="ignore"):
        for p in parts[1:]:
            for n in OUT:
                out[n] += p[n]
    return out


def _assert_pile(got, want, what):
    for n in OUT:
        assert got[n].shape == want[n].shape and got[n].dtype == want[n].dtype, f"{what}: {n} {got[n].shape} {got[n].dtype} vs {want[n].shape} {want[n].dtype}"
        np.testing.assert_array_equal(got[n], want[n], err_msg=f"{what}: {n}")


@pytest.mark.gpu
@pytest.mark.parametrize("name,mode", RUNS, ids=RUN_IDS)
def test_consumers_on_every_rank(name, mode):
    """every output of every consumer call on every rank's batch against the reference of that rank's reads, and against the plain single
    context's rows of those reads; the rank with the empty range makes every call succeed with zero rows.  The accumulating calls of
    the chain -- sqg_batch_pileup_rows over the rows the collapse steps take, under every cfg of pile_cfgs, and the frequency table
    "call observed" adds to (a sampled rank under the NULL origin: the keys from its own range of the sampler's records) -- go into
    objects of the rank's own: their sums over the ranks, the single context's and the references' over the whole job are the same
    bytes, and so are the statistics"""
    su = SC.Setup(name)
    job = su.oracle_job()
    cfgs = su.pile_cfgs()
    new = lambda gen, c: gen.new_pileup(norm=cfgs[c][1], trim=cfgs[c][2], **cfgs[c][0])      # noqa: E731
    window = su.window()

    def consume(b, bi, idx, piles, stats, freq, want=None):
        """every group of the batch; the rows' pileups into piles / stats (c -> the Pileup, the four statistics), the calls into freq"""
        kept, o = {}, job[bi]
        origin = su.origin(o, idx)

        def pile_rows(c):
            def step(out):
                st = b.pileup_rows(piles[c], *kept["rows"], origin=origin if cfgs[c][0]["by"] == "ref" else None)
                stats[c] = [a + v for a, v in zip(stats[c], st)]
            return "align scaled", step
        return su.consume(b, extra=[pile_rows(c) for c in cfgs], origin=origin, freq=freq, want=want, kept=kept)

    got, piles, stats, freqs = {}, {}, {}, {}
    for bi, g, b, idx in SC.DRIVERS[su.job["kind"]](su, mode):
        reads = [job[bi]["reads"][i] for i in idx]
        assert b.n_reads == len(idx)
        if g not in piles:
            piles[g], stats[g], freqs[g] = {c: new(b.gen, c) for c in cfgs}, {c: [0, 0, 0, 0] for c in cfgs}, b.gen.new_call_freq(*window) if su.calls else None
        want = su.expected(reads, origin=(job[bi]["key0"][idx], job[bi]["step"][idx]))
        out = consume(b, bi, idx, piles[g], stats[g], freqs[g], want)
        SC.assert_groups(out, want, f"{name} batch {bi} rank {g}")
        if len(idx) == 0:
            assert (bi, g) in su.job.get("empty", ())
            for gname, grp in out.items():
                assert len(grp["read"]) == 0 and list(grp["off"]) == [0], gname
            assert list(out["sites 256"]["plan"]) == [0]
            _empty_detect_and_align(b)
            for cname, call in _raw_calls(su, b).items():   # (Batch.chunks and .chunk_targets do not call the library for a plan without chunks)
                assert call() == 0, f"{cname} on the empty range: {b.gen.L.sqg_last_error(b.gen.ctx)}"
            lo, hi = su.window()
            for kw in (dict(by="kmer"), dict(by="ref", lo=lo, hi=lo + 4096)):
                p = b.gen.new_pileup(**kw)
                for n in OUT:
                    getattr(p, n).fill_(7)
                assert b.pileup(p) == (0, 0)
                assert all((a == 7).all() for a in SC.pile_arrays(p).values()), "an empty range touched the pileup"
        got[(bi, g)] = out
    assert len(got) == su.G * len(job)
    one = None
    for bi, b in SC.single(su, mode):
        one = one or ({c: new(b.gen, c) for c in cfgs}, {c: [0, 0, 0, 0] for c in cfgs}, b.gen.new_call_freq(*window) if su.calls else None)
        whole = consume(b, bi, np.arange(b.n_reads), *one)
        for g in range(su.G):
            SC.assert_groups(got[(bi, g)], SC.restrict(whole, su.rank_reads(b.n_reads, g)), f"{name} batch {bi} rank {g} against the single context")
    for c, (kw, norm, trim) in cfgs.items():
        want, st = su.expected_pileup_rows(kw, norm, trim)
        print(f"{name} {c}: rows piled up: (counted, outside, unseen, dropped) {st}, most reads on one key {int(want['n'].max())}")
        assert st[0] > 0 and st[2] > 0 and int(want["n"].max()) >= 2
        _assert_pile(_pile_sum([SC.pile_arrays(piles[g][c]) for g in range(su.G)]), want, f"{name} {c}: the sum of the ranks' pileups of rows")
        _assert_pile(SC.pile_arrays(one[0][c]), want, f"{name} {c}: the single context's pileup of rows")
        assert tuple(sum(stats[g][c][i] for g in range(su.G)) for i in range(4)) == tuple(one[1][c]) == st, f"{name} {c}: the statistics of the rows piled up"
    if su.calls:
        want = su.expected_call_freq()
        ranks = [SC.freq_arrays(freqs[g]) for g in range(su.G)]
        print(f"{name}: call frequency: {int(want['cov'].sum())} sites on {int((want['cov'] > 0).sum())} keys, most on one key {int(want['cov'].max())}, {int(want['called'].sum())} called, "
              f"{int(want['meth'].sum())} as methylated; per rank {[int(r['cov'].sum()) for r in ranks]}")
        assert int(want["cov"].max()) >= 2 and min(int(r["cov"].sum()) for r in ranks) > 0
        for n in api.CALL_FREQ:
            np.testing.assert_array_equal(sum(r[n] for r in ranks), want[n], err_msg=f"{name}: the sum of the ranks' call frequencies: {n}")
            np.testing.assert_array_equal(SC.freq_arrays(one[2])[n], want[n], err_msg=f"{name}: the single context's call frequency: {n}")


@pytest.mark.gpu
@pytest.mark.parametrize("name,mode", RUNS, ids=RUN_IDS)
def test_the_pileups_of_the_ranks_add_up(name, mode):
    """every rank adds its batches into a pileup of its own, and all ranks into one shared pileup one after the other: the shared sums,
    the element-wise sum of the ranks', pileup_ref over the whole job and the plain single context's pileup are the same bytes, and the
    ranks' (counted, outside) add up to the single context's"""
    su = SC.Setup(name)
    job = su.oracle_job()
    cfgs = su.pile_cfgs()
    assert cfgs
    new = lambda gen, c: gen.new_pileup(norm=cfgs[c][1], trim=cfgs[c][2], **cfgs[c][0])      # noqa: E731
    shared, own, stats = {}, {}, {c: [0, 0] for c in cfgs}
    for bi, g, b, idx in SC.DRIVERS[su.job["kind"]](su, mode):
        for c in cfgs:
            if c not in shared:
                shared[c] = new(b.gen, c)
            if (c, g) not in own:
                own[(c, g)] = new(b.gen, c)
            origin = su.origin(job[bi], idx) if cfgs[c][0]["by"] == "ref" else None
            st = b.pileup(own[(c, g)], origin=origin)
            assert b.pileup(shared[c], origin=origin) == st
            stats[c][0] += st[0]; stats[c][1] += st[1]
    one = {}
    for bi, b in SC.single(su, mode):
        for c in cfgs:
            if c not in one:
                one[c] = [new(b.gen, c), 0, 0]
            st = b.pileup(one[c][0], origin=su.origin(job[bi], np.arange(b.n_reads)) if cfgs[c][0]["by"] == "ref" else None)
            one[c][1] += st[0]; one[c][2] += st[1]
    for c, (kw, norm, trim) in cfgs.items():
        want, counted, outside = su.expected_pileup(kw, norm, trim)
        print(f"{name} {c}: counted {counted}, outside {outside}, most reads on one key {int(want['n'].max())}")
        assert counted > 0 and (outside > 0 or c != "ref_window") and int(want["n"].max()) >= 2
        for q in range(want["n"].shape[0]):                 # (an RNA read is never sampled from the '-' strand: that plane stays empty)
            assert want["n"][q].any() != (su.rna and q == 1), f"{c}: plane {q}"
        _assert_pile(SC.pile_arrays(shared[c]), want, f"{name} {c}: the shared pileup against pileup_ref")
        _assert_pile(_pile_sum([SC.pile_arrays(own[(c, g)]) for g in range(su.G)]), want, f"{name} {c}: the sum of the ranks' pileups")
        _assert_pile(SC.pile_arrays(one[c][0]), want, f"{name} {c}: the single context")
        assert tuple(stats[c]) == (one[c][1], one[c][2]) == (counted, outside)


def _empty_detect_and_align(b):
    """a rank without reads: no rows, det_off is [0], and outputs handed in prefilled with guard values come back as they were"""
    dt = b.detect("dna", "medmad", True)
    al = b.align(np.zeros(1, np.int64), dt.sum, dt.dt_len)
    assert dt.n_rows == al.n_rows == 0 and dt.det_off.tolist() == [0] and b.detect_plan()[1] == 0
    assert all(tuple(getattr(dt, key).shape) == (0,) for key in api.DETECT_OUTPUTS) and all(tuple(getattr(al, key).shape) == (0,) for key in api.ALIGN_OUTPUTS)
    dev = torch.device("cuda", b.gen.device)
    guard = {key: torch.full((8,), -77, dtype=t, device=dev) for key, t in (("i64", torch.int64), ("i32", torch.int32), ("i16", torch.int16), ("f32", torch.float32))}
    torch.cuda.synchronize(dev)
    dtypes = dict(dt_read="i32", dt_start="i64", dt_len="i32", sum="i64", sumsq="i64", vmin="i16", vmax="i16", mean="f32", sd="f32", true_ev="i64", med2="i32", mad4="i32")
    dout = api.CDetectOut(*(guard[dtypes[key]].data_ptr() for key in api.DETECT_OUTPUTS))
    aout = api.CAlignOut(guard["i64"].data_ptr(), guard["i64"].data_ptr(), guard["i32"].data_ptr())
    gen, Lb = b.gen, b.gen.L
    assert Lb.sqg_batch_detect(gen.ctx, b.handle, C.byref(api.CDetectCfg(3, 6, 1.4, 9.0, 0.2, api.CHUNK_MEDMAD, 1)), C.byref(dout)) == 0
    off = np.zeros(1, np.int64)
    ain = api.CAlignIn(guard["i64"].data_ptr(), guard["i32"].data_ptr())
    assert Lb.sqg_batch_align(gen.ctx, b.handle, C.byref(api.CAlignCfg(*SC.ALIGN_TRUTH)), off.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(ain), C.byref(aout)) == 0
    torch.cuda.synchronize(dev)
    assert all(bool((g == -77).all()) for g in guard.values()), "an empty range wrote to an output of detect or align"


def _raw_calls(su, b):
    """the C call's name -> the call itself on batch b, nothing wanted: what refuses must refuse before it looks at the outputs"""
    gen, Lb = b.gen, b.gen.L
    L, St, W = SC.CHUNK
    cc = api.CChunkCfg(L, St, W, api.CHUNK_F16, api.CHUNK_MEDMAD)
    sc = api.CSiteCfg(256, 128, su.focus, 0, 0, api.CHUNK_F16, api.CHUNK_MEDMAD)
    ec = api.CEventCfg(api.CHUNK_MEDMAD, 1)
    pc = api.CPileupCfg(api.PILEUP_BY_KMER, 0, api.CHUNK_PA, 0, 0, 0, len(su.mean))
    dc = api.CDetectCfg(3, 6, 1.4, 9.0, 0.2, api.CHUNK_MEDMAD, 1)
    ac = api.CAlignCfg(*SC.ALIGN_TRUTH)
    row_off = np.zeros(b.n_reads + 1, np.int64)             # a valid plan without rows, and inputs that are not NULL: both are checked first
    one = torch.zeros(1, dtype=torch.int64, device=torch.device("cuda", gen.device))
    ain = api.CAlignIn(one.data_ptr(), one.data_ptr())
    n64 = C.c_int64()
    return {
        "sqg_detect_plan": lambda: Lb.sqg_detect_plan(gen.ctx, b.handle, C.byref(dc), None, C.byref(n64)),
        "sqg_batch_detect": lambda: Lb.sqg_batch_detect(gen.ctx, b.handle, C.byref(dc), C.byref(api.CDetectOut())),
        "sqg_batch_align": lambda keep=one: Lb.sqg_batch_align(gen.ctx, b.handle, C.byref(ac), row_off.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(ain),
                                                               C.byref(api.CAlignOut())),
        "sqg_chunk_plan": lambda: Lb.sqg_chunk_plan(gen.ctx, b.handle, C.byref(cc), None, C.byref(n64)),
        "sqg_batch_chunks": lambda: Lb.sqg_batch_chunks(gen.ctx, b.handle, C.byref(cc), C.byref(api.CChunkOut())),
        "sqg_batch_chunk_targets": lambda: Lb.sqg_batch_chunk_targets(gen.ctx, b.handle, C.byref(cc), C.byref(api.CChunkTargets())),
        "sqg_batch_segments": lambda: Lb.sqg_batch_segments(gen.ctx, b.handle, C.byref(api.CSegments(None, None))),
        "sqg_chunk_plan_trimmed": lambda: Lb.sqg_chunk_plan_trimmed(gen.ctx, b.handle, C.byref(cc), None, C.byref(n64)),
        "sqg_batch_chunks_trimmed": lambda: Lb.sqg_batch_chunks_trimmed(gen.ctx, b.handle, C.byref(cc), C.byref(api.CChunkOut())),
        "sqg_batch_chunk_targets_trimmed": lambda: Lb.sqg_batch_chunk_targets_trimmed(gen.ctx, b.handle, C.byref(cc), C.byref(api.CChunkTargets())),
        "sqg_site_plan": lambda: Lb.sqg_site_plan(gen.ctx, b.handle, C.byref(sc), None, C.byref(n64)),
        "sqg_batch_sites": lambda: Lb.sqg_batch_sites(gen.ctx, b.handle, C.byref(sc), C.byref(api.CSiteOut())),
        "sqg_batch_events": lambda: Lb.sqg_batch_events(gen.ctx, b.handle, C.byref(ec), C.byref(api.CEventOut())),
        "sqg_batch_pileup": lambda: Lb.sqg_batch_pileup(gen.ctx, b.handle, C.byref(pc), None, C.byref(api.CPileupOut()), None),
    }


def _trimmed_and_pileup(su, b, reads, what):
    """what consume() leaves out on a context without a prefix: the segments and the trimmed calls (the whole read is the insert), and a
    pileup by pore-table row"""
    p = su.prof
    L, St, W = SC.CHUNK
    seg, shift = b.segments()
    wseg, wshift = SR.batch_segments(reads, su.k, su.rna, su.prefix, su.sps)
    np.testing.assert_array_equal(seg.cpu().numpy(), wseg, err_msg=f"{what}: seg")
    np.testing.assert_array_equal(shift.cpu().numpy(), wshift, err_msg=f"{what}: shift")
    want = SR.batch_chunks_trimmed(reads, su.k, su.rna, su.meth, su.prefix, su.sps, L, St, W, "f16", "medmad", p.range, p.digitisation)
    ch = b.chunks(L, St, W, trim=True)
    plan, nc = b.chunk_plan(L, St, trim=True)
    np.testing.assert_array_equal(plan, want["chunk_off"], err_msg=f"{what}: the trimmed plan")
    assert nc == ch.n_chunks == want["chunk_off"][-1] > 0
    for key in ("signal", "labels", "label_len", "chunk_read", "chunk_start", "med2", "mad4"):
        np.testing.assert_array_equal(R.bits(getattr(ch, key).cpu().numpy()), R.bits(want[key]), err_msg=f"{what}: trimmed chunks: {key}")
    want = SR.batch_targets_trimmed(reads, su.mean, su.k, su.rna, su.meth, su.prefix, su.sps, L, St, "f16", "medmad", p.range, p.digitisation)
    tg = b.chunk_targets(L, St, clean=True, clean_raw=True, moves=True, kmer=True, trim=True)
    for key in ("clean", "clean_raw", "moves", "kmer"):
        a = tg.__dict__[key].cpu().numpy()
        np.testing.assert_array_equal(R.bits(a.view(np.uint32) if key == "kmer" else a), R.bits(want[key]), err_msg=f"{what}: trimmed targets: {key}")
    pile = b.gen.new_pileup(by="kmer", norm="medmad", trim=True)
    ev = su.pileup_table(reads, "medmad", True, True)
    n = len(reads)
    wp, counted, outside = PR.pileup(ev, ev["ev_off"], np.zeros(n, np.int64), np.ones(n, np.int8), [len(r["seq"]) for r in reads], su.k, su.rna, su.prefix,
                                     PR.BY_KMER, 0, 0, 0, len(su.mean))
    assert b.pileup(pile) == (counted, outside) and counted > 0
    _assert_pile(SC.pile_arrays(pile), wp, f"{what}: pileup by row")


@pytest.mark.gpu
def test_lifetime_of_a_batch_in_range_mode():
    """Range mode hands the slot of batch r to batch r + 2 at sqg_batch_run_begin, not at the end of a run: from then on every consumer call
    refuses batch r with SQG_ESEQUENCE and names itself (sqg_chunk_plan alone, host arithmetic over the batch's own sig_off, keeps
    answering, as its header says), batch r + 1 is still served bit for bit, and the batch that is begun but not ended is refused, not
    waited for.  A site plan or insert-span plan in the context's scratch is not served to a batch staged where a freed one was"""
    su = SC.Setup("lifetime_g1")
    rk = SC.RangeRanks(su)
    try:
        _lifetime(su, rk, su.staged_reads(), su.oracle_job())
    finally:
        rk.close()


def _lifetime(su, rk, bts, job):
    run = lambda b: rk.end([b], rk.begin([b]))               # noqa: E731
    reads = [o["reads"] for o in job]
    expected = lambda bi: su.expected(reads[bi], origin=(job[bi]["key0"], job[bi]["step"]))      # noqa: E731
    # (the call groups among them: the caller's origin, a frequency table of the batch's own, stat against the reference)
    consume = lambda b, bi, want: su.consume(b, origin=su.origin(job[bi], np.arange(b.n_reads)), freq=b.gen.new_call_freq(*su.window()), want=want)      # noqa: E731
    b0, b1, b2 = (rk.stage(bt)[0] for bt in bts[:3])
    for name, call in _raw_calls(su, b0).items():           # staged, not run
        assert call() == -4 and name.encode() in b0.gen.L.sqg_last_error(b0.gen.ctx), name
    run(b0); run(b1)
    want0 = expected(0)
    SC.assert_groups(consume(b0, 0, want0), want0, "batch 0")      # (leaves plans of batch 0 in the scratch)
    _trimmed_and_pileup(su, b0, reads[0], "batch 0")
    plan0 = b0.chunk_plan(*SC.CHUNK[:2])
    counts = rk.begin([b2])                                 # batch 2 takes the slot of batch 0
    err = lambda: b0.gen.L.sqg_last_error(b0.gen.ctx)        # noqa: E731
    for name, call in _raw_calls(su, b0).items():
        if name == "sqg_chunk_plan":
            assert call() == 0
            continue
        assert call() == -4 and name.encode() in err() and b"handed to a later batch" in err(), f"{name}: {err()}"
    none = torch.zeros(1, dtype=torch.int64, device=torch.device("cuda", b0.gen.device))
    for call in (lambda: b0.sites(256, 128, su.focus), lambda: b0.events(), lambda: b0.chunks(*SC.CHUNK), lambda: b0.pileup(b0.gen.new_pileup(by="kmer")),
                 lambda: b0.detect(), lambda: b0.align(np.zeros(b0.n_reads + 1, np.int64), none, none.to(torch.int32))):
        with pytest.raises(api.SqgError) as e:
            call()
        assert e.value.code == -4
    np.testing.assert_array_equal(b0.chunk_plan(*SC.CHUNK[:2])[0], plan0[0])
    for name, call in _raw_calls(su, b2).items():           # begun, not ended: refused at once
        assert call() == -4 and name.encode() in err() and b"not been run" in err(), f"{name}: {err()}"
    want1 = expected(1)
    SC.assert_groups(consume(b1, 1, want1), want1, "batch 1 while batch 2 is begun")
    _trimmed_and_pileup(su, b1, reads[1], "batch 1 while batch 2 is begun")
    rk.end([b2], counts)
    want2 = expected(2)
    SC.assert_groups(consume(b2, 2, want2), want2, "batch 2")
    _trimmed_and_pileup(su, b2, reads[2], "batch 2")        # (the trimmed pileup comes last: the scratch holds batch 2's insert spans ...
    plan2 = b2.site_plan(256, 128, su.focus)[0]             # ... and its site plan at the geometry batch 3 is asked for first)
    b0.free()
    old = b2.handle.value
    b2.free()
    b3 = rk.stage(bts[3])[0]                                # straight away: the allocator may hand out batch 2's block again
    if b3.handle.value != old:                              # (the cache is keyed by handle and run index: only a reused handle can find it)
        warnings.warn("the batch staged after the free did not get the freed handle: the stale-plan check below checked nothing in this run")
    assert b3.n_reads == len(bts[3]) == len(bts[2])         # (as many reads: a plan of the freed batch would fit)
    run(b3)
    L, St, _ = SC.CHUNK
    want3 = expected(3)
    np.testing.assert_array_equal(b3.site_plan(256, 128, su.focus)[0], want3["sites 256"]["off"])
    np.testing.assert_array_equal(b3.chunk_plan(L, St, trim=True)[0], want3["chunks f16 medmad"]["off"])
    assert not np.array_equal(want3["sites 256"]["off"], plan2)                                       # (batch 2's plan would show)
    SC.assert_groups(consume(b3, 3, want3), want3, "batch 3")
    _trimmed_and_pileup(su, b3, reads[3], "batch 3")
    for b in (b1, b3):
        b.free()


def _threaded(extra_flags=0):
    name = "workers_t4_g2"
    su = SC.Setup(name, extra_flags)
    origin = SC.Setup(name).oracle_job()                    # (the caller's origin of the job; the oracle's reads are not used here)
    batches = su.staged_reads()
    kw, norm, trim = su.pile_cfgs()["ref_split"]
    quiet, p1 = [], None
    for bi, b in SC.single(su):
        quiet.append(su.consume(b, threaded=True))
        p1 = p1 or b.gen.new_pileup(norm=norm, trim=trim, **kw)
        b.pileup(p1, origin=(origin[bi]["key0"], origin[bi]["step"]))
    got = [[None] * len(batches) for _ in range(su.G)]
    piles, errors = [None] * su.G, []
    gate = threading.Barrier(su.G)                          # every context created and its batches staged before any of them runs

    def rank_thread(g):
        try:
            gen = su.generator(api.MODE_CERTIFIED, *shard.worker_range(g, su.G, su.T))
            staged = [SC.worker_batch(su, gen, g, len(bt), bt) for bt in batches]
            p = gen.new_pileup(norm=norm, trim=trim, **kw)
            gate.wait(timeout=60)
            for b, _ in staged[:2]:
                b.run()
            for bi, (b, idx) in enumerate(staged):          # batch bi + 1 is in flight and batch bi + 2 staged while batch bi is consumed
                b.wait()
                got[g][bi] = su.consume(b, threaded=True)
                b.pileup(p, origin=(origin[bi]["key0"][idx], origin[bi]["step"][idx]))
                b.free()
                if bi + 2 < len(staged):
                    staged[bi + 2][0].run()
            piles[g] = SC.pile_arrays(p)
            gen.close()
        except Exception as e:  # noqa: BLE001
            gate.abort()
            errors.append((g, repr(e)))

    th = [threading.Thread(target=rank_thread, args=(g,), daemon=True) for g in range(su.G)]
    for t in th:
        t.start()
    deadline = time.monotonic() + 120                       # (the whole step takes seconds)
    for t in th:
        t.join(timeout=max(deadline - time.monotonic(), 0))
    assert not any(t.is_alive() for t in th), "a rank's thread is still running"
    assert not errors, errors
    for g in range(su.G):
        for bi, bt in enumerate(batches):
            SC.assert_groups(got[g][bi], SC.restrict(quiet[bi], su.rank_reads(len(bt), g)), f"{name} batch {bi} rank {g} on a thread")
    _assert_pile(_pile_sum(piles), SC.pile_arrays(p1), f"{name}: the threads' pileups")
    assert SC.pile_arrays(p1)["n"].max() >= 2


@pytest.mark.gpu
def test_consumers_beside_another_contexts_kernels():
    """one host thread per worker-sharded context: events, chunks with labels, sites and a pileup of its own from batch i while batch i + 1
    is in flight, batch i + 2 staged and the other context's kernels share the CUs -- equal to the quiet single context's"""
    _threaded()


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["order-free", "per-link-rows"])
def test_consumers_beside_another_contexts_kernels_on_the_fallback_paths(variant, monkeypatch):
    if variant == "per-link-rows":
        monkeypatch.setenv("SQG_NO_PART", "1")
    _threaded(profiles.SQ_ORDER_FREE if variant == "order-free" else 0)
