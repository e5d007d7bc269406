"""Randomised parity for the consumer calls: sqg_batch_chunks / _trimmed, sqg_batch_chunk_targets / _trimmed, sqg_batch_segments,
sqg_batch_sites, sqg_batch_events, sqg_batch_pileup, sqg_batch_detect, sqg_batch_align, sqg_batch_scale, sqg_batch_align_scaled,
sqg_batch_collapse, sqg_batch_pileup_rows and sqg_call_plan / sqg_batch_call, all of them on every drawn context of
tests/consumer_cases.py -- flag set, k in 5 ... 9, dwell, model, ragged batches and the cfg of every call drawn together, so that the
cross products run on the device that the typed-out cases of the calls' own test files keep apart.  The references are the numpy
statements of the headers over the oracle's reads, as tests/shard_cases.py's Setup groups them; every comparison is bit for bit (floats as
integers), plan calls included."""
import numpy as np
import pytest
import torch  # noqa: F401  (before the library is loaded: the HIP runtime torch brings is the one the library then uses)

import call_ref as CL
import consumer_cases as CC
import events_ref as EV
import scale_ref as SCL
import shard_cases as SC
from squigulator_amd import api

SEEDS = range(100)


# ---------------------------------------------------------------------------------------------------------- no GPU
def test_the_drawn_cases_hold_what_can_go_wrong():
    """from the oracle and the numpy references alone, over the whole table: every family of calls meets every k, every flag set two k or
    more, every dwell mean is there and a constant dwell without an ideal flag; the five batch shapes; chunk strides below, at and above
    the chunk length, a read without a chunk beside reads with some, labels cut by the row width, no labels; sites with label 1, dropped
    at the front and at the back, a batch with candidates and no site, ctx_start clamped at either end; both detectors recording (the
    long one, and the short one masking it), a read shorter than two short windows; a path on the band's rim, reads with more rows than
    events and with fewer; pileup keys outside the window, all three steps, and a key that reads of two batches add to.  The size
    conditions of every case are asserted by consumer_cases.facts"""
    table = [CC.facts(CC.draw(seed)) for seed in SEEDS]
    for t in table:
        print({key: (sorted(v) if isinstance(v, set) else v) for key, v in t.items()})
    ks = set(range(5, 10))
    families = {name: {t["k"] for t in table if on(t)} for name, on in (("every context", lambda t: True), ("trimmed", lambda t: t["prefix"]), ("sites", lambda t: t["sites"]))}
    assert all(v == ks for v in families.values()), families
    for f in range(len(CC.FLAG_SETS)):
        assert len({t["k"] for t in table if t["flag_set"] == f}) >= 2, f"flag set {f}"
    assert {t["dwell"][0] for t in table} == set(CC.DWELL_MEANS)
    assert any(t["dwell"][1] == 0 and not t["flags"] & CC.IDEAL_FLAGS for t in table)
    assert set().union(*[t["shapes"] for t in table]) == set(CC.SHAPES)
    assert all(t["shape"] in t["shapes"] for t in table)                    # (the shape a seed plants is the shape its batches have)
    assert {t["stride"] for t in table} == {-1, 0, 1}
    assert any(t["no_chunk_beside"] for t in table) and any(t["label_over"] for t in table) and any(t["W"] == 0 for t in table)
    some = lambda key: [t["seed"] for t in table if t[key]]                  # noqa: E731
    for key in ("label1", "front", "back", "barren", "ctx_low", "ctx_high", "brief", "edge", "more_rows", "more_events", "outside", "shared"):
        assert some(key), key
        print(f"{key}: seeds {some(key)}")
    assert some("long") and set(some("masks")) - {some("long")[0]}, "the long detector records in one case, the short one masks it in another"
    assert any(t["steps"] == {-1, 0, 1} for t in table)
    # the scale, collapse and call groups (consumer_cases.chain_facts).  collapse: a read with an event no row is assigned to and an event
    # that two rows or more are summed into, a read with a dropped row; scale fit: a gain other than 65536, a shift other than 0, a read
    # with fewer than two assigned rows (no fit: the fallback); call observed: a site with some of its span's events observed and one
    # with none, all three call values and both labels, sites outside the table, calls that agree with the label and calls that do
    # not, a key that sites of two batches add to, sites in reads of every step; call true: a k-mer that holds two candidates (NEIGH_SAME
    # and NEIGH_READ then differ), a site at p = 0 and one at p = len - 2
    for key in ("unseen_beside_summed", "rd_dropped", "fit_gain", "fit_shift", "fit_fallback", "part_obs", "no_obs", "call_outside", "site_shared", "two_in_kmer",
                "site_first", "site_last"):
        assert some(key), key
        print(f"{key}: seeds {some(key)}")
    called = [t for t in table if t["labels"]]
    assert {t["k"] for t in called} == ks and all(t["flag_set"] in (8, 9) for t in called)
    assert any(t["calls"] == {0, 1, 2} for t in called) and any(t["labels"] == {0, 1} for t in called)
    assert any(t["called"] > t["agree"] > 0 for t in called) and any(t["site_steps"] == {-1, 0, 1} for t in called)
    assert {t["collapse_shift"] for t in table} == set(CC.COLLAPSE_SHIFTS)
    assert any(t["collapse_shift"] == 0 and t["calls"] == {0, 1, 2} and t["part_obs"] and t["no_obs"] for t in called)   # (on the aligner's own answer)


@pytest.mark.parametrize("seed", SEEDS)
def test_the_two_statements_of_each_reference_agree(seed):
    """detect_ref.batch_rows against detect_vec and align_ref.banded against the oracle's compiled recurrence (align_ref.full too for the
    reads of at most 32 events), on every batch of the case and under the case's own cfgs, bit for bit: the groups as the GPU test takes
    them against the plain ones, as expected_detect_align(plain=True) gives them.  And on the case's own chained rows (Setup.job_chain):
    scale_ref.by_read against scale_ref.vectorised in both modes, on every batch; call_ref.by_site against call_ref.vectorised for
    "call true" and "call observed", on the case's first batch that has a site (the walk by site takes seconds on the larger ones)"""
    su = CC.draw(seed)
    p = su.prof
    walked = False
    for bi, (o, (groups, inner, _)) in enumerate(zip(su.oracle_job(), su.job_chain())):
        ev = EV.batch_events(o["reads"], su.mean, su.k, su.rna, su.meth, su.prefix, su.sps, "pa", False, p.range, p.digitisation)
        fast, plain = {}, {}
        SC.assert_groups(su.expected_detect_align(o["reads"], ev, seen=fast), su.expected_detect_align(o["reads"], ev, seen=plain, plain=True), f"seed {seed} batch {bi}")
        assert fast == plain
        d = inner["det"]
        rows = (d["off"], d["rows"]["sum"], d["rows"]["dt_len"], ev["ev_off"], ev["level_raw"])
        for name, mode, kw in (("scale moments", SCL.MOMENTS, {}), ("scale fit", SCL.FIT, dict(ev=groups["align scaled"]["rows"]["al_ev"]))):
            plain = SCL.by_read(*rows, mode, **kw)
            for key in SCL.OUTPUTS:
                v = groups[name]["per_read"][key]
                assert v.dtype == plain[key].dtype, (name, key)
                np.testing.assert_array_equal(v, plain[key], err_msg=f"seed {seed} batch {bi}: {name}: the two statements differ in {key}")
        if su.calls and not walked and len(groups["call true"]["read"]):
            walked = True
            for name in ("call true", "call observed"):
                a, kw = inner[f"{name} args"]
                u = CL.both(*a, what=f"seed {seed} batch {bi}: {name}", **kw)
                np.testing.assert_array_equal(u["llr"], groups[name]["rows"]["llr"])
    assert walked or not su.calls or not any(len(g["call true"]["read"]) for g, _, _ in su.job_chain())


# ---------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_drawn_context_through_every_consumer_call(seed):
    """one plain context that owns every worker (MODE_CERTIFIED on even seeds, MODE_EXACT on odd).  Every batch's signal and dwells against
    the oracle's, then every group of Setup.consume against Setup.expected, the calls -- the pileups among them -- in an order shuffled
    from the seed; seeds that are a multiple of 3 consume batch i while batch i + 1 runs and batch i + 2 is staged.  The pileups --
    those of sqg_batch_pileup and, under the same cfgs, of sqg_batch_pileup_rows over the rows the collapse steps take -- and the call
    frequency table that "call observed" adds to are compared after the last batch"""
    su = CC.draw(seed)
    what = CC.describe(su)
    job = su.oracle_job()
    batches = su.staged_reads()
    cfgs = su.pile_cfgs()
    rng = np.random.default_rng(9000 + seed)
    gen = su.generator(api.MODE_EXACT if seed % 2 else api.MODE_CERTIFIED)
    piles = {c: gen.new_pileup(norm=norm, trim=trim, **kw) for c, (kw, norm, trim) in cfgs.items()}
    stats = {c: [0, 0] for c in cfgs}
    row_piles = {c: gen.new_pileup(norm=norm, trim=trim, **kw) for c, (kw, norm, trim) in cfgs.items()}      # the same cfgs under sqg_batch_pileup_rows
    row_stats = {c: [0, 0, 0, 0] for c in cfgs}
    freq = gen.new_call_freq(*su.window()) if su.calls else None

    def check(b, bi):
        o = job[bi]
        reads = o["reads"]
        assert b.n_reads == len(reads)
        np.testing.assert_array_equal(b.signal(), np.concatenate([r["sig"] for r in reads] + [np.zeros(0, np.int16)]), err_msg=f"{what}: batch {bi}: the signal")
        np.testing.assert_array_equal(b.dwell(), np.concatenate([np.asarray(r["ss"], np.int32) for r in reads] + [np.zeros(0, np.int32)]), err_msg=f"{what}: batch {bi}: the dwells")
        assert all(b.offset[i] == r["offset"] for i, r in enumerate(reads))

        def pile(c):
            def step(out):
                st = b.pileup(piles[c], origin=su.origin(o, np.arange(len(reads))))       # (by="kmer" too: a read whose step is 0 is not counted)
                stats[c][0] += st[0]; stats[c][1] += st[1]
            return step
        kept = {}

        def pile_rows(c):                                   # the rows the collapse steps take, behind the step that leaves them in `kept`
            def step(out):
                st = b.pileup_rows(row_piles[c], *kept["rows"], origin=origin)
                row_stats[c] = [a + v for a, v in zip(row_stats[c], st)]
            return "align scaled", step
        origin = su.origin(o, np.arange(len(reads)))
        extra = [pile(c) for c in cfgs] + [pile_rows(c) for c in cfgs]
        order = rng.permutation(len(su.consume_steps(b)) + len(extra))
        want = su.expected(reads, origin=(o["key0"], o["step"]))
        SC.assert_groups(su.consume(b, order=order, extra=extra, origin=origin, freq=freq, want=want, kept=kept), want, f"{what}: batch {bi}, calls in the order {order.tolist()}")

    stage = lambda bt: gen.stage(bt, su.workers_of(len(bt)))    # noqa: E731
    try:
        if seed % 3:
            for bi, bt in enumerate(batches):
                b = stage(bt).run().wait()
                check(b, bi)
                b.free()
        else:                                               # streamed: batch i + 2 staged, batch i + 1 queued, batch i consumed
            cur = stage(batches[0]).run()
            nxt = stage(batches[1])
            for bi in range(len(batches)):
                nn = stage(batches[bi + 2]) if bi + 2 < len(batches) else None
                if nxt is not None:
                    nxt.run()
                cur.wait()
                check(cur, bi)
                cur.free()
                cur, nxt = nxt, nn
        for c, (kw, norm, trim) in cfgs.items():
            want, counted, outside = su.expected_pileup(kw, norm, trim)
            got = SC.pile_arrays(piles[c])
            for n in api.PILEUP_OUTPUTS:
                assert got[n].shape == want[n].shape and got[n].dtype == want[n].dtype, f"{what}: pileup {c}: {n} {got[n].shape} {got[n].dtype}"
                np.testing.assert_array_equal(got[n], want[n], err_msg=f"{what}: pileup {c}: {n}")
            assert tuple(stats[c]) == (counted, outside), f"{what}: pileup {c}: (counted, outside)"
            want, st = su.expected_pileup_rows(kw, norm, trim)
            got = SC.pile_arrays(row_piles[c])
            for n in api.PILEUP_OUTPUTS:
                assert got[n].shape == want[n].shape and got[n].dtype == want[n].dtype, f"{what}: pileup_rows {c}: {n} {got[n].shape} {got[n].dtype}"
                np.testing.assert_array_equal(got[n], want[n], err_msg=f"{what}: pileup_rows {c}: {n}")
            assert tuple(row_stats[c]) == st, f"{what}: pileup_rows {c}: (counted, outside, unseen, dropped) {row_stats[c]}, expected {st}"
        if su.calls:
            want, got = su.expected_call_freq(), SC.freq_arrays(freq)
            for n in api.CALL_FREQ:
                assert got[n].shape == want[n].shape, f"{what}: call frequency: {n} {got[n].shape}"
                np.testing.assert_array_equal(got[n], want[n], err_msg=f"{what}: call frequency: {n}")
    finally:
        gen.close()
