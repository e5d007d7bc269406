"""The calls that read a finished batch on the device share scratch of the context (the reads' constants, the inserts' spans, the chunk
and site plans, the event columns, the detector's plan, the aligner's levels, the caller's row offsets, the methylation caller's plan and
skip marks, the per-read origin table of pileups and calls): what a call writes must not depend on which other calls
ran before it on that context.  Every call alone on a fresh context is the reference; the same calls in the listed order, in reverse,
and across two consecutive batches -- those for batch 0 made after batch 1 has run, while batch 0 still owns its device results --
must give the same tensors, bit for bit."""
import ctypes

import numpy as np
import pytest
import torch  # noqa: F401  (before the library is loaded: the HIP runtime torch brings is the one the library then uses)

from chunk_support import _context, _fixture_reads
from refvec_cases import REFVEC_CASES
from shard_cases import stored_order
from squigulator_amd import api

L, S, W = 64, 8, 16


def _keyed(who, origin):
    """what a result says of the origin its call took: who ("pileup" or "call") wrote the context's per-read origin table, and from what"""
    return {} if origin is None else dict(origin_of=who, origin_key0=np.asarray(origin[0]), origin_step=np.asarray(origin[1]))


def _pileup(b, origin=None, **kw):
    p = b.gen.new_pileup(**kw)
    counted, outside = b.pileup(p, origin=origin)
    return api.Chunks(counted=counted, outside=outside, **{n: getattr(p, n) for n in api.PILEUP_OUTPUTS}, **_keyed("pileup", origin))


def _segments(b):
    seg, shift = b.segments()
    return api.Chunks(seg=seg, shift=shift)


def _align_detected(b):
    """the detected rows of the DNA preset, the tensors handed on as they are, aligned under SQG_ALIGN_DEFAULT"""
    dt = b.detect("dna", outputs=("sum", "dt_len"))
    return b.align(dt.det_off, dt.sum, dt.dt_len)


def _align_truth(b):
    """the true table's own sum / ev_len as the rows, every read's in stored-sample order (an RNA read's events are stored last to first)"""
    ev = b.events(outputs=("sum", "ev_len"))
    idx = torch.from_numpy(stored_order(b.ev_off, True)).to(ev.sum.device)
    return b.align(b.ev_off, ev.sum[idx].contiguous(), ev.ev_len[idx].contiguous(), (256, 1024, 16384))


def _detected_rows(b, preset):
    """(row_off, ev, sum, sumsq, len): the detected rows of a preset, assigned to events by the detector's own true_ev"""
    dt = b.detect(preset, outputs=("sum", "sumsq", "dt_len", "true_ev"))
    return dt.det_off, dt.true_ev, dt.sum, dt.sumsq, dt.dt_len


def _truth_rows(b, rna):
    """(row_off, ev, sum, sumsq, len): the true table's own rows, every read's in stored-sample order like _align_truth, each assigned to itself"""
    ev = b.events(outputs=("sum", "sumsq", "ev_len"))
    idx = torch.from_numpy(stored_order(b.ev_off, rna)).to(ev.sum.device)
    return b.ev_off, idx, ev.sum[idx].contiguous(), ev.sumsq[idx].contiguous(), ev.ev_len[idx].contiguous()


def _scale_fit_detected(b):
    off, ev, s, _, ln = _detected_rows(b, "dna")
    return b.scale(off, s, ln, ev=ev, mode="fit")


def _align_scaled_truth(b):
    """the truth rows aligned under the scaling estimated from the detected ones: the two calls' row_off differ"""
    est = _scale_fit_detected(b)
    off, _, s, _, ln = _truth_rows(b, False)
    return b.align(off, s, ln, scale=(est.gain, est.shift))


def _scale_moments_truth(b):
    off, _, s, _, ln = _truth_rows(b, True)
    return b.scale(off, s, ln, mode="moments")


def _pileup_rows(b, rows, origin=None, **kw):
    p = b.gen.new_pileup(**kw)
    counted, outside, unseen, dropped = b.pileup_rows(p, *rows, origin=origin)
    return api.Chunks(counted=counted, outside=outside, unseen=unseen, dropped=dropped, row_off=np.asarray(rows[0]),
                      **{n: getattr(p, n) for n in api.PILEUP_OUTPUTS}, **_keyed("pileup", origin))


def _origin(b):
    """one origin per read, the second on the minus strand; the window [200, 4000) leaves events of every read outside"""
    n = b.n_reads
    return (200 * np.arange(n, dtype=np.int64) + np.where(np.arange(n) & 1, 5000, 100)), np.where(np.arange(n) & 1, -1, 1).astype(np.int8)


def _other_origin(b):
    """_origin seven keys further on and every read on the other strand: a per-read origin table that the neighbouring pileup or call left
    in the scratch would change every site_key and every frequency sum"""
    key0, step = _origin(b)
    return key0 + 7, (-step).astype(np.int8)


def _call_plan(b):
    off, ns = b.call_plan()
    return api.Chunks(site_off=torch.from_numpy(off), n_sites=ns)


def _called(b, ch, fq, origin):
    """a Batch.call's tensors, site_off, n_sites and stat, with the four sums of the frequency table it added to"""
    return api.Chunks(**vars(ch), **{f"freq_{n}": getattr(fq, n) for n in api.CALL_FREQ}, **_keyed("call", origin))


def _call_true(b, origin):
    """the true table's rows under the binding's defaults, a frequency table over [200, 4000)"""
    ev = b.events(outputs=("sum", "ev_len"))
    fq = b.gen.new_call_freq(200, 4000)
    return _called(b, b.call(ev.sum, ev.ev_len, origin=origin, freq=fq), fq, origin)


def _call_observed(b, origin):
    """the detected rows collapsed into the events their true_ev names -- int64 lengths, events without a row -- under the scaling fitted
    to the same rows"""
    rows = _detected_rows(b, "dna")
    est = b.scale(rows[0], rows[2], rows[4], ev=rows[1], mode="fit")
    co = b.collapse(*rows, outputs=("ob_sum", "ob_len"))
    fq = b.gen.new_call_freq(200, 4000)
    return _called(b, b.call(co.ob_sum, co.ob_len, scale=(est.gain, est.shift), origin=origin, freq=fq, neigh="read", llr_min=0, min_obs=2), fq, origin)


JOBS = {
    # DNA, no prefix, SQG_METH
    "r9_meth": [
        ("chunks", lambda b: b.chunks(L, S, W)),
        ("chunk_targets", lambda b: b.chunk_targets(L, S, clean=True, clean_raw=True, moves=True, kmer=True)),
        ("detect medmad", lambda b: b.detect("dna", "medmad")),
        ("sites", lambda b: b.sites(64, ctx_len=5)),
        ("events medmad", lambda b: b.events("medmad")),
        ("align detected", _align_detected),
        ("events pa", lambda b: b.events("pa")),
        # the caller's rows, whose offsets share one scratch array: neighbours take rows of different row_off (detected, truth, detected)
        ("scale fit detected", _scale_fit_detected),
        ("align scaled truth", _align_scaled_truth),
        ("collapse detected medmad", lambda b: b.collapse(*_detected_rows(b, "dna"), norm="medmad")),
        # the caller's per-batch plan, and the per-read origin table that pileups and calls share: a call between two pileups takes another
        # origin than both, so a pileup and a call of different origins are neighbours in either direction
        ("call plan", _call_plan),
        ("call true ref-origin", lambda b: _call_true(b, _origin(b))),
        ("pileup ref medmad", lambda b: _pileup(b, origin=_origin(b), by="ref", norm="medmad", lo=200, hi=4000)),
        ("call observed other-origin", lambda b: _call_observed(b, _other_origin(b))),
        ("pileup_rows ref truth", lambda b: _pileup_rows(b, _truth_rows(b, False), origin=_origin(b), by="ref", norm="medmad", lo=200, hi=4000)),
    ],
    # RNA, SQG_PREFIX
    "rna004_prefix": [
        ("segments", _segments),
        ("detect medmad trim", lambda b: b.detect("rna", "medmad", True)),
        ("chunks trim", lambda b: b.chunks(L, S, W, trim=True)),
        ("align truth", _align_truth),
        ("chunk_targets trim", lambda b: b.chunk_targets(L, S, clean=True, clean_raw=True, moves=True, kmer=True, trim=True)),
        ("events medmad trim", lambda b: b.events("medmad", trim=True)),
        ("detect pa", lambda b: b.detect("rna")),
        ("events medmad", lambda b: b.events("medmad", trim=False)),
        ("pileup kmer trim", lambda b: _pileup(b, by="kmer", norm="medmad", trim=True)),
        # (truth, detected, truth)
        ("scale moments truth", _scale_moments_truth),
        ("collapse detected trim", lambda b: b.collapse(*_detected_rows(b, "rna"), norm="medmad", trim=True)),
        ("pileup_rows kmer trim truth", lambda b: _pileup_rows(b, _truth_rows(b, True), by="kmer", norm="medmad", trim=True)),
    ],
}


def _batches(cid, mode, n_batches):
    """a fresh context with the fixture's reads run as n_batches consecutive batches (the same reads each time: the generator's state moves
    on, so the batches' signals differ), all waited for"""
    _, _, gen = _context(dict(REFVEC_CASES)[cid], mode)
    seqs = [r["seq"] for r in _fixture_reads(cid)]
    bs = [gen.stage(seqs).run() for _ in range(n_batches)]
    return gen, [b.wait() for b in bs]


def _close(gen, bs):
    for b in bs:
        b.free()
    gen.close()


def _same(got, want, what):
    assert vars(got).keys() == vars(want).keys(), what
    n = 0
    for key, w in vars(want).items():
        g = getattr(got, key)
        if isinstance(w, torch.Tensor):
            assert isinstance(g, torch.Tensor) and g.dtype == w.dtype and torch.equal(g.cpu(), w.cpu()), f"{what}: {key}"
            n += w.numel()
        elif isinstance(w, np.ndarray):
            assert np.array_equal(g, w), f"{what}: {key}"
        else:
            assert g == w, f"{what}: {key}"
    return n


def _sites_raw(b, off, ns):
    """sqg_batch_sites as Batch.sites(64, ctx_len=5) calls it, through the library itself and with no plan call in front of it: the
    tensors of a table of ns sites"""
    cfg = api.CSiteCfg(64, 32, b.gen.kmer_size // 2, 5, 2, api.CHUNK_F16, api.CHUNK_MEDMAD)
    dev = torch.device("cuda", b.gen.device)
    shapes = dict(signal=((ns, 64), torch.float16), label=((ns,), torch.uint8), site_read=((ns,), torch.int32), site_pos=((ns,), torch.int32),
                  win_start=((ns,), torch.int64), context=((ns, 5), torch.uint8), ctx_start=((ns, 6), torch.int32),
                  med2=((b.n_reads,), torch.int32), mad4=((b.n_reads,), torch.int32))
    st = api.Chunks(n_sites=ns, site_off=off, **{n: torch.zeros(shapes[n][0], dtype=shapes[n][1], device=dev) for n in api.SITE_OUTPUTS})
    out = api._ptrs(api.CSiteOut, (getattr(st, n) for n in api.SITE_OUTPUTS))
    torch.cuda.synchronize(dev)
    rc = b.gen.L.sqg_batch_sites(b.gen.ctx, b.handle, ctypes.byref(cfg), ctypes.byref(out))
    assert rc == 0, b.gen.L.sqg_last_error(b.gen.ctx).decode()
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [api.MODE_CERTIFIED, api.MODE_EXACT], ids=["certified", "exact"])
def test_site_plan_found_in_the_scratch_behind_other_plans(mode):
    """sqg_batch_sites finds the plan sqg_site_plan left in the scratch when (win_len, before, focus) agree.  Batch.sites() always plans
    right in front of it; here the detector's plan -- the other per-read plan of the context -- and an event table run between the two,
    and the sites must still be those of Batch.sites() alone on a fresh context, bit for bit.  Both orders of the two plans."""
    gen, bs = _batches("r9_meth", mode, 1)
    want = bs[0].sites(64, ctx_len=5)
    _close(gen, bs)
    assert want.n_sites > 0
    for what in ("site plan first", "detect plan first"):
        gen, bs = _batches("r9_meth", mode, 1)
        b = bs[0]
        if what == "detect plan first":
            b.detect_plan("dna")
        off, ns = b.site_plan(64)
        b.detect("dna")
        b.events("medmad")
        # (the plan call again finds the plan in the scratch, as the raw call will, and runs no kernel: a plan that changed is reported
        # here, before a kernel writes that plan's rows into tensors sized by the first one)
        off2, ns2 = b.site_plan(64)
        assert ns2 == ns == want.n_sites and np.array_equal(off2, off), f"r9_meth {what}: the plan in the scratch"
        assert _same(_sites_raw(b, off, ns), want, f"r9_meth {what}") > 0
        _close(gen, bs)


def _call_raw(b, rows, off, ns):
    """sqg_batch_call as Batch.call(sum, ev_len) calls it, through the library itself and with no plan call in front of it: the tensors
    of a table of ns sites, and stat"""
    dev = torch.device("cuda", b.gen.device)
    dts = dict(site_read=torch.int32, site_pos=torch.int32, label=torch.uint8, n_obs=torch.int32, nll_c=torch.int32, nll_m=torch.int32, llr=torch.int32, call=torch.uint8)
    ch = api.Chunks(n_sites=ns, site_off=off, **{n: (torch.zeros(ns, dtype=dts[n], device=dev) if n in dts else None) for n in api.CALL_OUTPUTS})
    mw, mc = b.gen.call_model()
    cfg, cin, cmod = api.CCallCfg(*api.CALL_DEFAULT), api.CCallIn(rows[0].data_ptr(), None, rows[1].data_ptr()), api.CCallModel(mw.data_ptr(), mc.data_ptr())
    out = api._ptrs(api.CCallOut, (getattr(ch, n) for n in api.CALL_OUTPUTS))
    st = api.CCallStat()
    torch.cuda.synchronize(dev)
    rc = b.gen.L.sqg_batch_call(b.gen.ctx, b.handle, ctypes.byref(cfg), ctypes.byref(cin), ctypes.byref(cmod), None, None, ctypes.byref(out), None, ctypes.byref(st))
    assert rc == 0, b.gen.L.sqg_last_error(b.gen.ctx).decode()
    ch.stat = (int(st.sites), int(st.outside), int(st.called), int(st.agree))
    return ch


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [api.MODE_CERTIFIED, api.MODE_EXACT], ids=["certified", "exact"])
@pytest.mark.parametrize("short", [1, 0], ids=["short read in batch 1", "short read in batch 0"])
def test_call_plan_found_in_the_scratch_behind_other_plans(short, mode):
    """sqg_batch_call finds the plan sqg_call_plan left in the context, by (batch, run).  Batch.call() always plans right in front of it;
    here the site plan, the detector's plan and a plan and a call of the OTHER batch run between the two.  One of the two batches holds
    a read shorter than a k-mer and the other none, so the per-read skip marks, uploaded when a plan is made, change hands with the
    plan.  The plan call on batch 0 again gives what it gave, and the raw call behind it what Batch.call() alone gives on a fresh
    context, bit for bit"""
    seqs = [r["seq"] for r in _fixture_reads("r9_meth")]
    batches = [list(seqs), list(seqs)]
    batches[short].insert(1, seqs[0][:3])                  # three bases: shorter than the 6-mer, between reads with sites

    def context():
        _, k, gen = _context(dict(REFVEC_CASES)["r9_meth"], mode)
        assert k == 6
        bs = [gen.stage(bt).run() for bt in batches]
        return gen, [b.wait() for b in bs]
    rows = lambda b: (lambda ev: (ev.sum, ev.ev_len))(b.events(outputs=("sum", "ev_len")))      # noqa: E731
    gen, bs = context()
    want = bs[0].call(*rows(bs[0]))
    other = bs[1].call_plan()[1]
    _close(gen, bs)
    assert want.n_sites > 0 and want.stat[2] > 0
    gen, bs = context()
    r0, r1 = rows(bs[0]), rows(bs[1])
    off, ns = bs[0].call_plan()
    bs[1].site_plan(64)
    bs[1].detect("dna")
    off1, ns1 = bs[1].call_plan()
    assert bs[1].call(*r1).n_sites == ns1 == other and len(off1) == len(off) + (1 if short else -1)
    off2, ns2 = bs[0].call_plan()
    assert ns2 == ns == want.n_sites and np.array_equal(off2, off) and np.array_equal(off, want.site_off), "the plan of batch 0, asked for again"
    assert _same(_call_raw(bs[0], r0, off, ns), want, "the raw call behind the other batch's plan") > 0
    _close(gen, bs)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [api.MODE_CERTIFIED, api.MODE_EXACT], ids=["certified", "exact"])
@pytest.mark.parametrize("cid", list(JOBS))
def test_outputs_do_not_depend_on_the_calls_before(cid, mode):
    calls = JOBS[cid]
    alone = {}
    for bi in (0, 1):
        for name, call in calls:
            gen, bs = _batches(cid, mode, bi + 1)
            alone[(bi, name)] = call(bs[bi])
            _close(gen, bs)
    for name, _ in calls:                                  # the reference says something: rows were written, and the two batches differ
        a0, a1 = alone[(0, name)], alone[(1, name)]
        assert sum(t.numel() for t in vars(a0).values() if isinstance(t, torch.Tensor)) > 0, name
        if name in ("segments", "call plan"):              # (rna004-prom has dwell_std 0: the segments, dwell sums, are the same in every batch;
            continue                                       # the sites of a plan are the reads' CpGs, and the batches stage the same reads)
        assert any(isinstance(t, torch.Tensor) and (t.shape != getattr(a1, k).shape or not torch.equal(t, getattr(a1, k))) for k, t in vars(a0).items()), name
    assert alone[(0, calls[-1][0])].counted > 0
    # neighbouring calls that take rows take different ones, detected against truth: offsets left in the scratch by one would change the other
    taken = [getattr(alone[(0, name)], "row_off", None) for name, _ in calls]
    pairs = [(a, b) for a, b in zip(taken, taken[1:]) if a is not None and b is not None]
    assert len(pairs) >= 2 and all(not np.array_equal(a, b) for a, b in pairs), cid
    if cid == "r9_meth":
        assert alone[(0, "pileup ref medmad")].outside > 0
        # neighbouring calls that write the per-read origin table: a pileup in front of a call and a call in front of a pileup, of different
        # origins each time -- a table left in the scratch by one would change the other's keys
        keyed = [vars(alone[(0, name)]) for name, _ in calls]
        turns = {(a["origin_of"], b["origin_of"]) for a, b in zip(keyed, keyed[1:]) if "origin_of" in a and "origin_of" in b
                 and not np.array_equal(a["origin_key0"], b["origin_key0"]) and not np.array_equal(a["origin_step"], b["origin_step"])}
        assert {("pileup", "call"), ("call", "pileup")} <= turns, turns
        true, obs = alone[(0, "call true ref-origin")], alone[(0, "call observed other-origin")]
        assert alone[(0, "call plan")].n_sites == true.n_sites == obs.n_sites == true.stat[0] > 0 and torch.equal(alone[(0, "call plan")].site_off, torch.from_numpy(true.site_off))
        for ch in (true, obs):                             # sites inside the table and outside it, calls that agree with the label; the keys differ
            assert 0 < ch.stat[1] < ch.stat[0] and ch.stat[3] > 0 and int(ch.freq_cov.sum()) == ch.stat[0] - ch.stat[1]
        assert not torch.equal(true.site_key, obs.site_key) and bool((obs.n_obs < true.n_obs).any())
        rows = alone[(0, "pileup_rows ref truth")]
        assert rows.counted == alone[(0, "pileup ref medmad")].counted and rows.unseen == rows.dropped == 0      # (every event its own row)
    else:                                                  # the trimmed job took the inserts' spans: the same sums, other statistics
        t, w = alone[(0, "events medmad trim")], alone[(0, "events medmad")]
        assert torch.equal(t.sum, w.sum) and not torch.equal(t.med2, w.med2) and not torch.equal(t.mean, w.mean)
    for what, order in (("listed order", calls), ("reverse order", calls[::-1])):
        gen, bs = _batches(cid, mode, 1)
        for name, call in order:
            assert _same(call(bs[0]), alone[(0, name)], f"{cid} {what}: {name}") > 0
        _close(gen, bs)
    # two batches: both have run before the first call; every call on batch 1, then on batch 0 (the shared scratch changes hands each time)
    gen, bs = _batches(cid, mode, 2)
    for name, call in calls:
        for bi in (1, 0):
            _same(call(bs[bi]), alone[(bi, name)], f"{cid} two batches: {name} on batch {bi}")
    for name, call in calls[::-1]:                         # ... and every call on batch 0 once more, with batch 1's scratch left behind
        _same(call(bs[0]), alone[(0, name)], f"{cid} two batches, again: {name} on batch 0")
    _close(gen, bs)
