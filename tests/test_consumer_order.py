"""The calls that read a finished batch on the device share scratch of the context (the reads' constants, the inserts' spans, the chunk
and site plans, the event columns, the detector's plan, the aligner's levels, the caller's row offsets): what a call writes must not depend on which other calls
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


def _pileup(b, origin=None, **kw):
    p = b.gen.new_pileup(**kw)
    counted, outside = b.pileup(p, origin=origin)
    return api.Chunks(counted=counted, outside=outside, **{n: getattr(p, n) for n in api.PILEUP_OUTPUTS})


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


def _pileup_rows(b, rows, **kw):
    p = b.gen.new_pileup(**kw)
    counted, outside, unseen, dropped = b.pileup_rows(p, *rows)
    return api.Chunks(counted=counted, outside=outside, unseen=unseen, dropped=dropped, row_off=np.asarray(rows[0]),
                      **{n: getattr(p, n) for n in api.PILEUP_OUTPUTS})


def _origin(b):
    """one origin per read, the second on the minus strand; the window [200, 4000) leaves events of every read outside"""
    n = b.n_reads
    return (200 * np.arange(n, dtype=np.int64) + np.where(np.arange(n) & 1, 5000, 100)), np.where(np.arange(n) & 1, -1, 1).astype(np.int8)


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
        ("pileup ref medmad", lambda b: _pileup(b, origin=_origin(b), by="ref", norm="medmad", lo=200, hi=4000)),
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
        if name == "segments":                             # (rna004-prom has dwell_std 0: the segments, dwell sums, are the same in every batch)
            continue
        assert any(isinstance(t, torch.Tensor) and (t.shape != getattr(a1, k).shape or not torch.equal(t, getattr(a1, k))) for k, t in vars(a0).items()), name
    assert alone[(0, calls[-1][0])].counted > 0
    # neighbouring calls that take rows take different ones, detected against truth: offsets left in the scratch by one would change the other
    taken = [getattr(alone[(0, name)], "row_off", None) for name, _ in calls]
    pairs = [(a, b) for a, b in zip(taken, taken[1:]) if a is not None and b is not None]
    assert len(pairs) >= 2 and all(not np.array_equal(a, b) for a, b in pairs), cid
    if cid == "r9_meth":
        assert alone[(0, "pileup ref medmad")].outside > 0
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
