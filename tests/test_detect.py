"""include/sqg_detect.h: the t-statistic event detector on a batch's stored signal (sqg_detect_plan, sqg_batch_detect), against the plain
Python statement of the header's rule (detect_ref.py) on natural and on injected signals, and against sqg_batch_events on the same batch.
Every comparison is bit for bit (floats as integers)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (before the library is loaded: the HIP runtime torch brings is the one the library then uses)

import chunks_ref as R
import detect_ref as D
import inject
from chunk_support import _context, _declared, _fixture_reads
from refvec_cases import REFVEC_CASES
from squigulator_amd import api, build, model, options, profiles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_LIB = os.path.join(ROOT, "oracle", "libsqg_cpu.so")
OUT_KEYS = api.DETECT_OUTPUTS
TILE, HALO = 256, 64   # k_detect.h's DET_T and DET_H: a lane walks its read in tiles of 256 samples with 64 more on either side
CFGS = {"dna": D.DNA, "rna": D.RNA, "both": (3, 6, 4.0, 3.0, 0.2), "narrow": (1, 2, 1.0, 1.0, 0.1), "wide": (32, 64, 2.0, 2.0, 0.2)}


def _case(cid):
    """(options, k, rna, prefix, (int)dwell_mean) of a committed vector's command line"""
    o = options.parse_args(dict(REFVEC_CASES)[cid])
    return o, o.kmer_size_default, bool(o.flags & profiles.SQ_RNA), bool(o.flags & profiles.SQ_PREFIX), int(o.profile.dwell_mean)


# ---------------------------------------------------------------------------------------------------------- no GPU
def test_header_declares_the_detect_exports_and_the_libraries_have_them():
    assert _declared("sqg_detect.h") == set(api.EXPORTS_DETECT) == {"sqg_detect_plan", "sqg_batch_detect"}
    others = (set(api.EXPORTS) | set(api.EXPORTS_CHUNKS) | set(api.EXPORTS_TARGETS) | set(api.EXPORTS_SEGMENTS) | set(api.EXPORTS_SITES)
              | set(api.EXPORTS_EVENTS) | set(api.EXPORTS_PILEUP))
    assert not set(api.EXPORTS_DETECT) & others
    build.build()
    for lib in (build.LIB, build.LIB_DEV):
        L = api.load_library(lib)
        for n in api.EXPORTS_DETECT:
            assert hasattr(L, n), f"{n} not exported by {lib}"
    assert os.path.join(ROOT, "include", "sqg_detect.h") in build.headers()
    for h in ("k_detect.h", "h_detect.h"):
        assert os.path.join(ROOT, "squigulator_amd", "csrc", h) in build.headers()
    raw = open(os.path.join(ROOT, "include", "sqg_detect.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for struct, ctype in (("sqg_detect_cfg_t", api.CDetectCfg), ("sqg_detect_out_t", api.CDetectOut)):
        body = hdr[:hdr.index("} " + struct)]
        body = body[body.rindex("typedef struct"):]
        fields = [f[0] for f in ctype._fields_]
        at = [body.index(name + ";") for name in fields]     # every field is declared, in the binding's order
        assert at == sorted(at), f"{struct}: {fields}"
        assert body.count(";") == len(fields), f"{struct}: the header has fields the binding lacks"
    assert [f[0] for f in api.CDetectCfg._fields_] == ["w_short", "w_long", "thr_short", "thr_long", "peak_height", "norm", "trim"]
    assert C.sizeof(api.CDetectCfg) == 40 and api.CDetectCfg.thr_short.offset == 8 and api.CDetectCfg.norm.offset == 32
    assert tuple(f[0] for f in api.CDetectOut._fields_) == OUT_KEYS == D.PER_ROW + D.PER_READ
    for name, five in (("SQG_DETECT_DNA", D.DNA), ("SQG_DETECT_RNA", D.RNA)):       # the presets: header, binding and reference alike
        got = re.search(r"#define\s+" + name + r"\s*\{([^}]*)\}", hdr).group(1).split(",")
        assert tuple(float(v) for v in got) == five == api.DETECT_PRESETS[name[-3:].lower()]
    assert "NOT bit-equal" in raw and "exact integers" in raw and "strictly ascending" in raw and "capped at 64" in raw


def test_the_cpu_backend_has_no_detector_and_says_so():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "libsqg_cpu.so"])
    prof, fl = profiles.get_profile("dna-r9-prom")
    mean, stdv = model.synthetic_model(6)
    gen = api.SignalGenerator(prof, fl, 6, mean, stdv, 42, lib_path=CPU_LIB)
    for n in api.EXPORTS_DETECT:
        assert not hasattr(gen.L, n)
    b = gen.submit([b"ACGTACGTACGTTTGACA" * 40])
    for call in (b.detect, b.detect_plan):
        with pytest.raises(api.SqgError) as e:
            call()
        assert e.value.code == -1 and "sqg_batch_detect" in str(e.value)
    b.free(); gen.close()


def test_the_two_statements_of_the_t_statistic_agree():
    rng = np.random.default_rng(11)
    signals = [rng.integers(-32768, 32768, 300).astype(np.int16), np.where(np.arange(200) & 1, 32767, -32768).astype(np.int16),
               np.full(150, -7, np.int16), (rng.normal(600, 10, 400) + 200 * (np.arange(400) // 37 % 2)).astype(np.int16)]
    for x in signals:
        for w in (1, 2, 3, 6, 7, 14, 32, 64):
            for n in (len(x), 2 * w - 1, 2 * w, 2 * w + 1, 1):
                a, b = D.tstat(x[:n], w), D.tstat_slices(x[:n], w)
                np.testing.assert_array_equal(a.view(np.int64), b.view(np.int64))
                assert (a[:w] == 0).all() and (a[max(n - w + 1, 0):] == 0).all() and (n >= 2 * w or not a.any())
    assert D.tstat(signals[1], 64).max() == 0 and D.tstat(signals[1], 3).min() == 0 < D.tstat(signals[1], 3)[3:-3].min()       # the windows' sums cancel only where w is even
    assert not D.tstat(signals[2], 6).any()                                                # a constant: N = 0 and D = 0
    t = D.tstat(np.array([500] * 8 + [900] * 8, np.int16), 3)                              # D = 0 and N > 0 at the step: sqrt(3 * 1200^2)
    assert t[8] == np.sqrt(np.float64(3 * 1200 * 1200)) and t[7] > 0 and (t[:6] == 0).all() and (t[11:] == 0).all()


def test_helper_on_a_hand_worked_read():
    """150 samples of 500, then 150 of 900: under the DNA preset the one boundary 150 and two rows, typed out"""
    x = np.array([500] * 150 + [900] * 150, np.int16)
    info = {}
    assert D.boundaries(x, D.DNA, info) == [150] and info == dict(short=1, long=0, masks=info["masks"], dropped=0) and info["masks"] >= 1
    assert D.boundaries(x, D.RNA) == [150] and D.boundaries(x[:5], D.DNA) == [] and D.boundaries(x[:150], D.DNA) == []
    read = dict(sig=x, ss=[100, 50, 1, 149], seq=b"ACGTAC", offset=0.5)
    w = D.read_rows(read, D.DNA, 3, False, False, 2, "pa", False, 2.0, 4.0, index=4, ev_off=10)
    assert w["dt_read"].tolist() == [4, 4] and w["dt_start"].tolist() == [0, 150] and w["dt_len"].tolist() == [150, 150]
    assert w["sum"].tolist() == [75000, 135000] and w["sumsq"].tolist() == [150 * 250000, 150 * 810000]
    assert w["vmin"].tolist() == w["vmax"].tolist() == [500, 900] and w["true_ev"].tolist() == [10, 12]
    np.testing.assert_array_equal(w["mean"], np.array([500.5 * 2 / 4, 900.5 * 2 / 4], np.float32))
    np.testing.assert_array_equal(w["sd"], np.zeros(2, np.float32))
    w = D.read_rows(read, D.DNA, 3, True, False, 2, "medmad", False, index=0, ev_off=0)       # the same stored samples as an RNA read's
    assert w["true_ev"].tolist() == [3, 1] and (w["med2"], w["mad4"]) == (1400, 800)             # events stored at 200, 150, 149, 0
    inv = np.float64(np.float32(1.0 / (1.4826 * 200.0)))
    np.testing.assert_array_equal(w["mean"], np.array([(500 - 700) * inv, (900 - 700) * inv], np.float32))


@pytest.mark.parametrize("cid", ("r10_t1", "rna004_prefix", "r9_prefix"))
def test_helper_against_the_reference_vectors(cid):
    """the compiled reference's own reads, dwells and signal: the rows tile every read in strictly ascending order, their sums add up to
    the read's, and true_ev names an event that holds the row's first sample"""
    o, k, rna, prefix, sps = _case(cid)
    reads = _fixture_reads(cid)
    for cfg in ((D.RNA if rna else D.DNA), CFGS["both"]):
        info = {}
        w = D.batch_rows(reads, cfg, k, rna, prefix, sps, "medmad", True, o.profile.range, o.profile.digitisation, info)
        assert info["short"] > 0 and info["dropped"] == 0 and (cfg[2] < 4 or info["long"] > 0)
        ev_off = np.concatenate(([0], np.cumsum([len(r["ss"]) for r in reads])))
        for i, r in enumerate(reads):
            rows = slice(int(w["det_off"][i]), int(w["det_off"][i + 1]))
            st, ln, n = w["dt_start"][rows], w["dt_len"][rows].astype(np.int64), len(r["sig"])
            assert st[0] == 0 and (st[1:] == (st + ln)[:-1]).all() and (st + ln)[-1] == n and (ln >= 1).all() and (np.diff(st) > 0).all()
            raw = r["sig"].astype(np.int64)
            assert w["sum"][rows].sum() == raw.sum() and w["sumsq"][rows].sum() == (raw * raw).sum()
            assert w["vmin"][rows].min() == raw.min() and w["vmax"][rows].max() == raw.max() and (w["dt_read"][rows] == i).all()
            d = np.asarray(r["ss"], np.int64)
            E = np.cumsum(d) - d
            es = n - E - d if rna else E
            e = w["true_ev"][rows] - ev_off[i]
            assert (e >= 0).all() and (e < len(d)).all() and (d[e] >= 1).all() and (es[e] <= st).all() and (st < es[e] + d[e]).all()
            assert len(np.unique(e)) > len(e) // 4          # the detector follows the events, loosely
        assert np.isfinite(w["mean"]).all() and (w["sd"] >= 0).all()


# ---------------------------------------------------------------------------------------------------------- GPU
def _cpu(t):
    return None if t is None else t.cpu().numpy()


def _own_reads(b, seqs):
    """the batch's own fetched signal and dwells with the reads it was staged from, as detect_ref takes them"""
    sig, dw = b.signal(), b.dwell()
    return [dict(sig=sig[b.sig_off[i]:b.sig_off[i + 1]], ss=dw[b.ev_off[i]:b.ev_off[i + 1]], seq=s, offset=float(b.offset[i])) for i, s in enumerate(seqs)]


def _assert_rows(dt, want, what, keys=OUT_KEYS):
    assert dt.n_rows == want["det_off"][-1], f"{what}: {dt.n_rows} rows, expected {want['det_off'][-1]}"
    np.testing.assert_array_equal(dt.det_off, want["det_off"], err_msg=f"{what}: det_off")
    for key in keys:
        got = _cpu(getattr(dt, key))
        assert got is not None, f"{what}: {key} missing"
        assert got.shape == want[key].shape and got.dtype == want[key].dtype, f"{what}: {key} {got.shape} {got.dtype} vs {want[key].shape} {want[key].dtype}"
        np.testing.assert_array_equal(R.bits(got), R.bits(want[key]), err_msg=f"{what}: {key}")
    if dt.dt_start is not None and dt.n_rows:                # strictly ascending within every read, whatever the reference says
        st, rd = _cpu(dt.dt_start), _cpu(dt.dt_read)
        assert ((np.diff(st) > 0) | (np.diff(rd) > 0)).all() and (np.diff(rd) >= 0).all() and (st[dt.det_off[:-1][np.diff(dt.det_off) > 0]] == 0).all()


def _check(b, own, cfg, k, rna, prefix, sps, what, norm="pa", trim=False, info=None):
    prof = b.gen.profile
    want = D.batch_rows(own, cfg, k, rna, prefix, sps, norm, trim, prof.range, prof.digitisation, info)
    off, n_rows = b.detect_plan(cfg)
    np.testing.assert_array_equal(off, want["det_off"], err_msg=f"{what}: the plan")
    assert n_rows == want["det_off"][-1]
    _assert_rows(b.detect(cfg, norm, trim), want, what)
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ("r10_t1", "r9_t1", "rna004_noprefix", "rna004_prefix", "r9_prefix"))
def test_natural_signal(cid):
    """a fixture's first batch through the HIP path under the five cfgs, every output against detect_ref fed with the batch's own signal and
    dwells.  Checked on the reference, not on the kernel: under {3, 6, 4.0, 3.0, 0.2} both detectors record; under the DNA preset the
    short one masks the long one, which records nothing"""
    o, k, rna, prefix, sps = _case(cid)
    reads = _fixture_reads(cid)[:o.batch]
    _, _, gen = _context(dict(REFVEC_CASES)[cid], api.MODE_CERTIFIED)
    seqs = [r["seq"] for r in reads]
    b = gen.stage(seqs).run().wait()
    own = _own_reads(b, seqs)
    for name, cfg in CFGS.items():
        info = {}
        _check(b, own, cfg, k, rna, prefix, sps, f"{cid} {name}", info=info)
        if name == "both":
            assert info["short"] >= 1 and info["long"] >= 1
        if name == "dna":
            assert info["masks"] >= 1 and info["long"] == 0 and info["short"] >= 1
    _check(b, own, api.DETECT_PRESETS["rna" if rna else "dna"], k, rna, prefix, sps, f"{cid} medmad trimmed", "medmad", True)
    dt = b.detect("rna" if rna else "dna", "medmad", False)
    ev = b.events("medmad", False)
    assert torch.equal(dt.med2, ev.med2) and torch.equal(dt.mad4, ev.mad4)
    b.free(); gen.close()


def _step(n, at, lo=500, hi=900):
    return np.where(np.arange(n) < at, lo, hi).astype(np.int16)


# read lengths around 2 w_short and 2 w_long of the three cfgs run on them (3 / 6, 1 / 2, 32 / 64) and around the kernel's tile and halo
EDGE_LENGTHS = [1, 2, 3, 4, 5, 6, 11, 12, 13, 63, 64, 65, 127, 128, 129, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, TILE + HALO - 1, TILE + HALO, TILE + HALO + 1,
                3 * TILE, 3 * TILE, 3 * TILE, 3 * TILE, 3 * TILE, 3 * TILE]
EDGE_STEPS = {22: TILE - 1, 23: TILE, 24: TILE + 1, 25: 2 * TILE + 1, 26: TILE - HALO, 27: 2 * TILE - 2}      # read -> where its one step is
EDGE_SIGNALS = {
    "constant": lambda n, i, rng: np.full(n, 1234 - 40 * i, np.int16),                          # D = 0 and N = 0
    "step": lambda n, i, rng: _step(n, EDGE_STEPS.get(i, n // 2)),                               # D = 0 and N > 0, the peak at a tile's edge
    "noisy_step": lambda n, i, rng: (_step(n, EDGE_STEPS.get(i, n // 2)).astype(np.int64) + rng.integers(-9, 10, n)).astype(np.int16),
    "alternating": lambda n, i, rng: np.where(np.arange(n) & 1, 32767, -32768).astype(np.int16),   # the largest N and D
    "random": lambda n, i, rng: rng.integers(-32768, 32768, n).astype(np.int16),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(EDGE_SIGNALS))
def test_edges_with_injected_signals(name):
    """the exact1 geometry (one sample per event) with every read's samples overwritten: reads of 1, 2 w - 1, 2 w and 2 w + 1 samples for
    the windows in use, reads that end at T - 1, T, T + 1 and 2 T + 1 for the kernel's tile T, and one step at T - 1, T, T + 1, 2 T + 1,
    T - halo and 2 T - 2, so that a peak found in one tile is recorded in the next"""
    gen, prof, fl, k = inject.context("exact1")
    seqs = inject.seqs_for(inject.bases_for(EDGE_LENGTHS, k))
    b = inject.run_geometry(gen, seqs)
    assert np.diff(b.sig_off).tolist() == EDGE_LENGTHS
    rng = np.random.default_rng(17)
    inject.inject(b, np.concatenate([EDGE_SIGNALS[name](n, i, rng) for i, n in enumerate(EDGE_LENGTHS)]))
    own = _own_reads(b, seqs)
    for cname in ("dna", "narrow", "wide"):
        info = {}
        want = _check(b, own, CFGS[cname], k, False, False, 1, f"{name} {cname}", info=info)
        rows = np.diff(want["det_off"])
        ws = CFGS[cname][0]
        assert all(rows[i] == 1 for i, n in enumerate(EDGE_LENGTHS) if n < 2 * ws)
        if name == "constant":
            assert (rows == 1).all() and (want["sd"] == 0).all()
        if name == "step":
            for i, at in EDGE_STEPS.items():
                assert want["dt_start"][want["det_off"][i]:want["det_off"][i + 1]].tolist() == [0, at], (cname, i)
        if name in ("random", "noisy_step") and cname != "wide":
            assert info["short"] > 10
    b.free(); gen.close()


def _levels(n, rng, dwell=9, spread=150, noise=12):
    """a signal like a read's: levels held for a few samples each, with noise"""
    m = n // 2 + 2
    lv = np.repeat(rng.normal(700, spread, m), np.maximum(1, rng.normal(dwell, 4, m).astype(np.int64)))[:n]
    return (lv + rng.normal(0, noise, n)).astype(np.int16)


@pytest.mark.gpu
@pytest.mark.parametrize("n_reads", [1, 63, 64, 65, 129])
def test_wavefront_shapes(n_reads):
    """one read per lane: batches that fill no wavefront, one exactly, one and a lane, two and a lane, with a read of one sample next to
    one of 5000 in the first wavefront and reads of every length between them in all of them"""
    gen, prof, fl, k = inject.context("exact1")
    rng = np.random.default_rng(n_reads)
    lengths = ([1, 5000] + rng.integers(1, 1500, max(n_reads - 2, 0)).tolist())[-n_reads:]
    if n_reads > 64:
        lengths[-1] = 1; lengths[64] = 2 * TILE + 3         # the last wavefront has one or two reads
    b = inject.run_geometry(gen, inject.seqs_for(inject.bases_for(lengths, k)))
    assert np.diff(b.sig_off).tolist() == lengths and 5000 in lengths and (n_reads == 1 or 1 in lengths)
    inject.inject(b, np.concatenate([_levels(n, rng) for n in lengths]))
    own = _own_reads(b, [None] * n_reads)
    for cname in ("dna", "both"):
        info = {}
        _check(b, own, CFGS[cname], k, False, False, 1, f"{n_reads} reads {cname}", info=info)
        assert info["short"] > 100 and (cname == "dna" or info["long"] >= 1)
    b.free(); gen.close()


@pytest.mark.gpu
def test_consistency_with_the_plan_the_subsets_and_the_true_events():
    """the plan's det_off is what the fill's dt_read counts; outputs not asked for are skipped and a subset has the bytes it has among all
    of them; and a detected row that coincides with a true event has sqg_batch_events' mean and sd, float for float.  The signal is
    injected on drawn dwells: one clean level per true event, so that many rows coincide"""
    gen, prof, fl, k = inject.context("drawn")
    seqs = inject.seqs_for([700, 64, 1500, 6, 333])
    b = inject.run_geometry(gen, seqs)
    dw = b.dwell().astype(np.int64)
    rng = np.random.default_rng(23)
    level = rng.integers(-1500, 1500, len(dw)) + np.where(np.arange(len(dw)) & 1, 4000, 0)
    inject.inject(b, (np.repeat(level, dw) + rng.integers(-3, 4, int(dw.sum()))).astype(np.int16))
    own = _own_reads(b, seqs)
    for norm, trim in (("pa", False), ("medmad", True)):
        want = _check(b, own, D.DNA, k, False, False, int(prof.dwell_mean), f"levels {norm}", norm, trim)
        full = b.detect("dna", norm, trim)
        off, n_rows = b.detect_plan("dna")
        assert n_rows == full.n_rows and (np.bincount(_cpu(full.dt_read), minlength=b.n_reads) == np.diff(off)).all()
        for names in [(n,) for n in OUT_KEYS] + [("dt_len", "mean"), ("true_ev", "sd", "mad4"), ()]:
            part = b.detect("dna", norm, trim, outputs=names)
            for key in OUT_KEYS:
                got = getattr(part, key)
                assert (got is None) == (key not in names) and (got is None or torch.equal(got, getattr(full, key))), (names, key)
        ev = b.events(norm, trim)
        te = full.true_ev
        same = (ev.ev_start[te] == full.dt_start) & (ev.ev_len[te] == full.dt_len) & (ev.ev_read[te] == full.dt_read)
        assert int(same.sum()) >= 100, int(same.sum())
        for key in ("mean", "sd", "sum", "sumsq", "vmin", "vmax"):
            assert torch.equal(getattr(full, key)[same].view(torch.int32 if key in ("mean", "sd") else getattr(full, key).dtype),
                               getattr(ev, key)[te][same].view(torch.int32 if key in ("mean", "sd") else getattr(ev, key).dtype)), key
        inside = (ev.ev_start[te] <= full.dt_start) & (full.dt_start < ev.ev_start[te] + ev.ev_len[te]) & (ev.ev_read[te] == full.dt_read) & (ev.ev_len[te] >= 1)
        assert bool(inside.all())
        assert len(np.unique(want["true_ev"])) > b.n_events // 2
    b.free()
    b = gen.submit([])
    dt = b.detect("rna", "medmad", True)
    assert dt.n_rows == 0 and dt.det_off.tolist() == [0] and all(tuple(getattr(dt, key).shape) == (0,) for key in OUT_KEYS)
    assert b.detect_plan("dna")[1] == 0
    b.free(); gen.close()


def _raw(gen, b, cfg, out, plan=False):
    hb, pc = (b.handle if b is not None else None), (C.byref(cfg) if cfg is not None else None)
    if plan:
        return gen.L.sqg_detect_plan(gen.ctx, hb, pc, None, C.byref(out) if out is not None else None)
    return gen.L.sqg_batch_detect(gen.ctx, hb, pc, C.byref(out) if out is not None else None)


@pytest.mark.gpu
def test_errors():
    o, k, rna, prefix, sps = _case("r9_prefix")
    reads = _fixture_reads("r9_prefix")
    _, _, gen = _context(dict(REFVEC_CASES)["r9_prefix"], api.MODE_CERTIFIED)
    b = gen.stage([r["seq"] for r in reads])
    good = dict(w_short=3, w_long=6, thr_short=1.4, thr_long=9.0, peak_height=0.2, norm=api.CHUNK_PA, trim=0)
    none, nr = api.CDetectOut(), C.c_int64(-5)
    err = lambda: gen.L.sqg_last_error(gen.ctx)             # noqa: E731
    for call in (b.detect, b.detect_plan):                  # staged, not run: an error, not a hang
        with pytest.raises(api.SqgError) as e:
            call()
        assert e.value.code == -4 and "sqg_detect_plan" in str(e.value) and "not been run" in str(e.value)
    assert _raw(gen, b, api.CDetectCfg(**good), none) == -4 and b"sqg_batch_detect" in err() and b"not been run" in err()
    b.run().wait()
    assert b.detect().n_rows == b.detect_plan()[1] > b.n_reads
    bad_fields = [(dict(w_short=0), b"w_short"), (dict(w_short=-3), b"w_short"), (dict(w_short=6), b"w_long"), (dict(w_short=7), b"w_long"),
                  (dict(w_long=65), b"w_long"), (dict(w_short=64, w_long=65), b"w_long"),
                  (dict(thr_short=-0.5), b"thr_short"), (dict(thr_short=float("nan")), b"thr_short"), (dict(thr_long=float("inf")), b"thr_long"),
                  (dict(thr_long=-1e-300), b"thr_long"), (dict(peak_height=float("nan")), b"peak_height"), (dict(peak_height=-1.0), b"peak_height"),
                  (dict(norm=2), b"norm"), (dict(trim=2), b"trim"), (dict(trim=-1), b"trim")]
    for bad, what in bad_fields:
        cfg = api.CDetectCfg(**dict(good, **bad))
        assert _raw(gen, b, cfg, none) == -1 and b"sqg_batch_detect" in err() and what in err(), (bad, err())
        assert _raw(gen, b, cfg, nr, plan=True) == -1 and b"sqg_detect_plan" in err() and what in err(), (bad, err())
    assert nr.value == -5
    assert _raw(gen, b, api.CDetectCfg(**dict(good, w_short=63, w_long=64, thr_short=0.0, thr_long=0.0, peak_height=0.0)), nr, plan=True) == 0      # the ends of the ranges
    assert nr.value >= b.n_reads
    for bad in (dict(cfg="cdna"), dict(cfg=(3, 6, 1.4)), dict(norm="raw"), dict(outputs=("mean", "median"))):
        with pytest.raises(api.SqgError) as e:
            b.detect(**bad)
        assert e.value.code == -1 and "detect" in str(e.value), bad
    cfg = api.CDetectCfg(**good)
    Lb = gen.L
    assert Lb.sqg_batch_detect(None, None, None, None) == -1 and Lb.sqg_batch_detect(None, b.handle, C.byref(cfg), C.byref(none)) == -1
    assert Lb.sqg_detect_plan(None, b.handle, C.byref(cfg), None, C.byref(nr)) == -1
    assert _raw(gen, None, cfg, none) == -1 and b"sqg_batch_detect" in err() and b"batch" in err()
    assert _raw(gen, b, None, none) == -1 and b"sqg_batch_detect" in err() and b"cfg" in err()
    assert _raw(gen, b, cfg, None) == -1 and b"sqg_batch_detect" in err() and b"out" in err()
    assert _raw(gen, None, cfg, nr, plan=True) == -1 and b"sqg_detect_plan" in err() and b"batch" in err()
    assert _raw(gen, b, None, nr, plan=True) == -1 and b"sqg_detect_plan" in err() and b"cfg" in err()
    assert _raw(gen, b, cfg, None, plan=True) == -1 and b"sqg_detect_plan" in err() and b"n_rows" in err()
    assert _raw(gen, b, cfg, none) == 0                      # nothing wanted: nothing written
    assert _raw(gen, b, cfg, nr, plan=True) == 0 and nr.value == b.detect_plan()[1]          # det_off may be NULL
    b.free(); gen.close()


@pytest.mark.gpu
def test_lifetime_and_detection_while_the_generator_runs_ahead():
    """a batch keeps its detected table until two more batches have been run; taken while two later batches are staged and one is running it
    is what it was when the generator was quiet"""
    o, k, rna, prefix, sps = _case("rna004_tk4")
    reads = _fixture_reads("rna004_tk4")
    _, _, gen = _context(dict(REFVEC_CASES)["rna004_tk4"], api.MODE_EXACT)
    parts = [[r["seq"] for r in reads[0:4]], [r["seq"] for r in reads[4:8]], [r["seq"] for r in reads[0:4]], [r["seq"] for r in reads[4:8]]]
    b0 = gen.stage(parts[0]).run().wait()
    quiet = b0.detect("rna", "medmad", True)
    want = D.batch_rows(_own_reads(b0, parts[0]), D.RNA, k, rna, prefix, sps, "medmad", True, o.profile.range, o.profile.digitisation)
    _assert_rows(quiet, want, "quiet")
    assert quiet.n_rows > b0.n_reads
    b1, b2, b3 = (gen.stage(p) for p in parts[1:])
    b1.run()                                                # one running, two staged
    busy = b0.detect("rna", "medmad", True)
    b1.wait()
    again = b0.detect("rna", "medmad", True)                # after one more batch has run: the same
    for key in OUT_KEYS:
        assert torch.equal(getattr(busy, key), getattr(quiet, key)) and torch.equal(getattr(again, key), getattr(quiet, key)), key
    b2.run().wait()
    for call in (lambda: b0.detect("rna"), lambda: b0.detect_plan("rna")):      # two more batches: slabs and dwells are batch 2's
        with pytest.raises(api.SqgError) as e:
            call()
        assert e.value.code == -4 and "sqg_detect_plan" in str(e.value) and "handed to a later batch" in str(e.value)
    assert _raw(gen, b0, api.CDetectCfg(7, 14, 2.5, 9.0, 1.0, 0, 0), api.CDetectOut()) == -4 and b"sqg_batch_detect" in gen.L.sqg_last_error(gen.ctx)
    _assert_rows(b1.detect("rna", "pa", False), D.batch_rows(_own_reads(b1, parts[1]), D.RNA, k, rna, prefix, sps, "pa", False, o.profile.range, o.profile.digitisation),
                 "batch 1 after batch 2")
    for b in (b0, b1, b2, b3):
        b.free()
    gen.close()


@pytest.mark.gpu
def test_detection_between_run_begin_and_run_end_of_a_later_batch():
    """range mode: sqg_batch_run_begin of batch r + 2 takes the slot of batch r.  With the generator two batches ahead batch 0 is refused,
    batch 1 is served bit for bit, and the batch that is begun but not ended is refused, not waited for"""
    prof, fl = profiles.get_profile("dna-r9-prom")
    mean, stdv = model.synthetic_model(6)
    gen = api.SignalGenerator(prof, fl, 6, mean, stdv, 42, num_workers=1, mode=api.MODE_CERTIFIED)
    zero = torch.zeros(4096, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    gen.set_range_mode(True)
    seqs = [inject.seqs_for([700, 90, 1300, 5, 400], seed=s) for s in (1, 2, 3)]
    bs = [gen.stage(s) for s in seqs]
    for b in bs[:2]:
        b.run_begin()
        b.run_end(zero.data_ptr(), zero.data_ptr()).wait()
    sps = int(prof.dwell_mean)
    wants = [D.batch_rows(_own_reads(b, s), D.DNA, 6, False, False, sps, "pa", False, prof.range, prof.digitisation) for b, s in zip(bs[:2], seqs)]
    _assert_rows(bs[0].detect(), wants[0], "batch 0, two batches run")
    bs[2].run_begin()                                      # takes the slot of batch 0
    with pytest.raises(api.SqgError) as e:
        bs[0].detect()
    assert e.value.code == -4 and "handed to a later batch" in str(e.value)
    with pytest.raises(api.SqgError) as e:
        bs[2].detect()
    assert e.value.code == -4 and "not been run" in str(e.value)
    _assert_rows(bs[1].detect(), wants[1], "batch 1 while batch 2 is begun")
    bs[2].run_end(zero.data_ptr(), zero.data_ptr()).wait()
    _assert_rows(bs[2].detect(), D.batch_rows(_own_reads(bs[2], seqs[2]), D.DNA, 6, False, False, sps, "pa", False, prof.range, prof.digitisation), "batch 2")
    for b in bs:
        b.free()
    gen.close()
