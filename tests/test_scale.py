"""include/sqg_scale.h: the per-read shift and scale estimated from event rows (sqg_batch_scale) and the aligner under a per-read scaling
(sqg_batch_align_scaled), against the two plain statements of the header's rule (scale_ref.py) and align_ref's recurrence on the scaled
row values.  Every comparison is bit for bit: the sums are integers, gain and shift the integers the header derives from them."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (before the library is loaded: the HIP runtime torch brings is the one the library then uses)

import align_ref as A
import detect_ref as D
import events_ref as EV
import inject
import scale_ref as S
from chunk_support import _context, _declared, _fixture_reads
from refvec_cases import REFVEC_CASES
from squigulator_amd import api, build, model, options, profiles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = api.SCALE_OUTPUTS
AOUT = api.ALIGN_OUTPUTS
CFG = (256, 1024, 16384)
MODES = {"moments": S.MOMENTS, "fit": S.FIT}
WG = 256            # k_common.h's CHUNK_WG: the rows of one workgroup and trip of k_scale_sums
I64_MIN = -(1 << 63)
LOOP_GAIN, LOOP_OFFSET = 1.15, 40          # the miscalibration of the loop test: sum' = rint(1.15 sum) + 40 len


def _offsets(lens):
    return np.concatenate(([0], np.cumsum(lens))).astype(np.int64)


def _both(row_off, sums, lens, ev_off, level, mode, ev=None, what=""):
    """the two statements on one batch: they agree on every output -> the first one's"""
    a = S.by_read(row_off, sums, lens, ev_off, level, mode, ev)
    b = S.vectorised(row_off, sums, lens, ev_off, level, mode, ev)
    for key in S.OUTPUTS:
        assert a[key].dtype == b[key].dtype == S.DTYPES[key], key
        np.testing.assert_array_equal(a[key], b[key], err_msg=f"{what}: the two statements differ in {key}")
    return a


# ---------------------------------------------------------------------------------------------------------- no GPU
def _struct_fields(hdr, struct):
    body = hdr[:hdr.index("} " + struct)]
    body = body[body.rindex("typedef struct"):]
    body = body[body.index("{") + 1:]
    return [re.sub(r"[\s*]", "", name) for decl in body.split(";") if decl.strip() for name in re.sub(r"^\s*(const\s+)?\w+\s", "", decl.strip()).split(",")]


def test_the_header_and_the_binding_agree():
    assert _declared("sqg_scale.h") == set(api.EXPORTS_SCALE) == {"sqg_batch_scale", "sqg_batch_align_scaled"}
    others = set(api.EXPORTS) | set(api.EXPORTS_CHUNKS) | set(api.EXPORTS_TARGETS) | set(api.EXPORTS_SEGMENTS) | set(api.EXPORTS_SITES) | set(api.EXPORTS_EVENTS) | \
        set(api.EXPORTS_PILEUP) | set(api.EXPORTS_DETECT) | set(api.EXPORTS_ALIGN) | set(api.EXPORTS_COLLAPSE)
    assert not set(api.EXPORTS_SCALE) & others
    # the headers next to it export what they did
    assert _declared("sqg_align.h") == set(api.EXPORTS_ALIGN) == {"sqg_batch_align"}
    assert _declared("sqg_collapse.h") == set(api.EXPORTS_COLLAPSE) == {"sqg_batch_collapse", "sqg_batch_pileup_rows"}
    raw = open(os.path.join(ROOT, "include", "sqg_scale.h")).read()
    assert '#include "sqg_align.h"' in raw and "SQG_ABI_VERSION is unchanged" in raw and "wrap modulo 2^64" in raw and "CLAMPED" in raw
    assert "rint rounds half to even" in raw and "one rounding per" in raw
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for struct, ctype in (("sqg_scale_cfg_t", api.CScaleCfg), ("sqg_scale_in_t", api.CScaleIn), ("sqg_scale_out_t", api.CScaleOut), ("sqg_align_scale_t", api.CAlignScale)):
        assert _struct_fields(hdr, struct) == [f[0] for f in ctype._fields_], struct
    assert tuple(f[0] for f in api.CScaleOut._fields_) == OUT == S.OUTPUTS and tuple(f[0] for f in api.CScaleIn._fields_) == api.SCALE_INPUTS
    assert C.sizeof(api.CScaleCfg) == 4 and C.sizeof(api.CScaleIn) == 24 and C.sizeof(api.CScaleOut) == 80 and C.sizeof(api.CAlignScale) == 16
    assert int(re.search(r"#define\s+SQG_SCALE_MOMENTS\s+(\d+)u", hdr).group(1)) == api.SCALE_MOMENTS == S.MOMENTS == 0
    assert int(re.search(r"#define\s+SQG_SCALE_FIT\s+(\d+)u", hdr).group(1)) == api.SCALE_FIT == S.FIT == 1
    # the prototypes: the pointers behind (ctx, batch) in the order of the binding's table; the table's entry stands in front of the collapse's
    at = [names for names, _ in api._CONSUMER_EXPORTS].index(api.EXPORTS_SCALE)
    assert api._CONSUMER_EXPORTS[-1][0] == api.EXPORTS_COLLAPSE and at < len(api._CONSUMER_EXPORTS) - 1
    table = dict(api._CONSUMER_EXPORTS[at][1])
    names = {api.CScaleCfg: "sqg_scale_cfg_t", api.CScaleIn: "sqg_scale_in_t", api.CScaleOut: "sqg_scale_out_t", api.CAlignScale: "sqg_align_scale_t",
             api.CAlignCfg: "sqg_align_cfg_t", api.CAlignIn: "sqg_align_in_t", api.CAlignOut: "sqg_align_out_t", C.c_int64: "int64_t"}
    for fn in api.EXPORTS_SCALE:
        args = re.search(r"int\s+" + fn + r"\s*\((.*?)\)\s*;", hdr, re.S).group(1).split(",")
        types = [re.sub(r"\bconst\b|\*.*$", "", a).strip() for a in args]
        assert types == ["sqg_ctx_t", "sqg_batch_t"] + [names[t] for t in table[fn]], fn
    assert os.path.join(ROOT, "include", "sqg_scale.h") in build.headers()
    for h in ("k_scale.h", "h_scale.h"):
        assert os.path.join(ROOT, "squigulator_amd", "csrc", h) in build.headers()


def test_the_built_libraries_export_both_calls():
    build.build()
    for lib in (build.LIB, build.LIB_DEV):
        L = api.load_library(lib)
        for n in api.EXPORTS_SCALE + api.EXPORTS_ALIGN:
            assert hasattr(L, n), f"{n} not exported by {lib}"


def test_the_cpu_backend_has_no_scale_and_says_so():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "libsqg_cpu.so"])
    prof, fl = profiles.get_profile("dna-r9-prom")
    mean, stdv = model.synthetic_model(6)
    gen = api.SignalGenerator(prof, fl, 6, mean, stdv, 42, lib_path=os.path.join(ROOT, "oracle", "libsqg_cpu.so"))
    for n in api.EXPORTS_SCALE:
        assert not hasattr(gen.L, n)
    b = gen.submit([b"ACGTACGTACGTTTGACA" * 40])
    with pytest.raises(api.SqgError) as e:
        b.scale(np.zeros(2, np.int64), None, None)
    assert e.value.code == -1 and "sqg_batch_scale" in str(e.value) and "sqg_scale.h" in str(e.value)
    b.free(); gen.close()


def test_hand_worked_reads():
    """typed out.  Rows that are the targets: (65536, 0) in both modes.  Rows = 2 targets + 3 under FIT: the exact inverse, gain 1/2 and
    shift -3/2 code = -384.  One row, constant rows: no variance, gain 1 and the shift the difference of the means.  The floor of a
    negative quotient, len <= 0 taken as 1, the clamps at +-2^20, the product modulo 2^64.  No rows, no targets, dropped rows"""
    lv = np.array([100, 300, 200, 500, -40], np.int16)
    ev_off = [0, 5]
    ones, ar = np.ones(5, np.int32), np.arange(5)
    for mode, ev in ((S.MOMENTS, None), (S.FIT, ar)):
        o = _both([0, 5], lv.astype(np.int64) * 7, ones * 7, ev_off, lv, mode, ev, "identity")
        assert (o["gain"][0], o["shift"][0]) == (65536, 0) and o["n"][0] == o["nx"][0] == 5
        assert o["sy"][0] == o["sx"][0] == 16 * 1060 and o["syy"][0] == o["sxx"][0] == 256 * (100 ** 2 + 300 ** 2 + 200 ** 2 + 500 ** 2 + 40 ** 2)
    assert o["sxy"][0] == o["sxx"][0] and o["rd_dropped"][0] == 0
    assert _both([0, 5], lv * 7, ones * 7, ev_off, lv, S.MOMENTS)["sxy"][0] == 0
    o = _both([0, 5], 2 * lv.astype(np.int64) + 3, ones, ev_off, lv, S.FIT, ar[::-1][::-1], "affine")
    assert (o["gain"][0], o["shift"][0]) == (32768, -384)
    o = _both([0, 5], (2 * lv.astype(np.int64) + 3)[::-1], ones, ev_off, lv, S.FIT, ar[::-1], "affine, any order")
    assert (o["gain"][0], o["shift"][0]) == (32768, -384)
    o = _both([0, 5], 2 * lv.astype(np.int64) + 3, ones, ev_off, lv, S.MOMENTS, None, "affine, moments")
    assert (o["gain"][0], o["shift"][0]) == (32768, -384)       # (the rows are all the targets: the moments see the same map)
    o = _both([0, 1], [250], [1], ev_off, lv, S.MOMENTS, None, "one row")
    assert (o["gain"][0], o["shift"][0]) == (65536, (212 - 250) * 256) and o["n"][0] == 1
    o = _both([0, 1], [250], [1], ev_off, lv, S.FIT, [3], "one row, fit")
    assert (o["gain"][0], o["shift"][0]) == (65536, (500 - 250) * 256) and o["n"][0] == o["nx"][0] == 1
    o = _both([0, 4], [90] * 4, [3] * 4, ev_off, lv, S.MOMENTS, None, "constant rows")
    assert (o["gain"][0], o["shift"][0]) == (65536, (212 - 30) * 256) and o["syy"][0] == 4 * 480 * 480
    # the row value
    assert [S.row_value(s, n) for s, n in ((-1, 256), (1, 256), (-256, 3), (7, 0), (5, -9), (-7, 2))] == [-1, 0, -1366, 112, 80, -56]
    assert S.row_value(1 << 16, 1) == 1 << 20 and S.row_value((1 << 16) + 1, 1) == 1 << 20 and S.row_value(-(1 << 16) - 1, 1) == -(1 << 20)
    assert S.row_value((1 << 55) - 1, 3) == 1 << 20 and S.row_value(-(1 << 58), (1 << 31) - 1) == -(1 << 20)
    assert S.row_value(1 << 60, 1) == 0 and S.row_value((1 << 60) + 5, 1) == 80 and S.row_value(I64_MIN, 1) == 0 and S.row_value((1 << 59) + 3, 1) == -(1 << 20)
    o = _both([0, 6], [-1, 1 << 60, (1 << 59) + 3, 7, -(1 << 62) - 9, I64_MIN], [256, 1, 1, 0, -3, 5], ev_off, lv, S.MOMENTS, None, "the row value")
    assert o["sy"][0] == -1 + 0 - (1 << 20) + 112 - 144 + 0
    # no rows, no targets, rows that are dropped
    o = _both([0, 0, 3], [10, 20, 30], [1, 1, 1], [0, 5, 5], lv, S.MOMENTS, None, "no rows / no targets")
    assert o["n"].tolist() == [0, 3] and o["nx"].tolist() == [5, 0] and o["gain"].tolist() == [65536] * 2 and o["shift"].tolist() == [0, 0] and o["sx"].tolist() == [16 * 1060, 0]
    o = _both([0, 4, 6], [100, 300, 1, 1, 5, 5], [1] * 6, [0, 3, 5], lv, S.FIT, [0, 1, -1, 3, 2, 4], "dropped")
    assert o["rd_dropped"].tolist() == [2, 1] and o["n"].tolist() == [2, 1] and o["sx"].tolist() == [16 * 400, -16 * 40]
    o = _both([0, 0, 0], [], [], [0, 3, 5], lv, S.FIT, [], "n_rows == 0")
    assert all(o[k].tolist() == [0, 0] for k in OUT if k != "gain") and o["gain"].tolist() == [65536] * 2
    # the estimate's clamps: a variance of the rows far below the targets', and far above
    assert S.estimate(S.MOMENTS, 2, 2, 0, 2, 0, 2 << 40, 0) == (16 * 65536, 0) and S.estimate(S.MOMENTS, 2, 2, 0, 2 << 40, 0, 2, 0) == (1, 0)
    assert S.estimate(S.FIT, 2, 2, 0, 2, 16 << 40, 1 << 62, -2)[0] == 1 and S.estimate(S.FIT, 2, 2, 0, 2, 16 << 40, 1 << 62, -2)[1] == 1 << 26
    # the scaled row values: the floor of the Q16 product, the clamps of q0, gain, shift and q
    assert S.scaled_values([5, -5, 1 << 40, 7], [2, 2, 1, 1], 65536, 0) == [640, -640, 1 << 26, 1792]
    assert S.scaled_values([-1, 1], [256, 256], 32768, 0) == [-1, 0] and S.scaled_values([3], [1], 1, 0) == [0] and S.scaled_values([-3], [1], 0, 0) == [-1]
    assert S.scaled_values([1 << 40], [1], 1 << 21, 5) == [1 << 26] and S.scaled_values([100], [1], 1 << 21, -9) == [(100 * 256 << 4) - 9]
    assert S.scaled_values([0, -(1 << 40)], [1, 1], 65536, 1 << 27) == [1 << 26, 0] and S.scaled_values([0], [1], 7, -(1 << 30)) == [-(1 << 26)]


def _drawn_batch(rng, n_reads, wild):
    T = rng.integers(0, 40, n_reads)
    m = rng.integers(0, 60, n_reads)
    ev_off, row_off = _offsets(T), _offsets(m)
    level = rng.integers(-3000, 3000, int(ev_off[-1])).astype(np.int16)
    lens = rng.integers(-2 if wild else 1, 70, int(row_off[-1])).astype(np.int32)
    sums = rng.integers(-(1 << 12), 1 << 12, int(row_off[-1])) * np.maximum(lens, 1) + rng.integers(-30, 30, int(row_off[-1]))
    if wild:
        big = rng.random(len(sums)) < 0.1
        sums = np.where(big, rng.integers(I64_MIN, (1 << 63) - 1, len(sums)), sums)
    rd = np.repeat(np.arange(n_reads), m)
    ev = ev_off[rd] + rng.integers(0, np.maximum(T[rd], 1))
    ev = np.where(rng.random(len(ev)) < 0.15, rng.integers(-1, int(ev_off[-1]) + 2, len(ev)), ev)      # -1, another read's, past the batch
    return row_off, sums.astype(np.int64), lens, ev_off, level, ev.astype(np.int64)


def test_the_two_statements_agree_on_drawn_reads():
    rng = np.random.default_rng(11)
    seen = dict(dropped=0, off=0, clamp=0)
    for trial in range(300):
        row_off, sums, lens, ev_off, level, ev = _drawn_batch(rng, int(rng.integers(1, 6)), trial % 3 == 0)
        for mode in (S.MOMENTS, S.FIT):
            o = _both(row_off, sums, lens, ev_off, level, mode, ev, f"trial {trial} mode {mode}")
        seen["dropped"] += int(o["rd_dropped"].sum() > 0); seen["off"] += int((o["gain"] != 65536).any()); seen["clamp"] += int(((o["gain"] == 1 << 20) | (o["gain"] == 1) | (np.abs(o["shift"]) == 1 << 26)).any())
    assert seen["dropped"] > 100 and seen["off"] > 200 and seen["clamp"] > 3, seen


def _past_2_53():
    """three reads whose sums of squares leave the doubles' exact integers: 16384 rows at the clamp drive syy to 2^54; two rows more make it
    2^54 + 5 (rounds down to + 4), 2^54 + 10 (a tie: half to even, + 8) and, with half the rows at the lower clamp, the same around a mean of 0"""
    top = 1 << 16                               # sum / len of a row at y = 2^20
    parts = [[top] * 16384 + [0, 0], [top] * 16384 + [0, 0], [top, -top] * 8192 + [0, 0]]
    small = [(1, 2), (1, 3), (1, 3)]            # sixteenths of a code: sum = y, len = 16
    sums, lens = [], []
    for p, (u, v) in zip(parts, small):
        sums += p; lens += [1] * 16384 + [16, 16]
        sums[-2], sums[-1] = u, v
    level = np.array([100, 300, 200, 500] * 3, np.int16)
    return _offsets([16386] * 3), np.array(sums, np.int64), np.array(lens, np.int32), _offsets([4, 4, 4]), level


def test_sums_past_2_53():
    """(double) of a 64-bit sum is ONE rounding to nearest-even: both statements agree where syy is no exact double"""
    row_off, sums, lens, ev_off, level = _past_2_53()
    for mode in (S.MOMENTS, S.FIT):
        o = _both(row_off, sums, lens, ev_off, level, mode, np.repeat([1, 6, 11], 16386), "2^53")
        assert o["syy"].tolist() == [(1 << 54) + 5, (1 << 54) + 10, (1 << 54) + 10] and all(float(v) != v for v in o["syy"].tolist())
    assert float((1 << 54) + 10) == (1 << 54) + 8 and float((1 << 54) + 5) == (1 << 54) + 4


_loop = {}


def _loop_reference():
    """the loop on the reference alone, from the oracle's signal of r10_t1's first three reads (made once): detect_ref's rows under
    SQG_DETECT_DNA, miscalibrated by LOOP_GAIN / LOOP_OFFSET; align_ref on them as they stand; scale_ref's MOMENTS -> align -> FIT -> align"""
    if not _loop:
        o = options.parse_args(dict(REFVEC_CASES)["r10_t1"])
        k = o.kmer_size_default
        level = model.synthetic_model(k)[0]
        reads = _fixture_reads("r10_t1")[:3]
        sps, rng, dig = int(o.profile.dwell_mean), o.profile.range, o.profile.digitisation
        t = EV.batch_events(reads, level, k, False, False, False, sps, "pa", False, rng, dig)
        dt = D.batch_rows(reads, D.DNA, k, False, False, sps, "pa", False, rng, dig)
        ev_off = _offsets([len(r["ss"]) for r in reads])
        off, lens, lv, cfg = dt["det_off"], dt["dt_len"], t["level_raw"], api.ALIGN_DEFAULT
        sums = np.rint(LOOP_GAIN * dt["sum"]).astype(np.int64) + LOOP_OFFSET * lens.astype(np.int64)
        plain = A.batch(off, sums, lens, ev_off, lv, False, cfg)
        mom = _both(off, sums, lens, ev_off, lv, S.MOMENTS, None, "loop, moments")
        al1 = S.align_scaled(off, sums, lens, ev_off, lv, False, cfg, mom["gain"], mom["shift"])
        fit = _both(off, sums, lens, ev_off, lv, S.FIT, al1["al_ev"], "loop, fit")
        al2 = S.align_scaled(off, sums, lens, ev_off, lv, False, cfg, fit["gain"], fit["shift"])
        share = lambda al: float((al["al_ev"] == dt["true_ev"]).mean())      # noqa: E731
        _loop.update(reads=reads, dt=dt, ev_off=ev_off, level=lv, sums=sums, plain=plain, mom=mom, al1=al1, fit=fit, al2=al2,
                     shares=(share(plain), share(al1), share(al2)))
    return _loop


def test_the_loop_on_the_reference():
    """r10_t1, rows of gain 1.15 and offset 40 codes, SQG_ALIGN_DEFAULT.  The reference's shares of al_ev == true_ev over the 11151 rows:
        the plain aligner on the miscalibrated rows       0.001255
        scaled by MOMENTS                                 0.956596
        scaled by FIT over that alignment                 0.959286
    (the plain aligner on the untouched rows: 0.960183).  The estimates invert the injection: gain about 1 / 1.15, shift about -40 / 1.15"""
    L = _loop_reference()
    plain, moments, fit = L["shares"]
    assert len(L["dt"]["sum"]) == 11151 and (round(plain, 6), round(moments, 6), round(fit, 6)) == (0.001255, 0.956596, 0.959286)
    assert fit > plain and moments > plain
    for est in (L["mom"], L["fit"]):
        assert (np.abs(est["gain"] / 65536 - 1 / LOOP_GAIN) < 0.02).all() and (np.abs(est["shift"] / 256 + LOOP_OFFSET / LOOP_GAIN) < 8).all()


# ---------------------------------------------------------------------------------------------------------- GPU
def _dev(b):
    return torch.device("cuda", b.gen.device)


def _on(b, a, dt):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dt)).to(_dev(b))


def _scale(b, row_off, sums, lens, ev=None, mode=None, outputs=None):
    ch = b.scale(row_off, _on(b, sums, np.int64), _on(b, lens, np.int32), _on(b, ev, np.int64), mode=mode, outputs=outputs)
    return {n: (None if getattr(ch, n) is None else getattr(ch, n).cpu().numpy()) for n in OUT}


def _same(got, want, what):
    for key in OUT:
        g, w = got[key], want[key]
        assert g.shape == w.shape and g.dtype == w.dtype, f"{what}: {key} {g.shape} {g.dtype} vs {w.shape} {w.dtype}"
        np.testing.assert_array_equal(g, w, err_msg=f"{what}: {key}")


def _check(b, row_off, sums, lens, level, ev=None, what="", slow=True):
    """both modes (FIT when ev is given) against the statements -> {mode: the reference's outputs}"""
    out = {}
    for name, mode in MODES.items():
        if mode == S.FIT and ev is None:
            continue
        e = ev if mode == S.FIT else None
        want = _both(row_off, sums, lens, b.ev_off, level, mode, e, what) if slow else S.vectorised(row_off, sums, lens, b.ev_off, level, mode, e)
        _same(_scale(b, row_off, sums, lens, e, name), want, f"{what} {name}")
        out[name] = want
    return out


def _table(b):
    ev = b.events(outputs=("level_raw", "sum", "ev_len"))
    return ev.level_raw.cpu().numpy(), ev.sum.cpu().numpy(), ev.ev_len.cpu().numpy()


TRUTH = {"dna": "r10_t1", "rna_prefix": "rna004_prefix", "meth": "r9_meth_dense"}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TRUTH))
def test_truth_as_rows(name):
    """the true table's own sum / ev_len as the rows, ev = 0 .. n_events - 1, row_off = ev_off: both modes against the statements.  The
    samples carry noise, so the estimate (looked at on the reference) is near (65536, 0), not on it"""
    cid = TRUTH[name]
    o, k, gen = _context(dict(REFVEC_CASES)[cid], api.MODE_CERTIFIED)
    b = gen.stage([r["seq"] for r in _fixture_reads(cid)[:3]]).run().wait()
    level, sums, lens = _table(b)
    want = _check(b, b.ev_off, sums, lens, level, np.arange(b.n_events), name)
    for mode in MODES:
        assert (want[mode]["n"] == np.diff(b.ev_off)).all() and (want[mode]["rd_dropped"] == 0).all()
        if name != "rna_prefix":                            # (there the adaptor's samples are lowered by the level shift and level_raw is not: sqg_align.h)
            assert (np.abs(want[mode]["gain"] - 65536) < 6554).all() and (np.abs(want[mode]["shift"]) < 30 * 256).all(), (mode, want[mode]["gain"], want[mode]["shift"])
    b.free(); gen.close()


@pytest.mark.gpu
def test_noise_free_rows_give_the_identity():
    """--ideal-amp: every sample of an event is its level.  The premise, from Batch.events(): sum == ev_len * level_raw wherever an event
    has samples.  Then FIT over the true assignment is exactly (65536, 0), and sxy == sxx == syy"""
    o, k, gen = _context(dict(REFVEC_CASES)["r9_ideal_amp"], api.MODE_CERTIFIED)
    b = gen.stage([r["seq"] for r in _fixture_reads("r9_ideal_amp")]).run().wait()
    level, sums, lens = _table(b)
    assert (lens > 0).any() and (sums[lens > 0] == lens[lens > 0].astype(np.int64) * level[lens > 0]).all()
    keep = lens > 0                                         # an event without a sample is no row
    rd = np.repeat(np.arange(b.n_reads), np.diff(b.ev_off))
    row_off = _offsets(np.bincount(rd[keep], minlength=b.n_reads))
    want = _check(b, row_off, sums[keep], lens[keep], level, np.arange(b.n_events)[keep], "ideal-amp")
    assert (want["fit"]["gain"] == 65536).all() and (want["fit"]["shift"] == 0).all()
    assert (want["fit"]["sxy"] == want["fit"]["sxx"]).all() and (want["fit"]["sxx"] == want["fit"]["syy"]).all() and (want["fit"]["n"] > 100).all()
    b.free(); gen.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ("r10_t1", "rna004_prefix"))
def test_detected_rows(cid):
    """sqg_batch_detect's rows with true_ev and with sqg_batch_align's al_ev, some of them set to -1; with ev shuffled within the reads
    (rows and ev together: the sums are the same, the rule is order-free); with ev pointing into the next read (dropped and counted)"""
    o, k, gen = _context(dict(REFVEC_CASES)[cid], api.MODE_CERTIFIED)
    rna = bool(o.flags & profiles.SQ_RNA)
    b = gen.stage([r["seq"] for r in _fixture_reads(cid)[:3]]).run().wait()
    level, _, _ = _table(b)
    dt = b.detect("rna" if rna else "dna", outputs=("sum", "dt_len", "true_ev"))
    al = b.align(dt.det_off, dt.sum, dt.dt_len, CFG, outputs=("al_ev",))
    off, sums, lens = dt.det_off, dt.sum.cpu().numpy(), dt.dt_len.cpu().numpy()
    true_ev, al_ev = dt.true_ev.cpu().numpy(), al.al_ev.cpu().numpy().copy()
    want = _check(b, off, sums, lens, level, true_ev, f"{cid} true_ev")
    assert (want["fit"]["rd_dropped"] == 0).all() and (want["fit"]["n"] == np.diff(off)).all()
    al_ev[::7] = -1
    w2 = _check(b, off, sums, lens, level, al_ev, f"{cid} al_ev")
    assert (w2["fit"]["rd_dropped"] > 0).all()
    rng = np.random.default_rng(2)
    perm = np.concatenate([off[r] + rng.permutation(int(off[r + 1] - off[r])) for r in range(b.n_reads)])
    w3 = _check(b, off, sums[perm], lens[perm], level, al_ev[perm], f"{cid} shuffled")
    for mode in w3:
        for key in OUT:
            np.testing.assert_array_equal(w3[mode][key], w2[mode][key], err_msg=f"{cid}: {key} depends on the order of the rows")
    only_ev = _check(b, off, sums, lens, level, np.concatenate([rng.permutation(al_ev[off[r]:off[r + 1]]) for r in range(b.n_reads)]), f"{cid} ev alone shuffled")
    assert (only_ev["fit"]["n"] == w2["fit"]["n"]).all() and (only_ev["fit"]["sx"] == w2["fit"]["sx"]).all() and (only_ev["fit"]["sxx"] == w2["fit"]["sxx"]).all()      # (other rows are dropped: sy may differ)
    other = true_ev.copy()
    rd = np.repeat(np.arange(b.n_reads), np.diff(off))
    other[::5] = b.ev_off[(rd[::5] + 1) % b.n_reads]        # the first event of the next read
    w4 = _check(b, off, sums, lens, level, other, f"{cid} another read's events")
    assert w4["fit"]["rd_dropped"].tolist() == np.bincount(rd[::5], minlength=b.n_reads).tolist()
    b.free(); gen.close()


def _geometry(counts, seed=3, lib_path=None):
    """a DNA batch of reads with the given numbers of events, one sample per event (inject's exact1), and its level_raw"""
    gen, prof, fl, k = inject.context("exact1", lib_path=lib_path)
    b = inject.run_geometry(gen, inject.seqs_for([t + k - 1 for t in counts], seed))
    assert np.diff(b.ev_off).tolist() == list(counts)
    return gen, b, _table(b)[0]


def _made_up_rows(rng, b, level, m):
    """m[r] rows of read r: near the level of an event of the read, drawn lengths, and that event (one in twenty -1, one in twenty any index around the batch's events)"""
    row_off = _offsets(m)
    rd = np.repeat(np.arange(b.n_reads), m)
    T = np.diff(b.ev_off)
    ev = b.ev_off[rd] + rng.integers(0, T[rd])
    lens = rng.integers(1, 40, len(rd)).astype(np.int32)
    sums = (level[ev].astype(np.int64) * 23 // 20 + 35) * lens + rng.integers(-60, 60, len(rd))
    u = rng.random(len(ev))
    ev = np.where(u < 0.05, -1, np.where(u < 0.1, rng.integers(-1, b.n_events + 3, len(ev)), ev))
    return row_off, sums.astype(np.int64), lens, ev.astype(np.int64)


@pytest.mark.gpu
@pytest.mark.parametrize("n_reads", [1, 63, 64, 65, 130])
def test_batch_shapes(n_reads):
    """batches of 1 to 130 reads of 1 to 400 events with 0 to 200 rows each: read boundaries fall anywhere in a wavefront's 64 rows"""
    rng = np.random.default_rng(n_reads)
    counts = ([400, 1] + rng.integers(1, 150, max(n_reads - 2, 0)).tolist())[:n_reads]
    gen, b, level = _geometry(counts, seed=n_reads)
    m = rng.integers(0, 200, n_reads)
    m[0] = 300
    row_off, sums, lens, ev = _made_up_rows(rng, b, level, m)
    want = _check(b, row_off, sums, lens, level, ev, f"{n_reads} reads")
    assert want["fit"]["rd_dropped"].sum() > 0 and (want["fit"]["gain"] != 65536).any()
    b.free(); gen.close()


@pytest.mark.gpu
def test_read_shapes():
    """reads of 0, 1, 2, 63, 64, 65 and 129 rows in both orders, a read without rows first and last; then 200 reads of 1 .. 3 rows, dozens
    of read segments in one wavefront; a read shorter than a k-mer (its targets are the five stand-in events: every staged read has
    targets, the statements alone cover T == 0); no row at all"""
    rng = np.random.default_rng(6)
    ms = [0, 1, 2, 63, 64, 65, 129]
    gen, b, level = _geometry([40] * (2 * len(ms) + 1))
    row_off, sums, lens, ev = _made_up_rows(rng, b, level, np.array(ms + ms[::-1] + [0]))
    _check(b, row_off, sums, lens, level, ev, "rows per read")
    zero = np.zeros(b.n_reads + 1, np.int64)
    for name, mode in MODES.items():
        got = _scale(b, zero, sums[:0], lens[:0], ev[:0] if mode else None, name)
        _same(got, _both(zero, sums[:0], lens[:0], b.ev_off, level, mode, ev[:0]), f"no rows {name}")
        assert all((got[k] == 0).all() for k in OUT if k != "gain") and (got["gain"] == 65536).all()
    b.free(); gen.close()
    gen, b, level = _geometry([3] * 200)
    m = rng.integers(1, 4, 200)
    row_off, sums, lens, ev = _made_up_rows(rng, b, level, m)
    assert (np.diff(np.searchsorted(row_off, np.arange(0, row_off[-1], 64))) >= 20).all()       # read boundaries per 64 rows
    _check(b, row_off, sums, lens, level, ev, "many short reads")
    b.free(); gen.close()
    gen, prof, fl, k = inject.context("drawn")
    b = gen.stage([inject.seqs_for([200])[0], b"ACG", inject.seqs_for([90])[0]]).run().wait()
    assert 3 < k and b.ev_off[2] - b.ev_off[1] == 5
    level = _table(b)[0]
    row_off, sums, lens, ev = _made_up_rows(rng, b, level, np.array([70, 9, 30]))
    _check(b, row_off, sums, lens, level, ev, "a read shorter than a k-mer")
    b.free(); gen.close()


@pytest.mark.gpu
def test_the_second_trip(monkeypatch):
    """k_scale_sums' grid is capped and a wavefront owns consecutive trips.  The development library takes the cap from
    SQG_TEST_SCALE_GRID: with one workgroup (four wavefronts, 256 rows per trip of the grid) 3000 rows over reads of 1 to 700 rows give
    every wavefront a dozen trips -- accumulators kept over trips inside a read, flushed where the read changes, trips with boundaries
    in them -- and the targets' pass the same.  The release library on the same rows gives the same bytes"""
    build.build()
    counts = [700, 3, 500, 1, 2, 650, 40, 64, 300]
    m = np.array([700, 1, 2, 0, 64, 640, 63, 130, 0])
    m[-1] = 3000 - m.sum()
    got = {}
    for lib in (build.LIB_DEV, build.LIB):
        monkeypatch.setenv("SQG_TEST_SCALE_GRID", "1")
        gen, b, level = _geometry(counts, lib_path=lib)
        row_off, sums, lens, ev = _made_up_rows(np.random.default_rng(9), b, level, m)
        assert row_off[-1] == 3000 > 4 * WG and b.n_events > 4 * WG and ((row_off[1:-1] % 64) != 0).any()
        got[lib] = _check(b, row_off, sums, lens, level, ev, f"second trip {os.path.basename(lib)}")
        b.free(); gen.close()
    assert (got[build.LIB]["fit"]["n"] > 0).sum() >= 6


@pytest.mark.gpu
def test_adversarial_rows():
    """len <= 0, |sum| up to 2^55 and far beyond (the product wraps, the header says how), rows that all sit on one clamp, events of
    any read: the outputs against the statements, and guard values around every output untouched"""
    gen, b, level = _geometry([3, 32, 90, 200])
    rng = np.random.default_rng(4)
    m = np.array([50, 64, 130, 200])
    rd = np.repeat(np.arange(4), m)
    n_rows = int(m.sum())
    ev_in = (b.ev_off[rd] + rng.integers(0, np.diff(b.ev_off)[rd])).astype(np.int64)
    cases = {
        "len of 0 and below": (rng.integers(-4000, 4000, n_rows), rng.integers(-3, 1, n_rows), ev_in),
        "len of 2^31 - 1": (rng.integers(-(1 << 54), 1 << 54, n_rows), np.full(n_rows, (1 << 31) - 1), ev_in),
        "sums to 2^55": (np.where(np.arange(n_rows) & 1, (1 << 55) - 1, -(1 << 55) + 1), np.where(np.arange(n_rows) & 2, 1, 3), ev_in),
        "sums beyond": (rng.choice([1 << 59, (1 << 59) + 3, 1 << 60, (1 << 60) + 5, -(1 << 62) - 9, I64_MIN, (1 << 63) - 1, -(1 << 59)], n_rows), rng.integers(1, 9, n_rows), ev_in),
        "any 64 bits": (rng.integers(I64_MIN, (1 << 63) - 1, n_rows), rng.integers(-(1 << 31), (1 << 31) - 1, n_rows), rng.integers(I64_MIN, (1 << 63) - 1, n_rows)),
        "one clamp": (np.full(n_rows, 1 << 50), np.ones(n_rows), ev_in),
    }
    G = 16
    dev = _dev(b)
    size = {k: np.dtype(S.DTYPES[k]).itemsize for k in OUT}
    tdt = {k: torch.int32 if size[k] == 4 else torch.int64 for k in OUT}
    for name, (sums, lens, ev) in cases.items():
        sums, lens, ev = np.asarray(sums, np.int64), np.asarray(lens, np.int64).astype(np.int32), np.asarray(ev, np.int64)
        row_off = _offsets(m)
        want = _check(b, row_off, sums, lens, level, ev, name)
        s, n, e = _on(b, sums, np.int64), _on(b, lens, np.int32), _on(b, ev, np.int64)
        for mode, key in ((api.SCALE_MOMENTS, "moments"), (api.SCALE_FIT, "fit")):
            bufs = {k: torch.full((b.n_reads + 2 * G,), -77, dtype=tdt[k], device=dev) for k in OUT}
            out = api.CScaleOut(*(bufs[k].data_ptr() + G * size[k] for k in OUT))
            torch.cuda.synchronize(dev)
            assert gen.L.sqg_batch_scale(gen.ctx, b.handle, C.byref(api.CScaleCfg(mode)), row_off.ctypes.data_as(C.POINTER(C.c_int64)),
                                         C.byref(api.CScaleIn(s.data_ptr(), n.data_ptr(), e.data_ptr())), C.byref(out)) == 0
            for k in OUT:
                g = bufs[k].cpu().numpy()
                np.testing.assert_array_equal(g[G:-G], want[key][k], err_msg=f"{name} {key}: {k}")
                assert (g[:G] == -77).all() and (g[-G:] == -77).all(), f"{name} {key}: {k} written outside its reads"
    assert (want["moments"]["gain"] == 65536).all() and (want["moments"]["shift"] == (np.rint((want["moments"]["sx"] / want["moments"]["nx"] - (1 << 20)) * 16)).astype(np.int32)).all()
    b.free(); gen.close()


@pytest.mark.gpu
def test_sums_past_2_53_and_sums_that_wrap():
    """the reads of test_sums_past_2_53 on the device: the conversion of a 64-bit sum to double is one rounding there too.  Then one read of
    2^24 + 5 rows on the upper clamp: syy = (2^24 + 5) 2^40 wraps modulo 2^64 to 5 * 2^40, as the header says, and gain / shift are the
    header's expressions on the wrapped value"""
    row_off, sums, lens, ev_off, level = _past_2_53()
    gen, prof, fl, k = inject.context("exact1")
    b = inject.run_geometry(gen, inject.seqs_for([4 + k - 1] * 3))
    lv = _table(b)[0]
    assert (b.ev_off == ev_off).all()
    ev = np.repeat([1, 6, 11], 16386)
    want = _check(b, row_off, sums, lens, lv, ev, "2^53")
    assert want["moments"]["syy"].tolist() == [(1 << 54) + 5, (1 << 54) + 10, (1 << 54) + 10]
    b.free()
    b = inject.run_geometry(gen, inject.seqs_for([4 + k - 1]))
    lv = _table(b)[0].astype(np.int64)
    m = (1 << 24) + 5
    dev = _dev(b)
    ch = b.scale(np.array([0, m], np.int64), torch.full((m,), 1 << 40, dtype=torch.int64, device=dev), torch.ones(m, dtype=torch.int32, device=dev))
    sy, syy, sx, sxx = m << 20, S._wrap(m << 40), int(16 * lv.sum()), int(256 * (lv * lv).sum())
    assert syy == 5 << 40
    gain, shift = S.estimate(S.MOMENTS, m, 4, sy, syy, sx, sxx, 0)
    got = {key: int(getattr(ch, key).cpu()[0]) for key in OUT}
    assert got == dict(n=m, nx=4, sy=sy, syy=syy, sx=sx, sxx=sxx, sxy=0, gain=gain, shift=shift, rd_dropped=0), got
    b.free(); gen.close()


def _aligned(al):
    return {k: (None if getattr(al, k) is None else getattr(al, k).cpu().numpy()) for k in AOUT}


def _align_scaled(b, row_off, sums, lens, cfg, gain, shift, outputs=None):
    return b.align(row_off, _on(b, sums, np.int64), _on(b, lens, np.int32), cfg, outputs, scale=(_on(b, gain, np.int32), _on(b, shift, np.int32)))


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ("r10_t1", "rna004_prefix"))
def test_the_identity_scaling_is_the_plain_aligner(cid):
    """gain 65536, shift 0 on detected rows: all three outputs bit-equal to sqg_batch_align's, together and each wanted alone"""
    o, k, gen = _context(dict(REFVEC_CASES)[cid], api.MODE_CERTIFIED)
    rna = bool(o.flags & profiles.SQ_RNA)
    b = gen.stage([r["seq"] for r in _fixture_reads(cid)[:3]]).run().wait()
    dt = b.detect("rna" if rna else "dna", outputs=("sum", "dt_len"))
    one = (torch.full((b.n_reads,), 65536, dtype=torch.int32, device=_dev(b)), torch.zeros(b.n_reads, dtype=torch.int32, device=_dev(b)))
    for cfg in (CFG, api.ALIGN_DEFAULT):
        plain = b.align(dt.det_off, dt.sum, dt.dt_len, cfg)
        for names in [None] + [(key,) for key in AOUT]:
            got = b.align(dt.det_off, dt.sum, dt.dt_len, cfg, names, scale=one)
            for key in AOUT:
                g = getattr(got, key)
                assert (g is None) == (names is not None and key not in names) and (g is None or torch.equal(g, getattr(plain, key))), (cfg, names, key)
    b.free(); gen.close()


@pytest.mark.gpu
def test_scaled_rows_against_the_reference():
    """drawn (gain, shift) per read, the ends of both ranges and values outside them (clamped), on detected rows of r10_t1 and on made-up
    rows with huge and negative sums; then rows under sum' = 2 sum + 3 len with the exactly inverse scaling (32768, -384): q is
    floor((512 v + 768) / 2) - 384 = 256 v = the plain call's wherever 256 v is an integer; the reference decides, the device equals it"""
    cid = "r10_t1"
    o, k, gen = _context(dict(REFVEC_CASES)[cid], api.MODE_CERTIFIED)
    b = gen.stage([r["seq"] for r in _fixture_reads(cid)[:2]]).run().wait()
    level = _table(b)[0]
    nr = b.n_reads
    dt = b.detect("dna", outputs=("sum", "dt_len"))
    off, sums, lens = dt.det_off, dt.sum.cpu().numpy(), dt.dt_len.cpu().numpy()
    rng = np.random.default_rng(3)
    scalings = [(rng.integers(52000, 82000, nr), rng.integers(-15000, 15000, nr)), ([1, 1 << 20], [0, -(1 << 26)]), ([65536, 70000], [1 << 26, -(1 << 26)]),
                ([0, (1 << 20) + 1], [(1 << 26) + 1, -(1 << 26) - 1]), ([(1 << 31) - 1, -(1 << 31)], [(1 << 31) - 1, -(1 << 31)]), ([-5, 300], [3, 70000])]
    for gain, shift in scalings:
        gain, shift = np.asarray(gain, np.int64).astype(np.int32), np.asarray(shift, np.int64).astype(np.int32)
        want = S.align_scaled(off, sums, lens, b.ev_off, level, False, CFG, gain, shift)
        got = _aligned(_align_scaled(b, off, sums, lens, CFG, gain, shift))
        for key in AOUT:
            np.testing.assert_array_equal(got[key], want[key], err_msg=f"{gain} {shift}: {key}")
    wild = np.where(rng.random(len(sums)) < 0.2, rng.choice([-(1 << 54), 1 << 54, -1, 0, (1 << 40) + 7, -(1 << 33)], len(sums)), -sums)
    wlen = rng.integers(-2, 50, len(sums)).astype(np.int32)
    for gain, shift in scalings[:4]:
        gain, shift = np.asarray(gain, np.int64).astype(np.int32), np.asarray(shift, np.int64).astype(np.int32)
        want = S.align_scaled(off, wild, wlen, b.ev_off, level, False, (0, 1 << 24, 1 << 24), gain, shift)
        got = _aligned(_align_scaled(b, off, wild, wlen, (0, 1 << 24, 1 << 24), gain, shift))
        for key in AOUT:
            np.testing.assert_array_equal(got[key], want[key], err_msg=f"wild {gain} {shift}: {key}")
    # the exact affine map and its inverse
    s2 = 2 * sums + 3 * lens.astype(np.int64)
    half, back = np.full(nr, 32768, np.int32), np.full(nr, -384, np.int32)
    want = S.align_scaled(off, s2, lens, b.ev_off, level, False, CFG, half, back)
    got = _aligned(_align_scaled(b, off, s2, lens, CFG, half, back))
    plain = _aligned(b.align(off, dt.sum, dt.dt_len, CFG))
    for key in AOUT:
        np.testing.assert_array_equal(got[key], want[key], err_msg=f"affine: {key}")
    q_plain = np.array(A.row_values(sums, lens))
    q_back = np.concatenate([S.scaled_values(s2[off[r]:off[r + 1]], lens[off[r]:off[r + 1]], 32768, -384) for r in range(nr)])
    assert (np.abs(q_back - q_plain) <= 1).all() and (q_back == q_plain).mean() > 0.1        # the header's arithmetic: a floor apart at the most
    exact = [r for r in range(nr) if (q_back[off[r]:off[r + 1]] == q_plain[off[r]:off[r + 1]]).all()]
    for r in exact:                                         # (where every q agrees the alignment must: the reference has decided which reads)
        np.testing.assert_array_equal(got["al_ev"][off[r]:off[r + 1]], plain["al_ev"][off[r]:off[r + 1]])
    est = _scale(b, off, s2, lens, plain["al_ev"], "fit", ("gain", "shift"))
    assert (np.abs(est["gain"] - 32768) < 700).all() and (np.abs(est["shift"] + 384) < 3000).all()       # the fit over the plain alignment finds the inverse
    b.free(); gen.close()


@pytest.mark.gpu
def test_the_loop():
    """moments -> align -> fit -> align on the device, on r10_t1's detected rows miscalibrated by gain 1.15 and offset 40: the device
    equals the reference at every step (test_the_loop_on_the_reference holds its shares: 0.001255, 0.956596, 0.959286), and al_ev ==
    true_ev is more frequent after the loop than under the plain aligner on the same rows.  No row leaves the device between the steps"""
    L = _loop_reference()
    o, k, gen = _context(dict(REFVEC_CASES)["r10_t1"], api.MODE_CERTIFIED)
    b = gen.stage([r["seq"] for r in L["reads"]]).run().wait()
    dt = b.detect("dna", outputs=("sum", "dt_len", "true_ev"))
    assert (dt.det_off == L["dt"]["det_off"]).all() and np.array_equal(dt.sum.cpu().numpy(), L["dt"]["sum"]) and np.array_equal(dt.true_ev.cpu().numpy(), L["dt"]["true_ev"])
    sums = torch.from_numpy(L["sums"]).to(_dev(b))
    cfg = api.ALIGN_DEFAULT
    same = lambda got, want, keys, what: [np.testing.assert_array_equal(getattr(got, key).cpu().numpy(), want[key], err_msg=f"{what}: {key}") for key in keys]      # noqa: E731
    plain = b.align(dt.det_off, sums, dt.dt_len, cfg)
    same(plain, L["plain"], AOUT, "plain")
    mom = b.scale(dt.det_off, sums, dt.dt_len)
    same(mom, L["mom"], OUT, "moments")
    al1 = b.align(dt.det_off, sums, dt.dt_len, cfg, scale=(mom.gain, mom.shift))
    same(al1, L["al1"], AOUT, "aligned under moments")
    fit = b.scale(dt.det_off, sums, dt.dt_len, al1.al_ev)
    same(fit, L["fit"], OUT, "fit")
    al2 = b.align(dt.det_off, sums, dt.dt_len, cfg, scale=(fit.gain, fit.shift))
    same(al2, L["al2"], AOUT, "aligned under the fit")
    share = lambda al: float((al.al_ev == dt.true_ev).double().mean())      # noqa: E731
    print(f"al_ev == true_ev: plain {share(plain):.6f}, moments {share(al1):.6f}, fit {share(al2):.6f}")
    assert share(al2) > share(plain)
    b.free(); gen.close()


def _raw_scale(gen, b, cfg, row_off, cin, out):
    ptr = lambda x: C.byref(x) if x is not None else None   # noqa: E731
    off = row_off.ctypes.data_as(C.POINTER(C.c_int64)) if row_off is not None else None
    return gen.L.sqg_batch_scale(gen.ctx, b.handle if b is not None else None, ptr(cfg), off, ptr(cin), ptr(out))


def _raw_align(gen, b, cfg, row_off, cin, sc, out):
    ptr = lambda x: C.byref(x) if x is not None else None   # noqa: E731
    off = row_off.ctypes.data_as(C.POINTER(C.c_int64)) if row_off is not None else None
    return gen.L.sqg_batch_align_scaled(gen.ctx, b.handle if b is not None else None, ptr(cfg), off, ptr(cin), ptr(sc), ptr(out))


@pytest.mark.gpu
def test_interface():
    """a batch that has not been run; every SQG_EINVAL of the header with the field in sqg_last_error, for both calls; each output alone
    and none; the binding's own refusals; an empty batch; the batch after free()"""
    gen, prof, fl, k = inject.context("exact1")
    counts = [70, 5, 300]
    b = gen.stage(inject.seqs_for([t + k - 1 for t in counts]))
    dev = _dev(b)
    err = lambda: gen.L.sqg_last_error(gen.ctx)             # noqa: E731
    off0 = np.array([0, 1, 2, 3], np.int64)
    one = torch.zeros(8, dtype=torch.int64, device=dev)
    cin, none, cfg = api.CScaleIn(one.data_ptr(), one.data_ptr(), one.data_ptr()), api.CScaleOut(), api.CScaleCfg(api.SCALE_FIT)
    ain, anone, acfg, asc = api.CAlignIn(one.data_ptr(), one.data_ptr()), api.CAlignOut(), api.CAlignCfg(*CFG), api.CAlignScale(one.data_ptr(), one.data_ptr())
    assert _raw_scale(gen, b, cfg, off0, cin, none) == -4 and b"sqg_batch_scale" in err() and b"not been run" in err()
    assert _raw_align(gen, b, acfg, off0, ain, asc, anone) == -4 and b"sqg_batch_align_scaled" in err() and b"not been run" in err()
    with pytest.raises(api.SqgError) as e:
        b.scale(off0, one, one[:4].to(torch.int32))
    assert e.value.code == -4 and "not been run" in str(e.value)
    b.run().wait()
    level = _table(b)[0]
    rng = np.random.default_rng(1)
    row_off, sums, lens, ev = _made_up_rows(rng, b, level, np.array([90, 7, 200]))
    s, n, e_ = _on(b, sums, np.int64), _on(b, lens, np.int32), _on(b, ev, np.int64)
    cin = api.CScaleIn(s.data_ptr(), n.data_ptr(), e_.data_ptr())
    ain = api.CAlignIn(s.data_ptr(), n.data_ptr())
    # each output alone, a few together, and none; a second call gives the same bytes
    for name, mode in MODES.items():
        full = _scale(b, row_off, sums, lens, ev if mode else None, name)
        _same(full, _both(row_off, sums, lens, b.ev_off, level, mode, ev), f"interface {name}")
        _same(_scale(b, row_off, sums, lens, ev if mode else None, name), full, f"second call {name}")
        for names in [(key,) for key in OUT] + [("gain", "shift"), ("sxy", "n", "rd_dropped"), ()]:
            part = _scale(b, row_off, sums, lens, ev if mode else None, name, outputs=names)
            for key in OUT:
                assert (part[key] is None) == (key not in names) and (part[key] is None or np.array_equal(part[key], full[key])), (name, names, key)
    assert _raw_scale(gen, b, cfg, row_off, cin, none) == 0
    # mode by name, by number and by default
    assert np.array_equal(b.scale(row_off, s, n, e_).sxy.cpu().numpy(), full["sxy"]) and (b.scale(row_off, s, n).sxy == 0).all()
    assert (b.scale(row_off, s, n, e_, mode="moments").sxy == 0).all() and np.array_equal(b.scale(row_off, s, n, e_, mode=1).sxy.cpu().numpy(), full["sxy"])
    # SQG_EINVAL, each with its message
    outb = {key: torch.zeros(3, dtype=torch.int32 if S.DTYPES[key] == np.int32 else torch.int64, device=dev) for key in OUT}
    out = api.CScaleOut(*(outb[key].data_ptr() for key in OUT))
    aoutb = dict(al_ev=torch.zeros(int(row_off[-1]), dtype=torch.int64, device=dev), al_cost=torch.zeros(3, dtype=torch.int64, device=dev), al_edge=torch.zeros(3, dtype=torch.int32, device=dev))
    aout = api.CAlignOut(*(aoutb[key].data_ptr() for key in AOUT))
    g32, s32 = torch.full((3,), 65536, dtype=torch.int32, device=dev), torch.zeros(3, dtype=torch.int32, device=dev)
    asc = api.CAlignScale(g32.data_ptr(), s32.data_ptr())
    torch.cuda.synchronize(dev)
    assert _raw_scale(gen, b, cfg, row_off, cin, out) == 0 and _raw_align(gen, b, acfg, row_off, ain, asc, aout) == 0
    assert _raw_scale(gen, b, api.CScaleCfg(2), row_off, cin, out) == -1 and b"sqg_batch_scale" in err() and b"unknown mode" in err()
    assert _raw_scale(gen, b, cfg, row_off, api.CScaleIn(s.data_ptr(), n.data_ptr(), None), out) == -1 and b"in->ev" in err()
    assert _raw_scale(gen, b, api.CScaleCfg(api.SCALE_MOMENTS), row_off, api.CScaleIn(s.data_ptr(), n.data_ptr(), None), out) == 0
    for bad_off, what in [(row_off + 1, b"start at 0"), (np.array([0, 5, 4, 9], np.int64), b"decrease"), (np.array([0, 2 ** 31, 2 ** 31, 2 ** 31], np.int64), b"2^31 rows")]:
        assert _raw_scale(gen, b, cfg, bad_off, cin, out) == -1 and b"sqg_batch_scale" in err() and b"row_off" in err() and what in err(), err()
        assert _raw_align(gen, b, acfg, bad_off, ain, asc, aout) == -1 and b"sqg_batch_align_scaled" in err() and b"row_off" in err() and what in err(), err()
    assert gen.L.sqg_batch_scale(None, None, None, None, None, None) == -1 and gen.L.sqg_batch_align_scaled(None, None, None, None, None, None, None) == -1
    assert _raw_scale(gen, None, cfg, row_off, cin, out) == -1 and b"sqg_batch_scale" in err() and b"batch" in err()
    assert _raw_scale(gen, b, None, row_off, cin, out) == -1 and b"sqg_batch_scale" in err() and b"cfg" in err()
    assert _raw_scale(gen, b, cfg, None, cin, out) == -1 and b"row_off must not be NULL" in err()
    assert _raw_scale(gen, b, cfg, row_off, None, out) == -1 and b"in must not be NULL" in err()
    assert _raw_scale(gen, b, cfg, row_off, api.CScaleIn(None, n.data_ptr(), e_.data_ptr()), out) == -1 and b"in->sum" in err()
    assert _raw_scale(gen, b, cfg, row_off, api.CScaleIn(s.data_ptr(), None, e_.data_ptr()), out) == -1 and b"in->len" in err()
    assert _raw_scale(gen, b, cfg, row_off, cin, None) == -1 and b"out must not be NULL" in err()
    assert _raw_align(gen, None, acfg, row_off, ain, asc, aout) == -1 and b"sqg_batch_align_scaled" in err() and b"batch" in err()
    assert _raw_align(gen, b, None, row_off, ain, asc, aout) == -1 and b"sqg_batch_align_scaled" in err() and b"cfg" in err()
    assert _raw_align(gen, b, acfg, None, ain, asc, aout) == -1 and b"row_off must not be NULL" in err()
    assert _raw_align(gen, b, acfg, row_off, None, asc, aout) == -1 and b"in must not be NULL" in err()
    assert _raw_align(gen, b, acfg, row_off, api.CAlignIn(None, n.data_ptr()), asc, aout) == -1 and b"in->sum" in err()
    assert _raw_align(gen, b, acfg, row_off, api.CAlignIn(s.data_ptr(), None), asc, aout) == -1 and b"in->len" in err()
    assert _raw_align(gen, b, acfg, row_off, ain, asc, None) == -1 and b"out must not be NULL" in err()
    assert _raw_align(gen, b, acfg, row_off, ain, None, aout) == -1 and b"scale must not be NULL" in err()
    assert _raw_align(gen, b, acfg, row_off, ain, api.CAlignScale(None, s32.data_ptr()), aout) == -1 and b"scale->gain" in err()
    assert _raw_align(gen, b, acfg, row_off, ain, api.CAlignScale(g32.data_ptr(), None), aout) == -1 and b"scale->shift" in err()
    assert _raw_align(gen, b, api.CAlignCfg(-1, 0, 1), row_off, ain, asc, aout) == -1 and b"sqg_batch_align_scaled" in err() and b"stay_pen" in err()
    # the binding's own refusals
    for bad in (dict(mode="least squares"), dict(outputs=("gain", "offset"))):
        with pytest.raises(api.SqgError) as e:
            b.scale(row_off, s, n, e_, **bad)
        assert e.value.code == -1 and "scale" in str(e.value), bad
    for bad in ((row_off[:-1], s, n), (row_off, s.to(torch.int32), n), (row_off, s, n.cpu()), (row_off, s[:5], n), (row_off, s, n, e_.to(torch.int32))):
        with pytest.raises(api.SqgError) as e:
            b.scale(*bad)
        assert e.value.code == -1 and "scale" in str(e.value)
    for bad in ((g32,), (g32, s32.to(torch.int64)), (g32[:2], s32), g32, (g32.cpu(), s32)):
        with pytest.raises(api.SqgError) as e:
            b.align(row_off, s, n, CFG, scale=bad)
        assert e.value.code == -1 and "scale" in str(e.value)
    with pytest.raises(api.SqgError) as e:                  # FIT asked for by name, without ev: the library says so
        b.scale(row_off, s, n, mode="fit")
    assert e.value.code == -1 and "in->ev" in str(e.value)
    b.free()
    for call in (lambda: b.scale(row_off, s, n), lambda: b.align(row_off, s, n, CFG, scale=(g32, s32))):      # the batch after free()
        with pytest.raises(api.SqgError) as e:
            call()
        assert e.value.code == -1 and "batch" in str(e.value)
    b = gen.submit([])                                      # an empty batch
    z64, z32 = torch.zeros(0, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int32, device=dev)
    sc = b.scale(np.zeros(1, np.int64), z64, z32, z64)
    assert sc.n_rows == 0 and all(tuple(getattr(sc, key).shape) == (0,) for key in OUT)
    al = b.align(np.zeros(1, np.int64), z64, z32, CFG, scale=(z32, z32))
    assert al.n_rows == 0 and all(tuple(getattr(al, key).shape) == (0,) for key in AOUT)
    b.free(); gen.close()


@pytest.mark.gpu
def test_lifetime():
    """a batch keeps both calls until two more batches have been run, then SQG_ESEQUENCE"""
    o, k, gen = _context(dict(REFVEC_CASES)["rna004_tk4"], api.MODE_EXACT)
    reads = _fixture_reads("rna004_tk4")
    parts = [[r["seq"] for r in reads[0:2]], [r["seq"] for r in reads[2:4]], [r["seq"] for r in reads[4:6]]]
    b0 = gen.stage(parts[0]).run().wait()
    level, sums, lens = _table(b0)
    ev = np.arange(b0.n_events)
    want = _check(b0, b0.ev_off, sums, lens, level, ev, "quiet", slow=False)
    gain, shift = want["fit"]["gain"], want["fit"]["shift"]
    idx = np.concatenate([np.arange(int(b0.ev_off[r]), int(b0.ev_off[r + 1]))[::-1] for r in range(b0.n_reads)])      # stored order: RNA
    al = S.align_scaled(b0.ev_off, sums[idx], lens[idx], b0.ev_off, level, True, CFG, gain, shift)
    b1, b2 = gen.stage(parts[1]), gen.stage(parts[2])
    b1.run().wait()
    _same(_scale(b0, b0.ev_off, sums, lens, ev), want["fit"], "after one more batch")
    got = _aligned(_align_scaled(b0, b0.ev_off, sums[idx], lens[idx], CFG, gain, shift))
    for key in AOUT:
        np.testing.assert_array_equal(got[key], al[key], err_msg=f"after one more batch: {key}")
    b2.run().wait()
    for call, who in ((lambda: _scale(b0, b0.ev_off, sums, lens, ev), "sqg_batch_scale"), (lambda: _align_scaled(b0, b0.ev_off, sums[idx], lens[idx], CFG, gain, shift), "sqg_batch_align_scaled")):
        with pytest.raises(api.SqgError) as e:
            call()
        assert e.value.code == -4 and who in str(e.value) and "handed to a later batch" in str(e.value)
    for b in (b0, b1, b2):
        b.free()
    gen.close()
