"""include/sqg_call.h: the CpG sites of a batch (sqg_call_plan) and their methylation calls scored from event rows (sqg_batch_call),
against the two plain statements of the header's rule (call_ref.py).  Every comparison is bit for bit: every output is an integer."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (before the library is loaded: the HIP runtime torch brings is the one the library then uses)

import call_cases as CS
import call_ref as R
import pileup_ref as PR
from chunk_support import _declared
from squigulator_amd import api, build, model, profiles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUTS = os.path.join(ROOT, "tests", "golden", "inputs")
NCOV = os.path.join(INPUTS, "nCoV-2019.reference.fasta")
MFREQ_DENSE = os.path.join(INPUTS, "mfreq_dense.tsv")
OUT = api.CALL_OUTPUTS
WG = 256            # k_chunks.h's CHUNK_WG: the sites of one workgroup and trip of k_call_score


# ---------------------------------------------------------------------------------------------------------- no GPU
def _struct_fields(hdr, struct):
    body = hdr[:hdr.index("} " + struct)]
    body = body[body.rindex("typedef struct"):]
    body = body[body.index("{") + 1:]
    return [re.sub(r"[\s*]", "", name) for decl in body.split(";") if decl.strip() for name in re.sub(r"^\s*(const\s+)?\w+\s", "", decl.strip()).split(",")]


def test_the_header_and_the_binding_agree():
    assert _declared("sqg_call.h") == set(api.EXPORTS_CALL) == {"sqg_call_plan", "sqg_batch_call"}
    others = set(api.EXPORTS) | set(api.EXPORTS_CHUNKS) | set(api.EXPORTS_TARGETS) | set(api.EXPORTS_SEGMENTS) | set(api.EXPORTS_SITES) | set(api.EXPORTS_EVENTS) | \
        set(api.EXPORTS_PILEUP) | set(api.EXPORTS_DETECT) | set(api.EXPORTS_ALIGN) | set(api.EXPORTS_COLLAPSE) | set(api.EXPORTS_SCALE)
    assert not set(api.EXPORTS_CALL) & others
    # the headers it includes export what they did
    assert _declared("sqg_scale.h") == set(api.EXPORTS_SCALE) and _declared("sqg_pileup.h") == set(api.EXPORTS_PILEUP)
    raw = open(os.path.join(ROOT, "include", "sqg_call.h")).read()
    assert '#include "sqg_scale.h"' in raw and '#include "sqg_pileup.h"' in raw and "SQG_ABI_VERSION is unchanged" in raw
    assert "exact integer arithmetic" in raw and "CLAMPED" in raw and "nanopolish's" in raw and "not measured here" in raw and "INT64_MIN" in raw
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    structs = (("sqg_call_cfg_t", api.CCallCfg), ("sqg_call_in_t", api.CCallIn), ("sqg_call_model_t", api.CCallModel), ("sqg_call_out_t", api.CCallOut),
               ("sqg_call_freq_t", api.CCallFreq), ("sqg_call_stat_t", api.CCallStat))
    for struct, ctype in structs:
        assert _struct_fields(hdr, struct) == [f[0] for f in ctype._fields_], struct
    assert tuple(f[0] for f in api.CCallOut._fields_) == OUT == R.OUTPUTS and tuple(f[0] for f in api.CCallFreq._fields_)[2:] == api.CALL_FREQ == R.FREQ
    assert [C.sizeof(t) for _, t in structs] == [16, 24, 16, 72, 48, 32]
    assert int(re.search(r"#define\s+SQG_CALL_NEIGH_READ\s+(\d+)u", hdr).group(1)) == api.CALL_NEIGH_READ == R.NEIGH_READ == 0
    assert int(re.search(r"#define\s+SQG_CALL_NEIGH_SAME\s+(\d+)u", hdr).group(1)) == api.CALL_NEIGH_SAME == R.NEIGH_SAME == 1
    dflt = re.search(r"#define\s+SQG_CALL_DEFAULT\s+\{(.*?)\}", hdr).group(1).replace("SQG_CALL_NEIGH_SAME", "1")
    assert tuple(eval(v) for v in dflt.split(",")) == api.CALL_DEFAULT == R.DEFAULT == (1, 256 * 50, 256 * 2, 1)      # noqa: S307  (digits and *)
    # the prototypes: the pointers behind (ctx, batch) in the order of the binding's table; the table's entry is not the last one
    at = [names for names, _ in api._CONSUMER_EXPORTS].index(api.EXPORTS_CALL)
    assert api._CONSUMER_EXPORTS[-1][0] == api.EXPORTS_COLLAPSE and at < len(api._CONSUMER_EXPORTS) - 1
    table = dict(api._CONSUMER_EXPORTS[at][1])
    names = {t: n for n, t in structs}
    names.update({api.CAlignScale: "sqg_align_scale_t", api.COrigin: "sqg_pileup_origin_t", C.c_int64: "int64_t"})
    for fn in api.EXPORTS_CALL:
        args = re.search(r"int\s+" + fn + r"\s*\((.*?)\)\s*;", hdr, re.S).group(1).split(",")
        types = [re.sub(r"\bconst\b|\*.*$", "", a).strip() for a in args]
        assert types == ["sqg_ctx_t", "sqg_batch_t"] + [names[t] for t in table[fn]], fn
    assert os.path.join(ROOT, "include", "sqg_call.h") in build.headers()
    for h in ("k_call.h", "h_call.h"):
        assert os.path.join(ROOT, "squigulator_amd", "csrc", h) in build.headers()
    assert "SQG_TEST_CALL_GRID" in api.DEV_KNOBS


def test_the_built_libraries_export_both_calls():
    build.build()
    for lib in (build.LIB, build.LIB_DEV):
        L = api.load_library(lib)
        for n in api.EXPORTS_CALL:
            assert hasattr(L, n), f"{n} not exported by {lib}"


def test_the_cpu_backend_has_no_call_and_says_so():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "libsqg_cpu.so"])
    prof, fl = profiles.get_profile("dna-r9-prom")
    mean, stdv = model.synthetic_model(6)
    gen = api.SignalGenerator(prof, fl, 6, mean, stdv, 42, lib_path=os.path.join(ROOT, "oracle", "libsqg_cpu.so"))
    for n in api.EXPORTS_CALL:
        assert not hasattr(gen.L, n)
    b = gen.submit([b"ACGTACGTCGTTTGACA" * 40])
    for fn, name in ((lambda: b.call_plan(), "sqg_call_plan"), (lambda: b.call(None, None), "sqg_batch_call"), (lambda: gen.new_call_freq(0, 10), "sqg_batch_call")):
        with pytest.raises(api.SqgError) as e:
            fn()
        assert e.value.code == -1 and name in str(e.value) and "sqg_call.h" in str(e.value)
    b.free(); gen.close()


def _hand(read, x, L=None, cfg=(R.NEIGH_SAME, 12800, 512, 1), w=None, c=None, **kw):
    """one typed-out read of k = 5 under a model a hand can follow: level_raw of row R is R (level_mean = R, digitisation = range,
    offset 0), every event's row has mean x[e]; c[R] = R by default, so that with w = 0 a site's nll is the SUM OF ITS ROWS' RANKS"""
    k, n = 5, 5 ** 5
    ne = len(read) - k + 1
    L = np.full(ne, 7) if L is None else np.asarray(L)
    sums = np.asarray(x, np.int64) * np.maximum(L, 1)
    w = np.zeros(n, np.int32) if w is None else w
    c = np.arange(n, dtype=np.int32) if c is None else c
    return R.both([read], k, cfg, sums, L, [0, ne], np.arange(n, dtype=np.float32), [0.0], 1000.0, 1000.0, w, c, what=read.decode(), **kw)


def test_hand_worked_reads():
    """typed out, k = 5.  AACGT: one event, rows 39 (AACGT) and 89 (AAMGT); observed at 39 with w = 2^24 the M term is 256 * 50^2, capped.
    TACGCGA: two sites over the same three events; the k-mer TACGC ends in a candidate whose G lies at e + k.  AMGCGT: MG next to CG"""
    full = np.full(5 ** 5, 1 << 24, np.int32)
    for neigh in (R.NEIGH_READ, R.NEIGH_SAME):
        o = _hand(b"AACGT", [39], cfg=(neigh, 12800, 512, 1), w=full)
        assert o["site_off"].tolist() == [0, 1] and o["site_pos"].tolist() == [2] and o["label"].tolist() == [0] and o["n_obs"].tolist() == [1]
        assert o["nll_c"].tolist() == [39] and o["nll_m"].tolist() == [89 + 12800] and o["llr"].tolist() == [-12850] and o["call"].tolist() == [1]
        assert o["stat"] == (1, 0, 1, 1) and "site_key" not in o
        o = _hand(b"AACGT", [89], cfg=(neigh, 1 << 26, 512, 1), w=full)          # observed at the M row, no cap in reach: 256 * 50^2 under C
        assert o["nll_c"].tolist() == [39 + 640000] and o["nll_m"].tolist() == [89] and o["call"].tolist() == [2] and o["stat"] == (1, 0, 1, 0)
    o = _hand(b"TACGCGA", [0, 0, 0], cfg=(R.NEIGH_SAME, 0, 0, 0))
    assert o["site_pos"].tolist() == [2, 4] and o["n_obs"].tolist() == [3, 3]
    assert o["nll_c"].tolist() == [2536 + 182 + 910] * 2 and o["nll_m"].tolist() == [2588 + 442 + 2210] * 2      # TAMGM: the G of its last M is at e + k
    o = _hand(b"TACGCGA", [0, 0, 0], cfg=(R.NEIGH_READ, 0, 0, 0))
    assert o["nll_c"].tolist() == [3628, 3628] and o["nll_m"].tolist() == [2586 + 432 + 2160, 2538 + 192 + 960] and o["llr"].tolist() == [-1550, -62]
    o = _hand(b"AMGCGT", [0, 0], cfg=(R.NEIGH_SAME, 0, 0, 0))
    assert o["site_pos"].tolist() == [1, 3] and o["label"].tolist() == [1, 0]
    assert o["nll_c"].tolist() == [182 + 914] * 2 and o["nll_m"].tolist() == [442 + 2214] * 2
    o = _hand(b"AMGCGT", [0, 0], cfg=(R.NEIGH_READ, 0, 0, 0))                    # the other CpG stays as the read has it
    assert o["nll_c"].tolist() == [182 + 914, 432 + 2164] and o["nll_m"].tolist() == [432 + 2164, 442 + 2214]
    assert o["call"].tolist() == [1, 1] and o["stat"] == (2, 0, 2, 1)            # llr_min 0: llr < 0 is a call of 1; the first site's label is 1
    # unobserved events, min_obs, llr_min; the key on either strand, step 0, the window
    o = _hand(b"TACGCGA", [0, 0, 0], L=[0, 3, -1], cfg=(R.NEIGH_SAME, 0, 0, 2), origin=([100], [1]), window=(102, 104))
    assert o["n_obs"].tolist() == [1, 1] and o["nll_c"].tolist() == [182, 182] and o["call"].tolist() == [0, 0] and o["site_key"].tolist() == [102, 104]
    assert o["stat"] == (2, 1, 0, 0) and o["freq"]["cov"].tolist() == [1, 0] and o["freq"]["called"].tolist() == [0, 0]
    o = _hand(b"TACGCGA", [0, 0, 0], L=[0, 0, 0], origin=([100], [-1]), window=(0, 200))
    assert o["n_obs"].tolist() == [0, 0] and o["nll_c"].tolist() == o["nll_m"].tolist() == o["call"].tolist() == [0, 0]
    assert o["site_key"].tolist() == [100 + 5 - 2 - 2, 100 + 5 - 2 - 4] and o["freq"]["cov"][[99, 101]].tolist() == [1, 1]
    o = _hand(b"TACGCGA", [0, 0, 0], origin=([100], [0]), window=(0, 200))
    assert o["site_key"].tolist() == [R.I64_MIN] * 2 and o["stat"][:2] == (2, 2) and not o["freq"]["cov"].any()
    o = _hand(b"TACGCGA", [0, 0, 0], cfg=(R.NEIGH_READ, 0, 1551, 1))
    assert o["llr"].tolist() == [-1550, -62] and o["call"].tolist() == [0, 0]
    assert _hand(b"TACGCGA", [0, 0, 0], cfg=(R.NEIGH_READ, 0, 1550, 1))["call"].tolist() == [1, 0]
    # the row value and the term
    assert [R.row_value(s, n) for s, n in ((-1, 256), (1, 256), (-256, 3), (1 << 60, 1), ((1 << 55) + 1, 1), (1 << 40, 1))] == [-1, 1, -21846, 0, -(1 << 26), 1 << 26]
    assert R.row_value(100, 1, 32768, 7) == 12807 and R.row_value(100, 1, 0, 0) == 0 and R.row_value(-100, 1, 1, 0) == -1 and R.row_value(100, 1, 1 << 21, 1 << 27) == 1 << 26
    assert R.term(256 * 50, 0, 1 << 24, 5, 1 << 26) == 5 + 640000 and R.term(1 << 26, 0, 1 << 25, -(1 << 21), 1 << 26) == -(1 << 20) + (1 << 26)
    assert R.term(1 << 26, 0, 1 << 24, 0, 1 << 26) == 1 << 26 >> 0 and R.term(-(1 << 26), 0, 1, 0, 1 << 26) == (1 << 38) >> 32 and R.term(5, 0, -3, 9, 7) == 9


def test_the_two_statements_agree_on_drawn_cases():
    seen = dict(sites=0, outside=0, called=0, agree=0, unobserved=0, scaled=0)
    for seed in range(120):
        a, kw = CS.cpu_case(seed)
        o = R.both(*a, what=f"case {seed}", **kw)
        for n, v in zip(("sites", "outside", "called", "agree"), o["stat"]):
            seen[n] += v
        seen["unobserved"] += int((o["n_obs"] == 0).sum()); seen["scaled"] += int("scale" in kw and o["stat"][0] > 0)
    assert seen["sites"] > 500 and seen["outside"] > 50 and seen["agree"] > 50 and seen["called"] > seen["agree"] and seen["unobserved"] > 0 and seen["scaled"] > 20, seen


# ---------------------------------------------------------------------------------------------------------- GPU
def _dev(b):
    return torch.device("cuda", b.gen.device)


def _on(b, a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dt)).to(_dev(b))


def _gen(k=6, profile="dna-r9-prom", extra=0, T=2, lib_path=None, seed=42):
    prof, fl = profiles.get_profile(profile)
    mean, stdv = model.synthetic_model(k, meth=True)
    gen = api.SignalGenerator(prof, fl | profiles.SQ_METH | extra, k, mean, stdv, seed, num_workers=T, mode=api.MODE_CERTIFIED, lib_path=lib_path)
    gen.level_mean = np.asarray(mean, np.float32)
    return gen


def _true_rows(b):
    ev = b.events(outputs=("sum", "ev_len"))
    return ev.sum, ev.ev_len


def _check(b, reads, cfg=R.DEFAULT, rows=None, model_=None, scale=None, origin=None, window=None, freq=None, what="", ref_origin=None):
    """plan and call of batch b against both statements; rows: (sum, len) tensors, default the true table's; model_ / scale / origin: numpy
    arrays; window: a fresh frequency table over it unless `freq` brings one.  -> (the reference's dict, the Chunks, the CallFreq)"""
    gen = b.gen
    sums, lens = _true_rows(b) if rows is None else rows
    mw, mc = gen.call_model() if model_ is None else (_on(b, model_[0], np.int32), _on(b, model_[1], np.int32))
    ro = origin if origin is not None else ref_origin
    want = R.both(reads, gen.kmer_size, cfg, sums.cpu().numpy(), lens.cpu().numpy(), b.ev_off, gen.level_mean, b.offset, gen.profile.range,
                  gen.profile.digitisation, mw.cpu().numpy(), mc.cpu().numpy(), scale=scale, origin=ro, window=window, what=what)
    off, ns = b.call_plan()
    np.testing.assert_array_equal(off, want["site_off"], err_msg=f"{what}: site_off")
    assert ns == want["stat"][0] == len(want["site_read"]), what
    fq = freq if freq is not None else gen.new_call_freq(*window) if window is not None else None
    before = {n: getattr(fq, n).cpu().numpy().view(np.uint32).copy() for n in R.FREQ} if fq is not None else None
    ch = b.call(sums, lens, model=None if model_ is None else (mw, mc), scale=None if scale is None else tuple(_on(b, a, np.int32) for a in scale),
                origin=origin, freq=fq, neigh=cfg[0], term_cap=cfg[1], llr_min=cfg[2], min_obs=cfg[3])
    assert ch.n_sites == ns and ch.stat == want["stat"], f"{what}: stat {ch.stat}, expected {want['stat']}"
    np.testing.assert_array_equal(ch.site_off, want["site_off"])
    for n in OUT:
        if n not in want:
            assert getattr(ch, n) is None, n
            continue
        got = getattr(ch, n).cpu().numpy()
        assert got.dtype == want[n].dtype and got.shape == want[n].shape, f"{what}: {n} {got.dtype} {got.shape}"
        np.testing.assert_array_equal(got, want[n], err_msg=f"{what}: {n}")
    if fq is not None:
        for n in R.FREQ:
            np.testing.assert_array_equal(getattr(fq, n).cpu().numpy().view(np.uint32), before[n] + want["freq"][n], err_msg=f"{what}: freq.{n}")
    return want, ch, fq


@pytest.mark.gpu
@pytest.mark.parametrize("k", [5, 6, 9])
def test_small_shapes(k):
    """call_cases.small_reads: every shape of its docstring, the true table, both neigh modes, a caller's origin with all three steps and a
    window that cuts it; then the batch without a site"""
    gen = _gen(k, "dna-r10-prom" if k == 9 else "dna-r9-prom")
    reads = CS.small_reads(k)
    assert len(reads[0]) == k - 1 and len(reads[1]) == k and len(reads[2]) == k + 1 and max(len(r) for r in reads) > CS.TILE + CS.WAVE
    b = gen.submit(reads)
    rng = np.random.default_rng(k)
    origin = CS.drawn_origin(rng, len(reads), span=3000)
    rows = _true_rows(b)
    for neigh in (R.NEIGH_SAME, R.NEIGH_READ):
        want, ch, _ = _check(b, reads, cfg=(neigh,) + R.DEFAULT[1:], rows=rows, origin=origin, window=(origin[0].min() + 500, origin[0].min() + 2500), what=f"k {k} neigh {neigh}")
    per = np.diff(want["site_off"])
    assert per[0] == 0 and per[1] == 1 and per[2] == 1 and per[3] == per[4] == per[5] == per[6] == 0 and per[10] == CS.TILE // 2 + CS.WAVE // 2 + 37
    assert want["site_pos"][0] == 0 and want["site_pos"][1] == len(reads[2]) - 2 and want["stat"][1] > 0 and want["stat"][0] - want["stat"][1] > 100
    assert set(origin[1].tolist()) == {-1, 0, 1} and (want["site_key"] == R.I64_MIN).any()
    for at in (CS.LOAD, CS.WAVE, CS.TILE):                      # a C in the last byte of a load / wavefront / tile, whatever the read's alignment
        pos = want["site_pos"][want["site_off"][11]:want["site_off"][12]]
        assert len({int(p) % at for p in pos}) == at if at == CS.LOAD else (pos > at).any()
    b.free()
    reads = CS.barren_reads(k)
    b = gen.submit(reads)
    want, ch, fq = _check(b, reads, origin=CS.drawn_origin(rng, len(reads)), window=((1 << 40), (1 << 40) + 600), what=f"k {k}: no site")
    assert want["stat"] == (0, 0, 0, 0) and ch.n_sites == 0 and not fq.cov.any()
    b.free(); gen.close()


def _noisy_batch(gen, n=6, seed=5):
    rng = np.random.default_rng(seed)
    reads = [bytes(rng.choice(list(b"ACGTMCG"), int(m)).astype(np.uint8)) for m in rng.integers(300, 900, n)]
    return reads, gen.submit(reads)


@pytest.mark.gpu
def test_more_sites_than_one_trip(monkeypatch):
    """k_call_score's grid is capped.  The development library takes the cap from SQG_TEST_CALL_GRID: with one workgroup a batch of a few
    thousand sites takes a dozen trips.  The release library on the same batch gives the same bytes"""
    build.build()
    got = {}
    for lib in (build.LIB_DEV, build.LIB):
        monkeypatch.setenv("SQG_TEST_CALL_GRID", "1")
        gen = _gen(6, lib_path=lib)
        assert api.build_info(gen.L)["dev"] == ("1" if lib == build.LIB_DEV else "0")
        reads, b = _noisy_batch(gen, 20)
        want, ch, _ = _check(b, reads, what=f"trips {os.path.basename(lib)}")
        assert want["stat"][0] > 4 * WG
        got[lib] = {n: getattr(ch, n).cpu().numpy() for n in OUT if getattr(ch, n) is not None}
        b.free(); gen.close()
    for n in got[build.LIB]:
        np.testing.assert_array_equal(got[build.LIB][n], got[build.LIB_DEV][n], err_msg=n)


@pytest.mark.gpu
def test_rows_scale_and_model():
    """the true table; the observed table of detected and aligned rows, with unobserved events; all events unobserved; scale (65536, 0) is
    no scale; scale, w and c outside their ranges are clamped; term_cap 0, a term_cap that binds, min_obs above k"""
    gen = _gen(6)
    reads, b = _noisy_batch(gen)
    n, k = len(reads), 6
    true = _true_rows(b)
    base, ch0, _ = _check(b, reads, rows=true, what="true rows")
    assert base["stat"][2] > 50 and 0 < base["stat"][3] <= base["stat"][2]
    dt = b.detect("dna", outputs=("sum", "sumsq", "dt_len"))
    al = b.align(dt.det_off, dt.sum, dt.dt_len, outputs=("al_ev",))
    co = b.collapse(dt.det_off, al.al_ev, dt.sum, dt.sumsq, dt.dt_len, outputs=("ob_sum", "ob_len"))
    assert co.ob_len.dtype == torch.int64 and bool((co.ob_len == 0).any()) and bool((co.ob_len > 0).any())
    obs, _, _ = _check(b, reads, rows=(co.ob_sum, co.ob_len), what="collapsed rows")
    assert (obs["n_obs"] < base["n_obs"]).any() and obs["stat"][2] > 0
    none, _, _ = _check(b, reads, rows=(true[0], torch.zeros_like(true[1])), what="all unobserved")
    assert not none["n_obs"].any() and not none["llr"].any() and not none["call"].any() and none["stat"][2:] == (0, 0)
    unit, ch1, _ = _check(b, reads, rows=true, scale=(np.full(n, 65536, np.int32), np.zeros(n, np.int32)), what="scale (65536, 0)")
    for name in ("nll_c", "nll_m", "llr", "call", "n_obs"):
        np.testing.assert_array_equal(unit[name], base[name], err_msg=name)
        assert torch.equal(getattr(ch0, name), getattr(ch1, name))
    rng = np.random.default_rng(3)
    wild = (np.array([-7, 0, (1 << 20) + 5, (1 << 31) - 1, 70000, 60000], np.int32), np.array([-(1 << 31), (1 << 26) + 1, 300, -300, (1 << 31) - 1, 0], np.int32))
    clamped = (np.clip(wild[0], 1, 1 << 20), np.clip(wild[1], -(1 << 26), 1 << 26))
    a, _, _ = _check(b, reads, rows=true, scale=wild, what="scale out of range")
    c_, _, _ = _check(b, reads, rows=true, scale=clamped, what="scale at the range's ends")
    assert all((a[name] == c_[name]).all() for name in ("nll_c", "nll_m", "call")) and (a["llr"] != base["llr"]).any()
    w, c = CS.drawn_model(rng, k, wild=True)
    assert (w < 0).any() and (w > 1 << 24).any() and (c < -(1 << 20)).any() and (c > 1 << 20).any()
    a, _, _ = _check(b, reads, rows=true, model_=(w, c), what="model out of range")
    c_, _, _ = _check(b, reads, rows=true, model_=(np.clip(w, 0, 1 << 24), np.clip(c, -(1 << 20), 1 << 20)), what="model at the range's ends")
    assert all((a[name] == c_[name]).all() for name in ("nll_c", "nll_m", "call"))
    mw, mc = (t.cpu().numpy() for t in gen.call_model())
    rw, rc = R.call_model(model.synthetic_model(k, meth=True)[1], gen.profile.range, gen.profile.digitisation)
    np.testing.assert_array_equal(mw, rw); np.testing.assert_array_equal(mc, rc)
    zero, _, _ = _check(b, reads, rows=true, cfg=(R.NEIGH_SAME, 0, 512, 1), what="term_cap 0")       # only c is left of a term
    assert (zero["nll_c"] != base["nll_c"]).any()
    shifted = (true[0] + 3000 * true[1].to(torch.int64), true[1])                                       # 3000 codes above every level: every term at the cap
    bind, _, _ = _check(b, reads, rows=shifted, cfg=(R.NEIGH_SAME, 300, 0, 1), model_=(mw, np.zeros_like(mc)), what="term_cap binds")
    assert (bind["nll_c"] == 300 * bind["n_obs"]).all() and (bind["nll_m"] == 300 * bind["n_obs"]).all() and bind["n_obs"].max() == k
    most, _, _ = _check(b, reads, rows=true, cfg=(R.NEIGH_SAME, 12800, 0, k + 1), what="min_obs above k")
    assert not most["call"].any() and most["llr"].any()
    b.free(); gen.close()


@pytest.mark.gpu
@pytest.mark.parametrize("ideal", [0, profiles.SQ_IDEAL_TIME, profiles.SQ_IDEAL], ids=["noisy", "ideal_time", "ideal"])
def test_the_true_hypothesis_costs_nothing(ideal):
    """sum = level_raw * ev_len from the true table, c = 0, w > 0, NEIGH_READ: the row of the read's own k-mer is one of the two hypothesis
    rows, q - Lv = 0 there, so that hypothesis has nll 0 and the other one nll >= 0: label 1 gives llr >= 0, label 0 gives llr <= 0"""
    gen = _gen(6, extra=ideal)
    reads, b = _noisy_batch(gen, 5, seed=8)
    ev = b.events(outputs=("level_raw", "ev_len"))
    rows = (ev.level_raw.to(torch.int64) * ev.ev_len.to(torch.int64), ev.ev_len)
    n = 5 ** 6
    want, ch, _ = _check(b, reads, cfg=(R.NEIGH_READ, 1 << 26, 0, 1), rows=rows, model_=(np.full(n, 1 << 20, np.int32), np.zeros(n, np.int32)), what="noise-free rows")
    lab, llr, seen = want["label"] == 1, want["llr"], want["n_obs"] > 0
    assert lab.sum() > 20 and (~lab).sum() > 20
    assert (want["nll_m"][lab] == 0).all() and (want["nll_c"][~lab] == 0).all() and (llr[lab] >= 0).all() and (llr[~lab] <= 0).all()
    assert (llr[lab & seen] > 0).any() and (llr[~lab & seen] < 0).any()
    b.free(); gen.close()


def _fasta(path):
    names, seqs = [], []
    for ln in open(path, "rb"):
        if ln.startswith(b">"):
            names.append(ln[1:].split()[0].decode()); seqs.append([])
        else:
            seqs[-1].append(ln.strip())
    return [b"".join(s) for s in seqs], names


@pytest.mark.gpu
def test_sampled_reads_of_both_strands():
    """load_genome + set_meth(mfreq_dense.tsv) + sample, two batches, the sampler's origin: every site_key indexes a CpG's C of the genome,
    on either strand; every site with label 1 has a frequency byte above 0 there, but for the draws below 1 / 254 that the sampler's rule
    lets methylate over a byte of 0 (batch 0 has one such site: byte 0, label 1), and every site over a byte of 253 or more has label 1; cov over the two batches is the two batches' sites per
    key; a window and a caller's origin with a step of 0 leave outside what the statement leaves outside"""
    gen = _gen(6, T=3)
    contigs, names = _fasta(NCOV)
    gen.load_genome(contigs, 1500)
    gen.set_meth(contigs, names, MFREQ_DENSE)
    genome = np.frombuffer(b"".join(contigs), np.uint8)
    fbyte, _ = api.load_meth_freq(contigs, names, MFREQ_DENSE)
    off = np.concatenate(([0], np.cumsum([len(c) for c in contigs])))
    whole = gen.new_call_freq()
    assert (whole.lo, whole.hi) == (0, len(genome))
    keys, strands, sure = [], set(), 0
    for bi, nb in enumerate((14, 10)):
        b = gen.sample(nb).run().wait()
        reads = b.reads()
        s = b.sampled
        sampler = PR.sampler_origin(off, s["ref_idx"], s["ref_pos"], s["rlen"], s["strand"], 6)
        want, ch, _ = _check(b, reads, freq=whole, window=(0, len(genome)), ref_origin=sampler, what=f"sampled batch {bi}")
        key = want["site_key"]
        assert want["stat"][1] == 0 and len(key) > 100
        up = np.char.upper(genome.view("S1"))
        assert (up[key] == b"C").all() and (up[key + 1] == b"G").all()
        # the label against the byte, by the sampler's rule (methylate_dna: 'M' iff (int)(u * 254) <= byte, one draw u in [0, 1) per CpG): a
        # byte of 253 or more always methylates; a byte of 0 does when the draw is below 1 / 254, so "label 1 has a byte above 0" holds
        # but for such draws -- at most m of the n0 sites over a byte of 0, m the smallest count a Binomial(n0, 1 / 254) exceeds with a
        # probability below 1e-9; sites keyed to a wrong CpG would carry 'M' over a byte of 0 at the rate of the bytes themselves
        lab, byte = want["label"] == 1, fbyte[key]
        assert lab.sum() > 10 and (lab[byte >= 253]).all()
        sure += int((byte >= 253).sum())
        n0, stray = int((byte == 0).sum()), int((lab & (byte == 0)).sum())
        tail, m = 1.0, -1
        while tail >= 1e-9:
            m += 1
            tail -= math.comb(n0, m) * (1 / 254) ** m * (253 / 254) ** (n0 - m)
        print(f"batch {bi}: {len(key)} sites, {int(lab.sum())} with label 1, {n0} over a byte of 0, {stray} of them with label 1 (at most {m})")
        assert stray <= m and (byte[lab] > 0).sum() >= lab.sum() - m
        keys.append(key); strands |= set(s["strand"])
        # a window, then a caller's origin in which every third read has no step
        lo, hi = int(np.sort(key)[len(key) // 4]), int(np.sort(key)[3 * len(key) // 4])
        cut, _, _ = _check(b, reads, window=(lo, hi), ref_origin=sampler, what=f"sampled batch {bi}, window")
        assert 0 < cut["stat"][1] < cut["stat"][0]
        step = np.where(np.arange(nb) % 3 == 1, 0, sampler[1]).astype(np.int8)
        cut, _, _ = _check(b, reads, origin=(sampler[0], step), window=(0, len(genome)), what=f"sampled batch {bi}, steps of 0")
        assert cut["stat"][1] == int((step[want["site_read"]] == 0).sum()) > 0
        b.free()
    assert strands == set(b"+-") and sure > 0
    np.testing.assert_array_equal(whole.cov.cpu().numpy().view(np.uint32), np.bincount(np.concatenate(keys), minlength=len(genome)).astype(np.uint32))
    assert int(whole.cov.max()) >= 2                            # a CpG that reads of both batches cover
    gen.close()


def _raw(gen, b, cfg=None, cin=None, cmod=None, csc=None, org=None, out=None, fq=None, drop=()):
    """sqg_batch_call through ctypes alone, for the arguments the binding would not pass; drop: the arguments handed over as NULL"""
    a = dict(cfg=cfg, cin=cin, cmod=cmod, csc=csc, org=org, out=out, fq=fq, st=api.CCallStat())
    ref = lambda n: C.byref(a[n]) if a[n] is not None and n not in drop else None      # noqa: E731
    rc = gen.L.sqg_batch_call(gen.ctx, b.handle, *(ref(n) for n in ("cfg", "cin", "cmod", "csc", "org", "out", "fq", "st")))
    return rc, gen.L.sqg_last_error(gen.ctx).decode()


@pytest.mark.gpu
def test_errors_and_lifetime():
    gen = _gen(6)
    reads, b = _noisy_batch(gen, 3)
    sums, lens = _true_rows(b)
    mw, mc = gen.call_model()
    good = dict(cfg=api.CCallCfg(*R.DEFAULT), cin=api.CCallIn(sums.data_ptr(), None, lens.data_ptr()), cmod=api.CCallModel(mw.data_ptr(), mc.data_ptr()), out=api.CCallOut())
    assert _raw(gen, b, **good)[0] == 0
    both_len = api.CCallIn(sums.data_ptr(), sums.data_ptr(), lens.data_ptr())
    key0, step = np.zeros(3, np.int64), np.array([1, 2, 0], np.int8)
    p64, p8 = C.POINTER(C.c_int64), C.POINTER(C.c_int8)
    keyed = api.CCallOut(); keyed.site_key = sums.data_ptr()
    for change, text in ((dict(drop=("cfg",)), "cfg must not be NULL"), (dict(drop=("cin",)), "in must not be NULL"), (dict(drop=("cmod",)), "model must not be NULL"),
                         (dict(drop=("out",)), "out must not be NULL"), (dict(cin=api.CCallIn(None, None, lens.data_ptr())), "in->sum"),
                         (dict(cmod=api.CCallModel(None, mc.data_ptr())), "model->w"), (dict(cmod=api.CCallModel(mw.data_ptr(), None)), "model->c"),
                         (dict(cin=both_len), "in->len64 and in->len32"), (dict(cin=api.CCallIn(sums.data_ptr(), None, None)), "in->len64 and in->len32"),
                         (dict(cfg=api.CCallCfg(2, 0, 0, 0)), "neigh"), (dict(cfg=api.CCallCfg(1, -1, 0, 0)), "term_cap"), (dict(cfg=api.CCallCfg(1, (1 << 26) + 1, 0, 0)), "term_cap"),
                         (dict(cfg=api.CCallCfg(1, 0, -1, 0)), "llr_min"), (dict(cfg=api.CCallCfg(1, 0, 0, -1)), "min_obs"), (dict(cfg=api.CCallCfg(1, 0, 0, (1 << 20) + 1)), "min_obs"),
                         (dict(csc=api.CAlignScale(None, mc.data_ptr())), "scale->gain"), (dict(csc=api.CAlignScale(mc.data_ptr(), None)), "scale->shift"),
                         (dict(fq=api.CCallFreq(5, 4, None, None, None, None)), "hi must not be below lo"),
                         (dict(fq=api.CCallFreq(0, 4, None, None, None, None)), "origin must not be NULL"), (dict(out=keyed), "origin must not be NULL"),
                         (dict(org=api.COrigin(key0.ctypes.data_as(p64), None)), "origin: key0 and step"),
                         (dict(org=api.COrigin(key0.ctypes.data_as(p64), step.ctypes.data_as(p8))), "step must be -1, 0 or +1")):
        rc, msg = _raw(gen, b, **{**good, **change})
        assert rc == -1 and "sqg_batch_call" in msg and text in msg, (change, rc, msg)
    assert gen.L.sqg_batch_call(None, b.handle, *([None] * 8)) == -1
    total = C.c_int64()
    assert gen.L.sqg_call_plan(gen.ctx, b.handle, None, None) == -1 and "n_sites" in gen.L.sqg_last_error(gen.ctx).decode()
    assert gen.L.sqg_call_plan(gen.ctx, b.handle, None, C.byref(total)) == 0 and total.value == b.call_plan()[1] > 0
    with pytest.raises(api.SqgError) as e:
        b.call(sums, lens, neigh="other")
    assert e.value.code == -1
    with pytest.raises(api.SqgError) as e:
        b.call(sums[:5], lens)
    assert "sum must be" in str(e.value)
    # a batch that has not been run; a batch two more batches have been run behind
    fresh = gen.stage(reads)
    for fn in (fresh.call_plan, lambda: fresh.call(sums, lens)):
        with pytest.raises(api.SqgError) as e:
            fn()
        assert e.value.code == -4 and "has not been run" in str(e.value)
    fresh.run().wait()
    assert fresh.call_plan()[1] == b.call_plan()[1]
    third = gen.submit(reads)
    for fn in (b.call_plan, lambda: b.call(sums, lens)):
        with pytest.raises(api.SqgError) as e:
            fn()
        assert e.value.code == -4 and "handed to a later batch" in str(e.value)
    assert third.call(*_true_rows(third)).n_sites == fresh.call(*_true_rows(fresh)).n_sites
    empty = gen.submit([])
    ch = empty.call(torch.zeros(0, dtype=torch.int64, device=_dev(b)), torch.zeros(0, dtype=torch.int32, device=_dev(b)))
    assert ch.n_sites == 0 and ch.stat == (0, 0, 0, 0) and empty.call_plan()[0].tolist() == [0]
    for x in (b, fresh, third, empty):
        x.free()
    gen.close()


@pytest.mark.gpu
@pytest.mark.parametrize("profile,extra,meth,flag", [("rna-r9-prom", 0, False, "SQG_RNA"), ("dna-r9-prom", profiles.SQ_PREFIX, False, "SQG_PREFIX"), ("dna-r9-prom", 0, False, "SQG_METH")])
def test_other_contexts_are_refused(profile, extra, meth, flag):
    prof, fl = profiles.get_profile(profile)
    fl |= extra | (profiles.SQ_METH if meth else 0)
    k = 6
    mean, stdv = model.synthetic_model(k, meth=meth)
    gen = api.SignalGenerator(prof, fl, k, mean, stdv, 42, mode=api.MODE_CERTIFIED)
    b = gen.submit([b"ACGTACGTTTGACGA" * 30])
    ev = b.events(outputs=("sum", "ev_len"))
    n = 5 ** k
    tables = (torch.zeros(n, dtype=torch.int32, device=_dev(b)),) * 2           # (5^k rows: the binding's own check passes, the library refuses)
    for fn in (b.call_plan, lambda: b.call(ev.sum, ev.ev_len, model=tables)):
        with pytest.raises(api.SqgError) as e:
            fn()
        assert e.value.code == -1 and flag in str(e.value)
    b.free(); gen.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", CS.GPU_SEEDS)
def test_drawn_contexts(seed):
    """consumer_cases.draw's contexts with SQ_METH -- k in 5 ... 9, the dwell, the model's salt, ragged batches with empty ones and reads
    shorter than a k-mer -- and, drawn here from the seed, neigh and the cfg, the rows (the true table's; or made up around the true levels
    with unobserved events and sums of any size), a model, a scaling, a caller's origin and a window: plan and call against the statement"""
    import consumer_cases as CC
    su = CC.draw(seed)
    assert su.meth and not su.rna and not su.prefix
    rng = np.random.default_rng(4000 + seed)
    gen = su.generator(api.MODE_EXACT if seed % 2 else api.MODE_CERTIFIED)
    gen.level_mean = np.asarray(su.mean, np.float32)
    lo = (1 << 40) + 77 + int(rng.integers(0, 200))
    freq, total = gen.new_call_freq(lo, lo + 300), np.zeros(300, np.int64)
    try:
        for bi, bt in enumerate(su.staged_reads()):
            b = gen.stage(bt, su.workers_of(len(bt))).run().wait()
            ev = b.events(outputs=("sum", "ev_len", "level_raw"))
            rows = (ev.sum, ev.ev_len)
            if (seed // 10 + bi) % 2:
                s, ln = CS.drawn_rows(rng, b.n_events, ev.level_raw.cpu().numpy(), wild=bool(bi % 2))
                rows = (_on(b, s, np.int64), _on(b, ln, np.int64 if seed % 10 == 8 else np.int32))
            want, ch, _ = _check(b, bt, cfg=CS.drawn_cfg(rng), rows=rows, model_=CS.drawn_model(rng, su.k, wild=bool(seed % 3)) if bi % 2 == 0 else None,
                                 scale=CS.drawn_scale(rng, len(bt)) if (seed + bi) % 3 else None, origin=CS.drawn_origin(rng, len(bt)), window=(lo, lo + 300), freq=freq,
                                 what=f"{CC.describe(su)}: batch {bi}")
            total += want["freq"]["cov"]
            b.free()
        np.testing.assert_array_equal(freq.cov.cpu().numpy().view(np.uint32), total.astype(np.uint32))
    finally:
        gen.close()
