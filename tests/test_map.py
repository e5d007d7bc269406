"""include/sqg_map.h: the genome's level track (sqg_map_track) and subsequence DTW of event rows against it (sqg_batch_map), against the two
plain statements of the header's rule (map_ref.py).  Every comparison is bit for bit: every output is an integer."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (before the library is loaded: the HIP runtime torch brings is the one the library then uses)

import inject
import map_cases as MC
import map_ref as R
import pileup_ref as PR
import targets_ref as T
from chunk_support import _declared
from squigulator_amd import api, build, model, profiles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NCOV = os.path.join(ROOT, "tests", "golden", "inputs", "nCoV-2019.reference.fasta")
CPU_LIB = os.path.join(ROOT, "oracle", "libsqg_cpu.so")
OUT = api.MAP_OUTPUTS
TILE = 1024         # k_map.h's MAP_TILE: the positions a wavefront holds at a time, 16 per lane
NONE = R.NONE
ROWS = 96           # rows mapped on the sampled batches
MAPCFG = api.MAP_DEFAULT[:4] + (ROWS, 3)


# ---------------------------------------------------------------------------------------------------------- no GPU
def _struct_fields(hdr, struct):
    body = hdr[:hdr.index("} " + struct)]
    body = body[body.rindex("typedef struct"):]
    body = body[body.index("{") + 1:]
    return [re.sub(r"[\s*]", "", name) for decl in body.split(";") if decl.strip() for name in re.sub(r"^\s*(const\s+)?\w+\s", "", decl.strip()).split(",")]


def test_the_header_and_the_binding_agree():
    assert _declared("sqg_map.h") == set(api.EXPORTS_MAP) == {"sqg_map_track", "sqg_batch_map"}
    others = set(api.EXPORTS) | set(api.EXPORTS_CHUNKS) | set(api.EXPORTS_TARGETS) | set(api.EXPORTS_SEGMENTS) | set(api.EXPORTS_SITES) | set(api.EXPORTS_EVENTS) | \
        set(api.EXPORTS_PILEUP) | set(api.EXPORTS_DETECT) | set(api.EXPORTS_ALIGN) | set(api.EXPORTS_COLLAPSE) | set(api.EXPORTS_SCALE) | set(api.EXPORTS_CALL)
    assert not set(api.EXPORTS_MAP) & others
    raw = open(os.path.join(ROOT, "include", "sqg_map.h")).read()
    for phrase in ("exact integers", "FIRST", "free start", "lowest u", "SQG_ABI_VERSION is unchanged", "CLAMPED", "not measured", "3-Gb genome", "2^30"):
        assert phrase in raw, phrase
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    structs = (("sqg_map_cfg_t", api.CMapCfg), ("sqg_map_track_t", api.CMapTrack), ("sqg_map_out_t", api.CMapOut))
    for struct, ctype in structs:
        assert _struct_fields(hdr, struct) == [f[0] for f in ctype._fields_], struct
    assert tuple(f[0] for f in api.CMapOut._fields_) == OUT == R.OUTPUTS and tuple(f[0] for f in api.CMapCfg._fields_) == api.MAP_CFG
    assert [C.sizeof(t) for _, t in structs] == [24, 32, 40]
    dflt = re.search(r"#define\s+SQG_MAP_DEFAULT\s+\{(.*?)\}", hdr).group(1).replace("u", "")
    assert tuple(int(v) for v in dflt.split(",")) == api.MAP_DEFAULT == R.DEFAULT == (4096, 4096, 65536, 0, 256, 3)
    assert api.MAP_DEFAULT[:3] == tuple(min(v, 1 << 17) for v in api.ALIGN_DEFAULT)
    assert re.search(r"#define\s+SQG_MAP_NONE\s+INT32_MIN", hdr) and api.MAP_NONE == R.NONE == -(1 << 31)
    assert eval(re.search(r"#define\s+SQG_MAP_MAX_WINDOW\s+\((.*?)\)", hdr).group(1)) == api.MAP_MAX_WINDOW == 1 << 24      # noqa: S307  (digits and <<)
    assert int(re.search(r"#define\s+SQG_MAP_MAX_ROWS\s+(\d+)", hdr).group(1)) == api.MAP_MAX_ROWS == 4096
    # the prototypes against the binding's table; the table's entry is not the last one
    at = [names for names, _ in api._CONSUMER_EXPORTS].index(api.EXPORTS_MAP)
    assert api._CONSUMER_EXPORTS[-1][0] == api.EXPORTS_COLLAPSE and at < len(api._CONSUMER_EXPORTS) - 1
    table = dict(api._CONSUMER_EXPORTS[at][1])
    names = {t: n for n, t in structs}
    names.update({api.CAlignIn: "sqg_align_in_t", api.CAlignScale: "sqg_align_scale_t", C.c_int64: "int64_t"})
    assert set(table) == {"sqg_batch_map"}                          # (sqg_map_track takes no batch: bound on its own)
    args = re.search(r"int\s+sqg_batch_map\s*\((.*?)\)\s*;", hdr, re.S).group(1).split(",")
    assert [re.sub(r"\bconst\b|\*.*$", "", a).strip() for a in args] == ["sqg_ctx_t", "sqg_batch_t"] + [names[t] for t in table["sqg_batch_map"]]
    args = [a.strip() for a in re.search(r"int\s+sqg_map_track\s*\((.*?)\)\s*;", hdr, re.S).group(1).split(",")]
    assert args == ["sqg_ctx_t *ctx", "int64_t lo", "int64_t hi", "const int32_t *levels", "int32_t *fwd", "int32_t *rev"]
    assert api._MAP_TRACK_ARGS == tuple(C.c_void_p if "*" in a else C.c_int64 for a in args)
    assert os.path.join(ROOT, "include", "sqg_map.h") in build.headers()
    for h in ("k_map.h", "h_map.h"):
        assert os.path.join(ROOT, "squigulator_amd", "csrc", h) in build.headers()
    assert "SQG_TEST_MAP_TILES" in api.DEV_KNOBS
    sqg_h = open(os.path.join(ROOT, "include", "sqg.h")).read()
    assert "sqg_map_track" not in sqg_h and "sqg_batch_map" not in sqg_h


def test_the_built_libraries_export_both_calls():
    build.build()
    for lib in (build.LIB, build.LIB_DEV):
        L = api.load_library(lib)
        for n in api.EXPORTS_MAP:
            assert hasattr(L, n), f"{n} not exported by {lib}"


def _cpu_gen(k=6, T=2):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "libsqg_cpu.so"])
    prof, fl = profiles.get_profile("dna-r9-prom")
    mean, stdv = model.synthetic_model(k)
    gen = api.SignalGenerator(prof, fl, k, mean, stdv, 42, num_workers=T, lib_path=CPU_LIB)
    gen.level_mean = np.asarray(mean, np.float32)
    return gen


def test_the_cpu_backend_has_no_map_and_says_so():
    gen = _cpu_gen()
    for n in api.EXPORTS_MAP:
        assert not hasattr(gen.L, n)
    b = gen.submit([b"ACGTACGTCGTTTGACA" * 40])
    calls = ((lambda: gen.map_levels(), "sqg_map_track"), (lambda: gen.new_map_track(0, 10), "sqg_map_track"), (lambda: b.map_shift(), "sqg_batch_map"),
             (lambda: b.map([0, 0], None, None, None), "sqg_batch_map"))
    for fn, name in calls:
        with pytest.raises(api.SqgError) as e:
            fn()
        assert e.value.code == -1 and name in str(e.value) and "sqg_map.h" in str(e.value)
    b.free(); gen.close()


def test_the_two_statements_agree_on_drawn_cases():
    """400 drawn cases, (a) by_rows against (b) by_matrix: two-level tracks without jitter, penalties of 0, constant tracks, NONE runs, m in
    {0, 1, 2}, W in {0, 1, 2, 3}.  More than a quarter of them hold a tie.  On a constant track that the rows sit on every path without a
    penalty costs 0: with stay_pen == 0 the end is u = 0 (all stays), with stay_pen > 0 and m <= W it is u = m - 1 (all steps from u = 0)
    -- and the start is what the rule gives, the same in both statements."""
    rng = np.random.default_rng(20240611)
    ties, kinds, small = 0, set(), set()
    for i in range(400):
        q, Lv, cfg, kind = MC.drawn(rng, i)
        a, b = R.by_rows(q, Lv, cfg), R.by_matrix(q, Lv, cfg)
        assert a == b, (i, kind, q, Lv.tolist(), cfg, a, b)
        kinds.add(kind)
        small.add((min(len(q), 3), min(len(Lv), 4)))
        if a is None:
            assert len(q) == 0 or len(Lv) == 0
            continue
        ties += R.has_tie(q, Lv, cfg)
        if kind == "constant" and (cfg[0] == 0 or len(q) <= len(Lv)):
            assert a == (0, 0 if cfg[0] == 0 else len(q) - 1, 0), (i, a)
    assert ties > 100, ties
    assert len(kinds) == 8 and {(m, w) for m in range(3) for w in range(4)} <= small, sorted(small)


def test_row_values_are_the_scale_reference_s():
    """map_ref.row_values against scale_ref.scaled_values, the statement of sqg_scale.h's q that the aligner's tests use: drawn sums up to
    |2^54|, len <= 0 among the lengths, gains and shifts inside and outside their ranges, and no scale (gain 65536, shift 0)"""
    import scale_ref as SR
    rng = np.random.default_rng(8)
    for _ in range(60):
        n = 50
        sums = np.where(rng.random(n) < 0.2, rng.choice([1 << 54, -(1 << 54), (1 << 54) - 1, 0], n), rng.integers(-10 ** 7, 10 ** 7, n))
        lens = rng.integers(-2, 40, n)
        g, sh = int(rng.choice([65536, 1, 0, -5, 1 << 20, (1 << 20) + 1, 30000])), int(rng.choice([0, 1 << 26, (1 << 26) + 1, -(1 << 27), 777]))
        assert R.row_values(sums, lens, g, sh) == SR.scaled_values(sums, lens, g, sh)
        assert R.row_values(sums, lens) == SR.scaled_values(sums, lens, 65536, 0)


def _hand(q, fwd, rev, cfg=(5, 7, 1000, 0, 256, 3), lo=100):
    hi = lo + len(fwd)
    a = R.one_read(q, lo, hi, np.asarray(fwd), np.asarray(rev), cfg, R.by_rows)
    assert a == R.one_read(q, lo, hi, np.asarray(fwd), np.asarray(rev), cfg, R.by_matrix)
    return a


def test_hand_worked_cases():
    """typed out: (cost, step, key0, key1, other), the window starting at 100"""
    fwd = [1000, 2000, 3000, 4000, 5000, 6000]
    far = [900000] * 6
    assert _hand([3000, 4000, 5000], fwd, far) == (0, 1, 102, 104, 3000)                 # a stretch of the track: cost 0, its two ends
    assert _hand([3000, 3000, 4000], fwd, far) == (5, 1, 102, 103, 3000)                 # one stay
    assert _hand([2000, 4000, 5000], fwd, far) == (7, 1, 101, 104, 3000)                 # one skip
    # the tie order: row 1 at u = 2 has step (from u = 1) and skip (from u = 0) both at 0: step, the first, wins, so the start is u = 1
    assert _hand([5, 9], [5, 5, 9], [900000] * 3, cfg=(0, 0, 100, 0, 256, 1)) == (0, 1, 101, 102, -1)
    # a constant track: everything ties, the end is the lowest u, and there the only candidate is the stay
    assert _hand([5, 5, 5], [5, 5, 5, 5], [5, 5, 5, 5], cfg=(0, 0, 100, 0, 256, 3)) == (0, 1, 100, 100, 0)
    # a '-' read: u counts down the forward coordinate, rev[g - lo] is the level at g; key0 > key1
    rev = [6007, 5007, 4007, 3007, 2007, 1007]
    assert _hand([2007, 3007, 4007], fwd, rev) == (0, -1, 104, 102, 21)
    assert _hand([2007, 3007, 4007], fwd, rev, cfg=(5, 7, 1000, 0, 256, 2)) == (0, -1, 104, 102, -1)     # strands = 2
    assert _hand([2007, 3007, 4007], fwd, rev, cfg=(5, 7, 1000, 0, 256, 1)) == (21, 1, 101, 103, -1)     # strands = 1
    # a strand tie goes to '+'
    assert _hand([1000, 2000], [1000, 2000, 3000], [3000, 2000, 1000]) == (0, 1, 100, 101, 0)
    # NONE costs cost_cap; no rows, no window
    assert _hand([1000, 2000], [NONE, NONE], [NONE, NONE]) == (2000, 1, 100, 101, 2000)
    assert _hand([], fwd, far) == (-1, 0, R.I64_MIN, R.I64_MIN, -1) == _hand([5], [], [])
    # row_first and row_count choose the rows
    ro, s, ln = [0, 5], np.array([0, 3000, 4000, 5000, 0]), np.full(5, 256)
    o = R.batch(ro, s, ln, 100, 106, np.asarray(fwd), np.asarray(far), (5, 7, 1000, 1, 3, 3))
    assert [int(o[k][0]) for k in OUT] == [0, 1, 102, 104, 3000]
    assert int(R.batch(ro, s, ln, 100, 106, np.asarray(fwd), np.asarray(far), (5, 7, 1000, 5, 3, 3))["map_step"][0]) == 0      # row_first at the read's end


def test_the_track_rule_by_hand():
    """k = 3, contigs ACGTNACgtA | AC | TTTGGA: a contig seam, an N, lower case, a contig shorter than k, the k-mer that runs past hi, the
    last k - 1 positions of the genome; levels 10 * row, then under SQG_METH the base-5 rows"""
    contigs = [b"ACGTNACgtA", b"AC", b"TTTGGA"]
    g = b"".join(contigs)
    off = np.concatenate(([0], np.cumsum([len(c) for c in contigs])))
    f, r = R.track(g, off, 3, False, 0, len(g), np.arange(64) * 10)
    # ACG CGT GTN TNA NAC ACg Cgt gtA | tA. A.. | AC. C.. | TTT TTG TGG GGA GA. A..      (rows: ACG 6, CGT 27, gtA 44, TTT 63, TTG 62, TGG 58, GGA 40)
    assert f.tolist() == [60, 270, NONE, NONE, NONE, 60, 270, 440, NONE, NONE, NONE, NONE, 630, 620, 580, 400, NONE, NONE]
    # their reverse complements: CGT ACG . . . CGT ACG TAC | . . | . . | AAA CAA CCA TCC . .       (TAC 49, CAA 16, CCA 20, TCC 53)
    assert r.tolist() == [270, 60, NONE, NONE, NONE, 270, 60, 490, NONE, NONE, NONE, NONE, 0, 160, 200, 530, NONE, NONE]
    assert R.track(g, off, 3, False, 0, 1, np.arange(64) * 10)[0].tolist() == [60]             # the k-mer runs past hi
    assert R.track(g, off, 3, False, 7, 7, np.arange(64))[0].tolist() == []
    f, r = R.track(g, off, 3, True, 0, 8, np.arange(125))
    assert f.tolist() == [7, 39, NONE, NONE, NONE, 5, 25, 0]                                     # a lower-case byte has digit 0 on '+' ...
    assert r.tolist() == [39, 7, NONE, NONE, NONE, 39, 7, 4 * 25 + 0 + 1]                        # ... and is a base on '-': TAC
    assert R.track(g, off, 3, False, 0, 2, np.array([1 << 30] * 64))[0].tolist() == [1 << 23] * 2   # levels are clamped


def _fasta(path):
    seqs = []
    for ln in open(path, "rb"):
        if ln.startswith(b">"):
            seqs.append([])
        else:
            seqs[-1].append(ln.strip())
    return [b"".join(s) for s in seqs]


def _levels(level_mean, prof):
    """map_levels() in numpy"""
    return np.clip(np.rint(256.0 * np.asarray(level_mean, np.float32).astype(np.float64) * np.float64(prof.digitisation) / np.float64(prof.range)),
                   -(1 << 23), 1 << 23).astype(np.int32)


def _recovered(out, key0, step, k, row_first=0):
    return (out["map_step"] == step) & (np.abs(out["map_key0"] - (key0 + step.astype(np.int64) * row_first)) <= k)


@functools.lru_cache(maxsize=None)
def _noise_free():
    """64 nCoV reads of 600 bases from the oracle backend, their noise-free rows (256 * level_raw, one per event), and statement (a)'s map of
    the first 96 of them under the shift of Batch.map_shift()"""
    k = 6
    gen = _cpu_gen(k)
    contigs = _fasta(NCOV)
    gen.load_genome(contigs, 600)
    b = gen.sample(64).run().wait()
    reads, s = b.reads(), b.sampled
    genome = b"".join(contigs)
    off = np.concatenate(([0], np.cumsum([len(c) for c in contigs])))
    prof = gen.profile
    fwd, rev = R.track(genome, off, k, False, 0, len(genome), _levels(gen.level_mean, prof))
    sums, row_off = [], [0]
    for r, read in enumerate(reads):
        lvl = gen.level_mean[T.kmer_ranks(read, k, False)].astype(np.float64)
        sums.append(T.to_i16(lvl * np.float64(prof.digitisation) / np.float64(prof.range) - np.float64(b.offset[r])).astype(np.int64))
        row_off.append(row_off[-1] + len(sums[-1]))
    sums = np.concatenate(sums)
    shift = np.rint(256.0 * np.asarray(b.offset, np.float64)).astype(np.int32)
    out = R.batch(row_off, sums, np.ones(len(sums), np.int32), 0, len(genome), fwd, rev, MAPCFG, scale=(np.full(64, 65536), shift))
    key0, step = PR.sampler_origin(off, s["ref_idx"], s["ref_pos"], s["rlen"], s["strand"], k)
    offsets = np.asarray(b.offset, np.float64).copy()
    b.free(); gen.close()
    return out, key0, step, offsets


def test_the_reference_recovers_noise_free_reads():
    """Statement (a) on the noise-free rows of 64 sampled nCoV reads, 96 rows, both strands: at least 0.9 of the reads map to their origin
    within k with the right strand.  Observed: 64 of 64."""
    out, key0, step, _ = _noise_free()
    hit = int(_recovered(out, key0, step, 6).sum())
    print(f"recovered {hit} of 64; strands {sorted(set(step.tolist()))}")
    assert len(set(step.tolist())) == 2
    assert hit >= 0.9 * 64, hit


# ---------------------------------------------------------------------------------------------------------- GPU
def _dev(gen):
    return torch.device("cuda", gen.device)


def _on(gen, a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dt)).to(_dev(gen))


def _map(b, row_off, sums, lens, lo, hi, fwd, rev, cfg, scale=None, outputs=None):
    gen = b.gen
    tr = api.MapTrack(lo, hi, None if fwd is None else _on(gen, fwd, np.int32), None if rev is None else _on(gen, rev, np.int32))
    sc = None if scale is None else tuple(_on(gen, a, np.int32) for a in scale)
    return b.map(row_off, _on(gen, sums, np.int64), _on(gen, lens, np.int32), tr, cfg=cfg, scale=sc, outputs=outputs)


def _check(b, row_off, sums, lens, lo, hi, fwd, rev, cfg, scale=None, what=""):
    want = R.batch(row_off, sums, lens, lo, hi, fwd, rev, cfg, scale=scale)
    got = _map(b, row_off, sums, lens, lo, hi, fwd, rev, cfg, scale)
    for n in OUT:
        t = getattr(got, n)
        assert t.dtype == getattr(torch, np.dtype(R.DTYPES[n]).name) and t.shape == (b.n_reads,)
        np.testing.assert_array_equal(t.cpu().numpy(), want[n], err_msg=f"{what}: {n}")
    return want, got


@pytest.fixture(scope="module")
def ctx():
    gen, prof, fl, k = inject.context("exact1")
    yield gen
    gen.close()


def _batch(gen, n):
    return inject.run_geometry(gen, inject.seqs_for([30 + i for i in range(n)], 6))


def _rows_for(reads_q, rng=None):
    """(row_off, sum, len) of per-read lists of row values"""
    row_off = np.concatenate(([0], np.cumsum([len(q) for q in reads_q]))).astype(np.int64)
    flat = np.asarray([v for q in reads_q for v in q], np.int64)
    s, ln = MC.rows_of(flat, rng)
    return row_off, s, ln


@pytest.mark.gpu
@pytest.mark.parametrize("W", [1, 2, 3, TILE - 1, TILE, TILE + 1, 2 * TILE + 3])
def test_windows_around_the_tile(ctx, W):
    """reads of m in {0, 1, 2, 63, 64, 65, row_count} rows walked along a random track of W positions with NONE runs, on either strand,
    stays and skips among the steps; planted at u = 0, so as to end at u = W - 1, and across the tile seam"""
    rng = np.random.default_rng(W)
    fwd, rev = MC.track_of(rng, W, none_runs=2 if W > 8 else 0)
    ms = [0, 1, 2, 63, 64, 65, 100, 100, 100, 100]
    b = _batch(ctx, len(ms))
    reads = []
    for r, m in enumerate(ms):
        minus = r % 2 == 1
        lv = np.where((rev[::-1] if minus else fwd) == NONE, 0, rev[::-1] if minus else fwd)
        at = (0, 0, 0, 5, W // 2, 1, 0, max(W - 60, 0), max(TILE - 30, 0), max(W - 100, 0))[r] % W
        moves = (1,) if r in (7, 9) else (0, 1, 1, 1, 1, 2)
        reads.append(MC.walk(rng, lv, at, m, moves=moves)[0])
    row_off, s, ln = _rows_for(reads, rng)
    want, _ = _check(b, row_off, s, ln, 1000, 1000 + W, fwd, rev, (300, 500, 20000, 0, 100, 3), what=f"W {W}")
    assert want["map_step"][0] == 0 and (want["map_step"][1:] != 0).all()
    if W > 200:
        assert want["map_key0"][6] == 1000 and want["map_step"][6] == 1                            # planted at u = 0
        assert want["map_key1"][9] == 1000 + W - 1 or want["map_step"][9] == -1                      # ends at u = W - 1
        assert want["map_step"][9] == -1 and want["map_key1"][9] == 1000                             # ('-': u = W - 1 is g = lo)
    if W > TILE:
        assert want["map_key0"][8] < 1000 + TILE <= want["map_key1"][8] and want["map_step"][8] == 1      # across the seam
    b.free()


@pytest.mark.gpu
def test_constant_and_empty_tracks_and_a_ragged_batch(ctx):
    """a constant track (everything ties: the end is u = 0 without a stay penalty, u = m - 1 with one), a track that is NONE everywhere (the cost is m * cost_cap and there is still a
    result), row_first past the read's end, reads without rows between reads with rows"""
    W = TILE + 77
    rng = np.random.default_rng(5)
    reads = [[777] * 40, [], [777] * 3, [], [], [777] * 70, [5] * 10, []]
    b = _batch(ctx, len(reads))
    row_off, s, ln = _rows_for(reads, rng)
    const = np.full(W, 777, np.int32)
    for pens in ((0, 0), (3, 9)):
        want, _ = _check(b, row_off, s, ln, 0, W, const, const, pens + (1000, 0, 64, 3), what="constant")
        assert want["map_key0"][0] == 0 and want["map_key1"][0] == (39 if pens[0] else 0) and want["map_step"][0] == 1 and want["map_cost"][0] == 0
        assert want["map_step"][1] == 0
    nothing = np.full(W, NONE, np.int32)
    want, _ = _check(b, row_off, s, ln, 0, W, nothing, nothing, (3, 9, 1000, 0, 64, 3), what="NONE everywhere")
    assert want["map_cost"].tolist() == [40000, -1, 3000, -1, -1, 64000, 10000, -1]
    want, _ = _check(b, row_off, s, ln, 0, W, const, nothing, (3, 9, 1000, 20, 30, 3), what="row_first")
    assert want["map_step"].tolist() == [1, 0, 0, 0, 0, 1, 0, 0] and want["map_cost"][5] == 0 and want["map_key1"][5] == 29
    _check(b, row_off, s, ln, 7, 7, const[:0], const[:0], (3, 9, 1000, 0, 64, 3), what="W == 0")
    b.free()


@pytest.mark.gpu
@pytest.mark.parametrize("stay,skip,cap", [(0, 0, 1), (1 << 17, 1 << 17, 1 << 17), (0, 1 << 17, 1 << 17), (1 << 17, 0, 1)])
def test_the_bounds_of_a_cell(ctx, stay, skip, cap):
    """4096 rows under the smallest and the largest penalties and caps, over two tiles and a bit: D reaches its bound (4096 caps and 4095
    stays of 2^17 each on a track two positions wide).  (One span holds these windows; the spans whose halo is cut at u = 0 are
    test_one_tile_per_launch_gives_the_same_bytes'.)"""
    rng = np.random.default_rng(stay + cap)
    W = TILE + 40
    fwd, rev = MC.track_of(rng, W, none_runs=1)
    lv = np.where(fwd == NONE, 0, fwd)
    reads = [MC.walk(rng, lv, 3, 4096, jitter=2)[0], [1 << 25] * 4096, MC.walk(rng, lv, TILE - 2000 % TILE, 300)[0]]
    b = _batch(ctx, 3)
    row_off, s, ln = _rows_for(reads)
    _check(b, row_off, s, ln, 0, W, fwd, rev, (stay, skip, cap, 0, 4096, 3), what="bounds")
    two = np.array([-(1 << 23), 1 << 23], np.int32)
    want, _ = _check(b, row_off, s, ln, 0, 2, two, two, (stay, skip, cap, 0, 4096, 3), what="two positions")
    if stay == skip == cap == 1 << 17:
        assert want["map_cost"][1] == 4096 * (1 << 17) + 4094 * (1 << 17)                             # one step, then stays
    b.free()


@pytest.mark.gpu
def test_clamps_of_rows_and_scales(ctx):
    """|sum| at 2^54 with len <= 0, gains and shifts outside their ranges, levels outside +-2^23: all clamped, as the header says"""
    rng = np.random.default_rng(11)
    W = 300
    fwd, rev = MC.track_of(rng, W)
    fwd[:40] = rng.choice([1 << 30, -(1 << 30), (1 << 23) + 1, -(1 << 23) - 1], 40)
    n, m = 8, 20
    b = _batch(ctx, n)
    row_off = np.arange(n + 1, dtype=np.int64) * m
    s = rng.integers(-40000, 40000, n * m) * 256
    ln = np.full(n * m, 256, np.int32)
    s[:m] = rng.choice([1 << 54, -(1 << 54), (1 << 54) - 1], m); ln[:m] = rng.choice([0, -5, 1, 2], m)
    s[m:2 * m] = rng.choice([(1 << 62), -(1 << 62), (1 << 55) + 12345], m); ln[m:2 * m] = 1
    gain = np.array([65536, 1, 0, -7, 1 << 20, (1 << 20) + 1, 1 << 30, 40000], np.int32)
    shift = np.array([0, 1 << 26, (1 << 26) + 1, -(1 << 26) - 1, -(1 << 30), 1 << 30, 77, -3000], np.int32)
    _check(b, row_off, s, ln, -50, W - 50, fwd, rev, (300, 500, 1 << 17, 0, 64, 3), what="no scale")
    _check(b, row_off, s, ln, -50, W - 50, fwd, rev, (300, 500, 1 << 17, 0, 64, 3), scale=(gain, shift), what="wild scale")
    b.free()


@pytest.mark.gpu
def test_outputs_one_at_a_time_and_guards(ctx):
    """every output NULL in turn: the others keep their bytes; the words around every output array stay as they were; strands 1 and 2"""
    rng = np.random.default_rng(3)
    W, n = TILE + 9, 6
    fwd, rev = MC.track_of(rng, W, none_runs=2)
    lv = np.where(fwd == NONE, 0, fwd)
    reads = [MC.walk(rng, lv, int(rng.integers(0, W - 80)), 50)[0] for _ in range(n)]
    reads[2] = []
    b = _batch(ctx, n)
    row_off, s, ln = _rows_for(reads)
    cfg = (300, 500, 20000, 0, 64, 3)
    want, full = _check(b, row_off, s, ln, 10, 10 + W, fwd, rev, cfg)
    for strands in (1, 2):
        w1, _ = _check(b, row_off, s, ln, 10, 10 + W, fwd if strands == 1 else None, rev if strands == 2 else None, cfg[:5] + (strands,))
        assert (w1["map_cost_other"] == -1).all() and set(w1["map_step"].tolist()) == {0, 1 if strands == 1 else -1}
    for skip in OUT:
        got = _map(b, row_off, s, ln, 10, 10 + W, fwd, rev, cfg, outputs=[o for o in OUT if o != skip])
        assert getattr(got, skip) is None
        for o in OUT:
            if o != skip:
                np.testing.assert_array_equal(getattr(got, o).cpu().numpy(), want[o], err_msg=f"without {skip}: {o}")
    # guard words: the outputs as slices of larger tensors full of a pattern, through the library's own entry point
    gen = b.gen
    G = 16
    big = {o: torch.full((n + 2 * G,), 0x5a, dtype=getattr(torch, np.dtype(R.DTYPES[o]).name), device=_dev(gen)) for o in OUT}
    out = api.CMapOut(*(big[o][G:G + n].data_ptr() for o in OUT))
    ds, dl = _on(gen, s, np.int64), _on(gen, ln, np.int32)
    df, dr = _on(gen, fwd, np.int32), _on(gen, rev, np.int32)
    cin, ctr, c = api.CAlignIn(ds.data_ptr(), dl.data_ptr()), api.CMapTrack(10, 10 + W, df.data_ptr(), dr.data_ptr()), api.CMapCfg(*cfg)
    torch.cuda.synchronize()
    b._call("sqg_batch_map", C.byref(c), row_off.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(cin), None, C.byref(ctr), C.byref(out))
    for o in OUT:
        a = big[o].cpu().numpy()
        np.testing.assert_array_equal(a[G:G + n], want[o], err_msg=o)
        assert (a[:G] == 0x5a).all() and (a[G + n:] == 0x5a).all(), o
    b.free()


def _fixed_case(gen):
    rng = np.random.default_rng(77)
    W = 2 * TILE + 3
    fwd, rev = MC.track_of(rng, W, none_runs=3)
    ms = [150, 0, 64, 100, 1, 100, 100, 33, 600, 600, 700]
    reads = []
    for r, m in enumerate(ms):
        minus = r % 2 == 1
        lv = np.where((rev[::-1] if minus else fwd) == NONE, 0, rev[::-1] if minus else fwd)
        at = (TILE - 70, 0, 2 * TILE - 20, TILE + 5, 9, 2 * TILE - 99, 0, TILE - 1, 2, TILE + 300, TILE - 350)[r]
        reads.append(MC.walk(rng, lv, at, m)[0])
    return (fwd, rev, W) + _rows_for(reads, rng)


@pytest.mark.gpu
def test_one_tile_per_launch_gives_the_same_bytes(monkeypatch):
    """k_map_dp walks spans of tiles.  The development library takes a cap N from SQG_TEST_MAP_TILES.  With 1 every tile of a window of
    2 T + 3 positions is a span and a launch of its own, and every read's two wavefronts are: the reads of 600 and 700 rows have a halo
    of two tiles, which is cut at u = 0 in front of the second tile and walked in full in front of the third -- one planted near u = 0,
    one inside the second tile, one across the first seam; the reads of up to 150 rows a halo of one.  With 2 a span is two tiles; with 4
    one span holds the window and a launch two reads, so launches begin at reads other than 0.  The outputs are the bytes of the release
    library's single span and launch, and statement (a)'s."""
    res = []
    for knob in (None, "1", "2", "4"):
        if knob is None:
            monkeypatch.delenv("SQG_TEST_MAP_TILES", raising=False)
        else:
            monkeypatch.setenv("SQG_TEST_MAP_TILES", knob)
        gen, prof, fl, k = inject.context("exact1", lib_path=build.LIB_DEV if knob else None)
        fwd, rev, W, row_off, s, ln = _fixed_case(gen)
        b = _batch(gen, len(row_off) - 1)
        want, got = _check(b, row_off, s, ln, 0, W, fwd, rev, (300, 500, 20000, 0, 1024, 3), what=f"knob {knob}")
        res.append({o: getattr(got, o).cpu().numpy().tobytes() for o in OUT})
        assert {(int(a) >= TILE) for a in want["map_key0"][want["map_step"] == 1]} == {False, True}
        assert want["map_key0"][8] == 2 and TILE <= 2 * TILE + 2 - want["map_key0"][9] < 2 * TILE and want["map_key0"][10] < TILE <= want["map_key1"][10]
        b.free(); gen.close()
    assert res[0] == res[1] == res[2] == res[3]


TOY = [b"ACGTTGCANNNNACGGTACCGTTAGGCATcgatcgatTTGACCAGT" * 6 + b"GATTACA", b"ACGT", b"NNACGTAGCTAGCTAGGATCCGATCGAtcgaGGCTAGCTAGGCTANNNNNNNNCGATCGGATCGATC" * 6 + b"AC"]


def _hip_gen(k, meth=False, T=2, lib_path=None):
    prof, fl = profiles.get_profile("dna-r9-prom")
    mean, stdv = model.synthetic_model(k, meth=True) if meth else model.synthetic_model(k)
    gen = api.SignalGenerator(prof, fl | (profiles.SQ_METH if meth else 0), k, mean, stdv, 42, num_workers=T, mode=api.MODE_CERTIFIED, lib_path=lib_path)
    gen.level_mean = np.asarray(mean, np.float32)
    return gen


@pytest.mark.gpu
@pytest.mark.parametrize("k,meth", [(5, False), (6, False), (9, False), (5, True), (6, True)])
def test_the_track_on_the_device(k, meth):
    """sqg_map_track against the numpy rule: a 3-contig toy genome of about 700 bases with N runs, lower case and a contig shorter than k,
    and the nCoV reference; the whole genome, an empty window, one position, a window inside a contig; fwd only and rev only; levels drawn
    beyond +-2^23 and the binding's map_levels()"""
    gen = _hip_gen(k, meth)
    rng = np.random.default_rng(k)
    rows = 5 ** k if meth else 4 ** k
    drawn = rng.integers(-(1 << 23) - 50, (1 << 23) + 50, rows).astype(np.int32)
    np.testing.assert_array_equal(gen.map_levels().cpu().numpy(), _levels(gen.level_mean, gen.profile))
    for contigs in (TOY, _fasta(NCOV)):
        gen.load_genome(contigs, 200)
        g = b"".join(contigs)
        off = np.concatenate(([0], np.cumsum([len(c) for c in contigs])))
        n = len(g)
        for levels in (drawn, None):
            lv = _levels(gen.level_mean, gen.profile) if levels is None else levels
            wf, wr = R.track(g, off, k, meth, 0, n, lv)
            assert (wf == NONE).sum() == (wr == NONE).sum() > 0
            for lo, hi in ((0, n), (n // 3, n // 3), (n - 1, n), (0, 1), (300, 500), (n - 200, n)):
                tr = gen.new_map_track(lo, hi, levels=None if levels is None else _on(gen, levels, np.int32))
                assert (tr.lo, tr.hi) == (lo, hi)
                np.testing.assert_array_equal(tr.fwd.cpu().numpy(), wf[lo:hi], err_msg=f"fwd [{lo}, {hi})")
                np.testing.assert_array_equal(tr.rev.cpu().numpy(), wr[lo:hi], err_msg=f"rev [{lo}, {hi})")
            tr = gen.new_map_track(levels=_on(gen, lv, np.int32), rev=False)
            assert tr.rev is None and (tr.lo, tr.hi) == (0, n)
            np.testing.assert_array_equal(tr.fwd.cpu().numpy(), wf)
            tr = gen.new_map_track(5, n - 5, levels=_on(gen, lv, np.int32), fwd=False)
            assert tr.fwd is None
            np.testing.assert_array_equal(tr.rev.cpu().numpy(), wr[5:n - 5])
    gen.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k,meth", [(6, False), (9, False), (6, True)])
def test_sampled_ncov_reads(k, meth):
    """64 sampled nCoV reads of 600 bases: the true rows and the detector's, 96 of each, both strands, under Batch.map_shift(), and the true rows
    without a scale on a window inside the genome: the device equals statement (a); twice in a row gives the same bytes; after events, align and call have run on the batch their
    outputs and map's are unchanged.  k = 6 without SQG_METH: the reads statement (a) recovers from noise-free rows are the reads the device
    recovers from the true rows"""
    gen = _hip_gen(k, meth)
    contigs = _fasta(NCOV)
    gen.load_genome(contigs, 600)
    n_g = sum(len(c) for c in contigs)
    b = gen.sample(64).run().wait()
    s = b.sampled
    key0, step = PR.sampler_origin(np.concatenate(([0], np.cumsum([len(c) for c in contigs]))), s["ref_idx"], s["ref_pos"], s["rlen"], s["strand"], k)
    tr = gen.new_map_track()
    fwd, rev = tr.fwd.cpu().numpy(), tr.rev.cpu().numpy()
    ev = b.events(outputs=("sum", "ev_len", "level_raw"))
    dt = b.detect(outputs=("sum", "dt_len"))
    gain, shift = b.map_shift()
    assert gain.tolist() == [65536] * 64 and shift.cpu().numpy().tolist() == np.rint(256.0 * b.offset).astype(np.int64).tolist()
    sc = (gain.cpu().numpy(), shift.cpu().numpy())
    first = {}
    for name, (off, sm, ln) in (("true", (b.ev_off, ev.sum, ev.ev_len)), ("detected", (dt.det_off, dt.sum, dt.dt_len))):
        want = R.batch(off, sm.cpu().numpy(), ln.cpu().numpy(), 0, n_g, fwd, rev, MAPCFG, scale=sc)
        got = b.map(off, sm, ln, tr, cfg=MAPCFG, scale=(gain, shift))
        for o in OUT:
            np.testing.assert_array_equal(getattr(got, o).cpu().numpy(), want[o], err_msg=f"{name} rows: {o}")
        first[name] = want
    # without a scale, on a window inside the genome: rows in stored codes are an offset away from the levels
    lo, hi = 7001, 10003
    cut = api.MapTrack(lo, hi, tr.fwd[lo:hi].contiguous(), tr.rev[lo:hi].contiguous())
    want = R.batch(b.ev_off, ev.sum.cpu().numpy(), ev.ev_len.cpu().numpy(), lo, hi, fwd[lo:hi], rev[lo:hi], MAPCFG)
    got = b.map(b.ev_off, ev.sum, ev.ev_len, cut, cfg=MAPCFG)
    for o in OUT:
        np.testing.assert_array_equal(getattr(got, o).cpu().numpy(), want[o], err_msg=f"true rows, no scale, [{lo}, {hi}): {o}")
    hit = _recovered(first["true"], key0, step, k)
    print(f"k {k} meth {meth}: true rows recovered {int(hit.sum())} of 64, detected {int(_recovered(first['detected'], key0, step, k).sum())}, "
          f"true rows without a scale on [{lo}, {hi}) {int(_recovered(want, key0, step, k).sum())}")
    if k == 6 and not meth:
        ref, rkey0, rstep, roff = _noise_free()
        np.testing.assert_array_equal(rkey0, key0); np.testing.assert_array_equal(rstep, step); np.testing.assert_array_equal(roff, b.offset)
        np.testing.assert_array_equal(hit, _recovered(ref, key0, step, k))
    # twice in a row, and around the other consumer calls
    again = b.map(b.ev_off, ev.sum, ev.ev_len, tr, cfg=MAPCFG, scale=(gain, shift))
    al = b.align(b.ev_off, ev.sum, ev.ev_len)
    ev2 = b.events(outputs=("sum", "ev_len", "level_raw"))
    cl = b.call(ev.sum, ev.ev_len) if meth else None
    third = b.map(b.ev_off, ev.sum, ev.ev_len, tr, cfg=MAPCFG, scale=(gain, shift))
    for o in OUT:
        np.testing.assert_array_equal(getattr(again, o).cpu().numpy(), first["true"][o])
        np.testing.assert_array_equal(getattr(third, o).cpu().numpy(), first["true"][o])
    al2 = b.align(b.ev_off, ev.sum, ev.ev_len)
    for o in api.ALIGN_OUTPUTS:
        assert torch.equal(getattr(al, o), getattr(al2, o)), o
    for o in ("sum", "ev_len", "level_raw"):
        assert torch.equal(getattr(ev, o), getattr(ev2, o)), o
    if meth:
        cl2 = b.call(ev.sum, ev.ev_len)
        for o in ("llr", "call", "site_key"):
            assert torch.equal(getattr(cl, o), getattr(cl2, o)), o
    b.free(); gen.close()


@pytest.mark.gpu
def test_every_error_names_its_field_and_leaves_the_context_usable(ctx):
    gen = ctx
    rng = np.random.default_rng(1)
    W, n = 200, 3
    fwd, rev = MC.track_of(rng, W)
    reads = [MC.walk(rng, fwd, 10 * r, 30)[0] for r in range(n)]
    b = _batch(gen, n)
    row_off, s, ln = _rows_for(reads)
    ds, dl, df, dr = _on(gen, s, np.int64), _on(gen, ln, np.int32), _on(gen, fwd, np.int32), _on(gen, rev, np.int32)
    gs = torch.full((n,), 65536, dtype=torch.int32, device=_dev(gen))
    outs = {o: torch.zeros(n, dtype=getattr(torch, np.dtype(R.DTYPES[o]).name), device=_dev(gen)) for o in OUT}
    good = dict(cfg=api.CMapCfg(300, 500, 20000, 0, 64, 3), row_off=row_off, cin=api.CAlignIn(ds.data_ptr(), dl.data_ptr()), scale=None,
                track=api.CMapTrack(0, W, df.data_ptr(), dr.data_ptr()), out=api.CMapOut(*(outs[o].data_ptr() for o in OUT)))

    def call(**kw):
        a = dict(good, **kw)
        ref = lambda v: None if v is None else C.byref(v)       # noqa: E731
        ro = a["row_off"]
        return gen.L.sqg_batch_map(gen.ctx, b.handle, ref(a["cfg"]), None if ro is None else ro.ctypes.data_as(C.POINTER(C.c_int64)), ref(a["cin"]),
                                   ref(a["scale"]), ref(a["track"]), ref(a["out"]))

    def works(bb=None):
        _check(bb or b, row_off, s, ln, 0, W, fwd, rev, (300, 500, 20000, 0, 64, 3), what="after an error")

    EINVAL, ESEQ = -1, -4
    bad = [(dict(cfg=None), "cfg"), (dict(row_off=None), "row_off"), (dict(cin=None), "in"), (dict(cin=api.CAlignIn(None, dl.data_ptr())), "in->sum"),
           (dict(cin=api.CAlignIn(ds.data_ptr(), None)), "in->len"), (dict(track=None), "track"), (dict(out=None), "out"),
           (dict(scale=api.CAlignScale(None, gs.data_ptr())), "scale->gain"), (dict(scale=api.CAlignScale(gs.data_ptr(), None)), "scale->shift"),
           (dict(cfg=api.CMapCfg(-1, 500, 20000, 0, 64, 3)), "stay_pen"), (dict(cfg=api.CMapCfg((1 << 17) + 1, 500, 20000, 0, 64, 3)), "stay_pen"),
           (dict(cfg=api.CMapCfg(300, -1, 20000, 0, 64, 3)), "skip_pen"), (dict(cfg=api.CMapCfg(300, (1 << 17) + 1, 20000, 0, 64, 3)), "skip_pen"),
           (dict(cfg=api.CMapCfg(300, 500, 0, 0, 64, 3)), "cost_cap"), (dict(cfg=api.CMapCfg(300, 500, (1 << 17) + 1, 0, 64, 3)), "cost_cap"),
           (dict(cfg=api.CMapCfg(300, 500, 20000, -1, 64, 3)), "row_first"), (dict(cfg=api.CMapCfg(300, 500, 20000, 0, 0, 3)), "row_count"),
           (dict(cfg=api.CMapCfg(300, 500, 20000, 0, 4097, 3)), "row_count"), (dict(cfg=api.CMapCfg(300, 500, 20000, 0, 64, 0)), "strands"),
           (dict(cfg=api.CMapCfg(300, 500, 20000, 0, 64, 4)), "strands"), (dict(track=api.CMapTrack(5, 4, df.data_ptr(), dr.data_ptr())), "hi"),
           (dict(track=api.CMapTrack(0, (1 << 24) + 1, df.data_ptr(), dr.data_ptr())), "1<<24"),
           (dict(track=api.CMapTrack(0, W, None, dr.data_ptr())), "track->fwd"), (dict(track=api.CMapTrack(0, W, df.data_ptr(), None)), "track->rev"),
           (dict(row_off=np.array([1, 30, 60, 90], np.int64)), "row_off"), (dict(row_off=np.array([0, 60, 30, 90], np.int64)), "row_off"),
           (dict(row_off=np.array([0, 1 << 31, 1 << 31, 1 << 31], np.int64)), "2^31 rows")]
    for kw, field in bad:
        assert call(**kw) == EINVAL, field
        msg = gen.L.sqg_last_error(gen.ctx).decode()
        assert "sqg_batch_map" in msg and field in msg, (field, msg)
        works()
    assert call() == 0
    # a batch that has not been run
    st = gen.stage(inject.seqs_for([40, 41, 42], 6))
    rc = gen.L.sqg_batch_map(gen.ctx, st.handle, C.byref(good["cfg"]), row_off.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(good["cin"]), None,
                             C.byref(good["track"]), C.byref(good["out"]))
    assert rc == ESEQ and "has not been run" in gen.L.sqg_last_error(gen.ctx).decode()
    st.run().wait(); st.free()
    works()
    # sqg_map_track: no genome, then the window
    lv = gen.map_levels()
    one = torch.zeros(8, dtype=torch.int32, device=_dev(gen))
    assert gen.L.sqg_map_track(gen.ctx, 0, 4, lv.data_ptr(), one.data_ptr(), None) == ESEQ and "no genome" in gen.L.sqg_last_error(gen.ctx).decode()
    works()
    gen.load_genome([b"ACGTACGTTTGACCA" * 4], 30)
    for lo, hi, levels, field in ((-1, 4, lv, "lo"), (5, 4, lv, "hi"), (0, 61, lv, "hi"), (0, 4, None, "levels")):
        assert gen.L.sqg_map_track(gen.ctx, lo, hi, None if levels is None else levels.data_ptr(), one.data_ptr(), None) == EINVAL
        msg = gen.L.sqg_last_error(gen.ctx).decode()
        assert "sqg_map_track" in msg and field in msg, msg
        works()
    assert gen.L.sqg_map_track(gen.ctx, 0, 4, lv.data_ptr(), one.data_ptr(), None) == 0 and (one[4:] == 0).all()
    works()
    # a batch whose device results have gone to later batches
    for _ in range(3):
        later = _batch(gen, n)
    assert call() == ESEQ and "handed to a later batch" in gen.L.sqg_last_error(gen.ctx).decode()
    works(later)
    later.free(); b.free()
    # the contexts: SQG_RNA and SQG_PREFIX are refused by both calls, and the message says which
    for name, extra, flag in (("rna-r9-prom", 0, "SQG_RNA"), ("dna-r9-prom", profiles.SQ_PREFIX, "SQG_PREFIX")):
        prof, fl = profiles.get_profile(name)
        kk = profiles.default_kmer_size(fl)
        mean, stdv = model.synthetic_model(kk)
        g2 = api.SignalGenerator(prof, fl | extra, kk, mean, stdv, 42, num_workers=1)
        with pytest.raises(api.SqgError) as e:
            g2.new_map_track(0, 0, levels=torch.zeros(4 ** kk, dtype=torch.int32, device=_dev(g2)))
        assert e.value.code == EINVAL and flag in str(e.value) and "sqg_map_track" in str(e.value)
        b2 = g2.submit(inject.seqs_for([60], kk))
        with pytest.raises(api.SqgError) as e:
            b2.map([0, 0], torch.zeros(1, dtype=torch.int64, device=_dev(g2)), torch.zeros(1, dtype=torch.int32, device=_dev(g2)),
                   api.MapTrack(0, 0, None, None))
        assert e.value.code == EINVAL and flag in str(e.value) and "sqg_batch_map" in str(e.value)
        b2.free(); g2.close()
