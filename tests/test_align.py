"""include/sqg_align.h: banded alignment of event rows to the true events of their read (sqg_batch_align), against the two plain numpy
statements of the header's rule (align_ref.py): (a) the banded recurrence for everything, (b) the full matrix for reads of at most 32
events.  Every comparison is bit for bit.  Every case passes its cfg explicitly: none depends on SQG_ALIGN_DEFAULT."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (before the library is loaded: the HIP runtime torch brings is the one the library then uses)

import align_ref as A
import inject
import orc
from chunk_support import _context, _declared, _fixture_reads
from refvec_cases import REFVEC_CASES
from squigulator_amd import api, build, model, profiles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_LIB = os.path.join(ROOT, "oracle", "libsqg_cpu.so")
OUT = ("al_ev", "al_cost", "al_edge")
DTYPES = dict(al_ev=np.int64, al_cost=np.int64, al_edge=np.int32)
CFG = (256, 1024, 16384)
CFGS = {"plain": CFG, "free": (0, 0, 1 << 24), "stay_free": (0, 4096, 4096), "skip_free": (4096, 0, 65536)}
TILE = 64   # k_align.h fetches q, and walks the trace back, 64 rows at a time; a lane's Lv registers hold 64 targets each


# ---------------------------------------------------------------------------------------------------------- no GPU
def test_header_declares_the_align_export_and_the_libraries_have_it():
    assert _declared("sqg_align.h") == set(api.EXPORTS_ALIGN) == {"sqg_batch_align"}
    others = (set(api.EXPORTS) | set(api.EXPORTS_CHUNKS) | set(api.EXPORTS_TARGETS) | set(api.EXPORTS_SEGMENTS) | set(api.EXPORTS_SITES)
              | set(api.EXPORTS_EVENTS) | set(api.EXPORTS_PILEUP) | set(api.EXPORTS_DETECT))
    assert not set(api.EXPORTS_ALIGN) & others
    build.build()
    for lib in (build.LIB, build.LIB_DEV):
        assert hasattr(api.load_library(lib), "sqg_batch_align"), f"sqg_batch_align not exported by {lib}"
    assert os.path.join(ROOT, "include", "sqg_align.h") in build.headers()
    for h in ("k_align.h", "h_align.h"):
        assert os.path.join(ROOT, "squigulator_amd", "csrc", h) in build.headers()
    raw = open(os.path.join(ROOT, "include", "sqg_align.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for struct, ctype in (("sqg_align_cfg_t", api.CAlignCfg), ("sqg_align_in_t", api.CAlignIn), ("sqg_align_out_t", api.CAlignOut)):
        body = hdr[:hdr.index("} " + struct)]
        body = body[body.rindex("typedef struct"):]
        fields = [f[0] for f in ctype._fields_]
        at = [body.index(name + ";") for name in fields]     # every field is declared, in the binding's order
        assert at == sorted(at), f"{struct}: {fields}"
        assert body.count(";") == len(fields), f"{struct}: the header has fields the binding lacks"
    assert [f[0] for f in api.CAlignCfg._fields_] == ["stay_pen", "skip_pen", "cost_cap"] and C.sizeof(api.CAlignCfg) == 12
    assert [f[0] for f in api.CAlignIn._fields_] == ["sum", "len"] and tuple(f[0] for f in api.CAlignOut._fields_) == OUT == api.ALIGN_OUTPUTS
    got = re.search(r"#define\s+SQG_ALIGN_DEFAULT\s*\{([^}]*)\}", hdr).group(1).split(",")
    assert tuple(int(v) for v in got) == api.ALIGN_DEFAULT
    assert got[0].strip() in "0 256 1024 4096".split() and got[1].strip() in "0 256 1024 4096".split() and got[2].strip() in "4096 16384 65536".split()
    assert int(re.search(r"#define\s+SQG_ALIGN_BAND\s+(\d+)", hdr).group(1)) == api.ALIGN_BAND == A.BAND == 64
    assert "exact integers" in raw and "FIRST candidate" in raw and "of the arithmetic only, never of memory" in raw and "at most two targets" in raw
    assert "SQG_ABI_VERSION is unchanged" in raw and "sqg_batch_align" not in open(os.path.join(ROOT, "include", "sqg.h")).read()


def test_the_cpu_backend_has_no_aligner_and_says_so():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "libsqg_cpu.so"])
    prof, fl = profiles.get_profile("dna-r9-prom")
    mean, stdv = model.synthetic_model(6)
    gen = api.SignalGenerator(prof, fl, 6, mean, stdv, 42, lib_path=CPU_LIB)
    assert not hasattr(gen.L, "sqg_batch_align")
    b = gen.submit([b"ACGTACGTACGTTTGACA" * 40])
    with pytest.raises(api.SqgError) as e:
        b.align(np.zeros(2, np.int64), None, None, CFG)
    assert e.value.code == -1 and "sqg_batch_align" in str(e.value)
    b.free(); gen.close()


def test_helpers_on_hand_worked_reads():
    """typed out: rows that are the targets themselves, a stay, a skip, the tie-break order, the floor, the end's skip charge"""
    lv = [256 * v for v in (100, 300, 200, 500)]
    for one in (A.banded, A.full):
        js, cost, edge = one(lv, lv, CFG)                   # the diagonal
        assert js.tolist() == [0, 1, 2, 3] and (cost, edge) == (0, 0)
        js, cost, edge = one([lv[0], lv[1], lv[1] + 7, lv[2], lv[3]], lv, CFG)         # one row more: a stay on target 1
        assert js.tolist() == [0, 1, 1, 2, 3] and (cost, edge) == (7 + 256, 0)
        js, cost, edge = one([lv[0], lv[1], lv[3] - 2], lv, CFG)                       # one row fewer: target 2 is skipped
        assert js.tolist() == [0, 1, 3] and (cost, edge) == (2 + 1024, 0)
        js, cost, edge = one([lv[0]], lv, CFG)              # one row: it ends on target 0 and pays for the three behind it
        assert js.tolist() == [0] and (cost, edge) == (3 * 1024, 0)
        js, cost, edge = one([lv[3]], lv, (256, 10, 16384)) # ... or starts on target 3 and pays for the three in front
        assert js.tolist() == [3] and (cost, edge) == (30, 0)
        # all cell costs tie (one level, rows on it): with no penalty at all the end is the LOWEST target of the last row, and a path
        # that can only stay; with a skip penalty the end is the last target, and step, the first candidate, wins every tie on the way back
        js, cost, edge = one([5] * 6, [5] * 4, (0, 0, 100))
        assert cost == 0 and js.tolist() == [0] * 6
        js, cost, edge = one([5] * 6, [5] * 4, (0, 1, 100))
        assert cost == 0 and js.tolist() == [0, 0, 0, 1, 2, 3]
        assert one([], lv, CFG)[1:] == (-1, 0) and one([1, 2], [], CFG)[0].tolist() == [-1, -1] and one([1, 2], [], CFG)[1:] == (-1, 0)
    assert A.row_values([-1, 1, -256, 7, 5, -(1 << 54)], [256, 256, 3, 0, -9, 1]) == [-1, 1, -21846, 1792, 1280, -(1 << 62)]


def _random_case(rng, T, m, levels, jitter):
    lv = [256 * int(v) for v in rng.choice(levels, T)]
    q = [256 * int(v) + int(rng.integers(-jitter, jitter + 1)) for v in rng.choice(levels, m)]
    return q, lv


def test_the_two_statements_of_the_rule_agree():
    """reads of at most 32 events: the band never moves, so the banded recurrence and the full matrix are the same programme.  Two levels
    and no jitter make most costs tie; penalties of 0 make the candidates tie"""
    rng = np.random.default_rng(3)
    n_ties = 0
    for trial in range(400):
        T, m = int(rng.integers(0, 33)), int(rng.integers(0, 50))
        levels, jitter = ((400, 700), 0) if trial % 2 else (np.arange(300, 900, 50), 40)
        q, lv = _random_case(rng, T, m, levels, jitter)
        cfg = [CFG, (0, 0, 100000), (0, 0, 1), (1 << 24, 0, 77), (0, 1 << 24, 1 << 24), (300, 300, 300)][trial % 6]
        a, b = A.banded(q, lv, cfg), A.full(q, lv, cfg)
        assert a[0].tolist() == b[0].tolist() and a[1:] == b[1:], (trial, T, m, cfg)
        assert a[2] == 0 and (m == 0 or T == 0) == (a[1] == -1)
        n_ties += int(m > 2 and T > 2 and len(set(q)) < m)
    assert n_ties > 100
    q, lv = _random_case(rng, 32, 90, (500,), 0)            # every cost ties everywhere
    assert A.banded(q, lv, (0, 0, 9))[0].tolist() == A.full(q, lv, (0, 0, 9))[0].tolist()


def test_the_band_moves_with_the_path():
    """(a) alone: 300 distinct levels and rows that are the targets, then the targets merged in pairs and split in three.  The path is the
    diagonal, the band follows it, and no row lies on the rim"""
    rng = np.random.default_rng(8)
    lv = [256 * int(v) for v in rng.permutation(np.arange(200, 3200, 10))]
    js, cost, edge = A.banded(lv, lv, CFG)
    assert js.tolist() == list(range(300)) and (cost, edge) == (0, 0)
    js, cost, edge = A.banded(lv[1::2], lv, CFG)            # every second target: skip moves, the band shifts by 2
    assert js.tolist() == list(range(1, 300, 2)) and cost == 150 * 1024 and edge == 0
    js, cost, edge = A.banded(np.repeat(lv, 3).tolist(), lv, CFG)
    assert js.tolist() == np.repeat(np.arange(300), 3).tolist() and cost == 600 * 256 and edge == 0
    js, cost, edge = A.banded(lv[2::3], lv, CFG)            # every third: a row moves two targets at the most, the path is lost.  Every
    assert js.tolist() != list(range(2, 300, 3)) and cost >= 200 * 1024      # target that no row visits is charged skip_pen, 200 at least


def test_the_compiled_statement_is_the_banded_recurrence():
    """orc.align_banded, the oracle's plain C statement of the rule (the sharded suite's references walk hundreds of thousands of rows
    with it), against (a) bit for bit: the tie-heavy reads of the test above with T up to 400 and m up to 600 (the band moves), every
    penalty at 0 and at its maximum, the hand-made paths of the band test, rows far off every target, negative and huge q, no rows and
    no targets"""
    rng = np.random.default_rng(5)

    def same(q, lv, cfg, what):
        a, b = A.banded(q, lv, cfg), orc.align_banded(q, lv, cfg)
        assert a[0].tolist() == b[0].tolist() and a[1:] == b[1:] and b[0].dtype == np.int64, (what, cfg, a[1:], b[1:])
        return a

    cfgs = [CFG, api.ALIGN_DEFAULT, (0, 0, 100000), (0, 0, 1), (1 << 24, 0, 77), (0, 1 << 24, 1 << 24), (300, 300, 300), (1 << 24, 1 << 24, 1 << 24), (0, 1, 100)]
    n_ties = n_edge = n_moved = 0
    for trial in range(300):
        big = trial % 3 == 0
        T, m = int(rng.integers(0, 400 if big else 70)), int(rng.integers(0, 600 if big else 90))
        levels, jitter = ((400, 700), 0) if trial % 2 else (np.arange(300, 900, 50), 40)
        q, lv = _random_case(rng, T, m, levels, jitter)
        js, cost, edge = same(q, lv, cfgs[trial % len(cfgs)], trial)
        n_ties += int(m > 2 and T > 2 and len(set(q)) < m); n_edge += int(edge > 0); n_moved += int(len(js) > 0 and js.max() > 80)
    assert n_ties > 100 and n_edge > 5 and n_moved > 20, (n_ties, n_edge, n_moved)
    lv = [256 * int(v) for v in rng.permutation(np.arange(200, 3200, 10))]
    for q in (lv, lv[1::2], np.repeat(lv, 3).tolist(), lv[2::3], [40000 * 256] * 500, [-(1 << 60), 1 << 60] * 40, [5] * 6):
        for cfg in cfgs:
            same(q, lv, cfg, "made-up rows")
    for q, t in (([], lv), ([1, 2], []), ([], []), ([7], lv[:1]), ([1 << 61, -(1 << 62), 3], lv[:40])):
        same(q, t, CFG, "edges")


# ---------------------------------------------------------------------------------------------------------- GPU
def _dev(b):
    return torch.device("cuda", b.gen.device)


def _table(b):
    """the batch's true table: level_raw, sum, ev_len of every event (sqg_batch_events, pinned by its own tests)"""
    ev = b.events(outputs=("level_raw", "sum", "ev_len"))
    return ev.level_raw.cpu().numpy(), ev.sum.cpu().numpy(), ev.ev_len.cpu().numpy()


def _align(b, row_off, sums, lens, cfg, outputs=None):
    s = torch.from_numpy(np.ascontiguousarray(sums, np.int64)).to(_dev(b))
    n = torch.from_numpy(np.ascontiguousarray(lens, np.int32)).to(_dev(b))
    return b.align(row_off, s, n, cfg, outputs)


def _assert_equal(got, want, what):
    for key in OUT:
        g = getattr(got, key).cpu().numpy()
        assert g.dtype == DTYPES[key] and g.shape == want[key].shape, f"{what}: {key} {g.dtype} {g.shape}"
        np.testing.assert_array_equal(g, want[key], err_msg=f"{what}: {key}")


def _check(b, row_off, sums, lens, cfg, rna, level, what):
    """the three outputs against (a); the reads of at most 32 events against (b) as well.  -> (a)'s outputs"""
    row_off = np.asarray(row_off, np.int64)
    want = A.batch(row_off, sums, lens, b.ev_off, level, rna, cfg)
    got = _align(b, row_off, sums, lens, cfg)
    _assert_equal(got, want, what)
    ev, cost, edge = (getattr(got, k).cpu().numpy() for k in OUT)
    for r in range(b.n_reads):
        e0, e1, a, z = int(b.ev_off[r]), int(b.ev_off[r + 1]), int(row_off[r]), int(row_off[r + 1])
        if e1 - e0 <= 32:
            lv = level[e0:e1].astype(np.int64) * 256
            js, c, e = A.full(A.row_values(sums[a:z], lens[a:z]), [int(v) for v in (lv[::-1] if rna else lv)], cfg)
            np.testing.assert_array_equal(ev[a:z], np.where(js < 0, -1, (e1 - 1 - js) if rna else (e0 + js)), err_msg=f"{what}: read {r} against the full matrix")
            assert (cost[r], edge[r]) == (c, e), f"{what}: read {r} against the full matrix"
    return want


def _stored_order(b, rna):
    """the batch's event indices, every read's in stored-sample order"""
    idx = np.arange(b.n_events, dtype=np.int64)
    if rna:
        for r in range(b.n_reads):
            idx[int(b.ev_off[r]):int(b.ev_off[r + 1])] = idx[int(b.ev_off[r]):int(b.ev_off[r + 1])][::-1]
    return idx


TWO_WORKERS = "nCoV-2019.reference.fasta -x dna-r9-prom -n 4 --seed 42 -r 1000 -t 2 -K 2"
# id -> (command line of the context, fixture the reads are taken from, a read shorter than a k-mer or None)
TRUTH = {
    "dna_r9": (dict(REFVEC_CASES)["r9_t1"], "r9_t1", b"ACGTA"),
    "dna_r10": (dict(REFVEC_CASES)["r10_t1"], "r10_t1", None),
    "rna": (dict(REFVEC_CASES)["rna004_noprefix"], "rna004_noprefix", b"ACGUACGU"),
    "rna_prefix": (dict(REFVEC_CASES)["rna004_prefix"], "rna004_prefix", b"ACGU"),
    "dna_prefix": (dict(REFVEC_CASES)["r9_prefix"], "r9_prefix", b"AC"),
    "meth": (dict(REFVEC_CASES)["r9_meth_dense"], "r9_meth_dense", None),
    "constant_dwell": (dict(REFVEC_CASES)["r9_ideal_time"], "r9_ideal_time", None),
    "two_workers": (TWO_WORKERS, "r9_t1", None),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TRUTH))
def test_truth_as_rows(name):
    """the true table's own sum / ev_len in stored order as the rows: row_off is ev_off.  With the noise of the signal the best path
    is not the diagonal everywhere; what is asserted is (a), bit for bit, and that every read's path ascends through its own targets"""
    cmd, cid, short = TRUTH[name]
    o, k, gen = _context(cmd, api.MODE_CERTIFIED)
    rna = bool(o.flags & profiles.SQ_RNA)
    seqs = [r["seq"] for r in _fixture_reads(cid)[:3]]
    if short is not None:
        assert len(short) < k
        seqs.insert(1, short)
    b = gen.stage(seqs).run().wait()
    if short is not None and not o.flags & profiles.SQ_PREFIX:
        assert b.ev_off[2] - b.ev_off[1] == 5               # the five stand-in events; behind an attached prefix the chain is longer than a k-mer
    level, sums, lens = _table(b)
    idx = _stored_order(b, rna)
    for cfg in (CFG, CFGS["free"]):
        want = _check(b, b.ev_off, sums[idx], lens[idx], cfg, rna, level, f"{name} {cfg}")
        print(f"{name} {cfg}: {(want['al_ev'] == idx).mean():.3f} of the rows on their own event, al_edge {want['al_edge'].tolist()}")
        for r in range(b.n_reads):
            ev = want["al_ev"][int(b.ev_off[r]):int(b.ev_off[r + 1])]
            assert (ev >= b.ev_off[r]).all() and (ev < b.ev_off[r + 1]).all() and (np.diff(ev) * (-1 if rna else 1) >= 0).all()
        assert (want["al_cost"] >= 0).all()
    b.free(); gen.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ("r10_t1", "rna004_prefix"))
def test_detected_rows(cid):
    """sqg_batch_detect's sum / dt_len / det_off under both presets, the tensors handed on as they are"""
    o, k, gen = _context(dict(REFVEC_CASES)[cid], api.MODE_CERTIFIED)
    rna = bool(o.flags & profiles.SQ_RNA)
    b = gen.stage([r["seq"] for r in _fixture_reads(cid)[:3]]).run().wait()
    level, _, _ = _table(b)
    for preset in ("dna", "rna"):
        dt = b.detect(preset, outputs=("sum", "dt_len", "true_ev"))
        assert dt.n_rows > b.n_reads
        got = b.align(dt.det_off, dt.sum, dt.dt_len, CFG)
        want = A.batch(dt.det_off, dt.sum.cpu().numpy(), dt.dt_len.cpu().numpy(), b.ev_off, level, rna, CFG)
        _assert_equal(got, want, f"{cid} {preset}")
        assert got.n_rows == dt.n_rows and (got.row_off == dt.det_off).all()
        ev = got.al_ev.cpu().numpy()
        for r in range(b.n_reads):                          # every row is aligned to an event of its own read
            rows = ev[int(dt.det_off[r]):int(dt.det_off[r + 1])]
            assert (rows >= b.ev_off[r]).all() and (rows < b.ev_off[r + 1]).all() and (np.diff(rows) * (-1 if rna else 1) >= 0).all()
    b.free(); gen.close()


def _geometry(counts, seed=3):
    """a DNA batch of reads with the given numbers of events, one sample per event (inject's exact1), and its true table"""
    gen, prof, fl, k = inject.context("exact1")
    b = inject.run_geometry(gen, inject.seqs_for([t + k - 1 for t in counts], seed))
    assert np.diff(b.ev_off).tolist() == list(counts)
    return gen, b, _table(b)


def _rows_of(level, ev_off, r, kind, m=None):
    """made-up rows of read r from its targets' levels: (sums, lens).  exact: one row per target, on its level; pairs: the targets
    merged two by two (the mean of the two levels); thirds: every target three times; m given: m rows spread evenly over the read"""
    lv = level[int(ev_off[r]):int(ev_off[r + 1])].astype(np.int64)
    T = len(lv)
    if m is not None:
        at = (np.arange(m) * T) // max(m, 1) if T else np.zeros(m, np.int64)
        return (lv[at] * 3 if T else np.full(m, 1000, np.int64)), np.full(m, 3, np.int32)
    if kind == "pairs":
        lv2 = np.concatenate((lv, lv[-1:])) if T & 1 else lv
        return lv2[0::2] + lv2[1::2], np.full(len(lv2) // 2, 2, np.int32)
    if kind == "thirds":
        return np.repeat(lv, 3) * 5 + np.tile([-2, 0, 2], T), np.full(3 * T, 5, np.int32)
    return lv * 7, np.full(T, 7, np.int32)


def _concat(parts):
    sums = np.concatenate([p[0] for p in parts]).astype(np.int64) if parts else np.zeros(0, np.int64)
    lens = np.concatenate([p[1] for p in parts]).astype(np.int32) if parts else np.zeros(0, np.int32)
    return np.concatenate(([0], np.cumsum([len(p[0]) for p in parts]))).astype(np.int64), sums, lens


EVENT_COUNTS = [1, 2, 31, 32, 33, 63, 64, 65, 200, 1500]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["exact", "pairs", "thirds"])
def test_geometry_of_the_targets(kind):
    """T from 1 to 1500 around the band's 64 cells, its half (where the band starts to move) and the two 64-target registers of a lane;
    m = T, about T / 2 (the skip move, the band shifts by 2) and 3 T (stays)"""
    gen, b, (level, _, _) = _geometry(EVENT_COUNTS)
    row_off, sums, lens = _concat([_rows_of(level, b.ev_off, r, kind) for r in range(b.n_reads)])
    for name in ("plain", "free", "stay_free"):
        want = _check(b, row_off, sums, lens, CFGS[name], False, level, f"{kind} {name}")
    if kind == "exact":                                     # checked on the reference: the diagonal, free of cost
        assert (want["al_ev"] == np.arange(b.n_events)).all() and (want["al_cost"] == 0).all() and (want["al_edge"] == 0).all()
    b.free(); gen.close()


@pytest.mark.gpu
def test_geometry_of_the_rows():
    """m of 1, 63, 64, 65, 129 and around two and three of the kernel's tiles of 64 rows, against T of 5, 32, 64 and 700; a read without
    rows between reads with rows, as the first read and as the last one"""
    ms = [1, 63, 64, 65, 129, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1, 3 * TILE]
    counts = [5, 32, 64, 700]
    gen, b, (level, _, _) = _geometry([40] + [t for t in counts for _ in ms] + [40, 40, 40])
    rows = [0] + ms * len(counts) + [0, 50, 0]
    row_off, sums, lens = _concat([_rows_of(level, b.ev_off, r, None, m=m) for r, m in enumerate(rows)])
    for name in ("plain", "skip_free"):
        want = _check(b, row_off, sums, lens, CFGS[name], False, level, f"rows {name}")
        empty = np.diff(row_off) == 0
        assert empty.sum() == 3 and (want["al_cost"][empty] == -1).all() and (want["al_cost"][~empty] >= 0).all()
    b.free(); gen.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n_reads", [1, 63, 64, 65, 130])
def test_batch_shapes(n_reads):
    """one wavefront per read: batches of 1 to 130 reads of mixed lengths, 1 to 400 events, each with rows of its own kind"""
    rng = np.random.default_rng(n_reads)
    counts = ([400, 1] + rng.integers(1, 150, max(n_reads - 2, 0)).tolist())[:n_reads]
    gen, b, (level, _, _) = _geometry(counts, seed=n_reads)
    kinds = ["exact", "pairs", "thirds"]
    row_off, sums, lens = _concat([_rows_of(level, b.ev_off, r, kinds[r % 3]) for r in range(n_reads)])
    sums = sums + rng.integers(-40, 41, len(sums))          # off the levels: the costs are not 0
    _check(b, row_off, sums, lens, CFG, False, level, f"{n_reads} reads")
    b.free(); gen.close()


@pytest.mark.gpu
def test_adversarial_rows():
    """arrays made up here.  Ties everywhere: reads of one base repeated have one level, the rows lie on it, so the result is pure
    tie-break order.  Then on reads of random bases: negative sums, len of 0 and of 2^31 - 1, sums at the edge of the header's range,
    costs that all hit cost_cap, the cfg at its extremes, and rows that miss every target by more than cost_cap"""
    # every level the same: reads of one base repeated
    gen, prof, fl, k = inject.context("exact1")
    seqs = [b"A" * (t + k - 1) for t in (1, 20, 32, 33, 100, 300)]
    b = inject.run_geometry(gen, seqs)
    level, _, _ = _table(b)
    assert all(len(set(level[int(b.ev_off[r]):int(b.ev_off[r + 1])].tolist())) == 1 for r in range(b.n_reads))      # (the reads differ: their offsets)
    for m_of in (lambda t: t, lambda t: 2 * t + 1, lambda t: max(t // 3, 1)):
        parts = [(np.full(m_of(t), int(level[int(b.ev_off[r])]) * 4, np.int64), np.full(m_of(t), 4, np.int32)) for r, t in enumerate(np.diff(b.ev_off))]
        row_off, sums, lens = _concat(parts)
        for cfg in ((0, 0, 1), (0, 0, 1 << 24), (1 << 24, 1 << 24, 1 << 24), (1 << 24, 0, 1), (0, 1 << 24, 1), (5, 5, 5)):
            want = _check(b, row_off, sums, lens, cfg, False, level, f"ties {cfg}")
            if cfg[0] == 0 and cfg[1] == 0:
                assert (want["al_cost"] == 0).all()
    b.free(); gen.close()
    # extremes of the rows
    gen, b, (level, _, _) = _geometry([3, 32, 90, 200])
    rng = np.random.default_rng(4)
    T = np.diff(b.ev_off)
    cases = {
        "negative sums": [(-rng.integers(0, 1 << 20, t), rng.integers(1, 60, t).astype(np.int32)) for t in T],
        "len of 0 and below": [(level[int(b.ev_off[r]):int(b.ev_off[r + 1])].astype(np.int64), rng.integers(-3, 1, t).astype(np.int32)) for r, t in enumerate(T)],
        "len of 2^31 - 1": [(rng.integers(-(1 << 54), 1 << 54, t), np.full(t, (1 << 31) - 1, np.int32)) for t in T],
        "the largest sums": [(np.where(np.arange(t) & 1, (1 << 55) - 1, -(1 << 55) + 1), np.where(np.arange(t) & 2, 1, 3).astype(np.int32)) for t in T],
        "far from every target": [(np.full(2 * t, 40000 * 9, np.int64), np.full(2 * t, 9, np.int32)) for t in T],
        "far below every target": [(np.full(t + 3, -40000 * 9 - 1, np.int64), np.full(t + 3, 9, np.int32)) for t in T],
    }
    for name, parts in cases.items():
        row_off, sums, lens = _concat(parts)
        for cfg in (CFG, (0, 0, 1), (1 << 24, 1 << 24, 1 << 24), (0, 1 << 24, 1), (1 << 24, 0, 1 << 24)):
            want = _check(b, row_off, sums, lens, cfg, False, level, f"{name} {cfg}")
            if name.startswith("far") and cfg[2] <= 16384:      # every cell costs cost_cap: checked on the reference
                m = np.diff(row_off)
                assert (want["al_cost"] >= m * cfg[2]).all() and (want["al_cost"] <= m * (cfg[2] + max(cfg[:2])) + T * cfg[1]).all()
    b.free(); gen.close()


def _raw(gen, b, cfg, row_off, cin, out):
    ptr = lambda x: C.byref(x) if x is not None else None   # noqa: E731
    off = row_off.ctypes.data_as(C.POINTER(C.c_int64)) if row_off is not None else None
    return gen.L.sqg_batch_align(gen.ctx, b.handle if b is not None else None, ptr(cfg), off, ptr(cin), ptr(out))


@pytest.mark.gpu
def test_interface():
    """NULL outputs and each output alone; every SQG_EINVAL of the header with its message; a read of 2^31 rows; a batch that has not
    been run; an empty batch; a second call gives the same bytes; nothing outside [row_off[0], row_off[n]) is written (guard values
    around the arrays)"""
    gen, prof, fl, k = inject.context("exact1")
    counts = [70, 5, 300]
    seqs = inject.seqs_for([t + k - 1 for t in counts])
    b = gen.stage(seqs)
    dev = _dev(b)
    err = lambda: gen.L.sqg_last_error(gen.ctx)             # noqa: E731
    off0 = np.array([0, 1, 2, 3], np.int64)
    one = torch.zeros(8, dtype=torch.int64, device=dev)
    cin, none, cfg = api.CAlignIn(one.data_ptr(), one.data_ptr()), api.CAlignOut(), api.CAlignCfg(*CFG)
    assert _raw(gen, b, cfg, off0, cin, none) == -4 and b"sqg_batch_align" in err() and b"not been run" in err()
    with pytest.raises(api.SqgError) as e:
        b.align(off0, one, one[:4].to(torch.int32), CFG)
    assert e.value.code == -4 and "not been run" in str(e.value)
    b.run().wait()
    level, _, _ = _table(b)
    row_off, sums, lens = _concat([_rows_of(level, b.ev_off, r, "thirds") for r in range(3)])
    sums = sums + np.arange(len(sums)) % 7
    want = A.batch(row_off, sums, lens, b.ev_off, level, False, CFG)
    n_rows = int(row_off[-1])
    # guard values around the arrays, and a second call
    G = 16
    s = torch.from_numpy(sums).to(dev)
    n = torch.from_numpy(lens).to(dev)
    bufs = dict(al_ev=torch.full((n_rows + 2 * G,), -77, dtype=torch.int64, device=dev), al_cost=torch.full((3 + 2 * G,), -77, dtype=torch.int64, device=dev),
                al_edge=torch.full((3 + 2 * G,), -77, dtype=torch.int32, device=dev))
    cin = api.CAlignIn(s.data_ptr(), n.data_ptr())
    size = dict(al_ev=8, al_cost=8, al_edge=4)
    out = api.CAlignOut(*(bufs[key].data_ptr() + G * size[key] for key in OUT))
    torch.cuda.synchronize(dev)
    assert _raw(gen, b, cfg, row_off, cin, out) == 0
    first = {key: bufs[key].cpu().numpy().copy() for key in OUT}
    for key in OUT:
        np.testing.assert_array_equal(first[key][G:-G], want[key], err_msg=key)
        assert (first[key][:G] == -77).all() and (first[key][-G:] == -77).all(), f"{key}: written outside its rows"
    assert _raw(gen, b, cfg, row_off, cin, out) == 0        # the scratch is reused: the same bytes
    for key in OUT:
        np.testing.assert_array_equal(bufs[key].cpu().numpy(), first[key], err_msg=f"{key}: second call")
    # fewer rows than the arrays hold: the rows behind row_off[n] stay untouched
    short = row_off.copy(); short[3] = short[2] + 10; short[2] = short[1]       # read 1 without rows, read 2 with 10
    for key in OUT:
        bufs[key].fill_(-77)
    torch.cuda.synchronize(dev)
    assert _raw(gen, b, cfg, short, cin, out) == 0
    w2 = A.batch(short, sums, lens, b.ev_off, level, False, CFG)
    got = bufs["al_ev"].cpu().numpy()
    np.testing.assert_array_equal(got[G:G + int(short[-1])], w2["al_ev"])
    assert (got[G + int(short[-1]):] == -77).all() and (got[:G] == -77).all()
    np.testing.assert_array_equal(bufs["al_cost"].cpu().numpy()[G:-G], w2["al_cost"])
    assert w2["al_cost"][1] == -1 and w2["al_edge"][1] == 0
    # each output alone, and none
    full = _align(b, row_off, sums, lens, CFG)
    for names in [(key,) for key in OUT] + [("al_ev", "al_edge"), ()]:
        part = _align(b, row_off, sums, lens, CFG, outputs=names)
        for key in OUT:
            g = getattr(part, key)
            assert (g is None) == (key not in names) and (g is None or torch.equal(g, getattr(full, key))), (names, key)
    assert _raw(gen, b, cfg, row_off, cin, none) == 0
    # SQG_EINVAL, each with its message
    good = dict(stay_pen=256, skip_pen=1024, cost_cap=16384)
    for bad, what in [(dict(stay_pen=-1), b"stay_pen"), (dict(stay_pen=(1 << 24) + 1), b"stay_pen"), (dict(skip_pen=-1), b"skip_pen"),
                      (dict(skip_pen=(1 << 24) + 1), b"skip_pen"), (dict(cost_cap=0), b"cost_cap"), (dict(cost_cap=-5), b"cost_cap"),
                      (dict(cost_cap=(1 << 24) + 1), b"cost_cap")]:
        assert _raw(gen, b, api.CAlignCfg(**dict(good, **bad)), row_off, cin, out) == -1 and b"sqg_batch_align" in err() and what in err(), (bad, err())
    for bad_off, what in [(row_off + 1, b"start at 0"), (np.array([0, 5, 4, 9], np.int64), b"decrease"), (np.array([0, -1, 4, 9], np.int64), b"decrease")]:
        assert _raw(gen, b, cfg, bad_off, cin, out) == -1 and b"row_off" in err() and what in err(), err()
    # a read of 2^31 rows: refused from row_off alone, before any array is read (none of that size exists)
    before = {key: bufs[key].cpu().numpy().copy() for key in OUT}
    assert _raw(gen, b, cfg, np.array([0, 2 ** 31, 2 ** 31, 2 ** 31], np.int64), cin, out) == -1 and b"sqg_batch_align" in err() and b"row_off" in err() and b"2^31 rows" in err(), err()
    torch.cuda.synchronize(dev)
    for key in OUT:                                         # guards and rows as the call before left them
        np.testing.assert_array_equal(bufs[key].cpu().numpy(), before[key], err_msg=f"{key}: a refused row_off wrote")
        assert (before[key][:G] == -77).all() and (before[key][-G:] == -77).all()
    assert gen.L.sqg_batch_align(None, None, None, None, None, None) == -1
    assert gen.L.sqg_batch_align(None, b.handle, C.byref(cfg), row_off.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(cin), C.byref(out)) == -1
    assert _raw(gen, None, cfg, row_off, cin, out) == -1 and b"sqg_batch_align" in err() and b"batch" in err()
    assert _raw(gen, b, None, row_off, cin, out) == -1 and b"sqg_batch_align" in err() and b"cfg" in err()
    assert _raw(gen, b, cfg, None, cin, out) == -1 and b"row_off must not be NULL" in err()
    assert _raw(gen, b, cfg, row_off, None, out) == -1 and b"in must not be NULL" in err()
    assert _raw(gen, b, cfg, row_off, api.CAlignIn(None, n.data_ptr()), out) == -1 and b"in->sum" in err()
    assert _raw(gen, b, cfg, row_off, api.CAlignIn(s.data_ptr(), None), out) == -1 and b"in->len" in err()
    assert _raw(gen, b, cfg, row_off, cin, None) == -1 and b"out must not be NULL" in err()
    for key in OUT:                                         # no refused call wrote anything
        np.testing.assert_array_equal(bufs[key].cpu().numpy()[G:G + 3], w2[key][:3], err_msg=key)
    for bad in (dict(cfg=(1, 2)), dict(cfg="dna"), dict(outputs=("al_ev", "al_score"))):
        with pytest.raises(api.SqgError) as e:
            b.align(row_off, s, n, **dict(dict(cfg=CFG), **bad))
        assert e.value.code == -1 and "align" in str(e.value), bad
    for bad in ((row_off[:-1], s, n), (row_off, s.to(torch.int32), n), (row_off, s, n.cpu()), (row_off, s[:5], n)):
        with pytest.raises(api.SqgError) as e:
            b.align(*bad, CFG)
        assert e.value.code == -1 and "align" in str(e.value)
    b.free()
    b = gen.submit([])                                      # an empty batch
    al = b.align(np.zeros(1, np.int64), torch.zeros(0, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int32, device=dev), CFG)
    assert al.n_rows == 0 and all(tuple(getattr(al, key).shape) == (0,) for key in OUT)
    b.free(); gen.close()


@pytest.mark.gpu
def test_lifetime():
    """a batch keeps its alignment until two more batches have been run, then SQG_ESEQUENCE"""
    o, k, gen = _context(dict(REFVEC_CASES)["rna004_tk4"], api.MODE_EXACT)
    reads = _fixture_reads("rna004_tk4")
    parts = [[r["seq"] for r in reads[0:2]], [r["seq"] for r in reads[2:4]], [r["seq"] for r in reads[4:6]]]
    b0 = gen.stage(parts[0]).run().wait()
    level, sums, lens = _table(b0)
    idx = _stored_order(b0, True)
    want = _check(b0, b0.ev_off, sums[idx], lens[idx], CFG, True, level, "quiet")
    b1, b2 = gen.stage(parts[1]), gen.stage(parts[2])
    b1.run().wait()
    _assert_equal(_align(b0, b0.ev_off, sums[idx], lens[idx], CFG), want, "after one more batch")
    b2.run().wait()
    with pytest.raises(api.SqgError) as e:
        _align(b0, b0.ev_off, sums[idx], lens[idx], CFG)
    assert e.value.code == -4 and "sqg_batch_align" in str(e.value) and "handed to a later batch" in str(e.value)
    level, sums, lens = _table(b1)
    idx = _stored_order(b1, True)
    _check(b1, b1.ev_off, sums[idx], lens[idx], CFG, True, level, "batch 1 after batch 2")
    for b in (b0, b1, b2):
        b.free()
    gen.close()
