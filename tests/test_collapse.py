"""include/sqg_collapse.h: event rows summed per true event they are assigned to (sqg_batch_collapse) and the pileup of those sums
(sqg_batch_pileup_rows), against the numpy statement of the header's rules (collapse_ref.py), against Batch.events() and against
Batch.pileup where the rows are the true table itself.  Every comparison is bit for bit: the sums are integers, the floats are compared
as bit patterns."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (before the library is loaded: the HIP runtime torch brings is the one the library then uses)

import chunks_ref as R
import collapse_ref as CR
import events_ref as EV
import inject
import pileup_ref as PR
import shard_cases as SC
from chunk_support import _context, _declared, _fixture_reads
from refvec_cases import REFVEC_CASES
from squigulator_amd import api, build, model, options, profiles
from test_event_grids import assert_grid_shape, grid_event_counts, grid_seqs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = api.COLLAPSE_OUTPUTS
POUT = api.PILEUP_OUTPUTS
SUMS = ("ob_rows", "ob_len", "ob_sum", "ob_sumsq")
WG = 256            # k_common.h's CHUNK_WG: the rows of one workgroup and trip
I64_MIN = -(1 << 63)
SETTINGS = (("pa", False), ("medmad", False), ("pa", True), ("medmad", True))


def _offsets(lens):
    return np.concatenate(([0], np.cumsum(lens))).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------- no GPU
def _struct_fields(hdr, struct):
    body = hdr[:hdr.index("} " + struct)]
    body = body[body.rindex("typedef struct"):]
    body = body[body.index("{") + 1:]
    return [re.sub(r"[\s*]", "", name) for decl in body.split(";") if decl.strip() for name in re.sub(r"^\s*(const\s+)?\w+\s", "", decl.strip()).split(",")]


def test_the_header_and_the_binding_agree():
    assert _declared("sqg_collapse.h") == set(api.EXPORTS_COLLAPSE) == {"sqg_batch_collapse", "sqg_batch_pileup_rows"}
    others = set(api.EXPORTS) | set(api.EXPORTS_CHUNKS) | set(api.EXPORTS_TARGETS) | set(api.EXPORTS_SEGMENTS) | set(api.EXPORTS_SITES) | set(api.EXPORTS_EVENTS) | \
        set(api.EXPORTS_PILEUP) | set(api.EXPORTS_DETECT) | set(api.EXPORTS_ALIGN)
    assert not set(api.EXPORTS_COLLAPSE) & others
    assert _declared("sqg_pileup.h") == set(api.EXPORTS_PILEUP) and _declared("sqg_align.h") == set(api.EXPORTS_ALIGN)      # the other headers: unchanged
    raw = open(os.path.join(ROOT, "include", "sqg_collapse.h")).read()
    assert '#include "sqg_pileup.h"' in raw and "SQG_ABI_VERSION is unchanged" in raw and "wrap modulo 2^64" in raw
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for struct, ctype in (("sqg_collapse_cfg_t", api.CCollapseCfg), ("sqg_collapse_in_t", api.CCollapseIn), ("sqg_collapse_out_t", api.CCollapseOut),
                          ("sqg_pileup_rows_stat_t", api.CPileupRowsStat)):
        assert _struct_fields(hdr, struct) == [f[0] for f in ctype._fields_], struct
    assert tuple(f[0] for f in api.CCollapseOut._fields_) == OUT == CR.OUTPUTS and tuple(f[0] for f in api.CCollapseIn._fields_) == api.COLLAPSE_INPUTS
    assert C.sizeof(api.CCollapseCfg) == 8 and C.sizeof(api.CPileupRowsStat) == 32 and C.sizeof(api.CCollapseIn) == 32 and C.sizeof(api.CCollapseOut) == 56
    # the prototypes: the pointers behind (ctx, batch) in the order of the binding's table
    table = dict(api._CONSUMER_EXPORTS[-1][1])
    assert api._CONSUMER_EXPORTS[-1][0] == api.EXPORTS_COLLAPSE
    names = {api.CCollapseCfg: "sqg_collapse_cfg_t", api.CCollapseIn: "sqg_collapse_in_t", api.CCollapseOut: "sqg_collapse_out_t", api.CPileupCfg: "sqg_pileup_cfg_t",
             api.COrigin: "sqg_pileup_origin_t", api.CPileupOut: "sqg_pileup_out_t", api.CPileupRowsStat: "sqg_pileup_rows_stat_t", C.c_int64: "int64_t"}
    for fn in api.EXPORTS_COLLAPSE:
        args = re.search(r"int\s+" + fn + r"\s*\((.*?)\)\s*;", hdr, re.S).group(1).split(",")
        types = [re.sub(r"\bconst\b|\*.*$", "", a).strip() for a in args]
        assert types == ["sqg_ctx_t", "sqg_batch_t"] + [names[t] for t in table[fn]], fn
    assert os.path.join(ROOT, "include", "sqg_collapse.h") in build.headers()
    for h in ("k_collapse.h", "h_collapse.h"):
        assert os.path.join(ROOT, "squigulator_amd", "csrc", h) in build.headers()


def test_the_built_libraries_export_both_calls():
    build.build()
    for lib in (build.LIB, build.LIB_DEV):
        L = api.load_library(lib)
        for n in api.EXPORTS_COLLAPSE:
            assert hasattr(L, n), f"{n} not exported by {lib}"


def _true_rows(t):
    """the rows that are the table itself"""
    n = len(t["ev_len"])
    return t["ev_off"], np.arange(n, dtype=np.int64), t["sum"], t["sumsq"], t["ev_len"]


def _ref_consts(t, reads, prof, norm):
    return dict(offset=[r["offset"] for r in reads], rng=prof.range, dig=prof.digitisation) if norm == "pa" else dict(med2=t["med2"], mad4=t["mad4"])


def _assert_same(got, want, keys, what):
    for key in keys:
        g, w = np.asarray(got[key]), np.asarray(want[key])
        assert g.shape == w.shape and g.dtype == w.dtype, f"{what}: {key} {g.shape} {g.dtype} vs {w.shape} {w.dtype}"
        np.testing.assert_array_equal(R.bits(g), R.bits(w), err_msg=f"{what}: {key}")


def _split_rows(t, rng, shuffle):
    """every event's samples cut into 1 .. 4 rows whose sums add up (a row may have no sample), a read's rows shuffled"""
    off, ev, s1, s2, ln = _true_rows(t)
    parts = rng.integers(1, 5, len(ev))
    rev = np.repeat(ev, parts)
    first = np.concatenate(([0], np.cumsum(parts)[:-1]))
    rl, r1, r2 = np.zeros(len(rev), np.int64), np.zeros(len(rev), np.int64), np.zeros(len(rev), np.int64)
    for e in range(len(ev)):
        cuts = np.sort(rng.integers(0, int(ln[e]) + 1, parts[e] - 1))
        lens = np.diff(np.concatenate(([0], cuts, [ln[e]])))
        a = rng.integers(-1000, 1000, parts[e]); a[-1] += s1[e] - a.sum()
        c = rng.integers(0, 1000, parts[e]); c[-1] += s2[e] - c.sum()
        # the sums of a row without a sample are not added: such a row carries none of the event's
        empty = lens < 1
        if empty.all():
            lens[0], empty[0] = ln[e], ln[e] < 1
        keep = np.flatnonzero(~empty)
        if len(keep):
            a[keep[-1]] += a[empty].sum(); c[keep[-1]] += c[empty].sum()
        sl = slice(first[e], first[e] + parts[e])
        rl[sl], r1[sl], r2[sl] = lens, a, c
    row_off = _offsets([parts[off[r]:off[r + 1]].sum() for r in range(len(off) - 1)])
    if shuffle:
        for r in range(len(off) - 1):
            p = row_off[r] + rng.permutation(int(row_off[r + 1] - row_off[r]))
            sl = slice(row_off[r], row_off[r + 1])
            rev[sl], rl[sl], r1[sl], r2[sl] = rev[p], rl[p], r1[p], r2[p]
    return row_off, rev, r1, r2, rl.astype(np.int32), parts


@pytest.mark.parametrize("cid", ["r9_tk16", "rna9_prefix", "r9_meth_dense"])
def test_the_reference_on_the_true_rows_is_the_table_and_the_pileup(cid):
    """events_ref's table of the compiled reference's own reads: collapse_ref on the true rows returns the table's own columns and
    ob_rows == 1, pileup_rows on them equals pileup_ref.pileup; every event split into 1 .. 4 rows, the rows of a read shuffled, changes
    nothing"""
    o = options.parse_args(dict(REFVEC_CASES)[cid])
    k, meth, rna, prefix = o.kmer_size_default, bool(o.meth_freq), bool(o.flags & profiles.SQ_RNA), bool(o.flags & profiles.SQ_PREFIX)
    level = model.synthetic_model(k, meth=meth)[0]
    reads = _fixture_reads(cid)
    lens = np.array([len(r["seq"]) for r in reads], np.int64)
    key0, step = 500 + 11 * np.arange(len(reads), dtype=np.int64), np.where(np.arange(len(reads)) % 3 == 1, -1, 1).astype(np.int8)
    key0 = np.where(step < 0, key0 + np.maximum(lens - k, 0), key0)
    rng = np.random.default_rng(5)
    for norm, trim in SETTINGS if prefix else SETTINGS[:2]:
        t = EV.batch_events(reads, level, k, rna, meth, prefix, int(o.profile.dwell_mean), norm, trim, o.profile.range, o.profile.digitisation)
        consts = _ref_consts(t, reads, o.profile, norm)
        assert (t["ev_len"] > 0).all()
        for rows in (_true_rows(t), _split_rows(t, rng, False)[:5], _split_rows(t, rng, True)[:5]):
            ob = CR.collapse(*rows, t["ev_off"], norm, **consts)
            _assert_same(ob, dict(ob_len=t["ev_len"].astype(np.int64), ob_sum=t["sum"], ob_sumsq=t["sumsq"], mean=t["mean"], sd=t["sd"],
                                  rd_dropped=np.zeros(len(reads), np.int32)), ("ob_len", "ob_sum", "ob_sumsq", "mean", "sd", "rd_dropped"), f"{cid} {norm} {trim}")
            assert (ob["ob_rows"] >= 1).all() and (len(rows[1]) > len(t["ev_len"]) or (ob["ob_rows"] == 1).all())
            for by, segs, lo, hi in ((PR.BY_REF, 0, 520, 900), (PR.BY_KMER, 15, 0, len(level))):
                want, wc, wo = PR.pileup(t, t["ev_off"], key0, step, lens, k, rna, prefix, by, PR.SPLIT_STRAND, segs, lo, hi)
                got, c, x, unseen, dropped = CR.pileup_rows(ob, t, t["ev_off"], key0, step, lens, k, rna, prefix, by, PR.SPLIT_STRAND, segs, lo, hi)
                assert (c, x, unseen, dropped) == (wc, wo, 0, 0) and wc > 0
                _assert_same(got, want, PR.OUTPUTS, f"{cid} {norm} {trim} by {by}")


def test_a_hand_worked_collapse():
    """two reads of 3 and 2 events; rows out of order, a row of another read's event, -1, a row without a sample"""
    ev_off, row_off = [0, 3, 5], [0, 6, 9]
    ev = [2, 0, 2, 3, -1, 0, 4, 2, 4]            # read 0: event 3 is read 1's and -1 is none; read 1: event 2 is read 0's
    ln = [4, 2, 6, 9, 9, 0, 5, 9, -5]
    s1 = [40, 10, 90, 7, 7, 1000, 50, 7, 1000]
    s2 = [500, 60, 1500, 1, 1, 1, 600, 1, 1]
    ob = CR.collapse(row_off, ev, s1, s2, ln, ev_off, "pa", offset=[1.0, 2.0], rng=10.0, dig=5.0)
    assert ob["ob_rows"].tolist() == [2, 0, 2, 0, 2] and ob["ob_len"].tolist() == [2, 0, 10, 0, 5]
    assert ob["ob_sum"].tolist() == [10, 0, 130, 0, 50] and ob["ob_sumsq"].tolist() == [60, 0, 2000, 0, 600] and ob["rd_dropped"].tolist() == [2, 1]
    assert ob["mean"].tolist() == [12.0, 0.0, 28.0, 0.0, 24.0]                          # ((sum / len) + offset) * 10 / 5
    assert ob["sd"][1] == 0 and ob["sd"][0] == np.float32(np.sqrt((60 - 10 * 5.0) / 2) * 2) and ob["sd"][4] == np.float32(np.sqrt((600 - 50 * 10.0) / 5) * 2)
    wrap = CR.collapse([0, 4], [0] * 4, [1 << 62] * 4, [-(1 << 62)] * 4, [1 << 30] * 4, [0, 1], "pa", offset=[0.0])
    assert wrap["ob_sum"].tolist() == [0] and wrap["ob_sumsq"].tolist() == [0] and wrap["ob_len"].tolist() == [1 << 32] and wrap["ob_rows"].tolist() == [4]


def test_the_cpu_backend_has_no_collapse_and_says_so():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "libsqg_cpu.so"])
    prof, fl = profiles.get_profile("dna-r9-prom")
    mean, stdv = model.synthetic_model(6)
    gen = api.SignalGenerator(prof, fl, 6, mean, stdv, 42, lib_path=os.path.join(ROOT, "oracle", "libsqg_cpu.so"))
    for n in api.EXPORTS_COLLAPSE:
        assert not hasattr(gen.L, n)
    b = gen.submit([b"ACGTACGTACGTTTGACA" * 40])
    for call in (lambda: b.collapse(np.zeros(2, np.int64), None, None, None, None), lambda: b.pileup_rows(None, np.zeros(2, np.int64), None, None, None, None)):
        with pytest.raises(api.SqgError) as e:
            call()
        assert e.value.code == -1 and "sqg_collapse.h" in str(e.value)
    b.free(); gen.close()


# ---------------------------------------------------------------------------------------------------------- GPU
def _dev(b):
    return torch.device("cuda", b.gen.device)


def _cpu(t, key=None):
    a = t.cpu().numpy()
    return a.view(np.uint32) if key in ("kmer", "ob_rows", "n") else a


def _rows_on(b, ev, s1, s2, ln):
    """the rows as the tensors the calls take (s2 None: no sumsq)"""
    to = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dt)).to(_dev(b))      # noqa: E731
    return to(ev, np.int64), to(s1, np.int64), to(s2, np.int64), to(ln, np.int32)


def _collapse(b, row_off, rows, norm="pa", trim=False, outputs=None):
    ch = b.collapse(row_off, *rows, norm=norm, trim=trim, outputs=outputs)
    return {n: (None if getattr(ch, n) is None else _cpu(getattr(ch, n), n)) for n in OUT}


def _consts(b, norm, trim):
    """what mean / sd take of the read: the host's offsets, or the statistics Batch.events() hands out (its own tests pin them)"""
    if norm == "pa":
        prof = b.gen.profile
        return dict(offset=b.offset, rng=prof.range, dig=prof.digitisation)
    t = b.events(norm, trim, outputs=("med2", "mad4"))
    return dict(med2=_cpu(t.med2), mad4=_cpu(t.mad4))


def _table(b, norm="pa", trim=False, keys=api.EVENT_OUTPUTS):
    t = b.events(norm, trim, outputs=keys)
    return {n: _cpu(getattr(t, n), n) for n in keys}


def _pile(p):
    return {n: (None if getattr(p, n) is None else _cpu(getattr(p, n), n)) for n in POUT}


def _prefilled(gen, seed, **kw):
    """a pileup whose arrays already hold sums, and those sums"""
    p = gen.new_pileup(**kw)
    rng = np.random.default_rng(seed)
    into = {}
    for n in POUT:
        t = getattr(p, n)
        into[n] = rng.integers(0, 1 << 32, tuple(t.shape), dtype=np.uint32) if n == "n" else rng.integers(-1 << 63, (1 << 63) - 1, tuple(t.shape), dtype=np.int64)
        t.copy_(torch.from_numpy(into[n].view(np.int32) if n == "n" else into[n]))
    return p, into


CONTEXTS = {  # name -> (profile, extra flags, letters, bases of the reads)
    "dna": ("dna-r9-prom", 0, b"ACGT", (300, 41, 520, 77, 260)),
    "rna": ("rna004-prom", 0, b"ACGU", (300, 41, 520, 77)),
    "dna_prefix": ("dna-r9-prom", profiles.SQ_PREFIX, b"ACGT", (300, 41, 260)),
    "rna_prefix_stall": ("rna004-prom", profiles.SQ_PREFIX, b"ACGU", (300, 41, 260)),
    "meth": ("dna-r9-prom", profiles.SQ_METH, b"ACGTM", (300, 41, 520, 77)),
    "constant_dwell": ("dna-r9-prom", profiles.SQ_IDEAL_TIME, b"ACGT", (300, 41, 520)),
    "k5": ("rna-r9-prom", 0, b"ACGU", (300, 41, 520)),
    "k9": ("dna-r10-prom", 0, b"ACGT", (300, 41, 520)),
    "short_read": ("dna-r9-prom", 0, b"ACGT", (2, 300, 5, 150, 1)),
}
_made = {}


def _ctx(name):
    """one staged batch per context (made once), a caller's origin with a read of step 0, and what the references need to know"""
    if name not in _made:
        pname, extra, letters, bases = CONTEXTS[name]
        prof, fl = profiles.get_profile(pname)
        fl |= extra
        k = profiles.default_kmer_size(fl)
        meth, rna, prefix = bool(fl & profiles.SQ_METH), bool(fl & profiles.SQ_RNA), bool(fl & profiles.SQ_PREFIX)
        level, stdv = model.synthetic_model(k, meth=meth)
        gen = api.SignalGenerator(prof, fl, k, level, stdv, 11, num_workers=2, mode=api.MODE_CERTIFIED)
        gen.profile = prof
        rng = np.random.default_rng(8)
        seqs = [bytes(rng.choice(list(letters), m).astype(np.uint8)) for m in bases]
        b = gen.stage(seqs).run().wait()
        b.gen.profile = prof
        lens = np.array(bases, np.int64)
        step = np.array([1, -1, 1, 0, -1][:len(bases)], np.int8)
        if len(bases) < 4:
            step[-1] = 0
        key0 = 1000 + 90 * np.arange(len(bases), dtype=np.int64)
        key0 = np.where(step < 0, key0 + np.maximum(lens - k, 0), key0)
        _made[name] = dict(gen=gen, b=b, k=k, meth=meth, rna=rna, prefix=prefix, prof=prof, lens=lens, key0=key0, step=step, rows=len(level), name=name)
    return _made[name]


def _pile_cfgs(d):
    """new_pileup's keywords: every split the context has, segs 0 and 15, windows that cut the keys"""
    splits = [(), ("strand",)] + ([("meth",), ("strand", "meth")] if d["meth"] else [])
    out = [dict(by="ref", split=s, lo=1100, hi=1400) for s in splits]
    for segs in (None, (0, 1, 2, 3)):
        out += [dict(by="kmer", split=s, segs=segs, lo=d["rows"] // 3, hi=d["rows"] // 3 + d["rows"] // 2) for s in splits]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CONTEXTS))
def test_truth_identity(name):
    """the rows that are the batch's own table (ev = 0 .. n_events - 1, sum, sumsq, ev_len): the collapse is Batch.events(), and
    pileup_rows adds to a second pileup what Batch.pileup adds to the first -- arrays that already hold sums -- for both norms and trims"""
    d = _ctx(name)
    gen, b = d["gen"], d["b"]
    assert len(CONTEXTS) >= 8
    origin = (d["key0"], d["step"])
    for norm, trim in SETTINGS:
        t = _table(b, norm, trim)
        assert (t["ev_len"] > 0).all()
        rows = _rows_on(b, np.arange(b.n_events), t["sum"], t["sumsq"], t["ev_len"])
        got = _collapse(b, b.ev_off, rows, norm, trim)
        want = dict(ob_rows=np.ones(b.n_events, np.uint32), ob_len=t["ev_len"].astype(np.int64), ob_sum=t["sum"], ob_sumsq=t["sumsq"], mean=t["mean"], sd=t["sd"],
                    rd_dropped=np.zeros(b.n_reads, np.int32))
        _assert_same(got, want, OUT, f"{name} {norm} {trim}")
        ref = CR.collapse(b.ev_off, np.arange(b.n_events), t["sum"], t["sumsq"], t["ev_len"], b.ev_off, norm, **_consts(b, norm, trim))
        _assert_same(got, ref, OUT, f"{name} {norm} {trim}: collapse_ref")
        some = False
        for i, kw in enumerate(_pile_cfgs(d)):
            p1, into = _prefilled(gen, i, norm=norm, trim=trim, **kw)
            p2, _ = _prefilled(gen, i, norm=norm, trim=trim, **kw)
            counted, outside = b.pileup(p1, origin=origin)
            assert b.pileup_rows(p2, b.ev_off, *rows, origin=origin) == (counted, outside, 0, 0), f"{name} {norm} {trim} {kw}"
            for n in POUT:
                assert torch.equal(getattr(p1, n), getattr(p2, n)), f"{name} {norm} {trim} {kw}: {n}"
            some |= counted > 0 and outside > 0
            assert any(not np.array_equal(_pile(p2)[n], into[n]) for n in POUT) == (counted > 0)
        assert some, "no window cuts the keys"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["dna", "rna"])
def test_detected_and_aligned_rows(name):
    """detect -> align -> collapse under al_ev and under true_ev against collapse_ref, and pileup_rows with all four stats against
    collapse_ref.pileup_rows; the detector over-segments and misses: some event has two rows or more, some eligible event has none"""
    d = _ctx(name)
    gen, b, k = d["gen"], d["b"], d["k"]
    dt = b.detect("rna" if d["rna"] else "dna", outputs=("sum", "sumsq", "dt_len", "true_ev"))
    al = b.align(dt.det_off, dt.sum, dt.dt_len, outputs=("al_ev",))
    s1, s2, ln = _cpu(dt.sum), _cpu(dt.sumsq), _cpu(dt.dt_len)
    evt = _table(b, keys=("ev_read", "kmer", "seg"))
    for what, col in (("al_ev", al.al_ev), ("true_ev", dt.true_ev)):
        ev = _cpu(col)
        for norm, trim in SETTINGS[:2]:
            got = _collapse(b, dt.det_off, (col, dt.sum, dt.sumsq, dt.dt_len), norm, trim)
            ref = CR.collapse(dt.det_off, ev, s1, s2, ln, b.ev_off, norm, **_consts(b, norm, trim))
            _assert_same(got, ref, OUT, f"{name} {what} {norm}")
            assert got["ob_rows"].max() >= 2 and (got["ob_rows"] == 0).any() and int(got["ob_rows"].sum()) + int(got["rd_dropped"].sum()) == dt.n_rows
            for kw in (dict(by="ref", split=("strand",), lo=1050, hi=1500), dict(by="kmer", lo=0, hi=d["rows"])):
                p, into = _prefilled(gen, 3, norm=norm, trim=trim, **kw)
                st = b.pileup_rows(p, dt.det_off, col, dt.sum, dt.sumsq, dt.dt_len, origin=(d["key0"], d["step"]))
                want, *wst = CR.pileup_rows(ref, evt, b.ev_off, d["key0"], d["step"], d["lens"], k, d["rna"], d["prefix"], p.cfg.by, p.cfg.split, p.cfg.segs, p.cfg.lo, p.cfg.hi, into)
                assert st == tuple(wst) and st[0] > 0 and st[2] > 0, f"{name} {what} {norm} {kw}: {st} vs {wst}"
                _assert_same(_pile(p), want, POUT, f"{name} {what} {norm} {kw}")


def _geometry_rows(b, rng):
    """synthetic rows on a batch of six reads.  Read 0, 2 and 5 have none.  Read 1: one event given 1, 63, 64, 65, 255, 256, 257 and 1000
    consecutive rows (a row of another event between the runs), a run that starts at lane 63, 400 rows that alternate between two events,
    and a dropped row inside a run.  Read 3: every row dropped -- the neighbouring reads' first and last events, -1, INT64_MIN, n_events.
    Read 4: drawn events.  Some rows have a len of 0 or -5"""
    off = np.asarray(b.ev_off, np.int64)
    assert b.n_reads == 6 and (np.diff(off) >= 30).all()
    a, c, x = off[1] + 7, off[1] + 8, off[1] + 20
    r1 = []
    for run in (1, 63, 64, 65, 255, 256, 257, 1000):
        r1 += [a] * run + [c]
    while len(r1) % 64 != 63:                                  # (read 0 has no row: read 1's rows start at row 0 of the grid)
        r1 += [c, x][len(r1) & 1:][:1]
    lane63 = len(r1)
    r1 += [a] * 5
    r1 += [a, x] * 200
    r1 += [c] * 10 + [-1] + [c] * 10
    r3 = [off[4], off[3] - 1, off[2] - 1, off[4] + 1, -1, I64_MIN, b.n_events, off[5] - 1] * 9
    r4 = (off[4] + np.sort(rng.integers(0, off[5] - off[4], 700))).tolist()
    per = [[], r1, [], r3, r4, []]
    row_off = _offsets([len(p) for p in per])
    ev = np.array([v for p in per for v in p], np.int64)
    assert row_off[1] == 0 and lane63 % 64 == 63 and ev[lane63 - 1] != ev[lane63] == ev[lane63 + 1]
    n = len(ev)
    ln = rng.choice([0, -5, 1, 2, 3, 9, 40], n).astype(np.int32)
    s1, s2 = rng.integers(-(1 << 40), 1 << 40, n), rng.integers(0, 1 << 50, n)
    return row_off, ev, s1, s2, ln


class _Six:
    made = None

    @classmethod
    def get(cls):
        if cls.made is None:
            prof, fl = profiles.get_profile("dna-r9-prom")
            k = 6
            level, stdv = model.synthetic_model(k)
            gen = api.SignalGenerator(prof, fl, k, level, stdv, 5, num_workers=2, mode=api.MODE_CERTIFIED)
            gen.profile = prof
            lens = np.array([60, 90, 45, 70, 300, 38], np.int64)
            b = gen.stage(inject.seqs_for(lens)).run().wait()
            step = np.array([1, -1, 1, 1, -1, 1], np.int8)
            key0 = np.where(step < 0, 100 + lens - k, 100 + 10 * np.arange(6)).astype(np.int64)
            cls.made = dict(gen=gen, b=b, k=k, lens=lens, key0=key0, step=step, rows=len(level), evt=_table(b, keys=("ev_read", "kmer", "seg")))
        return cls.made


def _check_rows(d, row_off, ev, s1, s2, ln, what, settings=SETTINGS[:2], pile=True):
    """collapse and pileup_rows of these rows against collapse_ref -> the reference's collapse under the first setting"""
    gen, b = d["gen"], d["b"]
    rows = _rows_on(b, ev, s1, s2, ln)
    first = None
    for norm, trim in settings:
        got = _collapse(b, row_off, rows, norm, trim)
        ref = CR.collapse(row_off, ev, s1, s2, ln, b.ev_off, norm, **_consts(b, norm, trim))
        _assert_same(got, ref, OUT, f"{what} {norm}")
        first = first or ref
        for kw in (dict(by="ref", split=("strand",), lo=110, hi=330), dict(by="kmer", lo=0, hi=d["rows"])) if pile else ():
            p, into = _prefilled(gen, 1, norm=norm, trim=trim, **kw)
            st = b.pileup_rows(p, row_off, *rows, origin=(d["key0"], d["step"]))
            want, *wst = CR.pileup_rows(ref, d["evt"], b.ev_off, d["key0"], d["step"], d["lens"], d["k"], False, False, p.cfg.by, p.cfg.split, 0, p.cfg.lo, p.cfg.hi, into)
            assert st == tuple(wst), f"{what} {norm} {kw}: {st} vs {wst}"
            _assert_same(_pile(p), want, POUT, f"{what} {norm} {kw}")
    return first


@pytest.mark.gpu
def test_run_geometry():
    d = _Six.get()
    b = d["b"]
    rng = np.random.default_rng(4)
    row_off, ev, s1, s2, ln = _geometry_rows(b, rng)
    ref = _check_rows(d, row_off, ev, s1, s2, ln, "geometry")
    a = int(b.ev_off[1]) + 7
    assert ref["ob_rows"][a] == 1 + 63 + 64 + 65 + 255 + 256 + 257 + 1000 + 5 + 200 and ref["rd_dropped"].tolist() == [0, 1, 0, 72, 0, 0]
    assert (ln[ev == a] < 1).any() and not ref["ob_rows"][b.ev_off[3]:b.ev_off[4]].any()
    # the same rows shuffled within each read: no run longer than a few rows, the same sums
    p = np.concatenate([row_off[r] + rng.permutation(int(row_off[r + 1] - row_off[r])) for r in range(6)]).astype(np.int64)
    again = _check_rows(d, row_off, ev[p], s1[p], s2[p], ln[p], "geometry shuffled")
    _assert_same(again, ref, OUT, "shuffled against in order")
    # every row dropped
    none = np.full(len(ev), -1, np.int64)
    ref = _check_rows(d, row_off, none, s1, s2, ln, "all dropped")
    assert not ref["ob_rows"].any() and ref["rd_dropped"].tolist() == np.diff(row_off).tolist()


@pytest.mark.gpu
def test_arithmetic_edges():
    d = _Six.get()
    b = d["b"]
    off = np.asarray(b.ev_off, np.int64)
    e = off[4] + np.arange(8)                                  # events of read 4, whose step is -1: all of them count by position
    big = (1 << 31) - 1
    # (the wrapped sums are small: q(mean) is defined for |mean| * 4096 < 2^63 only)
    #         wraps to 0 (four rows of 2^62)   past -2^64 to 5 (four)                       len above 2^31                variance below 0        one sample
    ev = [e[0]] * 4 + [e[1]] * 4 + [e[2]] * 3 + [e[3]] * 2 + [e[4]]
    s1 = [1 << 62] * 4 + [-(1 << 62)] * 3 + [5 - (1 << 62)] + [3 * 10 ** 11, 10 ** 11, 2 * 10 ** 11] + [500, 700] + [-77]
    s2 = [1 << 62] * 4 + [1 << 62] * 3 + [(1 << 62) + 9] + [10 ** 16, 10 ** 16, 10 ** 16] + [10, 20] + [77 * 77]
    ln = [1, 2, 3, 4] + [5, 5, 5, 5] + [big] * 3 + [4, 6] + [1]
    row_off = np.array([0, 0, 0, 0, 0, len(ev), len(ev)], np.int64)
    ev, s1, s2, ln = np.array(ev, np.int64), np.array(s1, np.int64), np.array(s2, np.int64), np.array(ln, np.int32)
    ref = _check_rows(d, row_off, ev, s1, s2, ln, "edges")
    assert ref["ob_sum"][e[0]] == 0 and ref["ob_sumsq"][e[0]] == 0 and ref["ob_sum"][e[1]] == 5 and ref["ob_sumsq"][e[1]] == 9
    assert ref["ob_len"][e[2]] == 3 * big > 1 << 31 and ref["mean"][e[2]] != 0
    assert ref["sd"][e[3]] == 0 and ref["mean"][e[3]] != 0 and ref["sd"][e[4]] == 0
    # no sumsq: the outputs that need none
    some = ("ob_rows", "ob_len", "ob_sum", "mean")
    for norm in ("pa", "medmad"):
        got = _collapse(b, row_off, _rows_on(b, ev, s1, None, ln), norm, False, outputs=some)
        want = CR.collapse(row_off, ev, s1, None, ln, b.ev_off, norm, **_consts(b, norm, False))
        _assert_same(got, want, some, f"no sumsq {norm}")
        assert all(got[n] is None for n in OUT if n not in some)
    p = d["gen"].new_pileup(lo=100, hi=400, outputs=("n", "dwell", "dwell_sq", "mean_sum", "mean_sq"))
    st = b.pileup_rows(p, row_off, *_rows_on(b, ev, s1, None, ln), origin=(d["key0"], d["step"]))
    want, *wst = CR.pileup_rows(CR.collapse(row_off, ev, s1, None, ln, b.ev_off, "pa", **_consts(b, "pa", False)), d["evt"], b.ev_off, d["key0"], d["step"], d["lens"],
                                d["k"], False, False, lo=100, hi=400)
    assert st == tuple(wst) and st[0] == 5
    got = _pile(p)
    _assert_same(got, want, [n for n in POUT if got[n] is not None], "no sumsq pileup")
    assert (3 * big) ** 2 % (1 << 64) in got["dwell_sq"].view(np.uint64).ravel().tolist()


def _device_cap():
    return 32 * torch.cuda.get_device_properties(0).multi_processor_count * WG         # h_context.h: num_cu is the same attribute


@pytest.mark.gpu
def test_rows_behind_the_first_trip_of_the_grid():
    """more than 32 * CUs * 256 synthetic rows over the six reads' events: k_collapse_rows takes a second trip, a run crosses the trip
    boundary, the last wavefront is partly empty, and rows are dropped on both trips"""
    d = _Six.get()
    b = d["b"]
    cap = _device_cap()
    n = cap + cap // 8 + 37
    off = np.asarray(b.ev_off, np.int64)
    share = np.array([0.1, 0.3, 0.0, 0.2, 0.32, 0.08])
    counts = np.floor(share * n).astype(np.int64)
    counts[4] += n - counts.sum()
    row_off = _offsets(counts)
    ev = np.concatenate([off[r] + np.arange(counts[r]) * (off[r + 1] - off[r]) // max(counts[r], 1) for r in range(6)]).astype(np.int64)
    ev[::1009] = -1
    ev[cap - 3:cap + 3] = ev[cap + 5]
    assert n > cap and n % 64 != 0 and ev[cap - 1] == ev[cap] >= 0 and (ev[cap:] == -1).any() and ((row_off[1:-1] > cap) & (row_off[1:-1] < n)).any()
    rng = np.random.default_rng(6)
    ln = rng.choice([0, -5, 1, 2, 3, 9, 40], n).astype(np.int32)
    s1, s2 = rng.integers(-(1 << 40), 1 << 40, n), rng.integers(0, 1 << 50, n)
    ref = _check_rows(d, row_off, ev, s1, s2, ln, "second trip", settings=SETTINGS[:1])
    with_rows = np.repeat(counts > 0, np.diff(off))
    assert ref["ob_rows"][with_rows].min() > 1000 and not ref["ob_rows"][~with_rows].any() and int(ref["rd_dropped"].sum()) == int((ev == -1).sum())


@pytest.mark.gpu
def test_events_behind_the_first_trip_of_the_grid():
    """more events than 32 * CUs * 256 on an injected constant-dwell geometry: k_collapse_derive and k_pileup_rows take a second trip.  The
    rows are the true table: behind cap the collapse is Batch.events() and pileup_rows is Batch.pileup"""
    cap = _device_cap()
    gen, prof, fl, k = inject.context("exact1")
    counts = grid_event_counts(cap, 12)
    b = inject.run_geometry(gen, grid_seqs(counts, k))
    n = b.n_events
    assert_grid_shape(n, b.ev_off, cap)
    lens = np.array(counts + k - 1, np.int64)
    step = np.where(np.arange(12) & 1, -1, 1).astype(np.int8)
    key0 = np.where(step < 0, 3000 + lens - k, 17 * np.arange(12)).astype(np.int64)
    for norm in ("pa", "medmad"):
        t = b.events(norm, False, outputs=("sum", "sumsq", "ev_len", "mean", "sd"))
        rows = (torch.arange(n, dtype=torch.int64, device=_dev(b)), t.sum, t.sumsq, t.ev_len)
        ch = b.collapse(b.ev_off, *rows, norm=norm)
        for a, w in ((ch.mean, t.mean), (ch.sd, t.sd), (ch.ob_sum, t.sum), (ch.ob_sumsq, t.sumsq), (ch.ob_len, t.ev_len.to(torch.int64))):
            assert torch.equal(a[:cap].view(torch.int32 if a.dtype == torch.float32 else a.dtype), w[:cap].view(torch.int32 if w.dtype == torch.float32 else w.dtype))
            assert torch.equal(a[cap:].view(torch.int32 if a.dtype == torch.float32 else a.dtype), w[cap:].view(torch.int32 if w.dtype == torch.float32 else w.dtype)), "behind cap"
        assert torch.count_nonzero(ch.mean[cap:]) > (n - cap) // 2 and bool((ch.ob_rows == 1).all())
        width = int(lens.max()) + 3000
        for kw in (dict(by="ref", lo=2000, hi=width - 1000), dict(by="kmer", lo=0, hi=4 ** k // 2)):
            p1, p2 = gen.new_pileup(norm=norm, **kw), gen.new_pileup(norm=norm, **kw)
            counted, outside = b.pileup(p1, origin=(key0, step))
            assert b.pileup_rows(p2, b.ev_off, *rows, origin=(key0, step)) == (counted, outside, 0, 0) and counted > 0 and outside > 0
            for name in POUT:
                assert torch.equal(getattr(p1, name), getattr(p2, name)), f"{norm} {kw}: {name}"
    b.free(); gen.close()


def _raw_collapse(gen, b, cfg, off, cin, out):
    ref = lambda x: None if x is None else C.byref(x)          # noqa: E731
    return gen.L.sqg_batch_collapse(gen.ctx, b.handle if b is not None else None, ref(cfg), None if off is None else off.ctypes.data_as(C.POINTER(C.c_int64)), ref(cin), ref(out))


def _raw_pile(gen, b, cfg, org, off, cin, out, st=None):
    ref = lambda x: None if x is None else C.byref(x)          # noqa: E731
    return gen.L.sqg_batch_pileup_rows(gen.ctx, b.handle if b is not None else None, ref(cfg), ref(org), None if off is None else off.ctypes.data_as(C.POINTER(C.c_int64)),
                                       ref(cin), ref(out), ref(st))


@pytest.mark.gpu
def test_errors():
    d = _Six.get()
    gen, b = d["gen"], d["b"]
    err = lambda: gen.L.sqg_last_error(gen.ctx)                # noqa: E731
    t = _table(b, keys=("sum", "sumsq", "ev_len"))
    ev, s1, s2, ln = _rows_on(b, np.arange(b.n_events), t["sum"], t["sumsq"], t["ev_len"])
    ptr = dict(ev=ev.data_ptr(), sum=s1.data_ptr(), sumsq=s2.data_ptr(), len=ln.data_ptr())
    cin, off, cfg, none = api.CCollapseIn(**ptr), np.asarray(b.ev_off, np.int64).copy(), api.CCollapseCfg(api.CHUNK_PA, 0), api.CCollapseOut()
    pcfg, pnone = api.CPileupCfg(by=1, split=0, norm=api.CHUNK_PA, trim=0, segs=0, lo=0, hi=100), api.CPileupOut()
    assert _raw_collapse(gen, b, cfg, off, cin, none) == 0 and _raw_pile(gen, b, pcfg, None, off, cin, pnone) == 0
    assert gen.L.sqg_batch_collapse(None, b.handle, C.byref(cfg), off.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(cin), C.byref(none)) == -1
    assert gen.L.sqg_batch_pileup_rows(None, None, None, None, None, None, None, None) == -1
    for who, call in ((b"sqg_batch_collapse", lambda b_, c_, o_, i_, out_: _raw_collapse(gen, b_, c_, o_, i_, none if out_ else None)),
                      (b"sqg_batch_pileup_rows", lambda b_, c_, o_, i_, out_: _raw_pile(gen, b_, pcfg if c_ is not None else None, None, o_, i_, pnone if out_ else None))):
        assert call(None, cfg, off, cin, True) == -1 and who in err() and b"batch" in err()
        assert call(b, None, off, cin, True) == -1 and who in err() and b"cfg" in err()
        assert call(b, cfg, None, cin, True) == -1 and who in err() and b"row_off" in err()
        assert call(b, cfg, off, None, True) == -1 and who in err() and b"in must" in err()
        assert call(b, cfg, off, cin, False) == -1 and who in err() and b"out" in err()
        for field in ("ev", "sum", "len"):
            assert call(b, cfg, off, api.CCollapseIn(**dict(ptr, **{field: None})), True) == -1 and who in err() and b"in->" + field.encode() in err(), field
        for bad, what in ((lambda o: o.__setitem__(0, 1), b"start at 0"), (lambda o: o.__setitem__(3, o[2] - 1), b"decrease"), (lambda o: o.__setitem__(slice(3, None), o[3:] + (1 << 31)), b"2^31")):
            o2 = off.copy(); bad(o2)
            assert call(b, cfg, o2, cin, True) == -1 and who in err() and what in err(), what
    for bad, what in ((dict(norm=7), b"norm"), (dict(trim=2), b"trim"), (dict(trim=-1), b"trim")):
        assert _raw_collapse(gen, b, api.CCollapseCfg(**dict(dict(norm=api.CHUNK_PA, trim=0), **bad)), off, cin, none) == -1 and what in err()
    # no sumsq: refused where an output needs it, taken where none does
    nosq = api.CCollapseIn(**dict(ptr, sumsq=None))
    dev = _dev(b)
    buf = torch.zeros(b.n_events, dtype=torch.int64, device=dev)
    for field, ok in (("ob_sumsq", False), ("sd", False), ("mean", True), ("ob_sum", True), ("ob_rows", True)):
        rc = _raw_collapse(gen, b, cfg, off, nosq, api.CCollapseOut(**{field: buf.data_ptr()}))
        assert rc == (0 if ok else -1) and (ok or b"in->sumsq" in err()), field
    for field, ok in (("sd_sum", False), ("mean_sum", True), ("n", True)):
        pb = torch.zeros(100, dtype=torch.int64, device=dev)
        rc = _raw_pile(gen, b, pcfg, None, off, nosq, api.CPileupOut(**{field: pb.data_ptr()}))
        assert rc == (0 if ok else -1) and (ok or b"in->sumsq" in err()), field
    # the pileup's own cfg / origin errors
    good = dict(by=0, split=0, norm=api.CHUNK_PA, trim=0, segs=0, lo=0, hi=100)
    key0, step = np.zeros(6, np.int64), np.ones(6, np.int8)
    org = api.COrigin(key0.ctypes.data_as(C.POINTER(C.c_int64)), step.ctypes.data_as(C.POINTER(C.c_int8)))
    assert _raw_pile(gen, b, api.CPileupCfg(**good), org, off, cin, pnone) == 0
    for bad, what in ((dict(by=2), b"by"), (dict(split=4), b"split"), (dict(norm=2), b"norm"), (dict(trim=2), b"trim"), (dict(segs=16), b"segs"), (dict(lo=5, hi=4), b"hi"),
                      (dict(split=2), b"SQG_METH")):
        assert _raw_pile(gen, b, api.CPileupCfg(**dict(good, **bad)), org, off, cin, pnone) == -1 and b"sqg_batch_pileup_rows" in err() and what in err(), bad
    assert _raw_pile(gen, b, api.CPileupCfg(**good), None, off, cin, pnone) == -1 and b"origin" in err() and b"sampled" in err()
    assert _raw_pile(gen, b, api.CPileupCfg(**good), api.COrigin(None, org.step), off, cin, pnone) == -1 and b"origin" in err()
    step[2] = 2
    assert _raw_pile(gen, b, api.CPileupCfg(**good), org, off, cin, pnone) == -1 and b"step" in err()
    # the Python side's own checks
    for kw in (dict(row_off=off[:-1]), dict(ev=ev.to(torch.int32)), dict(ln=ln.cpu()), dict(s1=s1[:5]), dict(norm="z"), dict(outputs=("ob_rows", "median"))):
        a = dict(row_off=off, ev=ev, s1=s1, s2=s2, ln=ln, norm="pa", outputs=None); a.update(kw)
        with pytest.raises(api.SqgError) as e:
            b.collapse(a["row_off"], a["ev"], a["s1"], a["s2"], a["ln"], norm=a["norm"], outputs=a["outputs"])
        assert e.value.code == -1, kw


@pytest.mark.gpu
def test_guards_each_output_alone_no_rows_and_an_empty_batch():
    d = _Six.get()
    gen, b = d["gen"], d["b"]
    dev = _dev(b)
    rng = np.random.default_rng(2)
    row_off, ev, s1, s2, ln = _geometry_rows(b, rng)
    rows = _rows_on(b, ev, s1, s2, ln)
    ref = CR.collapse(row_off, ev, s1, s2, ln, b.ev_off, "medmad", **_consts(b, "medmad", False))
    dts = dict(ob_rows=torch.int32, ob_len=torch.int64, ob_sum=torch.int64, ob_sumsq=torch.int64, mean=torch.float32, sd=torch.float32, rd_dropped=torch.int32)
    guard, fill = 37, 0x5a5a5a5a
    off_p = row_off.ctypes.data_as(C.POINTER(C.c_int64))
    cin = api.CCollapseIn(*(t.data_ptr() for t in rows))
    cfg = api.CCollapseCfg(api.CHUNK_MEDMAD, 0)
    for names in (OUT,) + tuple((n,) for n in OUT):            # all of them, then each alone: guard values around every output, every element inside overwritten
        bufs, out = {}, api.CCollapseOut()
        for n in names:
            m = b.n_reads if n == "rd_dropped" else b.n_events
            bufs[n] = torch.full((m + 2 * guard,), fill, dtype=torch.int32, device=dev).view(torch.int32) if dts[n] != torch.int64 else torch.full((m + 2 * guard,), fill, dtype=torch.int64, device=dev)
            setattr(out, n, bufs[n].data_ptr() + guard * bufs[n].element_size())
        torch.cuda.synchronize(dev)
        assert gen.L.sqg_batch_collapse(gen.ctx, b.handle, C.byref(cfg), off_p, C.byref(cin), C.byref(out)) == 0
        for n in names:
            g = bufs[n].cpu().numpy()
            assert (g[:guard] == fill).all() and (g[len(g) - guard:] == fill).all(), f"{names}: a guard element of {n} was written"
            inner = g[guard:len(g) - guard]
            np.testing.assert_array_equal(R.bits(inner.view(ref[n].dtype) if n in ("mean", "sd", "ob_rows") else inner.astype(ref[n].dtype)), R.bits(ref[n]), err_msg=f"{names}: {n}")
    # no rows on a batch that is not empty: zeros everywhere (the API's tensors are pre-filled here, not zeroed), nothing added to a pileup
    zero_off = np.zeros(7, np.int64)
    none = _rows_on(b, np.zeros(0), np.zeros(0), np.zeros(0), np.zeros(0))
    bufs, out = {}, api.CCollapseOut()
    for n in OUT:
        bufs[n] = torch.full((b.n_reads if n == "rd_dropped" else b.n_events,), 7, dtype=dts[n], device=dev)
        setattr(out, n, bufs[n].data_ptr())
    keep = torch.zeros(1, dtype=torch.int64, device=dev)
    cin0 = api.CCollapseIn(*(keep.data_ptr(),) * 4)
    torch.cuda.synchronize(dev)
    assert gen.L.sqg_batch_collapse(gen.ctx, b.handle, C.byref(cfg), zero_off.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(cin0), C.byref(out)) == 0
    assert all(not bufs[n].cpu().numpy().view(np.int32).any() for n in OUT)
    got = _collapse(b, zero_off, none)
    assert all(not got[n].any() for n in OUT)
    p, into = _prefilled(gen, 9, by="kmer")
    assert b.pileup_rows(p, zero_off, *none) == (0, 0, b.n_events, 0)
    _assert_same(_pile(p), into, POUT, "no rows")
    # an empty batch succeeds and writes nothing
    e0 = gen.submit([])
    ch = e0.collapse(np.zeros(1, np.int64), *none)
    assert all(getattr(ch, n).numel() == 0 for n in OUT) and ch.n_rows == 0
    assert e0.pileup_rows(p, np.zeros(1, np.int64), *none) == (0, 0, 0, 0)
    _assert_same(_pile(p), into, POUT, "empty batch")
    e0.free()


@pytest.mark.gpu
def test_lifetime():
    """SQG_ESEQUENCE before the run and after two more batches, as sqg_batch_events"""
    _, _, gen = _context(dict(REFVEC_CASES)["rna004_tk4"], api.MODE_EXACT)
    reads = _fixture_reads("rna004_tk4")
    parts = [[r["seq"] for r in reads[0:4]], [r["seq"] for r in reads[4:8]], [r["seq"] for r in reads[0:4]]]
    b0 = gen.stage(parts[0])
    dev = torch.device("cuda", gen.device)
    one = (torch.zeros(4, dtype=torch.int64, device=dev),) * 3 + (torch.ones(4, dtype=torch.int32, device=dev),)
    off = np.arange(5, dtype=np.int64)
    new = lambda: gen.new_pileup(by="kmer")                    # noqa: E731
    for call, who in ((lambda: b0.collapse(off, *one), "sqg_batch_collapse"), (lambda: b0.pileup_rows(new(), off, *one), "sqg_batch_pileup_rows")):
        with pytest.raises(api.SqgError) as e:
            call()
        assert e.value.code == -4 and who in str(e.value) and "not been run" in str(e.value)
    b0.run().wait()
    t = b0.events()
    rows = (torch.arange(b0.n_events, dtype=torch.int64, device=dev), t.sum, t.sumsq, t.ev_len)
    quiet = b0.collapse(b0.ev_off, *rows)
    st = b0.pileup_rows(new(), b0.ev_off, *rows)
    assert torch.equal(quiet.mean.view(torch.int32), t.mean.view(torch.int32)) and st[0] > 0 and st[2:] == (0, 0)
    b1 = gen.stage(parts[1]).run().wait()
    again = b0.collapse(b0.ev_off, *rows)                      # after one more batch has run: the same
    assert all(torch.equal(getattr(again, n), getattr(quiet, n)) for n in SUMS) and b0.pileup_rows(new(), b0.ev_off, *rows) == st
    b2 = gen.stage(parts[2]).run().wait()
    for call, who in ((lambda: b0.collapse(b0.ev_off, *rows), "sqg_batch_collapse"), (lambda: b0.pileup_rows(new(), b0.ev_off, *rows), "sqg_batch_pileup_rows")):
        with pytest.raises(api.SqgError) as e:                  # two more batches: slabs and dwells are batch 2's
            call()
        assert e.value.code == -4 and who in str(e.value)
    for x in (b0, b1, b2):
        x.free()
    gen.close()


@pytest.mark.gpu
def test_call_order():
    """pileup, collapse, events, pileup_rows, align, collapse again on one batch: every result is what it is alone (the scratch of the
    event scan and of the pileup's reads is rewritten by the calls between)"""
    d = _ctx("dna")
    gen, b = d["gen"], d["b"]
    origin = (d["key0"], d["step"])
    dt = b.detect("dna", outputs=("sum", "sumsq", "dt_len", "true_ev"))
    rows = (dt.true_ev, dt.sum, dt.sumsq, dt.dt_len)
    kw = dict(by="ref", split=("strand",), norm="medmad", lo=1050, hi=1500)
    alone = {}
    p = gen.new_pileup(**kw); alone["pileup"] = (b.pileup(p, origin=origin), _pile(p))
    alone["collapse"] = _collapse(b, dt.det_off, rows, "medmad")
    alone["events"] = _table(b, "medmad")
    p = gen.new_pileup(**kw); alone["pileup_rows"] = (b.pileup_rows(p, dt.det_off, *rows, origin=origin), _pile(p))
    alone["align"] = _cpu(b.align(dt.det_off, dt.sum, dt.dt_len).al_ev)
    for trial in range(2):
        p = gen.new_pileup(**kw)
        assert b.pileup(p, origin=origin) == alone["pileup"][0]; _assert_same(_pile(p), alone["pileup"][1], POUT, "pileup")
        _assert_same(_collapse(b, dt.det_off, rows, "medmad"), alone["collapse"], OUT, "collapse")
        _assert_same(_table(b, "medmad"), alone["events"], api.EVENT_OUTPUTS, "events")
        p = gen.new_pileup(**kw)
        b.pileup_rows(p, dt.det_off, *rows, origin=(d["key0"] + 5, -d["step"]))      # (another origin between: the reads' table is rewritten)
        p = gen.new_pileup(**kw)
        assert b.pileup_rows(p, dt.det_off, *rows, origin=origin) == alone["pileup_rows"][0]; _assert_same(_pile(p), alone["pileup_rows"][1], POUT, "pileup_rows")
        np.testing.assert_array_equal(_cpu(b.align(dt.det_off, dt.sum, dt.dt_len).al_ev), alone["align"])
        _assert_same(_collapse(b, dt.det_off, rows, "medmad"), alone["collapse"], OUT, "collapse again")


@pytest.mark.gpu
@pytest.mark.parametrize("job", ["staged_t2_g2", "workers_t4_g2"])
def test_a_sharded_rank(job):
    """one range-sharded and one worker-sharded rank: detect -> align -> collapse and pileup_rows on the rank's batch against the
    reference over that rank's reads"""
    su = SC.Setup(job)
    done = False
    for bi, g, b, idx in SC.DRIVERS[su.job["kind"]](su):
        if done or g != su.G - 1 or b.n_reads < 3:
            continue
        done = True
        b.gen.profile = su.prof
        seqs = [su.staged_reads()[bi][i] for i in idx]
        lens = np.array([len(s) for s in seqs], np.int64)
        step = ((np.arange(len(idx)) % 3) - 1).astype(np.int8)
        key0 = SC.KEY_BASE + 50 * np.arange(len(idx), dtype=np.int64)
        dt = b.detect("dna", outputs=("sum", "sumsq", "dt_len"))
        al = b.align(dt.det_off, dt.sum, dt.dt_len, outputs=("al_ev",))
        evt = _table(b, keys=("ev_read", "kmer", "seg"))
        for norm, trim in SETTINGS[:2]:
            got = _collapse(b, dt.det_off, (al.al_ev, dt.sum, dt.sumsq, dt.dt_len), norm, trim)
            ref = CR.collapse(dt.det_off, _cpu(al.al_ev), _cpu(dt.sum), _cpu(dt.sumsq), _cpu(dt.dt_len), b.ev_off, norm, **_consts(b, norm, trim))
            _assert_same(got, ref, OUT, f"{job} {norm}")
            assert got["ob_rows"].max() >= 2
            p = b.gen.new_pileup(by="ref", split=("strand",), norm=norm, lo=SC.KEY_BASE, hi=SC.KEY_BASE + 3000)
            st = b.pileup_rows(p, dt.det_off, al.al_ev, dt.sum, dt.sumsq, dt.dt_len, origin=(key0, step))
            want, *wst = CR.pileup_rows(ref, evt, b.ev_off, key0, step, lens, su.k, su.rna, su.prefix, PR.BY_REF, PR.SPLIT_STRAND, 0, SC.KEY_BASE, SC.KEY_BASE + 3000)
            assert st == tuple(wst) and st[0] > 0
            _assert_same(_pile(p), want, POUT, f"{job} {norm}")
    assert done
