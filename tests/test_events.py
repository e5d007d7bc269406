"""include/sqg_events.h: the per-event signal table of a batch (sqg_batch_events), against the numpy statement of the header's rules
(events_ref.py), against the committed reference vectors and against the shipped calls on the same batch.  Every comparison is bit for
bit (floats as integers)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (before the library is loaded: the HIP runtime torch brings is the one the library then uses)

import chunks_ref as R
import events_ref as EV
import inject
import segments_ref as G
import targets_ref as T
from chunk_support import _context, _declared, _fixture_reads
from refvec_cases import REFVEC_CASES
from squigulator_amd import api, build, model, options, profiles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_LIB = os.path.join(ROOT, "oracle", "libsqg_cpu.so")
VECTORS = ("r9_t1", "r10_t1", "rna004_noprefix", "rna9_noprefix", "r9_prefix", "rna004_prefix", "rna9_prefix", "r9_meth", "r9_ideal", "r9_ideal_time")
OUT_KEYS = api.EVENT_OUTPUTS
SAMPLE_KEYS = ("sum", "sumsq", "vmin", "vmax", "mean", "sd")           # what the reduce pass writes
LANE_MAX = 64       # k_events_table.h's EVT_LANE_MAX: an event of up to 64 samples is reduced by one lane, a longer one by its wavefront


def _case(cid):
    """(options, k, rna, meth, prefix, (int)dwell_mean, level_mean) of a committed vector's command line"""
    o = options.parse_args(dict(REFVEC_CASES)[cid])
    k, meth = o.kmer_size_default, bool(o.meth_freq)
    return o, k, bool(o.flags & profiles.SQ_RNA), meth, bool(o.flags & profiles.SQ_PREFIX), int(o.profile.dwell_mean), model.synthetic_model(k, meth=meth)[0]


# ---------------------------------------------------------------------------------------------------------- no GPU
def test_header_declares_the_event_export_and_the_libraries_have_it():
    assert _declared("sqg_events.h") == set(api.EXPORTS_EVENTS) == {"sqg_batch_events"}
    others = set(api.EXPORTS) | set(api.EXPORTS_CHUNKS) | set(api.EXPORTS_TARGETS) | set(api.EXPORTS_SEGMENTS) | set(api.EXPORTS_SITES)
    assert not set(api.EXPORTS_EVENTS) & others
    assert _declared("sqg_sites.h") == set(api.EXPORTS_SITES) and _declared("sqg_segments.h") == set(api.EXPORTS_SEGMENTS)      # the other headers: unchanged
    assert _declared("sqg_targets.h") == set(api.EXPORTS_TARGETS) and _declared("sqg_chunks.h") == set(api.EXPORTS_CHUNKS) and _declared("sqg.h") == set(api.EXPORTS)
    build.build()
    for lib in (build.LIB, build.LIB_DEV):
        L = api.load_library(lib)
        for n in api.EXPORTS_EVENTS:
            assert hasattr(L, n), f"{n} not exported by {lib}"
    assert os.path.join(ROOT, "include", "sqg_events.h") in build.headers()
    for h in ("k_events_table.h", "h_events_table.h"):
        assert os.path.join(ROOT, "squigulator_amd", "csrc", h) in build.headers()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sqg_events.h")).read(), flags=re.S)
    for struct, ctype in (("sqg_event_cfg_t", api.CEventCfg), ("sqg_event_out_t", api.CEventOut)):
        body = hdr[:hdr.index("} " + struct)]
        body = body[body.rindex("typedef struct"):]
        fields = [f[0] for f in ctype._fields_]
        at = [body.index(name + ";") for name in fields]     # every field is declared, in the binding's order
        assert at == sorted(at), f"{struct}: {fields}"
        assert body.count(";") == len(fields), f"{struct}: the header has fields the binding lacks"
    assert [f[0] for f in api.CEventCfg._fields_] == ["norm", "trim"]
    assert tuple(f[0] for f in api.CEventOut._fields_) == OUT_KEYS == EV.PER_EVENT + EV.PER_READ


def test_the_cpu_backend_has_no_events_and_says_so():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "libsqg_cpu.so"])
    prof, fl = profiles.get_profile("dna-r9-prom")
    mean, stdv = model.synthetic_model(6)
    gen = api.SignalGenerator(prof, fl, 6, mean, stdv, 42, lib_path=CPU_LIB)
    for n in api.EXPORTS_EVENTS:
        assert not hasattr(gen.L, n)
    b = gen.submit([b"ACGTACGTACGTTTGACA" * 40])
    with pytest.raises(api.SqgError) as e:
        b.events()
    assert e.value.code == -1 and "sqg_batch_events" in str(e.value)
    b.free(); gen.close()


@pytest.mark.parametrize("cid", VECTORS)
def test_helper_against_the_reference_vectors(cid):
    """the compiled reference's own reads, dwells and signal: the rows tile every read, their sums add up to the read's, the segments'
    dwells to segments_ref's bounds, and k-mer and level are targets_ref's at every event's first generation-order sample"""
    o, k, rna, meth, prefix, sps, level = _case(cid)
    reads = _fixture_reads(cid)
    rng, dig = o.profile.range, o.profile.digitisation
    seen = set()
    for i, r in enumerate(reads):
        n = len(r["sig"])
        for norm, trim in (("pa", False), ("medmad", True)):
            w = EV.read_events(r, level, k, rna, meth, prefix, sps, norm, trim, rng, dig, i)
            ln, st = w["ev_len"].astype(np.int64), w["ev_start"]
            assert ln.sum() == n and (ln >= 1).all()
            order = np.argsort(st, kind="stable")
            assert st[order][0] == 0 and (st[order][1:] == (st + ln)[order][:-1]).all() and (st + ln)[order][-1] == n      # no gap, no overlap
            assert (np.diff(st) < 0).all() if rna else (np.diff(st) > 0).all()
            raw = r["sig"].astype(np.int64)
            assert w["sum"].sum() == raw.sum() and w["sumsq"].sum() == (raw * raw).sum()
            assert w["vmin"].min() == raw.min() and w["vmax"].max() == raw.max()
            sg = G.segments(r["ss"], len(r["seq"]), k, rna, prefix, sps)["seg"]
            for q in range(4):
                assert ln[w["seg"] == q].sum() == sg[q + 1] - sg[q], f"{cid} read {i} segment {q}"
            seen |= set(w["seg"].tolist())
            span = r["sig"][int(sg[3]):] if trim else r["sig"]
            assert (w["med2"], w["mad4"]) == R.stats(span)
            assert np.isfinite(w["mean"]).all() and (w["sd"] >= 0).all()
        if not prefix:
            clean_raw, moves, kmer = T.read_samples(r["seq"], r["ss"], r["offset"], level, k, rna, meth, rng, dig)
            first = st + ln - 1 if rna else st                # RNA: the first generation-order sample is the last stored one
            np.testing.assert_array_equal(w["kmer"], kmer[first]); np.testing.assert_array_equal(w["level_raw"], clean_raw[first])
            assert moves[first].all() and moves.sum() == len(st)
    assert seen == ({0, 1, 2, 3} if prefix and rna else {0, 1, 3} if prefix else {3})


def test_helper_on_a_hand_worked_read():
    """k = 3, level = rank, offset 0.5: the columns typed out"""
    level = np.arange(64, dtype=np.float32)
    read = dict(sig=np.array([5, 7, -3, 10, 10, 10, 1], np.int16), ss=[2, 1, 3, 1], seq=b"ACGTAC", offset=0.5)
    w = EV.read_events(read, level, 3, False, False, False, 2, "pa", False, 2.0, 4.0)
    assert w["ev_start"].tolist() == [0, 2, 3, 6] and w["ev_len"].tolist() == [2, 1, 3, 1] and w["seg"].tolist() == [3] * 4
    assert w["sum"].tolist() == [12, -3, 30, 1] and w["sumsq"].tolist() == [74, 9, 300, 1] and w["vmin"].tolist() == [5, -3, 10, 1] and w["vmax"].tolist() == [7, -3, 10, 1]
    assert w["kmer"].tolist() == [0b000110, 0b011011, 0b101100, 0b110001]                     # ACG CGT GTA TAC
    assert w["level_raw"].tolist() == [int(r * 4.0 / 2.0 - 0.5) for r in (6, 27, 44, 49)]
    np.testing.assert_array_equal(w["mean"], np.array([(6 + .5) * 2 / 4, (-3 + .5) * 2 / 4, (10 + .5) * 2 / 4, (1 + .5) * 2 / 4], np.float32))
    np.testing.assert_array_equal(w["sd"], np.array([1 * 2 / 4, 0, 0, 0], np.float32))
    w = EV.read_events(read, level, 3, True, False, False, 2, "medmad", False)                # the same samples as an RNA read's: stored reversed
    assert w["ev_start"].tolist() == [5, 4, 1, 0] and w["sum"].tolist() == [11, 10, 14, 5]
    assert (w["med2"], w["mad4"]) == (14, 12)                                                  # sorted -3 1 5 7 10 10 10; |2 raw - 14|: 20 12 4 0 6 6 6
    inv = np.float64(np.float32(1.0 / (1.4826 * 3.0)))
    np.testing.assert_array_equal(w["mean"], np.array([(5.5 - 7) * inv, (10 - 7) * inv, (14 / 3 - 7) * inv, (5 - 7) * inv], np.float32))


# ---------------------------------------------------------------------------------------------------------- GPU
def _cpu(t):
    return None if t is None else t.cpu().numpy()


def _own_reads(b, seqs):
    """the batch's own fetched signal and dwells with the reads it was staged from, as events_ref takes them"""
    sig, dw = b.signal(), b.dwell()
    return [dict(sig=sig[b.sig_off[i]:b.sig_off[i + 1]], ss=dw[b.ev_off[i]:b.ev_off[i + 1]], seq=s, offset=float(b.offset[i])) for i, s in enumerate(seqs)]


def _assert_events(ev, want, what, keys=OUT_KEYS):
    assert ev.n_events == want["ev_off"][-1], f"{what}: {ev.n_events} rows, expected {want['ev_off'][-1]}"
    for key in keys:
        got = _cpu(getattr(ev, key))
        assert got is not None, f"{what}: {key} missing"
        if key == "kmer":
            got = got.view(np.uint32)
        assert got.shape == want[key].shape and got.dtype == want[key].dtype, f"{what}: {key} {got.shape} {got.dtype} vs {want[key].shape} {want[key].dtype}"
        np.testing.assert_array_equal(R.bits(got), R.bits(want[key]), err_msg=f"{what}: {key}")


def _check(b, own, level, k, rna, meth, prefix, sps, what, settings=(("pa", False), ("medmad", False), ("pa", True), ("medmad", True))):
    prof, wants = b.gen.profile, {}
    for norm, trim in settings:
        want = wants[(norm, trim)] = EV.batch_events(own, level, k, rna, meth, prefix, sps, norm, trim, prof.range, prof.digitisation)
        np.testing.assert_array_equal(want["ev_off"], b.ev_off)
        _assert_events(b.events(norm, trim), want, f"{what} {norm} trim {trim}")
    if not prefix and len(settings) == 4:                   # without SQG_PREFIX trim changes nothing
        for key in OUT_KEYS:
            np.testing.assert_array_equal(R.bits(wants[("medmad", False)][key]), R.bits(wants[("medmad", True)][key]))
    return wants


@pytest.mark.gpu
@pytest.mark.parametrize("cid,mode", [(cid, api.MODE_CERTIFIED) for cid in VECTORS] + [("rna004_prefix", api.MODE_EXACT)],
                         ids=[f"{cid}-certified" for cid in VECTORS] + ["rna004_prefix-exact"])
def test_events_of_the_reference_vectors(cid, mode):
    """the fixture's reads through the HIP path: every output, both norms, trim 0 and 1, against events_ref fed with the batch's own signal
    and dwells -- which are the fixture's"""
    o, k, rna, meth, prefix, sps, level = _case(cid)
    reads = _fixture_reads(cid)
    _, _, gen = _context(dict(REFVEC_CASES)[cid], mode)
    for lo in range(0, len(reads), o.batch):
        part = reads[lo:lo + o.batch]
        b = gen.stage([r["seq"] for r in part]).run().wait()
        own = _own_reads(b, [r["seq"] for r in part])
        for r, w in zip(part, own):
            np.testing.assert_array_equal(w["sig"], r["sig"]); np.testing.assert_array_equal(w["ss"], r["ss"])
        _check(b, own, level, k, rna, meth, prefix, sps, f"{cid} reads {lo}..")
        b.free()
    gen.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ("r10_t1", "rna004_noprefix", "r9_meth", "r9_prefix", "rna004_prefix"))
def test_agreement_with_the_shipped_calls_on_the_same_batch(cid):
    """med2 / mad4 are Batch.chunks' (the trimmed call's for trim), the segments' dwells add up to Batch.segments' bounds, and k-mer and
    level of a row are what Batch.chunk_targets writes at the row's first generation-order sample, for one chunk per read"""
    o, k, rna, meth, prefix, sps, level = _case(cid)
    reads = _fixture_reads(cid)[:o.batch]
    _, _, gen = _context(dict(REFVEC_CASES)[cid], api.MODE_CERTIFIED)
    b = gen.stage([r["seq"] for r in reads]).run().wait()
    plain, trimmed = b.events("medmad", False), b.events("medmad", True)
    ch = b.chunks(2048, 2048, 0, labels=False, signal=False, trim=True)
    assert torch.equal(trimmed.med2, ch.med2) and torch.equal(trimmed.mad4, ch.mad4)
    if not prefix:
        ch = b.chunks(2048, 2048, 0, labels=False, signal=False)
        assert torch.equal(plain.med2, ch.med2) and torch.equal(plain.mad4, ch.mad4)
    seg, shift = (_cpu(t) for t in b.segments())
    ln, code, start = _cpu(plain.ev_len).astype(np.int64), _cpu(plain.seg), _cpu(plain.ev_start)
    kmer, lvl = _cpu(plain.kmer), _cpu(plain.level_raw)
    L = 1024
    ch = b.chunks(L, L, 0, labels=False, signal=False, trim=prefix)
    tg = b.chunk_targets(L, L, clean=False, clean_raw=True, moves=True, kmer=True, trim=prefix)
    cstart, traw, tk, tm = _cpu(ch.chunk_start), _cpu(tg.clean_raw), _cpu(tg.kmer), _cpu(tg.moves)
    compared = 0
    for i in range(b.n_reads):
        rows = slice(int(b.ev_off[i]), int(b.ev_off[i + 1]))
        for q in range(4):
            assert ln[rows][code[rows] == q].sum() == seg[i][q + 1] - seg[i][q], f"{cid} read {i} segment {q}"
        assert ch.chunk_off[i + 1] > ch.chunk_off[i]
        c = int(ch.chunk_off[i] + ch.chunk_off[i + 1]) // 2                     # one chunk of the read: its stored samples [c0, c0 + L)
        c0 = int(seg[i][3]) + int(cstart[c])
        first = start[rows] + ln[rows] - 1 if rna else start[rows]              # the row's first generation-order sample, as stored
        inside = (first >= c0) & (first < c0 + L) & (code[rows] == 3) & ~((first >= shift[i][0]) & (first < shift[i][1]))
        assert inside.sum() >= 10
        at = first[inside] - c0
        assert tm[c][at].all() and tm[c].sum() == ((first >= c0) & (first < c0 + L)).sum()
        np.testing.assert_array_equal(tk[c][at], kmer[rows][inside]); np.testing.assert_array_equal(traw[c][at], lvl[rows][inside])
        compared += int(inside.sum())
    assert compared >= 10 * b.n_reads
    b.free(); gen.close()


def _ideal_time(dwell, name="dna-r9-prom", extra=0):
    prof, fl = profiles.get_profile(name)
    prof = prof.replace(dwell_mean=float(dwell), dwell_std=0.0)
    fl |= profiles.SQ_IDEAL_TIME | extra
    k = profiles.default_kmer_size(fl)
    mean, stdv = model.synthetic_model(k)
    return api.SignalGenerator(prof, fl, k, mean, stdv, inject.SEED, num_workers=1, mode=api.MODE_CERTIFIED), k, mean


SIGNALS = {
    "low": lambda n: np.full(n, -32768, np.int16),
    "high": lambda n: np.full(n, 32767, np.int16),
    "alternating": lambda n: np.where(np.arange(n) & 1, 32767, -32768).astype(np.int16),
    "ramp": lambda n: ((np.arange(n, dtype=np.int64) * 7919) % 65536 - 32768).astype(np.int16),
}


@pytest.mark.gpu
@pytest.mark.parametrize("dwell", [1, 2, LANE_MAX - 1, LANE_MAX, LANE_MAX + 1, 5000])
def test_constant_dwell_with_injected_signals(dwell):
    """SQG_IDEAL_TIME with every dwell 1, 2, 63, 64 (the last a lane takes alone), 65 (the first its wavefront takes) and 5000; the samples
    overwritten with the extremes of int16, their alternation and a ramp.  Reads of 3, 1 and 70 events: the second starts at an odd
    sample of the slab when the dwell is odd, and the third fills a wavefront with long events"""
    gen, k, level = _ideal_time(dwell)
    seqs = inject.seqs_for(inject.bases_for([3 * dwell, dwell, 70 * dwell, 2 * dwell], k, dwell))
    b = inject.run_geometry(gen, seqs)
    assert b.n_events == 76 and b.n_samples == 76 * dwell and (dwell % 2 == 0 or b.sig_off[1] % 2 == 1)
    for name, make in SIGNALS.items():
        inject.inject(b, make(b.n_samples))
        own = _own_reads(b, seqs)
        assert all((np.asarray(r["ss"]) == dwell).all() for r in own)
        wants = _check(b, own, level, k, False, False, False, dwell, f"dwell {dwell} {name}", settings=(("pa", False), ("medmad", True)))
        w = wants[("pa", False)]
        assert not np.isnan(w["mean"]).any() and not np.isnan(w["sd"]).any() and (w["sd"] >= 0).all()
        if dwell == 1:
            assert (w["sd"] == 0).all() and (w["vmin"] == w["sum"]).all() and (w["vmax"] == w["sum"]).all()
        if name in ("low", "high"):
            assert (w["sd"] == 0).all() and (w["vmin"] == w["vmax"]).all()
        if name == "alternating" and dwell == 5000:
            assert (w["sumsq"] > 1 << 32).all() and (w["vmin"] == -32768).all() and (w["vmax"] == 32767).all() and (w["sum"] == -2500).all()
    b.free(); gen.close()


DRAWN = {  # name -> (profile, extra flags, dwell_mean, dwell_std, bases of a read shorter than a k-mer)
    "r9": ("dna-r9-prom", 0, 40.0, 48.0, b"ACGTA"),
    "rna004": ("rna004-prom", 0, 40.0, 48.0, b"ACGUACGU"),
    "meth": ("dna-r9-prom", profiles.SQ_METH, 30.0, 40.0, b"ACM"),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(DRAWN))
def test_drawn_dwells_from_one_to_beyond_the_lane_limit(name):
    """dwells drawn with a spread larger than their mean: 1 up to several times 64 in one read, so that lanes and wavefront share the events
    of one launch.  Event counts around the scan's tile of 1024 events (tests/label_cases.py: TILE), a read of exactly k bases, a read
    shorter than a k-mer between two ordinary reads, reads with odd sample counts, an empty batch"""
    pname, extra, dmean, dstd, short = DRAWN[name]
    prof, fl = profiles.get_profile(pname)
    prof = prof.replace(dwell_mean=dmean, dwell_std=dstd)
    fl |= extra
    k = profiles.default_kmer_size(fl)
    meth, rna = bool(fl & profiles.SQ_METH), bool(fl & profiles.SQ_RNA)
    level, stdv = model.synthetic_model(k, meth=meth)
    gen = api.SignalGenerator(prof, fl, k, level, stdv, 7, num_workers=1, mode=api.MODE_CERTIFIED)
    rng = np.random.default_rng(5)
    letters = list(b"ACGT" + (b"M" if meth else b"") + b"acgtNRYU")
    counts = [1, 2, 1023, 1024, 1025, 2049, 300]
    seqs = [bytes(rng.choice(letters, ev + k - 1).astype(np.uint8)) for ev in counts]
    seqs.insert(3, short)
    assert len(short) < k and len(seqs[0]) == k
    b = gen.submit(seqs)
    own = _own_reads(b, seqs)
    assert [len(r["ss"]) for r in own] == counts[:3] + [5] + counts[3:]
    ss = np.concatenate([r["ss"] for r in own])
    assert ss.min() == 1 and ss.max() > 2 * LANE_MAX and {LANE_MAX - 1, LANE_MAX, LANE_MAX + 1} <= set(ss.tolist())
    assert int(np.asarray(own[6]["ss"]).max()) > LANE_MAX and int(np.asarray(own[6]["ss"]).min()) == 1        # both paths in one read
    assert (np.asarray(b.sig_off[1:-1]) % 2 == 1).any() and (np.diff(b.sig_off) % 2 == 1).any()
    wants = _check(b, own, level, k, rna, meth, False, int(dmean), f"drawn {name}")
    w = wants[("pa", False)]
    assert (w["seg"] == 3).all() and (w["kmer"][int(b.ev_off[3]):int(b.ev_off[4])] == T.kmer_ranks(G.SHORT_HACK[:5 + k - 1], k, meth)).all()
    b.free()
    b = gen.submit([])
    ev = b.events("medmad", True)
    assert ev.n_events == 0 and all(tuple(getattr(ev, key).shape) == (0,) for key in OUT_KEYS)
    b.free(); gen.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pname", ["dna-r9-prom", "rna-r9-prom", "rna004-prom"])
def test_short_inserts_behind_an_attached_prefix(pname):
    """SQG_PREFIX with reads of 1, 2 and k - 1 bases next to ordinary ones: the attached chain is longer than a k-mer whatever the read, the
    insert has few events or none (DNA: the adaptor loses events), and the RNA stall chain follows"""
    prof, fl = profiles.get_profile(pname)
    fl |= profiles.SQ_PREFIX
    k = profiles.default_kmer_size(fl)
    rna = bool(fl & profiles.SQ_RNA)
    level, stdv = model.synthetic_model(k)
    gen = api.SignalGenerator(prof, fl, k, level, stdv, 11, num_workers=1, mode=api.MODE_CERTIFIED)
    seqs = inject.seqs_for([1, 400, 2, k - 1, k, 77])
    b = gen.submit(seqs)
    own = _own_reads(b, seqs)
    wants = _check(b, own, level, k, rna, False, True, int(prof.dwell_mean), f"prefix {pname}")
    w = wants[("pa", False)]
    first = w["seg"][:int(b.ev_off[1])]
    assert set(first.tolist()) == ({0, 1, 2, 3} if rna else {0, 1}) and (first == 3).sum() == (1 if rna else 0)
    assert wants[("medmad", True)]["med2"][0] != wants[("medmad", False)]["med2"][0] or rna
    b.free(); gen.close()


def _raw_call(gen, b, cfg, ptrs):
    return gen.L.sqg_batch_events(gen.ctx, b.handle, C.byref(cfg), C.byref(api.CEventOut(*[ptrs.get(n) for n in OUT_KEYS])))


@pytest.mark.gpu
def test_nothing_but_the_rows_is_written():
    """caller arrays at their natural alignment and no more inside one guarded buffer, the byte array at an odd address: the bytes of every
    output are events_ref's, every other byte keeps its fill; every output alone, all, none, and the sample-derived ones alone"""
    prof, fl = profiles.get_profile("rna-r9-prom")
    fl |= profiles.SQ_PREFIX
    k = profiles.default_kmer_size(fl)
    level, stdv = model.synthetic_model(k)
    gen = api.SignalGenerator(prof, fl, k, level, stdv, 11, num_workers=1, mode=api.MODE_CERTIFIED)
    seqs = inject.seqs_for([31, 5, 90])
    b = gen.submit(seqs)
    own = _own_reads(b, seqs)
    buf = torch.empty(1 << 17, dtype=torch.uint8, device="cuda")
    base = buf.data_ptr()
    assert base % 16 == 0
    wants = {}

    def run(norm, trim, names):
        if (norm, trim) not in wants:
            wants[(norm, trim)] = EV.batch_events(own, level, k, True, False, True, int(prof.dwell_mean), norm, trim, prof.range, prof.digitisation)
        want = wants[(norm, trim)]
        at, place = 40, {}
        for name in OUT_KEYS:                               # every array at an odd multiple of its element size
            align = want[name].dtype.itemsize
            at = (at + align - 1) // align * align
            if at % (2 * align) == 0:
                at += align
            place[name] = at
            at += want[name].nbytes + 24
        assert at < buf.numel()
        buf.fill_(0xA5)
        torch.cuda.synchronize()
        cfg = api.CEventCfg(api.CHUNK_PA if norm == "pa" else api.CHUNK_MEDMAD, int(trim))
        assert _raw_call(gen, b, cfg, {n: base + place[n] for n in names}) == 0, gen.L.sqg_last_error(gen.ctx)
        got = buf.cpu().numpy()
        expect = np.full(buf.numel(), 0xA5, np.uint8)
        for n in names:
            expect[place[n]:place[n] + want[n].nbytes] = np.ascontiguousarray(want[n]).view(np.uint8).reshape(-1)
        bad = np.flatnonzero(got != expect)
        assert len(bad) == 0, f"{norm} trim {trim} {names}: byte {bad[0]} of the buffer ({[n for n in OUT_KEYS if place[n] <= bad[0]][-1:]} is at {place})"

    for norm, trim in (("medmad", True), ("pa", False)):
        for names in [(n,) for n in OUT_KEYS] + [OUT_KEYS, (), SAMPLE_KEYS]:
            run(norm, trim, names)
    b.free(); gen.close()


@pytest.mark.gpu
def test_errors():
    o, k, rna, meth, prefix, sps, level = _case("r9_prefix")
    reads = _fixture_reads("r9_prefix")
    _, _, gen = _context(dict(REFVEC_CASES)["r9_prefix"], api.MODE_CERTIFIED)
    b = gen.stage([r["seq"] for r in reads])
    with pytest.raises(api.SqgError) as e:                  # staged, not run: an error, not a hang
        b.events()
    assert e.value.code == -4 and "sqg_batch_events" in str(e.value)
    b.run().wait()
    assert b.events().n_events == b.n_events > 0
    for bad, what in ((dict(norm=2), "norm"), (dict(norm=7), "norm"), (dict(trim=2), "trim"), (dict(trim=-1), "trim")):
        with pytest.raises(api.SqgError) as e:
            b.events(**bad)
        assert e.value.code == -1 and "sqg_batch_events" in str(e.value) and what in str(e.value), bad
    with pytest.raises(api.SqgError) as e:
        b.events(outputs=("mean", "median"))
    assert e.value.code == -1 and "median" in str(e.value)
    Lb, cfg, none = gen.L, api.CEventCfg(api.CHUNK_PA, 0), api.CEventOut()
    err = lambda: Lb.sqg_last_error(gen.ctx)                # noqa: E731
    assert Lb.sqg_batch_events(None, None, None, None) == -1 and Lb.sqg_batch_events(None, b.handle, C.byref(cfg), C.byref(none)) == -1
    assert Lb.sqg_batch_events(gen.ctx, None, C.byref(cfg), C.byref(none)) == -1 and b"sqg_batch_events" in err() and b"batch" in err()
    assert Lb.sqg_batch_events(gen.ctx, b.handle, None, C.byref(none)) == -1 and b"sqg_batch_events" in err() and b"cfg" in err()
    assert Lb.sqg_batch_events(gen.ctx, b.handle, C.byref(cfg), None) == -1 and b"sqg_batch_events" in err() and b"out" in err()
    assert Lb.sqg_batch_events(gen.ctx, b.handle, C.byref(cfg), C.byref(none)) == 0          # nothing wanted: nothing written
    b.free(); gen.close()


@pytest.mark.gpu
def test_lifetime_and_events_while_the_generator_runs_ahead():
    """a batch keeps its table until two more batches have been run; taken while two later batches are staged and one is running it is
    what it was when the generator was quiet"""
    o, k, rna, meth, prefix, sps, level = _case("rna004_tk4")
    reads = _fixture_reads("rna004_tk4")
    _, _, gen = _context(dict(REFVEC_CASES)["rna004_tk4"], api.MODE_EXACT)
    parts = [[r["seq"] for r in reads[0:4]], [r["seq"] for r in reads[4:8]], [r["seq"] for r in reads[0:4]], [r["seq"] for r in reads[4:8]]]
    b0 = gen.stage(parts[0]).run().wait()
    quiet = b0.events("medmad", True)
    _assert_events(quiet, EV.batch_events(_own_reads(b0, parts[0]), level, k, rna, meth, prefix, sps, "medmad", True, o.profile.range, o.profile.digitisation), "quiet")
    assert quiet.n_events > 0
    b1, b2, b3 = (gen.stage(p) for p in parts[1:])
    b1.run()                                                # one running, two staged
    busy = b0.events("medmad", True)
    for key in OUT_KEYS:
        assert torch.equal(getattr(busy, key), getattr(quiet, key)), key
    b1.wait()
    again = b0.events("medmad", True)                       # after one more batch has run: the same
    for key in OUT_KEYS:
        assert torch.equal(getattr(again, key), getattr(quiet, key)), key
    b2.run().wait()
    with pytest.raises(api.SqgError) as e:                  # two more batches: slabs and dwells are batch 2's
        b0.events("medmad", True)
    assert e.value.code == -4 and "sqg_batch_events" in str(e.value)
    ev = b1.events("pa", False)
    _assert_events(ev, EV.batch_events(_own_reads(b1, parts[1]), level, k, rna, meth, prefix, sps, "pa", False, o.profile.range, o.profile.digitisation), "batch 1 after batch 2")
    for b in (b0, b1, b2, b3):
        b.free()
    gen.close()
