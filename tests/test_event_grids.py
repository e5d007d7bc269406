"""The flat grids of k_events_table.h, k_pileup.h and k_detect.h past their first trip, pileup keys past 32 bits, the sampler's origin on
several contigs and both strands, and long events beside lanes that are not taken.  k_evtab_reduce, k_pileup and k_detect_rows run on at
most 32 workgroups per compute unit and walk the events (k_detect_rows: the detected rows) with a stride of the whole grid: a batch of
more than cap = 32 * CUs * 256 of them is the only one whose events are met on a second trip.  Every comparison is bit for bit; every
precondition (the event count against cap, the dwells behind cap, strands, contigs, taken and skipped lanes) is asserted of the batch
itself, so that a device with another number of compute units either meets it or fails on it."""
import os

import numpy as np
import pytest
import torch  # noqa: F401  (before the library is loaded: the HIP runtime torch brings is the one the library then uses)

import chunks_ref as R
import detect_ref as D
import detect_vec as DVEC
import events_ref as EV
import events_vec as VEC
import inject
import pileup_ref as PR
import segments_ref as G
import signal_cases
from chunk_support import _fixture_reads
from refvec_cases import REFVEC_CASES
from squigulator_amd import api, build, model, options, profiles
from test_events import VECTORS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NCOV = os.path.join(ROOT, "tests", "golden", "inputs", "nCoV-2019.reference.fasta")
OUT = api.PILEUP_OUTPUTS
WG = 256            # k_common.h's CHUNK_WG: the events of one workgroup and trip
LANE_MAX = 64       # k_events_table.h's EVT_LANE_MAX

# The drawn-dwell batch of B and C.  A dwell is |round(N(mean, std))| folded at 1 (src/gensig.c:254-257), so a dwell above 128 among the
# few hundred thousand events behind cap needs std >= 28 or so whatever the mean: about 25 samples per event is the least such a batch
# can have (8 +- 30: P(dwell > 128) = 3e-5, some 10 events behind cap on 256 compute units).
GRID_PROFILE, GRID_K, GRID_DWELL, GRID_SEED, GRID_READS, GRID_WORKERS = "dna-r9-prom", 6, (8.0, 30.0), 7, 600, 4
LONG_READS = 12     # the constant-dwell batch: fewer, longer reads

# The batch of k_detect_rows' grid: injected samples on a constant-dwell geometry.  Under DETECT_CFG the short window is one sample, where
# t is |x[i] - x[i-1]| (D = 0): a square wave of two samples per level with +-9 of noise has a boundary at every change of level, rows of
# two samples, and a constant stretch is one row.
DETECT_CFG = (1, 2, 1.0, 1.0, 0.1)
DETECT_GEOMETRY, DETECT_DWELL, DETECT_READS = "exact15", 15, 300
DETECT_STRETCHES = (61, 62, 63, 64, 65, 66, 67, 129, 130, 200, 300) * 6      # samples of the constant stretches behind cap, in this order
DETECT_GAPS = (7, 60)                                                         # samples of square wave between two stretches: drawn, odd and even


def _case(cid):
    o = options.parse_args(dict(REFVEC_CASES)[cid])
    k, meth = o.kmer_size_default, bool(o.meth_freq)
    return o, k, bool(o.flags & profiles.SQ_RNA), meth, bool(o.flags & profiles.SQ_PREFIX), int(o.profile.dwell_mean), model.synthetic_model(k, meth=meth)[0]


def _offsets(lens):
    return np.concatenate(([0], np.cumsum(lens))).astype(np.int64)


def grid_event_counts(cap, n_reads, seed=1):
    """events per read: n_reads unequal counts that add up to cap + cap / 8 + cap / 32 + 37"""
    total = cap + cap // 8 + cap // 32 + 37
    w = np.random.default_rng(seed).uniform(0.25, 1.75, n_reads)
    counts = np.floor(w / w.sum() * total).astype(np.int64)
    counts[-1] += total - counts.sum()
    assert counts.sum() == total and counts.min() >= 16
    return counts


def grid_seqs(counts, k, seed=2):
    rng = np.random.default_rng(seed)
    return [np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(c) + k - 1)].tobytes() for c in counts]


def grid_generator(lib_path=None):
    prof, fl = profiles.get_profile(GRID_PROFILE)
    prof = prof.replace(dwell_mean=GRID_DWELL[0], dwell_std=GRID_DWELL[1])
    level, stdv = model.synthetic_model(GRID_K)
    return api.SignalGenerator(prof, fl, GRID_K, level, stdv, GRID_SEED, num_workers=GRID_WORKERS, mode=api.MODE_CERTIFIED, lib_path=lib_path), prof, level


def assert_grid_shape(n_events, ev_off, cap):
    """the event count against cap, and a read boundary inside the second trip"""
    assert cap + cap // 8 <= n_events <= cap + cap // 2 and n_events % 64 != 0, (n_events, cap)
    inner = np.asarray(ev_off)[1:-1]
    assert ((inner > cap) & (inner < n_events)).any(), "no read boundary behind cap"


def assert_dwell_mix(dw, cap):
    """the dwells the second trip meets: both ways of evtab_take, their border, and both in one wavefront"""
    dw = np.asarray(dw, np.int64)
    assert dw.min() == 1
    behind = dw[cap:]
    have = set(behind[(behind >= LANE_MAX - 1) & (behind <= LANE_MAX + 1)].tolist())
    assert have == {LANE_MAX - 1, LANE_MAX, LANE_MAX + 1}, f"behind cap the dwells around {LANE_MAX} are {sorted(have)}"
    assert behind.max() > 2 * LANE_MAX, f"the longest dwell behind cap is {behind.max()}"
    whole = behind[:len(behind) // 64 * 64].reshape(-1, 64)                     # (cap is a multiple of 64: these are wavefronts)
    assert cap % 64 == 0 and ((whole <= LANE_MAX).any(axis=1) & (whole > LANE_MAX).any(axis=1)).any(), "no wavefront behind cap with both kinds"


def detect_grid_lengths(cap, n_reads, dwell, seed=1):
    """samples per read: n_reads unequal multiples of the dwell that add up to the samples cap + cap / 8 rows of two take, and the stretches"""
    total = 2 * (cap + cap // 8) + sum(DETECT_STRETCHES) + len(DETECT_STRETCHES) * sum(DETECT_GAPS) // 2
    w = np.random.default_rng(seed).uniform(0.25, 1.75, n_reads)
    events = np.floor(w / w.sum() * (total / dwell)).astype(np.int64)
    events[-1] += -(-total // dwell) - events.sum()
    assert events.min() >= 8 and events.sum() * dwell >= total
    return events * dwell


def detect_grid_signal(n, cap, seed=5):
    """n samples: 2 cap + cap / 8 samples of square wave -- rows of two: cap + cap / 16 rows --, then, behind row cap, the constant
    stretches, each followed by a gap of square wave of a drawn length whose phase starts anew, then square wave to the end"""
    rng = np.random.default_rng(seed)
    wave = lambda m: np.where((np.arange(m) // 2) & 1, 900, 500)             # noqa: E731
    parts = [wave(2 * cap + cap // 8)]
    for ln in DETECT_STRETCHES:
        parts += [np.full(ln, 700), wave(int(rng.integers(DETECT_GAPS[0], DETECT_GAPS[1] + 1)))]
    used = sum(len(p) for p in parts)
    assert used < n, (used, n)
    x = np.concatenate(parts + [wave(n - used)])
    flat = np.concatenate([np.zeros(len(p), bool) if i % 2 == 0 else np.ones(len(p), bool) for i, p in enumerate(parts + [x[:0]])] + [np.zeros(n - used, bool)])
    return np.where(flat, x, x + rng.integers(-9, 10, n)).astype(np.int16)


def detect_grid_starts(sig, sig_off):
    """per read the first sample of every detected row: detect_ref's peak machine"""
    return [np.array([0] + D.boundaries(sig[sig_off[r]:sig_off[r + 1]], DETECT_CFG), np.int64) for r in range(len(sig_off) - 1)]


def assert_detect_mix(want, sig_off, cap):
    """of the reference's rows alone: more than cap of them, the last wavefront partly empty, a read boundary inside the second trip, and
    behind cap rows of 2, 63, 64, 65 and more than 128 samples, a group of 64 rows that holds both ways of evtab_take, and rows of either
    way that start at odd and at even samples of the slab"""
    n, ln = int(want["det_off"][-1]), want["dt_len"].astype(np.int64)
    assert n > cap and n % 64 != 0 and cap % 64 == 0, (n, cap)
    inner = want["det_off"][1:-1]
    assert ((inner > cap) & (inner < n)).any(), "no read boundary behind cap"
    behind = ln[cap:]
    assert {2, LANE_MAX - 1, LANE_MAX, LANE_MAX + 1} <= set(behind.tolist()) and behind.max() > 2 * LANE_MAX, sorted(set(behind.tolist()))
    whole = behind[:len(behind) // 64 * 64].reshape(-1, 64)
    assert ((whole <= LANE_MAX).any(axis=1) & (whole > LANE_MAX).any(axis=1)).any(), "no group of 64 rows behind cap with both kinds"
    at = (np.asarray(sig_off, np.int64)[want["dt_read"]] + want["dt_start"])[cap:]
    for kind in (behind <= LANE_MAX, behind > LANE_MAX):
        assert set((at[kind] & 1).tolist()) == {0, 1}, "rows behind cap start at samples of one parity only"


# ---------------------------------------------------------------------------------------------------------- no GPU
def _assert_same(got, want, keys, what):
    for key in keys:
        assert got[key].shape == want[key].shape and got[key].dtype == want[key].dtype, f"{what}: {key} {got[key].shape} {got[key].dtype} vs {want[key].shape} {want[key].dtype}"
        np.testing.assert_array_equal(R.bits(got[key]), R.bits(want[key]), err_msg=f"{what}: {key}")


@pytest.mark.parametrize("cid", VECTORS + ("rna9_prefix_again",))
def test_the_vectorised_rows_are_events_ref_bit_for_bit(cid):
    """events_vec.batch_rows against events_ref.batch_events on the compiled reference's own reads, dwells and signal: DNA and RNA, with
    and without a prefix (two chains, stored reversed), both norms, and trimmed statistics where there is a prefix.  The last case
    is an RNA-with-prefix vector cut to reads of unequal order, so that a read boundary is not where the vector had it"""
    again = cid == "rna9_prefix_again"
    cid = "rna9_prefix" if again else cid
    o, k, rna, meth, prefix, sps, level = _case(cid)
    reads = _fixture_reads(cid)
    if again:
        reads = reads[::-1]
        assert rna and prefix and len(reads) > 1
    sig = np.concatenate([r["sig"] for r in reads])
    dw = np.concatenate([np.asarray(r["ss"], np.int64) for r in reads])
    sig_off, ev_off = _offsets([len(r["sig"]) for r in reads]), _offsets([len(r["ss"]) for r in reads])
    offset = [r["offset"] for r in reads]
    rng, dig = o.profile.range, o.profile.digitisation
    for r in reads:
        assert VEC.stats_fast(r["sig"]) == R.stats(r["sig"])
    base = None
    for norm, trim in (("pa", False), ("medmad", False)) + ((("medmad", True),) if prefix else ()):
        want = EV.batch_events(reads, level, k, rna, meth, prefix, sps, norm, trim, rng, dig)
        stats = None
        if trim:
            spans = [G.segments(r["ss"], len(r["seq"]), k, rna, prefix, sps)["seg"] for r in reads]
            stats = [VEC.stats_fast(r["sig"][int(s[3]):int(s[4])]) for r, s in zip(reads, spans)]
        got = VEC.batch_rows(sig, sig_off, dw, ev_off, offset, rna, norm, rng, dig, stats)
        _assert_same(got, want, VEC.PLACE_KEYS + VEC.SAMPLE_KEYS + (() if norm == "pa" else EV.PER_READ), f"{cid} {norm} trim {trim}")
        if base is None:
            base = got
        else:                                                 # what a later call takes over from an earlier one is what it would compute
            _assert_same(VEC.batch_rows(sig, sig_off, dw, ev_off, offset, rna, norm, rng, dig, stats, reuse=base), got, VEC.PLACE_KEYS + VEC.SAMPLE_KEYS, f"{cid} reuse")
    assert len(dw) > 0 and (rna == bool((np.diff(got["ev_start"][:int(ev_off[1])]) < 0).all()))


def test_the_grid_batch_plan():
    """the plan of the drawn-dwell batch for any number of compute units: the event count rule, unequal reads, a boundary behind cap"""
    for cu in (64, 104, 256, 304):
        cap = 32 * cu * WG
        counts = grid_event_counts(cap, GRID_READS)
        assert_grid_shape(int(counts.sum()), _offsets(counts), cap)
        assert counts.max() > 3 * counts.min() and len(set(counts.tolist())) > GRID_READS // 2
        counts = grid_event_counts(cap, LONG_READS)
        assert_grid_shape(int(counts.sum()), _offsets(counts), cap)
    with pytest.raises(AssertionError):
        assert_dwell_mix(np.full(3 * 64, 5), 64)
    assert_dwell_mix(np.array([1] * 64 + [63, 64, 65, 129] + [2] * 60 + [7] * 5), 64)


@pytest.mark.parametrize("norm", ["pa", "medmad"])
def test_the_vectorised_detected_rows_are_detect_ref_bit_for_bit(norm):
    """detect_vec.batch_rows against detect_ref.batch_rows on a small batch made as the grid's: the same wave, stretches and geometry
    with a cap of 2048 rows, so the rows are of the same kinds (assert_detect_mix); every column, the statistics and det_off"""
    cap, k = 2048, 6
    prof, _ = profiles.get_profile("dna-r9-prom")
    lens = detect_grid_lengths(cap, 9, DETECT_DWELL)
    sig_off = _offsets(lens)
    sig = detect_grid_signal(int(sig_off[-1]), cap)
    offset = np.random.default_rng(2).uniform(-250, 50, len(lens))
    reads = [dict(sig=sig[sig_off[r]:sig_off[r + 1]], ss=np.full(n // DETECT_DWELL, DETECT_DWELL, np.int64), seq=b"A" * (n // DETECT_DWELL + k - 1), offset=float(offset[r]))
             for r, n in enumerate(lens)]
    want = D.batch_rows(reads, DETECT_CFG, k, False, False, DETECT_DWELL, norm, False, prof.range, prof.digitisation)
    dw = np.concatenate([r["ss"] for r in reads])
    got = DVEC.batch_rows(sig, sig_off, detect_grid_starts(sig, sig_off), dw, _offsets([len(r["ss"]) for r in reads]), offset, norm, prof.range, prof.digitisation)
    np.testing.assert_array_equal(got["det_off"], want["det_off"])
    _assert_same(got, want, D.PER_ROW + (D.PER_READ if norm != "pa" else ()), f"detected rows {norm}")
    assert_detect_mix(want, sig_off, cap)
    assert len(set(want["true_ev"].tolist())) > len(dw) // 2


# ---------------------------------------------------------------------------------------------------------- GPU
def _cpu(t):
    return None if t is None else t.cpu().numpy()


def _device_cap():
    return 32 * torch.cuda.get_device_properties(0).multi_processor_count * WG         # h_context.h: num_cu is the same attribute


def _table_of(ev, keys):
    out = {n: _cpu(getattr(ev, n)) for n in keys}
    if "kmer" in out:
        out["kmer"] = out["kmer"].view(np.uint32)
    return out


class _Grid:
    """one batch of GRID_READS reads and cap * 1.16 events with drawn dwells, in a context of its own, and what B and C share of it"""
    made = None

    @classmethod
    def get(cls):
        if cls.made is None:
            cap = _device_cap()
            counts = grid_event_counts(cap, GRID_READS)
            gen, prof, level = grid_generator()
            seqs = grid_seqs(counts, GRID_K)
            b = gen.stage(seqs).run().wait()
            dw = b.dwell()
            assert_grid_shape(b.n_events, b.ev_off, cap)
            np.testing.assert_array_equal(b.ev_off, _offsets(counts))
            assert_dwell_mix(dw, cap)
            cls.made = dict(gen=gen, b=b, cap=cap, prof=prof, level=level, seqs=seqs, dw=dw, sig=b.signal(), tables={}, rows={})
        return cls.made

    @classmethod
    def table(cls, norm):
        """all fourteen outputs of Batch.events(norm) as numpy arrays"""
        d = cls.get()
        if norm not in d["tables"]:
            d["tables"][norm] = _table_of(d["b"].events(norm, False), api.EVENT_OUTPUTS)
        return d["tables"][norm]

    @classmethod
    def rows(cls, norm):
        """events_vec's statement of the table from the batch's fetched signal and dwells"""
        d = cls.get()
        if norm not in d["rows"]:
            b, prof = d["b"], d["prof"]
            d["rows"][norm] = VEC.batch_rows(d["sig"], b.sig_off, d["dw"], b.ev_off, b.offset, False, norm, prof.range, prof.digitisation,
                                             reuse=next(iter(d["rows"].values()), None))
        return d["rows"][norm]


class _DetectGrid:
    """one injected batch of DETECT_READS reads whose detected table under DETECT_CFG has cap * 1.13 rows, and the reference's rows of it"""
    made = None

    @classmethod
    def get(cls):
        if cls.made is None:
            cap = _device_cap()
            gen, prof, fl, k = inject.context(DETECT_GEOMETRY)
            lens = detect_grid_lengths(cap, DETECT_READS, DETECT_DWELL)
            b = inject.run_geometry(gen, inject.seqs_for(inject.bases_for(lens, k, DETECT_DWELL)))
            np.testing.assert_array_equal(np.diff(b.sig_off), lens)
            sig = detect_grid_signal(b.n_samples, cap)
            inject.inject(b, sig)
            dw = b.dwell()
            assert (dw == DETECT_DWELL).all() and len(set(lens.tolist())) > DETECT_READS // 2 and lens.max() > 3 * lens.min()
            cls.made = dict(gen=gen, b=b, cap=cap, prof=prof, sig=sig, dw=dw, starts=detect_grid_starts(sig, b.sig_off), rows={})
        return cls.made

    @classmethod
    def rows(cls, norm):
        d = cls.get()
        if norm not in d["rows"]:
            b, prof = d["b"], d["prof"]
            d["rows"][norm] = DVEC.batch_rows(d["sig"], b.sig_off, d["starts"], d["dw"], b.ev_off, b.offset, norm, prof.range, prof.digitisation,
                                              reuse=next(iter(d["rows"].values()), None))
        return d["rows"][norm]


def _assert_rows_behind_cap(got, want, keys, cap, n, what):
    """rows [cap, n) are compared, on their own, and hold something: Batch.events() hands the library zeroed arrays (fill value 0)"""
    assert cap < n
    for key in keys:
        g, w = got[key], want[key]
        assert g.shape == w.shape == (n,) and g.dtype == w.dtype, f"{what}: {key} {g.shape} {g.dtype} vs {w.shape} {w.dtype}"
        np.testing.assert_array_equal(R.bits(g[:cap]), R.bits(w[:cap]), err_msg=f"{what}: {key}, first trip")
        np.testing.assert_array_equal(R.bits(g[cap:]), R.bits(w[cap:]), err_msg=f"{what}: {key}, rows behind cap")
        # (equal to a reference that is mostly not 0, the rows behind cap are not the fill: a medmad mean or the sd of one sample may be 0)
        assert np.count_nonzero(R.bits(w[cap:])) > (n - cap) // 2 and np.count_nonzero(R.bits(g[cap:])) > (n - cap) // 2, f"{what}: {key} behind cap holds the fill value"
    for key in ("ev_len", "sumsq"):
        if key in keys:
            assert (got[key][cap:] > 0).all(), f"{what}: {key} behind cap holds the fill value"


@pytest.mark.gpu
@pytest.mark.parametrize("norm", ["pa", "medmad"])
def test_events_behind_the_first_trip_of_the_grid(norm):
    """k_events_table.h:158, `base += gridDim.x * CHUNK_WG` of evtab_for_rows under k_evtab_reduce (:167): its second trip, which no earlier test takes (their
    batches hold a few thousand events, one trip covers 32 * CUs * 256).  Behind cap the batch has dwells of 1, 63, 64, 65 and above 128
    and a wavefront with both kinds, so evtab_take's lane loop and its ballot / shuffle loop both run there, in one wavefront too; the
    last wavefront is partly empty (n_events is no multiple of 64), and `if (have)` at line 170 is false on the second trip.  All
    twelve columns: the sample-derived ones against events_vec over the fetched signal and dwells, the places against np.repeat / cumsum
    of the dwells, k-mer, segment and level against events_ref on the first read, the last and the one that straddles cap"""
    d = _Grid.get()
    b, cap, dw, k = d["b"], d["cap"], d["dw"], GRID_K
    n = b.n_events
    got, want = _Grid.table(norm), _Grid.rows(norm)
    assert len(EV.PER_EVENT) == 12 and all(got[key] is not None and len(got[key]) == n for key in EV.PER_EVENT)
    _assert_rows_behind_cap(got, want, VEC.SAMPLE_KEYS, cap, n, f"grid {norm}")
    counts = np.diff(b.ev_off)
    place = dict(ev_read=np.repeat(np.arange(b.n_reads, dtype=np.int32), counts), ev_len=dw.astype(np.int32),
                 ev_start=(np.cumsum(dw, dtype=np.int64) - dw) - np.repeat(np.asarray(b.sig_off[:-1], np.int64), counts))
    _assert_rows_behind_cap(got, place, VEC.PLACE_KEYS, cap, n, f"grid {norm}")
    if norm == "medmad":
        np.testing.assert_array_equal(got["med2"], want["med2"]); np.testing.assert_array_equal(got["mad4"], want["mad4"])
    straddle = int(np.searchsorted(b.ev_off, cap, side="right")) - 1
    assert b.ev_off[straddle] < cap < b.ev_off[straddle + 1] and 0 < straddle < b.n_reads - 1
    assert (got["seg"] == 3).all()
    for r in (0, straddle, b.n_reads - 1):
        own = dict(sig=d["sig"][b.sig_off[r]:b.sig_off[r + 1]], ss=dw[b.ev_off[r]:b.ev_off[r + 1]], seq=d["seqs"][r], offset=float(b.offset[r]))
        w = EV.read_events(own, d["level"], k, False, False, False, int(d["prof"].dwell_mean), norm, False, d["prof"].range, d["prof"].digitisation, r)
        rows = slice(int(b.ev_off[r]), int(b.ev_off[r + 1]))
        for key in EV.PER_EVENT:
            np.testing.assert_array_equal(R.bits(got[key][rows]), R.bits(w[key].astype(EV.DTYPES[key])), err_msg=f"grid {norm} read {r}: {key}")
        if norm == "medmad":
            assert (int(got["med2"][r]), int(got["mad4"][r])) == (w["med2"], w["mad4"]) == R.stats(own["sig"])


@pytest.mark.gpu
@pytest.mark.parametrize("norm", ["pa", "medmad"])
def test_detected_rows_behind_the_first_trip_of_the_grid(norm):
    """k_events_table.h:158, `base += gridDim.x * CHUNK_WG` of evtab_for_rows under k_detect_rows (k_detect.h:183): its second trip, which no earlier test takes (their tables hold a
    few hundred thousand rows, one trip covers 32 * CUs * 256).  Behind cap the table has rows of 2, 63, 64, 65 and more than 128
    samples that start at odd and at even samples of the slab, and a wavefront with both kinds, so evtab_take's lane loop and its
    ballot / shuffle loop both run there; the last wavefront is partly empty, and `if (!have) return` at k_detect.h:187 is met on the second
    trip.  det_off of the plan call and all twelve outputs against detect_vec, which the test above pins to detect_ref"""
    d = _DetectGrid.get()
    b, cap = d["b"], d["cap"]
    want = _DetectGrid.rows(norm)
    n = int(want["det_off"][-1])
    assert_detect_mix(want, b.sig_off, cap)
    assert cap + cap // 16 <= n <= cap + cap // 4, (n, cap)
    plan, n_rows = b.detect_plan(DETECT_CFG)
    np.testing.assert_array_equal(plan, want["det_off"], err_msg="the plan")
    dt = b.detect(DETECT_CFG, norm, False)
    assert n_rows == dt.n_rows == n
    np.testing.assert_array_equal(dt.det_off, want["det_off"])
    got = _table_of(dt, api.DETECT_OUTPUTS)
    _assert_rows_behind_cap(got, want, D.PER_ROW, cap, n, f"detect grid {norm}")
    assert (got["dt_len"][cap:] > 0).all() and (got["sumsq"][cap:] > 0).all()
    stats = np.array([VEC.stats_fast(d["sig"][b.sig_off[r]:b.sig_off[r + 1]]) for r in range(b.n_reads)], np.int32)      # (the whole reads' under either norm)
    np.testing.assert_array_equal(got["med2"], stats[:, 0]); np.testing.assert_array_equal(got["mad4"], stats[:, 1])
    if norm == "medmad":
        np.testing.assert_array_equal(want["med2"], stats[:, 0]); np.testing.assert_array_equal(want["mad4"], stats[:, 1])


@pytest.mark.gpu
def test_constant_dwell_events_behind_the_first_trip():
    """k_events_table.h:112, the `Q.dwell == nullptr` branch (SQG_IDEAL_TIME) on the second trip of k_evtab_reduce, in the development
    build of the library: every dwell is 65, so behind cap every lane's event is reduced by its wavefront (evtab_take's ballot is full on a
    trip no earlier test takes, and partly empty in the last wavefront).  The samples are signal_cases' `uniform`: all of int16"""
    cap = _device_cap()
    prof, fl = profiles.get_profile("dna-r9-prom")
    dwell = LANE_MAX + 1
    prof = prof.replace(dwell_mean=float(dwell), dwell_std=0.0)
    fl |= profiles.SQ_IDEAL_TIME
    k = profiles.default_kmer_size(fl)
    level, stdv = model.synthetic_model(k)
    gen = api.SignalGenerator(prof, fl, k, level, stdv, inject.SEED, num_workers=1, mode=api.MODE_CERTIFIED, lib_path=build.LIB_DEV)
    assert api.build_info(gen.L)["dev"] == "1"
    counts = grid_event_counts(cap, LONG_READS)
    b = inject.run_geometry(gen, grid_seqs(counts, k))
    n = b.n_events
    assert_grid_shape(n, b.ev_off, cap)
    dw = b.dwell()
    assert (dw == dwell).all() and b.n_samples == n * dwell
    sig = signal_cases.CASES["uniform"](b.sig_off)
    inject.inject(b, sig)
    want = VEC.batch_rows(sig, b.sig_off, dw, b.ev_off, b.offset, False, "pa", prof.range, prof.digitisation)
    ev = b.events("pa", False)
    keys = VEC.PLACE_KEYS + VEC.SAMPLE_KEYS
    _assert_rows_behind_cap(_table_of(ev, keys), want, keys, cap, n, "constant dwell pa")
    assert want["vmin"][cap:].min() < -32000 and want["vmax"][cap:].max() > 32000
    # MEDMAD: the device's own statistics (test_chunks.py pins them; the shortest read's are checked here) with the header's formulas
    ev = b.events("medmad", False, outputs=("mean", "sd", "med2", "mad4"))
    med2, mad4 = _cpu(ev.med2), _cpu(ev.mad4)
    r = int(np.argmin(counts))
    assert (int(med2[r]), int(mad4[r])) == VEC.stats_fast(sig[b.sig_off[r]:b.sig_off[r + 1]])
    want = VEC.batch_rows(sig, b.sig_off, dw, b.ev_off, b.offset, False, "medmad", stats=list(zip(med2.tolist(), mad4.tolist())), reuse=want)
    _assert_rows_behind_cap(_table_of(ev, ("mean", "sd")), want, ("mean", "sd"), cap, n, "constant dwell medmad")
    b.free(); gen.close()


def _got(p):
    out = {}
    for n in OUT:
        t = getattr(p, n)
        out[n] = None if t is None else (t.cpu().numpy().view(np.uint32) if n == "n" else t.cpu().numpy())
    return out


def _assert_pile(p, want, what):
    got = _got(p)
    for n in OUT:
        if got[n] is None:
            continue
        assert got[n].shape == want[n].shape and got[n].dtype == want[n].dtype, f"{what}: {n} {got[n].shape} {got[n].dtype}"
        np.testing.assert_array_equal(got[n], want[n], err_msg=f"{what}: {n}")


def _laid_over_a_span(lens, k, width, seed):
    """a caller's origin: every read's leftmost k-mer somewhere in [0, width), every other read backwards"""
    rng = np.random.default_rng(seed)
    left = rng.integers(0, width, len(lens)).astype(np.int64)
    step = np.where(np.arange(len(lens)) & 1, -1, 1).astype(np.int8)
    return np.where(step < 0, left + (np.asarray(lens, np.int64) - k), left), step


@pytest.mark.gpu
@pytest.mark.parametrize("norm", ["pa", "medmad"])
def test_pileup_behind_the_first_trip_of_the_grid(norm):
    """k_events_table.h:158, `base += gridDim.x * CHUNK_WG` of evtab_for_rows under k_pileup (k_pileup.h:32): its second trip, with the
    two ballots of k_pileup.h:60 and the `return` of line 65 on it, which no earlier test takes.  The drawn-dwell batch of the event test under a caller's origin that lays 600 reads
    over some 9000 keys, half of them backwards (a few hundred adds per key), by position with a window that cuts the span at both ends
    and by pore-table row with a window over half the rows: events behind cap are counted and are outside, so evtab_take gets lanes that
    are taken and lanes that are not next to long events there.  All six outputs against pileup_ref over the batch's event table (which
    the event test compares) and np.bincount; two calls give the same bytes"""
    d = _Grid.get()
    gen, b, cap, k = d["gen"], d["b"], d["cap"], GRID_K
    ev = _Grid.table(norm)
    lens = np.array([len(s) for s in d["seqs"]], np.int64)
    key0, step = _laid_over_a_span(lens, k, 3000, 4)
    eligible = int((lens - k + 1).sum())
    assert eligible == b.n_events
    rows = 4 ** k
    span = int(3000 + (lens - k).max())
    for by, lo, hi in (("ref", 1500, span - 2500), ("kmer", rows // 3, rows // 3 + rows // 2)):
        byc = api.PILEUP_BY_REF if by == "ref" else api.PILEUP_BY_KMER
        ok, key, _ = PR.eligible_and_key(ev, b.ev_off, key0, step, lens, k, False, False, byc)
        inside = ok & (key >= lo) & (key < hi)
        assert ok.all() and inside[cap:].any() and (~inside[cap:]).any(), f"{by}: behind cap nothing is counted, or nothing is outside"
        if by == "ref":
            assert key.min() < lo and key.max() >= hi                      # the window cuts the span at both ends
        whole = slice(cap, cap + (b.n_events - cap) // 64 * 64)                 # the whole wavefronts behind cap
        taken_long = (inside[whole] & (ev["ev_len"][whole] > LANE_MAX)).reshape(-1, 64)
        skipped = ~inside[whole].reshape(-1, 64)
        assert (taken_long.any(axis=1) & skipped.any(axis=1)).any(), f"{by}: no wavefront behind cap with a long taken event beside a skipped one"
        p = gen.new_pileup(by=by, norm=norm, lo=lo, hi=hi)
        counted, outside = b.pileup(p, origin=(key0, step))
        want, wc, wo = PR.pileup(ev, b.ev_off, key0, step, lens, k, False, False, byc, 0, 0, lo, hi)
        assert (counted, outside) == (wc, wo) == (int(inside.sum()), int((~inside).sum())) and counted + outside == eligible and counted > 0 and outside > 0
        _assert_pile(p, want, f"grid {by} {norm}")
        g = _got(p)
        np.testing.assert_array_equal(g["n"][0], np.bincount((key[inside] - lo).astype(np.int64), minlength=hi - lo).astype(np.uint32))
        assert int(g["n"].sum()) == counted and g["n"].max() >= (100 if by == "ref" else 2)
        again = gen.new_pileup(by=by, norm=norm, lo=lo, hi=hi)
        assert b.pileup(again, origin=(key0, step)) == (counted, outside)
        for name in OUT:
            assert torch.equal(getattr(p, name), getattr(again, name)), f"{by} {name}: two calls differ"


@pytest.mark.gpu
def test_pileup_keys_beyond_32_bits_and_below_zero():
    """k_pileup.h:47 and 57, `key = pr.key0 + step * j` and the window comparison, and :66, `key - U.lo`, with keys that need more than
    32 bits (hg38 laid end to end passes 2^31 at chr13) and with negative ones: every earlier key is below 30 000.  A caller's origin is
    shifted by 2^31 - 150, 2^32 - 150, 2^40 + 7, -150 and -2^33 - 150 together with a window that cuts reads at both ends and straddles the
    power of two (or 0): the six arrays of both strand planes and (counted, outside) must be those of the unshifted call, which is
    compared with pileup_ref.  By row, a window [-5, rows + 5) puts the rows at offset 5 of guarded buffers"""
    prof, fl = profiles.get_profile("dna-r9-prom")
    k = 6
    mean, stdv = model.synthetic_model(k)
    gen = api.SignalGenerator(prof, fl, k, mean, stdv, 9, num_workers=4, mode=api.MODE_CERTIFIED)
    seqs = inject.seqs_for([300] * 11 + [7, 450] * 4 + [300])
    n_reads = len(seqs)
    b = gen.stage(seqs, workers=np.arange(n_reads) % 4).run().wait()
    lens = np.array([len(s) for s in seqs], np.int64)
    key0, step = _laid_over_a_span(lens, k, 400, 6)
    step[[3, 12]] = 0
    a, z = 100, 450
    left = np.where(step < 0, key0 - (lens - k), key0)
    live = (step != 0) & (lens >= k)
    assert (live & (left < a) & (left + lens - k >= a)).any() and (live & (left < z) & (left + lens - k >= z)).any()   # reads cut at both ends
    ev = _table_of(b.events("pa"), ("ev_read", "ev_len", "mean", "sd", "kmer", "seg"))
    plain = gen.new_pileup(split=("strand",), lo=a, hi=z)
    st = b.pileup(plain, origin=(key0, step))
    want, wc, wo = PR.pileup(ev, b.ev_off, key0, step, lens, k, False, False, PR.BY_REF, PR.SPLIT_STRAND, 0, a, z)
    assert st == (wc, wo) and wc > 0 and wo > 0 and plain.planes == 2
    _assert_pile(plain, want, "unshifted")
    assert all(_got(plain)["n"][q].any() for q in (0, 1))
    for base, edge in ((2 ** 31 - 150, 2 ** 31), (2 ** 32 - 150, 2 ** 32), (2 ** 40 + 7, None), (-150, 0), (-(2 ** 33) - 150, -(2 ** 33))):
        lo, hi = base + a, base + z
        assert lo < edge < hi - 1 if edge is not None else lo > 2 ** 40
        p = gen.new_pileup(split=("strand",), lo=lo, hi=hi)
        assert (p.cfg.lo, p.cfg.hi) == (lo, hi)
        assert b.pileup(p, origin=(key0 + base, step)) == st, f"base {base}"
        for name in OUT:
            assert torch.equal(getattr(p, name), getattr(plain, name)), f"base {base}: {name}"
    # by row, the window wider than the table at both ends: guarded buffers as in test_a_window_that_cuts_reads_and_guarded_outputs
    rows, pad, guard = 4 ** k, 5, 37
    width = rows + 2 * pad
    dev = torch.device("cuda", gen.device)
    p = gen.new_pileup(by="kmer", lo=-pad, hi=rows + pad, outputs=())
    bufs = {}
    for name in OUT:
        bufs[name] = torch.full((width + 2 * guard,), -0x5a5a5a5b, dtype=torch.int32 if name == "n" else torch.int64, device=dev)
        bufs[name][guard:guard + width] = 0
        setattr(p, name, bufs[name][guard:guard + width].view(1, width))
    counted, outside = b.pileup(p)
    sel = ev["seg"] == 3
    assert (counted, outside) == (int(sel.sum()), 0) and counted == b.n_events
    at = ev["kmer"].astype(np.int64) + pad
    q_mean, q_sd, ln = PR.q(ev["mean"]), PR.q(ev["sd"]), ev["ev_len"].astype(np.int64)
    g = _got(p)
    np.testing.assert_array_equal(g["n"][0], np.bincount(at, minlength=width).astype(np.uint32))
    for name, col in (("dwell", ln), ("dwell_sq", ln * ln), ("mean_sum", q_mean), ("mean_sq", q_mean * q_mean), ("sd_sum", q_sd)):
        w = np.zeros(width, np.int64)
        np.add.at(w, at, col)
        np.testing.assert_array_equal(g[name][0], w, err_msg=name)
    for name in OUT:
        x = bufs[name].cpu().numpy()
        assert not x[guard:guard + pad].any() and not x[guard + width - pad:guard + width].any(), f"{name}: an element outside the rows was added to"
        assert (x[:guard] == -0x5a5a5a5b).all() and (x[guard + width:] == -0x5a5a5a5b).all(), f"{name}: a guard element was written"
    b.free(); gen.close()


def _fasta(path):
    seqs = []
    for ln in open(path, "rb"):
        if ln.startswith(b">"):
            seqs.append([])
        else:
            seqs[-1].append(ln.strip())
    return [b"".join(s) for s in seqs]


def _revcomp(s):
    return s.translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1]


@pytest.mark.gpu
def test_the_sampler_origin_on_four_contigs_and_both_strands():
    """h_pileup.h:58, `h_contig_off[ref_idx] + ref_pos + (minus ? rlen - k : 0)`, with a contig offset that is not 0 on both strands: the
    DNA tests load one contig, the sequin test has '+' reads only, so the '-' rule on a later contig rested on pileup_ref.sampler_origin,
    which states the same formula.  Here the origin is not restated: every read's text (or its reverse complement) is found in the
    contigs laid end to end with bytes.find, and the whole-genome n of the pileup is the coverage of the k-mers of those matches, per
    strand plane by whether the read or its reverse complement matched"""
    prof, fl = profiles.get_profile("dna-r9-prom")
    k, rlen = 6, 600
    mean, stdv = model.synthetic_model(k)
    whole = _fasta(NCOV)[0]
    cuts = [0, 3001, 10007, 22003, len(whole)]
    contigs = [whole[cuts[i]:cuts[i + 1]] for i in range(4)]
    assert len(set(len(c) for c in contigs)) == 4 and b"".join(contigs) == whole
    gen = api.SignalGenerator(prof, fl, k, mean, stdv, 42, num_workers=3, mode=api.MODE_CERTIFIED)
    gen.load_genome(contigs, rlen)
    b = gen.sample(64).run().wait()
    s = b.sampled
    strand = np.frombuffer(s["strand"], np.uint8)
    assert len(set(s["ref_idx"].tolist())) >= 3
    assert any(set(strand[s["ref_idx"] == c].tolist()) == set(b"+-") for c in (1, 2, 3)), "no later contig with reads of both strands"
    g = whole.upper()
    cover = np.zeros((2, len(g)), np.uint32)
    seen = set()
    for i, read in enumerate(b.reads()):
        text = read.upper()
        assert len(text) == s["rlen"][i] >= k and set(text) <= set(b"ACGT")
        hits = [(m, t) for m, t in ((0, text), (1, _revcomp(text))) if g.find(t) >= 0]
        assert len(hits) == 1, f"read {i} matches the genome {len(hits)} times"
        m, t = hits[0]
        at = g.find(t)
        assert g.find(t, at + 1) < 0, f"read {i} is found twice"
        assert (m == 1) == (s["strand"][i:i + 1] == b"-")
        cover[m, at:at + len(t) - k + 1] += 1
        seen.add((int(np.searchsorted(cuts, at, side="right")) - 1, m))
    assert any((c, 0) in seen and (c, 1) in seen for c in (1, 2, 3))
    flat = gen.new_pileup(outputs=("n",))
    assert (flat.cfg.lo, flat.cfg.hi) == (0, len(g))
    counted, outside = b.pileup(flat)
    assert (counted, outside) == (int(cover.sum()), 0)
    np.testing.assert_array_equal(_got(flat)["n"][0], cover.sum(axis=0, dtype=np.uint32))
    planes = gen.new_pileup(split=("strand",), outputs=("n",))
    assert b.pileup(planes) == (counted, 0)
    np.testing.assert_array_equal(_got(planes)["n"], cover)
    assert cover[0].any() and cover[1].any() and cover.sum(axis=0).max() >= 2
    b.free(); gen.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dwell", [LANE_MAX + 1, 5000])
def test_long_events_beside_lanes_that_are_not_taken(dwell):
    """k_pileup.h:59, `evtab_take(W, inside && ..., ...)` with `take` false in some lanes of a wavefront whose other lanes hold events
    longer than EVT_LANE_MAX: evtab_take's ballot (k_events_table.h:81) then has holes, and the lanes that are not taken still load and
    shuffle for their neighbours.  The earlier constant-dwell test has all 76 events inside the window.  Dwells of 65 and 5000; by row with
    a window over a scattered subset of the events, and by position with a window that takes events 10 .. 40 of the 70-event read; the
    outputs against np.add.at over the columns of the event table"""
    prof, fl = profiles.get_profile("dna-r9-prom")
    prof = prof.replace(dwell_mean=float(dwell), dwell_std=0.0)
    fl |= profiles.SQ_IDEAL_TIME
    k = profiles.default_kmer_size(fl)
    mean, stdv = model.synthetic_model(k)
    gen = api.SignalGenerator(prof, fl, k, mean, stdv, inject.SEED, num_workers=1, mode=api.MODE_CERTIFIED)
    events = [3, 1, 70, 2]
    seqs = inject.seqs_for(inject.bases_for([e * dwell for e in events], k, dwell))
    b = inject.run_geometry(gen, seqs)
    assert b.n_events == 76 and b.n_samples == 76 * dwell
    rows = 4 ** k
    key0, step = np.array([1000, 2000, 69, 3000], np.int64), np.array([1, 1, -1, 1], np.int8)
    for name in ("uniform", "svb_wrap"):
        inject.inject(b, signal_cases.CASES[name](b.sig_off))
        for norm in ("pa", "medmad"):
            t = b.events(norm, False)
            ev = dict(ev_read=_cpu(t.ev_read), ev_len=_cpu(t.ev_len).astype(np.int64), kmer=_cpu(t.kmer).view(np.uint32).astype(np.int64), mean=_cpu(t.mean), sd=_cpu(t.sd))
            assert (ev["ev_len"] == dwell).all() and dwell > LANE_MAX
            e = np.arange(76) - np.asarray(b.ev_off)[ev["ev_read"]]                    # the event's index within its read
            by_ref = (ev["ev_read"] == 2) & (e >= 10) & (e <= 40)
            lo_k, hi_k = int(np.sort(ev["kmer"])[20]), int(np.sort(ev["kmer"])[55])
            by_kmer = (ev["kmer"] >= lo_k) & (ev["kmer"] < hi_k)
            for by, taken, lo, hi in (("ref", by_ref, 69 - 40, 69 - 10 + 1), ("kmer", by_kmer, lo_k, hi_k)):
                wave = taken[:64]                                                       # one aligned group of 64 events: the first wavefront
                assert wave.any() and not wave.all() and 10 <= taken.sum() <= 60, f"{by}: taken and skipped lanes do not share a wavefront"
                if by == "kmer":
                    assert (np.diff(wave.astype(np.int8)) != 0).sum() >= 8                 # scattered, not one run
                key = (69 - e) if by == "ref" else ev["kmer"]
                p = gen.new_pileup(by=by, norm=norm, lo=lo, hi=hi)
                counted, outside = b.pileup(p, origin=(key0, step))
                assert (counted, outside) == (int(taken.sum()), 76 - int(taken.sum()))
                at = (key[taken] - lo).astype(np.int64)
                q_mean, q_sd, ln = PR.q(ev["mean"]), PR.q(ev["sd"]), ev["ev_len"]
                g = _got(p)
                np.testing.assert_array_equal(g["n"][0], np.bincount(at, minlength=hi - lo).astype(np.uint32), err_msg=f"{by} {name} {norm} n")
                with np.errstate(over="ignore"):
                    for out, col in (("dwell", ln), ("dwell_sq", ln * ln), ("mean_sum", q_mean), ("mean_sq", q_mean * q_mean), ("sd_sum", q_sd)):
                        w = np.zeros(hi - lo, np.int64)
                        np.add.at(w, at, col[taken])
                        np.testing.assert_array_equal(g[out][0], w, err_msg=f"dwell {dwell} {by} {name} {norm} {out}")
                if name == "uniform":
                    assert g["sd_sum"].any() and len(set(g["mean_sum"][0][g["n"][0] > 0].tolist())) > 5
    b.free(); gen.close()
