"""include/sqg_segments.h: the segments of reads with an attached prefix (sqg_batch_segments) and chunks / targets of their inserts (the
trimmed calls), against the numpy statement of the header's rules (segments_ref.py), against the compiled reference's own vectors and
against the oracle's --ideal-amp signal of the same reads.  Every comparison is bit for bit (floats as integers)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (before the library is loaded: the HIP runtime torch brings is the one the library then uses)

import chunks_ref as R
import orc
import segments_ref as SR
import targets_ref as T
from chunk_support import ALL_SETTINGS, _assert_equal, _context, _declared, _fixture_reads
from refvec_cases import REFVEC_CASES
from squigulator_amd import api, build, model, options, profiles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEQUIN = os.path.join(ROOT, "tests", "golden", "inputs", "rnasequin_sequences_2.4.fa")
CPU_LIB = os.path.join(ROOT, "oracle", "libsqg_cpu.so")
PREFIX_VECTORS = ("r9_prefix", "rna9_prefix", "rna004_prefix", "rna004_tk4")
TKEYS = ("clean", "clean_raw", "moves", "kmer")


def _case(cid):
    """(options, k, rna, meth, prefix, (int)dwell_mean) of a committed vector's command line"""
    o = options.parse_args(dict(REFVEC_CASES)[cid])
    return o, o.kmer_size_default, bool(o.flags & profiles.SQ_RNA), bool(o.meth_freq), bool(o.flags & profiles.SQ_PREFIX), int(o.profile.dwell_mean)


@functools.lru_cache(maxsize=None)
def _amp_twin(cid):
    """the oracle (the CPU backend, as test_cpu_backend loads it) on the vector's reads with SQG_IDEAL_AMP added: the clean signal of every
    whole read, its dwells and offsets.  Computed once, shared, left unchanged."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "libsqg_cpu.so"], stdout=subprocess.DEVNULL)
    o, k, *_ = _case(cid)
    reads = _fixture_reads(cid)
    mean, stdv = model.synthetic_model(k)
    gen = api.SignalGenerator(o.profile, o.flags | profiles.SQ_IDEAL_AMP, k, mean, stdv, o.seed, num_workers=o.threads, amp_noise=o.amp_noise, lib_path=CPU_LIB)
    out = []
    for lo in range(0, len(reads), o.batch):
        b = gen.submit([r["seq"] for r in reads[lo:lo + o.batch]])
        sig, dw = b.signal(), b.dwell()
        for i in range(b.n_reads):
            s = sig[b.sig_off[i]:b.sig_off[i + 1]].copy()
            s.setflags(write=False)
            out.append(dict(sig=s, ss=dw[b.ev_off[i]:b.ev_off[i + 1]].copy(), offset=float(b.offset[i])))
        b.free()
    gen.close()
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------- no GPU
def test_header_declares_the_segment_exports_and_the_libraries_have_them():
    assert _declared("sqg_segments.h") == set(api.EXPORTS_SEGMENTS) == {"sqg_batch_segments", "sqg_chunk_plan_trimmed", "sqg_batch_chunks_trimmed",
                                                                        "sqg_batch_chunk_targets_trimmed"}
    assert _declared("sqg_targets.h") == set(api.EXPORTS_TARGETS) == {"sqg_batch_chunk_targets"}      # the other three headers: unchanged
    assert _declared("sqg_chunks.h") == set(api.EXPORTS_CHUNKS) == {"sqg_chunk_plan", "sqg_batch_chunks"}
    assert _declared("sqg.h") == set(api.EXPORTS)
    assert not set(api.EXPORTS_SEGMENTS) & (set(api.EXPORTS) | set(api.EXPORTS_CHUNKS) | set(api.EXPORTS_TARGETS))
    build.build()
    for lib in (build.LIB, build.LIB_DEV):
        L = api.load_library(lib)
        for n in api.EXPORTS_SEGMENTS:
            assert hasattr(L, n), f"{n} not exported by {lib}"
    assert os.path.join(ROOT, "include", "sqg_segments.h") in build.headers()
    for h in ("k_segments.h", "h_segments.h"):
        assert os.path.join(ROOT, "squigulator_amd", "csrc", h) in build.headers()
    assert [f[0] for f in api.CSegments._fields_] == ["seg", "shift"]


def test_the_cpu_backend_has_no_segments_and_says_so():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "libsqg_cpu.so"])
    prof, fl = profiles.get_profile("dna-r9-prom")
    mean, stdv = model.synthetic_model(6)
    gen = api.SignalGenerator(prof, fl | profiles.SQ_PREFIX, 6, mean, stdv, 42, lib_path=CPU_LIB)
    b = gen.submit([b"ACGTACGTACGTTTGACA" * 40])
    with pytest.raises(api.SqgError) as e:
        b.segments()
    assert e.value.code == -1 and "sqg_batch_segments" in str(e.value)
    b.free(); gen.close()


LEVEL = np.arange(125, dtype=np.float32)                    # level = rank; offset 0.5: code = trunc(rank - 0.5) = rank - 1
SIG11 = np.array([3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5], np.int16)                            # med2 = 8, mad4 = 4 (test_chunks)


def test_helper_on_a_hand_worked_dna_read():
    """k = 3, read ACGTCA (6 bases): chain 0 has 24 + 61 + 6 = 91 bases, 89 events: stall [0, 24), adaptor [24, 85), insert [85, 89)"""
    ss = [2] * 24 + [3] * 61 + [3, 2, 4, 2]                # stall 48 samples, adaptor 183: E[24] = 48, E[85] = 231, n = 231 + 11 = 242
    sg = SR.segments(ss, 6, 3, False, True, 9)
    np.testing.assert_array_equal(sg["seg"], [0, 48, 231, 231, 242])                     # no poly-A: seg[2] = seg[3]
    np.testing.assert_array_equal(sg["shift"], [0, 0])
    assert sg["events"] == [(0, 24), (24, 85), (85, 85), (85, 89)] and sg["win"] == (0, 0)
    # the insert alone is test_chunk_targets' hand-worked read: dwells 3 2 4 2, E = 0 3 5 9, n = 11, with ACG CGT GTC TCA = 6 27 45 52
    read = dict(sig=np.concatenate((np.full(231, 7, np.int16), SIG11)), ss=ss, seq=b"ACGTCA", offset=0.5)
    ch = SR.read_chunks_trimmed(read, 3, False, False, True, 9, 4, 2, 3, "f32")
    assert (ch["med2"], ch["mad4"]) == (8, 4)               # over the insert's 11 samples only: the 231 sevens in front do not count
    np.testing.assert_array_equal(ch["chunk_start"], [0, 2, 4, 6])                       # relative to the insert: (11 - 4) / 2 + 1 = 4 chunks
    np.testing.assert_array_equal(ch["label_len"], [2, 2, 1, 1])                         # E in [0,4): 0 3; [2,6): 3 5; [4,8): 5; [6,10): 9
    np.testing.assert_array_equal(ch["labels"], [[1, 2, 0], [2, 3, 0], [3, 0, 0], [4, 0, 0]])     # A C / C G / G / T: the read's own bases
    np.testing.assert_array_equal(ch["signal"][1], ((SIG11[2:6].astype(np.float32) - 4) * np.float32(1 / 1.4826)).astype(np.float32))
    tg = SR.read_targets_trimmed(read, LEVEL, 3, False, False, True, 9, 4, 2, "f32")
    np.testing.assert_array_equal(tg["kmer"], [[6, 6, 6, 27], [6, 27, 27, 45], [27, 45, 45, 45], [45, 45, 45, 52]])
    np.testing.assert_array_equal(tg["moves"], [[1, 0, 0, 1], [0, 1, 0, 1], [0, 1, 0, 0], [0, 0, 0, 1]])
    np.testing.assert_array_equal(tg["clean_raw"], [[5, 5, 5, 26], [5, 26, 26, 44], [26, 44, 44, 44], [44, 44, 44, 51]])
    # the whole read's level: the stall's first event is TTT = 63 -> 62, the insert sits at [231, 242)
    lvl = SR.read_level(b"ACGTCA", ss, 0.5, LEVEL, 3, False, False, True, 1.0, 1.0)
    assert len(lvl) == 242 and lvl[0] == 62 and lvl[1] == 62
    np.testing.assert_array_equal(lvl[231:], [5, 5, 5, 26, 26, 44, 44, 44, 44, 51, 51])


def test_helper_on_a_hand_worked_rna_read():
    """k = 3, read ACGT (4 bases): chain 0 has 4 + 158 + 79 = 241 bases, 239 events: insert [0, 4), poly-A [4, 162), adaptor [162, 239);
    chain 1 (the stall, 30 bases) has 28 events"""
    ss = [3, 2, 4, 2] + [1] * 158 + [2] * 77 + [3] * 28   # g1 = 11, g2 = 11 + 158 = 169, n0 = 169 + 154 = 323, n = 323 + 84 = 407
    sg = SR.segments(ss, 4, 3, True, True, 2)
    np.testing.assert_array_equal(sg["seg"], [0, 84, 238, 396, 407])                     # {0, n - n0, n - g2, n - g1, n}: stored reversed
    # (int)dwell_mean = 2: generation samples [323 - 158, 323) = [165, 323) were lowered: the adaptor's 154 and the poly-A's last 4,
    # so the window ends inside the poly-A: stored [407 - 323, 407 - 165)
    np.testing.assert_array_equal(sg["shift"], [84, 242])
    assert sg["shift"][1] > sg["seg"][2] and sg["shift"][1] < sg["seg"][3]
    assert sg["events"] == [(239, 267), (162, 239), (4, 162), (0, 4)] and sg["win"] == (11, 11)
    # the insert: stored samples [396, 407), generation order reversed; its k-mers reach into the poly-A: ACG CGT GTA TAA = 6 27 44 48
    sig = np.concatenate((np.full(396, 7, np.int16), SIG11))
    read = dict(sig=sig, ss=ss, seq=b"ACGT", offset=0.5)
    ch = SR.read_chunks_trimmed(read, 3, True, False, True, 2, 4, 2, 3, "f32")
    assert (ch["med2"], ch["mad4"]) == (8, 4)
    # chunk j covers generation samples [11 - 2j - 4, 11 - 2j): [7,11) holds E = 9; [5,9): 5; [3,7): 3 5; [1,5): 3
    np.testing.assert_array_equal(ch["label_len"], [1, 1, 2, 1])
    np.testing.assert_array_equal(ch["labels"], [[4, 0, 0], [3, 0, 0], [3, 2, 0], [2, 0, 0]])     # descending e: T / G / G C / C
    tg = SR.read_targets_trimmed(read, LEVEL, 3, True, False, True, 2, 4, 2, "f32")
    np.testing.assert_array_equal(tg["kmer"], [[48, 48, 44, 44], [44, 44, 44, 44], [44, 44, 27, 27], [27, 27, 6, 6]])
    np.testing.assert_array_equal(tg["clean_raw"], [[47, 47, 43, 43], [43, 43, 43, 43], [43, 43, 26, 26], [26, 26, 5, 5]])
    np.testing.assert_array_equal(tg["moves"], [[0, 1, 0, 0], [0, 0, 0, 1], [0, 1, 0, 1], [0, 1, 0, 0]])
    # (int)dwell_mean = 4: the window [323 - 316, 323) = [7, 323) reaches the insert's generation samples 7 .. 10 (events 2 and 3);
    # range = digitisation: the shift is 30.  Generation order 5 5 5 26 26 43 43 13 13 17 17, stored reversed
    sg = SR.segments(ss, 4, 3, True, True, 4)
    np.testing.assert_array_equal(sg["shift"], [84, 400])
    assert sg["win"] == (7, 11) and SR.shift_code(1.0, 1.0) == 30
    tg = SR.read_targets_trimmed(read, LEVEL, 3, True, False, True, 4, 4, 2, "f32", "pa", 1.0, 1.0)
    np.testing.assert_array_equal(tg["clean_raw"], [[17, 17, 13, 13], [13, 13, 43, 43], [43, 43, 26, 26], [26, 26, 5, 5]])
    np.testing.assert_array_equal(tg["clean"], tg["clean_raw"].astype(np.float32) + np.float32(0.5))         # PA: (raw + offset) * 1 / 1
    np.testing.assert_array_equal(tg["kmer"][0], [48, 48, 44, 44])                       # the shift changes the level, not the k-mer
    np.testing.assert_array_equal(SR.lower(np.array([-32760, 5], np.int16), 30), [32746, -25])     # int16 arithmetic wraps
    # the whole read: the unshifted level differs from a lowered copy exactly on shift
    lvl = SR.read_level(b"ACGT", ss, 0.5, LEVEL, 3, True, False, True, 1.0, 1.0)
    assert len(lvl) == 407
    np.testing.assert_array_equal(lvl[396:], [47, 47, 43, 43, 43, 43, 26, 26, 5, 5, 5])
    assert lvl[0] == 20 and lvl[83] == 0                    # the stall, reversed: its last event is CCC = 21, its first AAA = 0 -> trunc(-0.5) = 0


def test_helper_on_reads_without_prefix_and_shorter_than_a_kmer():
    ss = [3, 2, 4, 2]
    sg = SR.segments(ss, 6, 3, False, False, 9)             # no prefix: the whole read is insert
    np.testing.assert_array_equal(sg["seg"], [0, 0, 0, 0, 11])
    np.testing.assert_array_equal(sg["shift"], [0, 0])
    read = dict(sig=SIG11, ss=ss, seq=b"ACGTCA", offset=0.5)
    a, b = SR.read_chunks_trimmed(read, 3, False, False, False, 9, 4, 2, 3), R.read_chunks(SIG11, ss, b"ACGTCA", 3, False, False, 4, 2, 3)
    for key in a:
        np.testing.assert_array_equal(a[key], b[key])
    np.testing.assert_array_equal(SR.segments([3, 2, 4, 1, 1], 2, 3, False, False, 9)["seg"], [0, 0, 0, 0, 11])   # the five stand-in events
    assert SR.read_chunks_trimmed(dict(sig=SIG11, ss=[3, 2, 4, 1, 1], seq=b"AC"), 3, False, False, False, 9, 4, 2, 3)["signal"].shape == (0, 4)
    # DNA with prefix, a read of one base, k = 3: chain 0 has 86 bases, 84 events: the adaptor loses one, [24, 84); the insert has none
    ss = [2] * 24 + [3] * 60                                # E[24] = 48, E[84] = 228 = n
    sg = SR.segments(ss, 1, 3, False, True, 9)
    np.testing.assert_array_equal(sg["seg"], [0, 48, 228, 228, 228])
    assert sg["events"] == [(0, 24), (24, 84), (84, 84), (84, 84)]
    read = dict(sig=np.full(228, 7, np.int16), ss=ss, seq=b"A", offset=0.0)
    ch = SR.read_chunks_trimmed(read, 3, False, False, True, 9, 4, 2, 3)
    assert ch["signal"].shape == (0, 4) and (ch["med2"], ch["mad4"]) == (0, 0)
    assert SR.read_targets_trimmed(read, LEVEL, 3, False, False, True, 9, 4, 2)["moves"].shape == (0, 4)
    # RNA with prefix, a read of one base, k = 3: chain 0 has 238 bases, 236 events: insert [0, 1), poly-A [1, 159), adaptor [159, 236)
    ss = [5] + [1] * 158 + [2] * 77 + [3] * 28             # g1 = 5, g2 = 163, n0 = 317, n = 401
    sg = SR.segments(ss, 1, 3, True, True, 2)
    np.testing.assert_array_equal(sg["seg"], [0, 84, 238, 396, 401])
    np.testing.assert_array_equal(sg["shift"], [84, 401 - (317 - 158)])
    assert sg["events"] == [(236, 264), (159, 236), (1, 159), (0, 1)]
    read = dict(sig=np.concatenate((np.full(396, 7, np.int16), SIG11[:5])), ss=ss, seq=b"C", offset=0.5)
    tg = SR.read_targets_trimmed(read, LEVEL, 3, True, False, True, 2, 4, 1, "f32")      # 2 chunks of the 5 samples of CAA = 16
    np.testing.assert_array_equal(tg["kmer"], [[16] * 4] * 2)
    np.testing.assert_array_equal(tg["moves"], [[0, 0, 0, 0], [0, 0, 0, 1]])             # the event's first generation sample is its last stored one


@pytest.mark.parametrize("cid", PREFIX_VECTORS)
def test_segments_of_the_reference_vectors_and_the_oracle_ideal_amp_signal(cid):
    """the compiled reference's own sig / ss: the bounds add up, every read has insert chunks; and the oracle's --ideal-amp run of the same
    reads pins the insert's clean_raw and the shift range with no GPU"""
    o, k, rna, meth, prefix, sps = _case(cid)
    assert prefix and not meth
    reads, twin = _fixture_reads(cid), _amp_twin(cid)
    mean, _ = model.synthetic_model(k)
    assert len(reads) == len(twin) > 0
    for i, (r, t) in enumerate(zip(reads, twin)):
        assert 369 <= len(r["seq"]) <= 2794 and 4830 <= len(r["sig"]) <= 90372
        sg = SR.segments(r["ss"], len(r["seq"]), k, rna, prefix, sps)
        seg = sg["seg"]
        assert seg[0] == 0 and seg[4] == len(r["sig"]) and (np.diff(seg) >= 0).all()
        assert sum(hi - lo for lo, hi in sg["events"]) == len(r["ss"])
        for q, (lo, hi) in enumerate(sg["events"]):        # every segment's samples are its events' dwells
            assert int(np.sum(r["ss"][lo:hi])) == seg[q + 1] - seg[q], f"{cid} read {i} segment {q}"
        assert (seg[2] == seg[3]) == (not rna) and seg[1] > 0 and seg[3] > seg[1]
        ch = SR.read_chunks_trimmed(r, k, rna, meth, prefix, sps, 512, 256, 128, "f16", "medmad", o.profile.range, o.profile.digitisation)
        assert len(ch["label_len"]) == (seg[4] - seg[3] - 512) // 256 + 1 > 0, f"{cid} read {i}: no insert chunk"
        # the oracle's clean signal of the whole read
        np.testing.assert_array_equal(t["ss"], r["ss"])
        assert t["offset"] == r["offset"] and len(t["sig"]) == len(r["sig"])
        tg = SR.read_targets_trimmed(r, mean, k, rna, meth, prefix, sps, 512, 256, "f16", "medmad", o.profile.range, o.profile.digitisation)
        s3 = int(seg[3])
        for j, row in enumerate(tg["clean_raw"]):
            np.testing.assert_array_equal(row, t["sig"][s3 + 256 * j:s3 + 256 * j + 512], err_msg=f"{cid} read {i} chunk {j}")
        lvl = SR.read_level(r["seq"], r["ss"], r["offset"], mean, k, rna, meth, prefix, o.profile.range, o.profile.digitisation)
        differs = np.flatnonzero(lvl != t["sig"])
        w0, w1 = (int(x) for x in sg["shift"])
        np.testing.assert_array_equal(differs, np.arange(w0, w1), err_msg=f"{cid} read {i}: the shift range")
        if rna:
            assert w0 == seg[1] < w1 < seg[3] and sg["win"][0] == sg["win"][1]      # from the adaptor's far end to about the poly-A's; not the insert
            assert abs(int(w1 - seg[2])) < (seg[3] - seg[2]) // 2                       # (it follows no event boundary: short of the poly-A or a little inside)
            np.testing.assert_array_equal(SR.lower(lvl[w0:w1], SR.shift_code(o.profile.range, o.profile.digitisation)), t["sig"][w0:w1])
        else:
            assert (w0, w1) == (0, 0)


# ---------------------------------------------------------------------------------------------------------- GPU
def _cpu(t, key=None):
    a = t.cpu().numpy()
    return a.view(np.uint32) if key == "kmer" else a


def _compare_targets(tg, want, what):
    assert tg.n_chunks == want["chunk_off"][-1], f"{what}: {tg.n_chunks} chunks, expected {want['chunk_off'][-1]}"
    np.testing.assert_array_equal(tg.chunk_off, want["chunk_off"], err_msg=f"{what}: chunk_off")
    for key in TKEYS:
        got = _cpu(getattr(tg, key), key)
        assert got.shape == want[key].shape and got.dtype == want[key].dtype, f"{what}: {key} {got.shape} {got.dtype} vs {want[key].shape} {want[key].dtype}"
        np.testing.assert_array_equal(R.bits(got), R.bits(want[key]), err_msg=f"{what}: {key}")


def _check(b, reads, mean, k, rna, meth, prefix, prof, L, S, W, settings, what, sps=None):
    """segments, trimmed chunks and trimmed targets of a batch against segments_ref over `reads`; -> (seg, chunks, targets) of the last setting"""
    sps = int(prof.dwell_mean) if sps is None else sps
    seg, shift = b.segments()
    wseg, wshift = SR.batch_segments(reads, k, rna, prefix, sps)
    assert seg.dtype == torch.int64 and shift.dtype == torch.int64 and seg.is_cuda and shift.is_cuda
    assert tuple(seg.shape) == (len(reads), 5) and tuple(shift.shape) == (len(reads), 2)
    np.testing.assert_array_equal(_cpu(seg), wseg, err_msg=f"{what}: seg")
    np.testing.assert_array_equal(_cpu(shift), wshift, err_msg=f"{what}: shift")
    ch = tg = None
    for dtype, norm in settings:
        want = SR.batch_chunks_trimmed(reads, k, rna, meth, prefix, sps, L, S, W, dtype, norm, prof.range, prof.digitisation)
        ch = b.chunks(L, S, W, dtype=dtype, norm=norm, trim=True)
        _assert_equal(ch, want, f"{what} L {L} S {S} {dtype} {norm}: chunks")
        off, nc = b.chunk_plan(L, S, trim=True)
        assert nc == ch.n_chunks
        np.testing.assert_array_equal(off, want["chunk_off"])
        want = SR.batch_targets_trimmed(reads, mean, k, rna, meth, prefix, sps, L, S, dtype, norm, prof.range, prof.digitisation)
        tg = b.chunk_targets(L, S, dtype=dtype, norm=norm, clean=True, clean_raw=True, moves=True, kmer=True, trim=True)
        _compare_targets(tg, want, f"{what} L {L} S {S} {dtype} {norm}: targets")
    if ch is not None and ch.n_chunks:
        np.testing.assert_array_equal(_cpu(tg.moves).astype(np.int64).sum(1), _cpu(ch.label_len), err_msg=f"{what}: moves vs label_len")
    return wseg, ch, tg


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [api.MODE_EXACT, api.MODE_CERTIFIED], ids=["exact", "certified"])
@pytest.mark.parametrize("cid", PREFIX_VECTORS)
def test_trimmed_chunks_of_the_prefix_vectors(cid, mode):
    """the fixture's reads through the HIP path (rna004_tk4: four workers): segments, chunks in all four settings, all four targets, against
    segments_ref over the FIXTURE's seq / ss / sig; clean_raw against the oracle's --ideal-amp signal, f32 pa signal against the fixture's sig"""
    o, k, rna, meth, prefix, sps = _case(cid)
    reads, twin = _fixture_reads(cid), _amp_twin(cid)
    _, _, gen = _context(dict(REFVEC_CASES)[cid], mode)
    mean, _ = model.synthetic_model(k)
    L, S, W = 512, 256, 128
    for lo in range(0, len(reads), o.batch):
        part = reads[lo:lo + o.batch]
        b = gen.stage([r["seq"] for r in part]).run().wait()
        seg, ch, tg = _check(b, part, mean, k, rna, meth, prefix, o.profile, L, S, W, ALL_SETTINGS, f"{cid} reads {lo}..")
        assert (np.diff(ch.chunk_off) > 0).all()
        raw, sig, start = _cpu(tg.clean_raw), _cpu(ch.signal), _cpu(ch.chunk_start)      # (the last setting: f32 pa)
        for i, r in enumerate(part):
            s3 = int(seg[i][3])
            for c in range(int(ch.chunk_off[i]), int(ch.chunk_off[i + 1])):
                at = s3 + int(start[c])
                np.testing.assert_array_equal(raw[c], twin[lo + i]["sig"][at:at + L], err_msg=f"{cid} read {lo + i} chunk {c}: clean_raw vs the oracle")
                pa = ((r["sig"][at:at + L].astype(np.float64) + r["offset"]) * o.profile.range / o.profile.digitisation).astype(np.float32)
                np.testing.assert_array_equal(R.bits(sig[c]), R.bits(pa), err_msg=f"{cid} read {lo + i} chunk {c}: signal vs the fixture's sig")
        with pytest.raises(api.SqgError) as e:              # the plain calls keep refusing the context
            b.chunks(L, S, W)
        assert e.value.code == -1 and "SQG_PREFIX" in str(e.value)
        b.free()
    gen.close()


PLANTED = {  # name -> (profile, extra flags, workers)
    "dna_k6": ("dna-r9-prom", 0, 1), "dna_k9": ("dna-r10-prom", 0, 3), "rna_k5": ("rna-r9-prom", 0, 1), "rna_k9": ("rna004-prom", 0, 2),
    "dna_k6_meth": ("dna-r9-prom", profiles.SQ_METH, 1),
    "dna_k6_ideal_time": ("dna-r9-prom", profiles.SQ_IDEAL_TIME, 1), "rna_k9_ideal_time": ("rna004-prom", profiles.SQ_IDEAL_TIME, 1),
    "dna_k9_ideal": ("dna-r10-prom", profiles.SQ_IDEAL, 1), "rna_k5_ideal": ("rna-r9-prom", profiles.SQ_IDEAL, 1),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PLANTED))
def test_planted_reads_with_prefix(name):
    """k = 5, 6, 9, DNA and RNA, --prefix=yes: reads shorter than a k-mer and of one base next to normal ones, inserts shorter than a chunk,
    of exactly L and of L + S - 1 samples (constant dwell: the lengths are arithmetic), one event more than the 1024-event scan tile, insert
    spans at odd and at 8-sample-aligned addresses, contexts without a dwell stream, the methylation table; expected values over the ORACLE's reads"""
    pname, extra, workers = PLANTED[name]
    prof, fl = profiles.get_profile(pname)
    fl |= extra | profiles.SQ_PREFIX
    k = profiles.default_kmer_size(fl)
    rna, meth, const = bool(fl & profiles.SQ_RNA), bool(fl & profiles.SQ_METH), bool(fl & (profiles.SQ_IDEAL | profiles.SQ_IDEAL_TIME))
    mean, stdv = model.synthetic_model(k, meth=meth)
    sps = int(prof.dwell_mean)
    ev = lambda n_ev: n_ev if rna else n_ev + k - 1         # noqa: E731  bases of a read whose insert has n_ev events
    if const:                                               # L = 64 sps samples are 64 events; S = sps + 1: L + S - 1 samples are 65 events
        L, S, W = 64 * sps, sps + 1, 80
        lens = [ev(64), ev(65), ev(63), ev(66), k - 1, 1, ev(1025), 300]
    else:
        L, S, W = 256, 128, 96
        lens = [300, k - 1, 1, ev(5), 411, ev(1025), 200, 733] + [150 + 37 * i for i in range(12)]
    rng = np.random.default_rng(len(name) + 7 * k)
    letters = list(b"ACGT" + (b"M" if meth else b""))
    seqs = [bytes(rng.choice(letters, int(m)).astype(np.uint8)) for m in lens]
    orac = orc.Oracle(prof, fl, k, mean, stdv, 42, num_workers=workers)
    reads = [dict(sig=w.sig, ss=w.ss, seq=s, offset=w.offset) for w, s in zip(orac.run_batch_seqs(seqs), seqs)]
    orac.close()
    gen = api.SignalGenerator(prof, fl, k, mean, stdv, 42, num_workers=workers, mode=api.MODE_CERTIFIED)
    b = gen.submit(seqs)
    np.testing.assert_array_equal(b.signal(), np.concatenate([r["sig"] for r in reads]))
    np.testing.assert_array_equal(b.dwell(), np.concatenate([r["ss"] for r in reads]))
    settings = [("f16", "medmad"), ("f32", "pa")]
    seg, ch, tg = _check(b, reads, mean, k, rna, meth, True, prof, L, S, W, settings, name)
    n_ins = seg[:, 4] - seg[:, 3]
    nc = np.diff(ch.chunk_off)
    if const:
        assert list(n_ins[:4]) == [L, L + S - 1, L - sps, L + S - 1 + sps] and list(nc[:4]) == [1, 1, 0, 2]
        assert n_ins[6] == 1025 * sps
    else:
        lo = b.sig_off[:-1] + seg[:, 3]                     # where the insert spans start in the slab: the emit kernel's two load paths
        assert (lo[nc > 0] % 2 == 1).any() and (lo[nc > 0] % 8 == 0).any(), lo % 8
        assert len(reads[5]["ss"]) - (85 if not rna else 237 - k + 1 + 30 - k + 1) == 1025
    assert nc[lens.index(k - 1)] == 0 and nc[lens.index(1)] == 0 and (nc > 0).sum() >= 4
    if not rna:
        assert n_ins[lens.index(k - 1)] == 0 and n_ins[lens.index(1)] == 0                # DNA: a read shorter than a k-mer has no insert event
    else:
        assert n_ins[lens.index(1)] > 0                     # RNA: a base is an event
    # other geometries on the same batch: one long chunk per read at most, a stride that leaves gaps, eight-sample steps
    for L2, S2 in ((2048, 2048), (64, 200), (72, 8)):
        _check(b, reads, mean, k, rna, meth, True, prof, L2, S2, 40, [("f32", "medmad")], f"{name} L {L2}")
    b.free()
    b = gen.submit([])                                      # an empty batch
    seg, shift = b.segments()
    assert tuple(seg.shape) == (0, 5) and tuple(shift.shape) == (0, 2)
    assert b.chunks(64, 64, 8, trim=True).n_chunks == 0 and b.chunk_targets(64, trim=True).n_chunks == 0
    b.free(); gen.close()


@pytest.mark.gpu
@pytest.mark.parametrize("force", ["1", "2"])
def test_generic_statistics_paths_reach_the_trimmed_span(force, monkeypatch):
    """the development build's SQG_TEST_CHUNK_GENERIC: the inserts through the global-histogram path (1) / the several-workgroup path (2)"""
    monkeypatch.setenv("SQG_TEST_CHUNK_GENERIC", force)
    for cid in ("r9_prefix", "rna004_prefix"):
        o, k, rna, meth, prefix, sps = _case(cid)
        reads = _fixture_reads(cid)
        _, _, gen = _context(dict(REFVEC_CASES)[cid], api.MODE_CERTIFIED)
        assert api.build_info(gen.L)["dev"] == "1"
        mean, _ = model.synthetic_model(k)
        b = gen.stage([r["seq"] for r in reads]).run().wait()
        _check(b, reads, mean, k, rna, meth, prefix, o.profile, 512, 256, 128, [("f16", "medmad"), ("f32", "medmad")], f"{cid} forced {force}")
        b.free(); gen.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cid,sps", [("rna004_prefix", 300), ("rna9_prefix", 600)])
def test_level_shift_window_reaching_into_the_inserts(cid, sps, monkeypatch):
    """the development build's SQG_TEST_SEG_SPS: the window taken as 79 sps samples long, so that it ends inside two inserts and covers
    the third whole (clamped at the read's first generation sample): shift[] and k_target_shift's clean_raw / clean in all four
    settings against segments_ref's shift rule with the same sps -- the rule test_helper_on_a_hand_worked_rna_read works by hand"""
    monkeypatch.setenv("SQG_TEST_SEG_SPS", str(sps))
    o, k, rna, meth, prefix, _ = _case(cid)
    reads = _fixture_reads(cid)
    _, _, gen = _context(dict(REFVEC_CASES)[cid], api.MODE_CERTIFIED)
    assert api.build_info(gen.L)["dev"] == "1"
    mean, _ = model.synthetic_model(k)
    win = [SR.segments(r["ss"], len(r["seq"]), k, rna, prefix, sps)["win"] for r in reads]
    assert sum(0 < lo < hi for lo, hi in win) == 2 and sum(lo == 0 < hi for lo, hi in win) == 1
    b = gen.stage([r["seq"] for r in reads]).run().wait()
    np.testing.assert_array_equal(b.signal(), np.concatenate([r["sig"] for r in reads]))          # the generator's own window is untouched
    seg, ch, tg = _check(b, reads, mean, k, rna, meth, prefix, o.profile, 512, 256, 128, ALL_SETTINGS, f"{cid} sps {sps}", sps=sps)
    plain = SR.batch_targets_trimmed(reads, mean, k, rna, meth, prefix, int(o.profile.dwell_mean), 512, 256, "f32", "pa", o.profile.range, o.profile.digitisation)
    lowered = plain["clean_raw"] != _cpu(tg.clean_raw)
    assert lowered.any() and not lowered.all()              # some samples were lowered, some were not
    for L2, S2 in ((64, 8), (72, 200), (4096, 4099)):      # rows that start anywhere in the window; more than one 64-sample step per chunk
        _, ch2, tg2 = _check(b, reads, mean, k, rna, meth, prefix, o.profile, L2, S2, 16, [("f16", "medmad")], f"{cid} sps {sps} L {L2}", sps=sps)
        if (L2, S2) == (64, 8):                             # k_target_shift's grid is min(n_chunks, 4096) workgroups: chunks behind it are met on a second trip
            plain = SR.batch_targets_trimmed(reads, mean, k, rna, meth, prefix, int(o.profile.dwell_mean), L2, S2, "f16", "medmad", o.profile.range, o.profile.digitisation)
            lowered = (plain["clean_raw"] != _cpu(tg2.clean_raw)).any(axis=1)
            assert ch2.n_chunks > 4096 and lowered[4096:].any() and lowered[:4096].any()
    b.free(); gen.close()


@pytest.mark.gpu
def test_without_prefix_trim_changes_nothing():
    cid = "r10_tk8"
    o, k, rna, meth, prefix, sps = _case(cid)
    assert not prefix
    reads = _fixture_reads(cid)[:8]
    _, _, gen = _context(dict(REFVEC_CASES)[cid], api.MODE_CERTIFIED)
    b = gen.stage([r["seq"] for r in reads]).run().wait()
    seg, shift = b.segments()
    n = np.diff(b.sig_off)
    np.testing.assert_array_equal(_cpu(seg), np.stack([np.zeros_like(n)] * 4 + [n], 1))
    assert not _cpu(shift).any()
    for (dtype, norm), (L, S) in zip(ALL_SETTINGS, ((2048, 1024), (512, 256), (64, 8), (4096, 4099))):
        np.testing.assert_array_equal(b.chunk_plan(L, S)[0], b.chunk_plan(L, S, trim=True)[0])
        plain, trim = b.chunks(L, S, 200, dtype=dtype, norm=norm), b.chunks(L, S, 200, dtype=dtype, norm=norm, trim=True)
        assert plain.n_chunks == trim.n_chunks > 0
        for key in ("signal", "labels", "label_len", "chunk_read", "chunk_start", "med2", "mad4"):
            assert torch.equal(getattr(plain, key), getattr(trim, key)), f"{dtype} {norm} L {L}: {key}"
        kw = dict(dtype=dtype, norm=norm, clean=True, clean_raw=True, moves=True, kmer=True)
        plain, trim = b.chunk_targets(L, S, **kw), b.chunk_targets(L, S, trim=True, **kw)
        for key in TKEYS:
            assert torch.equal(getattr(plain, key), getattr(trim, key)), f"{dtype} {norm} L {L}: {key}"
    b.free(); gen.close()


def _fasta(path):
    out = []
    for line in open(path):
        if line.startswith(">"):
            out.append([])
        elif line.strip():
            out[-1].append(line.strip())
    return [("".join(x)).encode() for x in out]


@pytest.mark.gpu
def test_sampled_batches_of_the_sequin_transcripts():
    """gen_read on the device (SAMPLE_RNA), rna004 with prefix: segments and the trimmed chunks' integers and targets from the batch's own
    reads(), dwell() and signal()"""
    prof, fl = profiles.get_profile("rna004-prom")
    fl |= profiles.SQ_PREFIX
    k = profiles.default_kmer_size(fl)
    mean, stdv = model.synthetic_model(k)
    gen = api.SignalGenerator(prof, fl, k, mean, stdv, 42, num_workers=4, mode=api.MODE_CERTIFIED)
    gen.load_genome(_fasta(SEQUIN), 10000, api.SAMPLE_RNA)
    b = gen.sample(16).run().wait()
    sig, dw, seqs = b.signal(), b.dwell(), b.reads()
    reads = [dict(sig=sig[b.sig_off[i]:b.sig_off[i + 1]], ss=dw[b.ev_off[i]:b.ev_off[i + 1]], seq=seqs[i], offset=b.offset[i]) for i in range(b.n_reads)]
    assert len(reads) == 16 and len({len(s) for s in seqs}) > 4
    seg, ch, tg = _check(b, reads, mean, k, True, False, True, prof, 1024, 512, 256, [("f16", "medmad")], "sampled")
    assert ch.n_chunks > 100 and (seg[:, 1] > 0).all() and (seg[:, 3] > seg[:, 2]).all()
    b.free(); gen.close()


@pytest.mark.gpu
def test_lifetime_and_errors():
    cid = "rna004_tk4"
    o, k, rna, meth, prefix, sps = _case(cid)
    reads = _fixture_reads(cid)
    _, _, gen = _context(dict(REFVEC_CASES)[cid], api.MODE_EXACT)
    mean, _ = model.synthetic_model(k)
    parts = [reads[0:4], reads[4:8], reads[0:4]]
    L, S, W = 512, 256, 128
    b0 = gen.stage([r["seq"] for r in parts[0]])
    for call in (b0.segments, lambda: b0.chunk_plan(L, S, trim=True), lambda: b0.chunks(L, S, W, trim=True), lambda: b0.chunk_targets(L, S, trim=True)):
        with pytest.raises(api.SqgError) as e:              # staged, not run: an error, not a hang
            call()
        assert e.value.code == -4
    b0.run().wait()
    sig0, dw0 = b0.signal().copy(), b0.dwell().copy()
    _check(b0, parts[0], mean, k, rna, meth, prefix, o.profile, L, S, W, [("f16", "medmad")], "batch 0")
    first = (b0.segments(), b0.chunks(L, S, W, trim=True), b0.chunk_targets(L, S, clean_raw=True, kmer=True, trim=True))
    with pytest.raises(api.SqgError) as e:                  # the plain call on the prefix context: as before
        b0.chunks(L, S, W)
    assert e.value.code == -1 and "SQG_PREFIX" in str(e.value)
    with pytest.raises(api.SqgError) as e:
        b0.chunk_targets(L, S)
    assert e.value.code == -1 and "SQG_PREFIX" in str(e.value)
    for bad in (dict(chunk_len=63), dict(chunk_len=64, stride=0), dict(chunk_len=64, dtype=7), dict(chunk_len=(1 << 20) + 8)):
        with pytest.raises(api.SqgError) as e:
            b0.chunks(trim=True, **bad)
        assert e.value.code == -1 and "_trimmed" in str(e.value), bad
    # NULL arguments
    Lb, cfg, nc = gen.L, api.CChunkCfg(L, S, W, 0, 0), C.c_int64()
    dummy = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    assert Lb.sqg_batch_segments(None, None, None) == -1
    assert Lb.sqg_batch_segments(gen.ctx, None, C.byref(api.CSegments(None, None))) == -1
    assert Lb.sqg_batch_segments(gen.ctx, b0.handle, None) == -1 and b"sqg_batch_segments" in Lb.sqg_last_error(gen.ctx)
    assert Lb.sqg_batch_segments(gen.ctx, b0.handle, C.byref(api.CSegments(None, None))) == 0         # nothing wanted: nothing done
    assert Lb.sqg_chunk_plan_trimmed(None, None, None, None, None) == -1
    assert Lb.sqg_chunk_plan_trimmed(gen.ctx, b0.handle, None, None, C.byref(nc)) == -1
    assert Lb.sqg_chunk_plan_trimmed(gen.ctx, b0.handle, C.byref(cfg), None, None) == -1 and b"sqg_chunk_plan_trimmed" in Lb.sqg_last_error(gen.ctx)
    assert Lb.sqg_chunk_plan_trimmed(gen.ctx, b0.handle, C.byref(cfg), None, C.byref(nc)) == 0 and nc.value == first[1].n_chunks
    assert Lb.sqg_batch_chunks_trimmed(None, None, None, None) == -1 and Lb.sqg_batch_chunk_targets_trimmed(None, None, None, None) == -1
    assert Lb.sqg_batch_chunks_trimmed(gen.ctx, b0.handle, C.byref(cfg), None) == -1 and b"sqg_batch_chunks_trimmed" in Lb.sqg_last_error(gen.ctx)
    assert Lb.sqg_batch_chunk_targets_trimmed(gen.ctx, b0.handle, C.byref(cfg), None) == -1 and b"sqg_batch_chunk_targets_trimmed" in Lb.sqg_last_error(gen.ctx)
    assert Lb.sqg_batch_chunks_trimmed(gen.ctx, None, C.byref(cfg), C.byref(api.CChunkOut())) == -1
    out = api.CChunkTargets(None, None, dummy.data_ptr() + 4, None, None, None)
    assert Lb.sqg_batch_chunk_targets_trimmed(gen.ctx, b0.handle, C.byref(cfg), C.byref(out)) == -1
    # segments alone, either output NULL
    seg = torch.zeros((4, 5), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert Lb.sqg_batch_segments(gen.ctx, b0.handle, C.byref(api.CSegments(seg.data_ptr(), None))) == 0
    assert torch.equal(seg, first[0][0])
    shift = torch.zeros((4, 2), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert Lb.sqg_batch_segments(gen.ctx, b0.handle, C.byref(api.CSegments(None, shift.data_ptr()))) == 0
    assert torch.equal(shift, first[0][1])

    def same_as_first():
        again = (b0.segments(), b0.chunks(L, S, W, trim=True), b0.chunk_targets(L, S, clean_raw=True, kmer=True, trim=True))
        assert torch.equal(again[0][0], first[0][0]) and torch.equal(again[0][1], first[0][1])
        for key in ("signal", "labels", "label_len", "chunk_read", "chunk_start", "med2", "mad4"):
            assert torch.equal(getattr(again[1], key), getattr(first[1], key)), key
        for key in TKEYS:
            assert torch.equal(getattr(again[2], key), getattr(first[2], key)), key
    same_as_first()
    np.testing.assert_array_equal(b0.signal(), sig0)        # the calls leave the batch alone
    np.testing.assert_array_equal(b0.dwell(), dw0)
    b1 = gen.stage([r["seq"] for r in parts[1]]).run().wait()
    same_as_first()                                         # after one more batch has run: the same
    b2 = gen.stage([r["seq"] for r in parts[2]]).run().wait()
    for call in (b0.segments, lambda: b0.chunk_plan(L, S, trim=True), lambda: b0.chunks(L, S, W, trim=True), lambda: b0.chunk_targets(L, S, trim=True)):
        with pytest.raises(api.SqgError) as e:              # two more batches: slabs and dwells are batch 2's
            call()
        assert e.value.code == -4 and "sqg_" in str(e.value)
    _check(b1, parts[1], mean, k, rna, meth, prefix, o.profile, L, S, W, [("f16", "medmad")], "batch 1 after batch 2")
    for b in (b0, b1, b2):
        b.free()
    gen.close()
