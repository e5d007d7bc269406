"""sqg_batch_chunks (include/sqg_chunks.h): labelled, normalised signal chunks made on the device, against the numpy statement of the
rules (chunks_ref.py) -- applied to the compiled reference's committed vectors, to the oracle's signal, or to the batch's own fetched
results.  Every comparison is bit for bit (floats as integers)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch  # noqa: F401  (before the library is loaded: the HIP runtime torch brings is the one the library then uses)

import chunks_ref as R
import orc
from chunk_support import ALL_SETTINGS, CASES, _assert_equal, _context, _cpu, _declared, _fixture_reads
from refvec_cases import REFVEC_CASES
from squigulator_amd import api, build, model, profiles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------- no GPU
def test_header_declares_the_chunk_exports_and_the_library_has_them():
    assert _declared("sqg_chunks.h") == set(api.EXPORTS_CHUNKS) == {"sqg_chunk_plan", "sqg_batch_chunks"}
    assert _declared("sqg.h") == set(api.EXPORTS)                      # the surface every backend implements is unchanged
    assert not set(api.EXPORTS) & set(api.EXPORTS_CHUNKS)
    build.build()
    for lib in (build.LIB, build.LIB_DEV):
        L = api.load_library(lib)
        for n in api.EXPORTS_CHUNKS:
            assert hasattr(L, n), f"{n} not exported by {lib}"
    assert (api.CHUNK_F16, api.CHUNK_F32, api.CHUNK_MEDMAD, api.CHUNK_PA) == (0, 1, 0, 1)
    assert "SQG_TEST_CHUNK_GENERIC" in api.DEV_KNOBS
    assert os.path.join(ROOT, "include", "sqg_chunks.h") in build.headers()


def test_the_cpu_backend_has_no_chunks_and_says_so():
    import subprocess
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "libsqg_cpu.so"])
    prof, fl = profiles.get_profile("dna-r9-prom")
    mean, stdv = model.synthetic_model(6)
    gen = api.SignalGenerator(prof, fl, 6, mean, stdv, 42, lib_path=os.path.join(ROOT, "oracle", "libsqg_cpu.so"))
    b = gen.submit([b"ACGTACGTACGTTTGACA" * 40])
    with pytest.raises(api.SqgError) as e:
        b.chunk_plan(64, 64)
    assert e.value.code == -1
    with pytest.raises(api.SqgError) as e:
        b.chunks(64)
    assert e.value.code == -1
    b.free(); gen.close()


INV1 = np.float32(1.0 / 1.4826)


def test_reference_helper_on_hand_worked_reads():
    """the yardstick itself, pinned: every number below was worked out by hand from include/sqg_chunks.h"""
    raw = np.array([3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5], np.int16)       # n = 11 (odd): sorted 1 1 2 3 3 [4] 5 5 5 6 9 -> med2 = 8
    assert R.stats(raw) == (8, 4)                                      # |2 raw - 8| sorted 0 2 2 2 2 [2] 4 4 6 6 10 -> mad4 = 4
    assert R.stats(np.array([1, 2, 3, 4], np.int16)) == (5, 4)         # even n: med2 = 2 + 3; |2 raw - 5| = 3 1 1 3 -> 1 + 3
    assert R.stats(np.array([7, 7, 7, 7, 2, 7], np.int16)) == (14, 0)  # mad4 = 0
    assert R.stats(np.zeros(0, np.int16)) == (0, 0)
    # k = 3, 6 bases -> 4 events of 3 2 4 2 samples: E = 0 3 5 9
    seq, ss = b"AMGTCA", [3, 2, 4, 2]
    d = R.read_chunks(raw, ss, seq, 3, False, True, L=4, S=2, W=2, dtype="f32")
    assert (d["med2"], d["mad4"]) == (8, 4) and d["signal"].shape == (4, 4)           # (11 - 4) // 2 + 1 chunks; mad' = 1
    np.testing.assert_array_equal(R.bits(d["signal"][1]), R.bits((np.array([0, -3, 1, 5], np.float32) * INV1).astype(np.float32)))
    np.testing.assert_array_equal(d["chunk_start"], [0, 2, 4, 6])
    # [0,4): E 0 3 -> A M; [2,6): E 3 5 -> M G; [4,8): E 5 -> G; [6,10): E 9 -> T
    np.testing.assert_array_equal(d["labels"], [[1, 5], [5, 3], [3, 0], [4, 0]])
    np.testing.assert_array_equal(d["label_len"], [2, 2, 1, 1])
    d = R.read_chunks(raw, ss, seq, 3, False, False, L=4, S=2, W=1)                   # no methylation table: M is rank 0; W = 1 truncates
    np.testing.assert_array_equal(d["labels"], [[1], [1], [3], [4]])
    np.testing.assert_array_equal(d["label_len"], [2, 2, 1, 1])
    assert d["signal"].dtype == np.float16
    # RNA: chunk j covers generation-order samples [11 - 2j - 4, 11 - 2j): [7,11) T; [5,9) G; [3,7) E 3 5 -> G then M; [1,5) M
    d = R.read_chunks(raw, ss, seq, 3, True, True, L=4, S=2, W=3)
    np.testing.assert_array_equal(d["labels"], [[4, 0, 0], [3, 0, 0], [3, 5, 0], [5, 0, 0]])
    np.testing.assert_array_equal(d["label_len"], [1, 1, 2, 1])
    # mad4 = 0 -> mad' = 1; gaps (S > L); a read shorter than k has statistics and no chunks
    d = R.read_chunks(np.array([7, 7, 7, 7, 2, 7], np.int16), [6], b"ACG", 3, False, False, L=2, S=3, W=1, dtype="f32")
    np.testing.assert_array_equal(R.bits(d["signal"]), R.bits(np.array([[0, 0], [0, np.float32(-5) * INV1]], np.float32)))
    np.testing.assert_array_equal(d["labels"], [[1], [0]])
    d = R.read_chunks(raw, [3, 2, 4, 1, 1], b"AC", 3, False, False, L=4, S=2, W=1)
    assert (d["med2"], d["mad4"], len(d["label_len"])) == (8, 4, 0)
    # picoamperes: (raw + offset) * range / digitisation
    d = R.read_chunks(np.array([10, -2], np.int16), [2], b"ACG", 3, False, False, L=2, S=2, W=0, dtype="f32", norm="pa", offset=6.0, rng=3.0, dig=8.0)
    np.testing.assert_array_equal(d["signal"], [[6.0, 1.5]])


def _plan(sig_off, L, S, short=()):
    off = [0]
    for i in range(len(sig_off) - 1):
        n = sig_off[i + 1] - sig_off[i]
        off.append(off[-1] + (0 if (n < L or i in short) else (n - L) // S + 1))
    return off


def test_plan_arithmetic():
    """sqg_chunk_plan needs a batch that has been run; its arithmetic here, the call itself on the GPU (test_strides_and_plan)"""
    assert _plan([0, 63, 127, 191, 319], 64, 64) == [0, 0, 1, 2, 4]
    assert _plan([0, 64, 64, 1000], 64, 8) == [0, 1, 1, 1 + (936 - 64) // 8 + 1]
    assert _plan([0, 4096, 8192], 2048, 3072) == [0, 1, 2]
    assert _plan([0, 500, 1000], 64, 64, short={0}) == [0, 0, 7]
    assert [R.n_chunks_of(n, 64, 96) for n in (63, 64, 159, 160)] == [0, 1, 1, 2]


# ---------------------------------------------------------------------------------------------------------- GPU
def _run_case(cid, cmd, mode, settings, L=2048, S=1024, W=256, check_cover=True):
    """the case's reads through the HIP path batch by batch, Batch.chunks against chunks_ref over the FIXTURE's sig / ss / seq"""
    reads = _fixture_reads(cid)
    o, k, gen = _context(cmd, mode)
    rna, meth = bool(o.flags & profiles.SQ_RNA), bool(o.meth_freq)
    with_chunk = n_max_label = 0
    for lo in range(0, len(reads), o.batch):
        part = reads[lo:lo + o.batch]
        b = gen.stage([r["seq"] for r in part]).run().wait()
        for dtype, norm in settings:
            want = R.batch_chunks(part, k, rna, meth, L, S, W, dtype, norm, o.profile.range, o.profile.digitisation)
            ch = b.chunks(L, S, W, dtype=dtype, norm=norm)
            _assert_equal(ch, want, f"{cid} reads {lo}.. {dtype} {norm}")
        with_chunk += int(np.count_nonzero(np.diff(want["chunk_off"])))
        n_max_label = max(n_max_label, int(want["label_len"].max()) if len(want["label_len"]) else 0)
        b.free()
    gen.close()
    if check_cover:
        assert with_chunk >= 0.9 * len(reads), f"{cid}: only {with_chunk} of {len(reads)} reads have a chunk"
        assert n_max_label <= W, f"{cid}: a chunk has {n_max_label} bases, W = {W}"


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [api.MODE_EXACT, api.MODE_CERTIFIED], ids=["exact", "certified"])
@pytest.mark.parametrize("cid,cmd", CASES, ids=[c[0] for c in CASES])
def test_chunks_of_the_reference_vectors(cid, cmd, mode):
    assert len(CASES) == 18
    _run_case(cid, cmd, mode, ALL_SETTINGS)


@pytest.mark.gpu
@pytest.mark.parametrize("force", ["1", "2"], ids=["wide", "long"])
def test_generic_statistics_paths_forced(force, monkeypatch):
    """the development build's SQG_TEST_CHUNK_GENERIC: every read through the global-histogram path (1) / the several-workgroup path (2)"""
    monkeypatch.setenv("SQG_TEST_CHUNK_GENERIC", force)
    cmd = dict(CASES)["r10_t1"]
    _run_case("r10_t1", cmd, api.MODE_CERTIFIED, [("f16", "medmad"), ("f32", "medmad")])
    _run_case("rna004_noprefix", dict(CASES)["rna004_noprefix"], api.MODE_CERTIFIED, [("f16", "medmad")])


@pytest.mark.gpu
def test_narrow_label_rows_are_truncated():
    cid, cmd = "r9_t1", dict(CASES)["r9_t1"]
    reads = _fixture_reads(cid)
    o, k, gen = _context(cmd, api.MODE_EXACT)
    b = gen.stage([r["seq"] for r in reads]).run().wait()
    want = R.batch_chunks(reads, k, False, False, 2048, 1024, 64)
    ch = b.chunks(2048, 1024, 64)
    _assert_equal(ch, want, "W = 64")
    ll = _cpu(ch.label_len)
    assert ll.min() >= 208 and ll.max() <= 242 and (_cpu(ch.labels) != 0).all()
    ch = b.chunks(2048, 1024, 61)                           # a width the rows cannot be written in words
    _assert_equal(ch, R.batch_chunks(reads, k, False, False, 2048, 1024, 61), "W = 61")
    ch = b.chunks(2048, 1024, 0)                            # no labels: label_len still counts
    assert tuple(ch.labels.shape) == (ch.n_chunks, 0)
    np.testing.assert_array_equal(_cpu(ch.label_len), want["label_len"])
    b.free(); gen.close()


@pytest.mark.gpu
def test_strides_and_plan():
    cid, cmd = "r10_t1", dict(CASES)["r10_t1"]
    reads = _fixture_reads(cid)
    o, k, gen = _context(cmd, api.MODE_CERTIFIED)
    b = gen.stage([r["seq"] for r in reads]).run().wait()
    for L, S, dtype in ((2048, 2048, "f16"), (2048, 3072, "f32"), (64, 8, "f16"), (72, 8, "f32"), (4096, 1, "f16"), (1 << 20, 64, "f16")):
        want = R.batch_chunks(reads, k, False, False, L, S, 256, dtype)
        off, nc = b.chunk_plan(L, S)
        np.testing.assert_array_equal(off, want["chunk_off"])
        np.testing.assert_array_equal(off, _plan(list(b.sig_off), L, S))
        assert nc == off[-1]
        ch = b.chunks(L, S, 256, dtype=dtype)
        if L == 1 << 20:                                    # longer than every read: empty tensors, no device call
            assert nc == 0 and ch.n_chunks == 0 and tuple(ch.signal.shape) == (0, L) and tuple(ch.labels.shape) == (0, 256)
            assert ch.label_len.numel() == 0 and ch.chunk_read.numel() == 0 and ch.chunk_start.numel() == 0
            continue
        _assert_equal(ch, want, f"L {L} S {S}")
    assert b.chunks(2048).n_chunks == b.chunk_plan(2048, 2048)[1]          # stride defaults to the chunk length
    ch = b.chunks(2048, 1024, 256, signal=False, labels=False)              # the statistics pass alone
    want = R.batch_chunks(reads, k, False, False, 2048, 1024, 256)
    assert ch.signal is None and ch.labels is None
    _assert_equal(ch, want, "statistics only")
    b.free(); gen.close()


@pytest.mark.gpu
def test_degenerate_reads():
    """--ideal on a homopolymer (mad4 = 0 -> mad' = 1), a read shorter than k, a read of one k-mer, even and odd sample counts"""
    prof, fl = profiles.get_profile("dna-r9-prom")
    k = profiles.default_kmer_size(fl)
    mean, stdv = model.synthetic_model(k)
    rng = np.random.default_rng(5)
    seqs = [b"A" * 300, b"ACG", b"ACGTAC", bytes(rng.choice(list(b"ACGT"), 200).astype(np.uint8)), b"T" * 77, b"ACGTACG"]
    for flags in (fl | profiles.SQ_IDEAL, fl):
        orac = orc.Oracle(prof, flags, k, mean, stdv, 42, num_workers=1)
        want_reads = [dict(sig=w.sig, ss=w.ss, seq=s, offset=w.offset) for w, s in zip(orac.run_batch_seqs(seqs), seqs)]
        orac.close()
        gen = api.SignalGenerator(prof, flags, k, mean, stdv, 42, num_workers=1)
        b = gen.submit(seqs)
        np.testing.assert_array_equal(b.signal(), np.concatenate([w["sig"] for w in want_reads]))
        for L, S in ((64, 64), (64, 8), (128, 24)):
            for dtype, norm in ALL_SETTINGS:
                want = R.batch_chunks(want_reads, k, False, False, L, S, 32, dtype, norm, prof.range, prof.digitisation)
                _assert_equal(b.chunks(L, S, 32, dtype=dtype, norm=norm), want, f"flags {flags:#x} L {L} S {S} {dtype} {norm}")
        assert want["chunk_off"][2] == want["chunk_off"][1]                 # the read shorter than k has samples and no chunk
        assert len(want_reads[1]["sig"]) > 0
        if flags & profiles.SQ_IDEAL:
            assert want["mad4"][0] == 0 and want["mad4"][4] == 0
        assert {len(w["sig"]) & 1 for w in want_reads} == {0, 1} or flags & profiles.SQ_IDEAL
        b.free(); gen.close()


@pytest.mark.gpu
def test_statistics_of_a_batch_without_a_chunk():
    """med2 and mad4 are written for every read: also when no read of the batch has a chunk -- reads shorter than k, and reads with fewer
    samples than a chunk --, Batch.chunks makes the call and returns them, not zeros, beside tensors of no rows"""
    prof, fl = profiles.get_profile("dna-r9-prom")
    k = profiles.default_kmer_size(fl)
    mean, stdv = model.synthetic_model(k)
    seqs = [b"ACG", b"ACGTACGTAC", b"T", b"GATTACAGATT"]
    orac = orc.Oracle(prof, fl, k, mean, stdv, 42, num_workers=1)
    want_reads = [dict(sig=w.sig, ss=w.ss, seq=s, offset=w.offset) for w, s in zip(orac.run_batch_seqs(seqs), seqs)]
    orac.close()
    gen = api.SignalGenerator(prof, fl, k, mean, stdv, 42, num_workers=1)
    b = gen.submit(seqs)
    L = 2048
    assert all(0 < len(w["sig"]) < L for w in want_reads)
    for dtype, norm in ALL_SETTINGS:
        want = R.batch_chunks(want_reads, k, False, False, L, L, 16, dtype, norm, prof.range, prof.digitisation)
        ch = b.chunks(L, L, 16, dtype=dtype, norm=norm)
        assert ch.n_chunks == 0 and want["chunk_off"].tolist() == [0] * 5 and tuple(ch.signal.shape) == (0, L) and tuple(ch.labels.shape) == (0, 16)
        assert (want["med2"] != 0).all() and (want["mad4"] != 0).all()
        _assert_equal(ch, want, f"no chunk, {dtype} {norm}")
    b.free(); gen.close()


@pytest.mark.gpu
def test_codes_wider_than_the_lds_histogram():
    """a profile whose range is so small that a read's codes span tens of thousands of ADC values (and wrap the int16): the generic path,
    expected values from chunks_ref over the oracle's signal"""
    import dataclasses
    prof, fl = profiles.get_profile("dna-r9-prom")
    prof = dataclasses.replace(prof, range=prof.range / 60.0)
    k = profiles.default_kmer_size(fl)
    mean, stdv = model.synthetic_model(k)
    rng = np.random.default_rng(8)
    seqs = [bytes(rng.choice(list(b"ACGT"), int(m)).astype(np.uint8)) for m in rng.integers(300, 3000, 24)]
    orac = orc.Oracle(prof, fl, k, mean, stdv, 42, num_workers=1)
    want_reads = [dict(sig=w.sig, ss=w.ss, seq=s, offset=w.offset) for w, s in zip(orac.run_batch_seqs(seqs), seqs)]
    orac.close()
    spans = [int(w["sig"].max()) - int(w["sig"].min()) + 1 for w in want_reads]
    assert min(spans) > 4096, spans
    gen = api.SignalGenerator(prof, fl, k, mean, stdv, 42, num_workers=1)
    b = gen.submit(seqs)
    for dtype, norm in ALL_SETTINGS:
        want = R.batch_chunks(want_reads, k, False, False, 1024, 512, 128, dtype, norm, prof.range, prof.digitisation)
        _assert_equal(b.chunks(1024, 512, 128, dtype=dtype, norm=norm), want, f"wide codes {dtype} {norm}")
    b.free(); gen.close()


@pytest.mark.gpu
def test_a_read_too_long_for_one_workgroup():
    prof, fl = profiles.get_profile("dna-r10-prom")
    k = profiles.default_kmer_size(fl)
    mean, stdv = model.synthetic_model(k)
    rng = np.random.default_rng(22)
    seq = lambda n: bytes(rng.choice(list(b"ACGT"), int(n)).astype(np.uint8))   # noqa: E731
    seqs = [seq(900), seq(2.2e6), seq(1500)]
    gen = api.SignalGenerator(prof, fl, k, mean, stdv, 42, num_workers=1, mode=api.MODE_CERTIFIED)
    b = gen.submit(seqs)
    sig, dw = b.signal(), b.dwell()
    assert b.sig_off[2] - b.sig_off[1] > (1 << 22)
    reads = [dict(sig=sig[b.sig_off[i]:b.sig_off[i + 1]], ss=dw[b.ev_off[i]:b.ev_off[i + 1]], seq=seqs[i], offset=b.offset[i]) for i in range(3)]
    want = R.batch_chunks(reads, k, False, False, 4096, 4096, 512, "f16")
    _assert_equal(b.chunks(4096, 4096, 512), want, "long read")
    b.free(); gen.close()


@pytest.mark.gpu
def test_at_size_sampled_reads():
    """a few thousand sampled reads of mixed length: the per-read and per-chunk integers of all of them, signal and labels of a seeded
    subset of chunks, against chunks_ref over the batch's own fetched signal / dwell / reads"""
    prof, fl = profiles.get_profile("dna-r10-prom")
    k = profiles.default_kmer_size(fl)
    mean, stdv = model.synthetic_model(k)
    rng = np.random.default_rng(77)
    contigs = [bytes(rng.choice(list(b"ACGT"), 1500000).astype(np.uint8))]
    gen = api.SignalGenerator(prof, fl, k, mean, stdv, 42, num_workers=1, mode=api.MODE_CERTIFIED)
    gen.load_genome(contigs, 2500)
    b = gen.sample(2500).run().wait()
    sig, dw, seqs = b.signal(), b.dwell(), b.reads()
    reads = [dict(sig=sig[b.sig_off[i]:b.sig_off[i + 1]], ss=dw[b.ev_off[i]:b.ev_off[i + 1]], seq=seqs[i], offset=b.offset[i]) for i in range(b.n_reads)]
    L, S, W = 2048, 2048, 256
    want = R.batch_chunks(reads, k, False, False, L, S, W, "f16")
    ch = b.chunks(L, S, W)
    _assert_equal(ch, want, "at size", keys=("label_len", "chunk_read", "chunk_start", "med2", "mad4"))
    lens = np.diff(b.sig_off)
    assert lens.max() > 4 * lens.min() and ch.n_chunks > 10000
    longest = int(np.argmax(lens))
    must = [0, ch.n_chunks - 1, int(want["chunk_off"][longest]), int(want["chunk_off"][longest + 1]) - 1]
    pick = np.unique(np.concatenate((must, rng.choice(ch.n_chunks, 512, replace=False))))
    assert len(pick) >= 256
    idx = torch.as_tensor(pick, device=ch.signal.device)
    np.testing.assert_array_equal(R.bits(ch.signal[idx].cpu().numpy()), R.bits(want["signal"][pick]))
    np.testing.assert_array_equal(ch.labels[idx].cpu().numpy(), want["labels"][pick])
    b.free(); gen.close()


@pytest.mark.gpu
def test_lifetime_and_errors():
    cid, cmd = "r9_tk16", dict(CASES)["r9_tk16"]
    reads = _fixture_reads(cid)
    o, k, gen = _context(cmd, api.MODE_EXACT)
    parts = [reads[0:16], reads[16:32], reads[32:40]]
    b0 = gen.stage([r["seq"] for r in parts[0]])
    with pytest.raises(api.SqgError) as e:                  # staged, not run: an error, not a hang
        b0.chunks(2048, 1024, 256)
    assert e.value.code in (-1, -4)
    b0.run().wait()
    first = b0.chunks(2048, 1024, 256)
    _assert_equal(first, R.batch_chunks(parts[0], k, False, False, 2048, 1024, 256), "batch 0")
    for bad in (dict(chunk_len=63), dict(chunk_len=65), dict(chunk_len=0), dict(chunk_len=64, stride=0), dict(chunk_len=64, dtype=7),
                dict(chunk_len=64, norm=2), dict(chunk_len=64, max_label=70000), dict(chunk_len=(1 << 20) + 8)):
        with pytest.raises(api.SqgError) as e:
            b0.chunks(**bad)
        assert e.value.code == -1 and "sqg_" in str(e.value) and len(str(e.value)) > 30, bad
    b1 = gen.stage([r["seq"] for r in parts[1]]).run().wait()
    again = b0.chunks(2048, 1024, 256)                      # after batch 1 has been run: the same
    for key in ("signal", "labels", "label_len", "chunk_read", "chunk_start", "med2", "mad4"):
        np.testing.assert_array_equal(R.bits(_cpu(getattr(again, key))), R.bits(_cpu(getattr(first, key))), err_msg=key)
    b2 = gen.stage([r["seq"] for r in parts[2]]).run().wait()
    with pytest.raises(api.SqgError) as e:                  # two more batches: the slabs are batch 2's
        b0.chunks(2048, 1024, 256)
    assert e.value.code == -4
    _assert_equal(b1.chunks(2048, 1024, 256), R.batch_chunks(parts[1], k, False, False, 2048, 1024, 256), "batch 1 after batch 2")
    _assert_equal(b2.chunks(2048, 1024, 256), R.batch_chunks(parts[2], k, False, False, 2048, 1024, 256), "batch 2")
    for b in (b0, b1, b2):
        b.free()
    gen.close()
    # SQG_PREFIX contexts are rejected
    o, k, gen = _context(dict(REFVEC_CASES)["r9_prefix"], api.MODE_EXACT)
    b = gen.submit([r["seq"] for r in _fixture_reads("r9_prefix")])
    with pytest.raises(api.SqgError) as e:
        b.chunks(2048, 1024, 256)
    assert e.value.code == -1 and "SQG_PREFIX" in str(e.value)
    b.free(); gen.close()
    # NULL arguments at the C level
    L = api.load_library()
    cfg = api.CChunkCfg(64, 64, 0, 0, 0)
    nc = C.c_int64()
    assert L.sqg_chunk_plan(None, None, C.byref(cfg), None, C.byref(nc)) == -1
    assert L.sqg_batch_chunks(None, None, C.byref(cfg), None) == -1


@pytest.mark.gpu
def test_signal_tensor_is_a_view_and_chunks_leave_the_batch_alone():
    cid, cmd = "r10_tk8", dict(CASES)["r10_tk8"]
    reads = _fixture_reads(cid)[:8]
    o, k, gen = _context(cmd, api.MODE_CERTIFIED)
    b = gen.stage([r["seq"] for r in reads]).run().wait()
    sig, dw, off = b.signal().copy(), b.dwell().copy(), np.array(b.offset)
    t = b.signal_tensor()
    assert t.dtype == torch.int16 and t.is_cuda and t.numel() == b.n_samples
    assert t.data_ptr() == b.res.d_signal
    np.testing.assert_array_equal(t.cpu().numpy(), sig)
    np.testing.assert_array_equal(sig, np.concatenate([r["sig"] for r in reads]))
    for dtype, norm in ALL_SETTINGS:
        b.chunks(2048, 1024, 256, dtype=dtype, norm=norm)
    np.testing.assert_array_equal(b.signal(), sig)
    np.testing.assert_array_equal(b.dwell(), dw)
    np.testing.assert_array_equal(t.cpu().numpy(), sig)
    np.testing.assert_array_equal(np.array(b.wait().offset), off)
    del t
    b.free(); gen.close()
