"""sqg_batch_chunk_targets (include/sqg_targets.h): clean signal, moves and k-mer rows per chunk, made on the device, against the numpy
statement of the header's rules (targets_ref.py), against the compiled reference's own --ideal-amp vector, and against a twin run of the
same reads in an SQG_IDEAL_AMP context (HIP library and oracle).  Every comparison is bit for bit (floats as integers)."""
import ctypes as C
import dataclasses
import os
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (before the library is loaded: the HIP runtime torch brings is the one the library then uses)

import chunks_ref as R
import label_cases as LC
import orc
import targets_ref as T
from chunk_support import ALL_SETTINGS, CASES, _context, _declared, _fixture_reads
from refvec_cases import REFVEC_CASES
from squigulator_amd import api, build, model, options, profiles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VEC = os.path.join(ROOT, "tests", "golden", "refvec")
NCOV = os.path.join(ROOT, "tests", "golden", "inputs", "nCoV-2019.reference.fasta")
KEYS = ("clean", "clean_raw", "moves", "kmer")


# ---------------------------------------------------------------------------------------------------------- no GPU
def test_header_declares_the_target_export_and_the_libraries_have_it():
    assert _declared("sqg_targets.h") == set(api.EXPORTS_TARGETS) == {"sqg_batch_chunk_targets"}
    assert _declared("sqg_chunks.h") == set(api.EXPORTS_CHUNKS) == {"sqg_chunk_plan", "sqg_batch_chunks"}
    assert _declared("sqg.h") == set(api.EXPORTS)
    build.build()
    for lib in (build.LIB, build.LIB_DEV):
        L = api.load_library(lib)
        for n in api.EXPORTS_TARGETS:
            assert hasattr(L, n), f"{n} not exported by {lib}"
    assert os.path.join(ROOT, "include", "sqg_targets.h") in build.headers()
    assert [f[0] for f in api.CChunkTargets._fields_] == ["clean", "clean_raw", "moves", "kmer", "med2", "mad4"]


def test_the_cpu_backend_has_no_targets_and_says_so():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "libsqg_cpu.so"])
    prof, fl = profiles.get_profile("dna-r9-prom")
    mean, stdv = model.synthetic_model(6)
    gen = api.SignalGenerator(prof, fl, 6, mean, stdv, 42, lib_path=os.path.join(ROOT, "oracle", "libsqg_cpu.so"))
    b = gen.submit([b"ACGTACGTACGTTTGACA" * 40])
    with pytest.raises(api.SqgError) as e:
        b.chunk_targets(64)
    assert e.value.code == -1 and "sqg_batch_chunk_targets" in str(e.value)
    b.free(); gen.close()


def test_helper_reproduces_the_reference_ideal_amp_vector():
    """the reference's own --ideal-amp output, all 41 149 samples, from that file's seq / ss / offset and the synthetic model"""
    reads = _fixture_reads("r9_ideal_amp")
    o = options.parse_args(dict(REFVEC_CASES)["r9_ideal_amp"])
    mean, _ = model.synthetic_model(6)
    total = 0
    for r in reads:
        raw, moves, kmer = T.read_samples(r["seq"], r["ss"], r["offset"], mean, 6, False, False, o.profile.range, o.profile.digitisation)
        np.testing.assert_array_equal(raw, r["sig"])
        assert int(moves.sum()) == len(r["ss"]) and len(np.unique(kmer)) > 100
        total += len(raw)
    assert total == 41149
    noisy = _fixture_reads("r9_t1")[:3]                     # the same reads with the k-mer noise streams running
    for a, b in zip(reads, noisy):
        assert a["seq"] == b["seq"] and a["offset"] == b["offset"] and len(a["sig"]) == len(b["sig"])
        np.testing.assert_array_equal(a["ss"], b["ss"])


def test_helper_on_hand_worked_reads():
    """every number below was worked out by hand from include/sqg_targets.h: k = 3, dwells 3 2 4 2, E = 0 3 5 9, n = 11"""
    seq, ss = b"AMGTCA", [3, 2, 4, 2]
    np.testing.assert_array_equal(T.kmer_ranks(seq, 3, False), [2, 11, 45, 52])          # M is rank 0 of the 4-letter table
    np.testing.assert_array_equal(T.kmer_ranks(seq, 3, True), [17, 89, 71, 105])         # base 5: A C G M T
    np.testing.assert_array_equal(T.kmer_ranks(b"acgtNU", 3, False), [6, 27, 44, 51])     # lower case counts, N is A, U is T
    level = np.arange(125, dtype=np.float32)                # level = rank, offset 0.5: code = trunc(rank - 0.5) = rank - 1
    sig = np.array([3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5], np.int16)                         # med2 = 8, mad4 = 4 (test_chunks)
    d = T.read_targets(sig, seq, ss, 0.5, level, 3, False, False, 4, 2, "f32")
    np.testing.assert_array_equal(d["kmer"], [[2, 2, 2, 11], [2, 11, 11, 45], [11, 45, 45, 45], [45, 45, 45, 52]])   # chunks start mid-event
    np.testing.assert_array_equal(d["moves"], [[1, 0, 0, 1], [0, 1, 0, 1], [0, 1, 0, 0], [0, 0, 0, 1]])
    np.testing.assert_array_equal(d["clean_raw"], [[1, 1, 1, 10], [1, 10, 10, 44], [10, 44, 44, 44], [44, 44, 44, 51]])
    inv = np.float32(1.0 / 1.4826)
    np.testing.assert_array_equal(R.bits(d["clean"][0]), R.bits((np.array([-3, -3, -3, 6], np.float32) * inv).astype(np.float32)))
    np.testing.assert_array_equal(d["moves"].sum(1), [2, 2, 1, 1])                      # label_len of test_chunks' hand-worked read
    d = T.read_targets(sig, seq, ss, 0.5, level, 3, False, True, 4, 2)                  # the methylation table
    np.testing.assert_array_equal(d["kmer"][1], [17, 89, 89, 71])
    np.testing.assert_array_equal(d["clean_raw"][3], [70, 70, 70, 104])
    assert d["clean"].dtype == np.float16
    # RNA: stored p is generation-order 10 - p; chunk 0 = g 10 9 8 7, chunk 2 = g 6 5 4 3; a move sits on the event's LAST stored sample
    d = T.read_targets(sig, seq, ss, 0.5, level, 3, True, False, 4, 2)
    np.testing.assert_array_equal(d["kmer"], [[52, 52, 45, 45], [45, 45, 45, 45], [45, 45, 11, 11], [11, 11, 2, 2]])
    np.testing.assert_array_equal(d["moves"], [[0, 1, 0, 0], [0, 0, 0, 1], [0, 1, 0, 1], [0, 1, 0, 0]])
    np.testing.assert_array_equal(d["moves"].sum(1), [1, 1, 2, 1])
    # S > L: gaps; one event of six samples
    d = T.read_targets(np.array([7, 7, 7, 7, 2, 7], np.int16), b"ACG", [6], 0.0, level, 3, False, False, 2, 3)
    np.testing.assert_array_equal(d["moves"], [[1, 0], [0, 0]])
    np.testing.assert_array_equal(d["kmer"], [[6, 6], [6, 6]])
    assert T.read_targets(sig, b"AC", [3, 2, 4, 1, 1], 0.0, level, 3, False, False, 4, 2)["moves"].shape == (0, 4)   # shorter than k
    # levels that wrap: 1e6 = 0xF4240 -> 0x4240; -1e6 -> -0x4240; 3e9 does not fit int32 -> INT32_MIN -> low half 0
    np.testing.assert_array_equal(T.to_i16([1e6, -1e6, 3e9, -3e9, 32768.9, -32769.5, -0.9]), [16960, -16960, 0, 0, -32768, 32767, 0])
    wrap = np.zeros(64, np.float32); wrap[6] = 1e6
    d = T.read_targets(np.array([7, 7, 7, 7, 2, 7], np.int16), b"ACG", [6], 0.0, wrap, 3, False, False, 2, 3, "f32", "pa", 2.0, 4.0)
    np.testing.assert_array_equal(d["clean_raw"], [[-31616, -31616]] * 2)                # 1e6 * 4 / 2 = 2 000 000 = 0x1E8480 -> 0x8480
    np.testing.assert_array_equal(d["clean"], [[-15808.0, -15808.0]] * 2)                # (raw + 0) * 2 / 4


# ---------------------------------------------------------------------------------------------------------- GPU
def _cpu(t, key):
    a = t.cpu().numpy()
    return a.view(np.uint32) if key == "kmer" else a


def _compare(tg, want, what, keys=KEYS):
    assert tg.n_chunks == want["chunk_off"][-1], f"{what}: {tg.n_chunks} chunks, expected {want['chunk_off'][-1]}"
    np.testing.assert_array_equal(tg.chunk_off, want["chunk_off"], err_msg=f"{what}: chunk_off")
    for key in keys:
        got = _cpu(getattr(tg, key), key)
        assert got.shape == want[key].shape and got.dtype == want[key].dtype, f"{what}: {key} {got.shape} {got.dtype} vs {want[key].shape} {want[key].dtype}"
        np.testing.assert_array_equal(R.bits(got), R.bits(want[key]), err_msg=f"{what}: {key}")


def _invariants(b, tg, L, S, rna, what):
    """moves.sum(1) == label_len of Batch.chunks; clean_raw and kmer change only where moves says an event starts"""
    if tg.n_chunks == 0:
        return
    ll = b.chunks(L, S, 0, signal=False).label_len.cpu().numpy()
    moves, raw, kmer = (_cpu(getattr(tg, key), key) for key in ("moves", "clean_raw", "kmer"))
    np.testing.assert_array_equal(moves.astype(np.int64).sum(1), ll, err_msg=f"{what}: moves vs label_len")
    assert set(np.unique(moves)) <= {0, 1}
    starts = moves[:, :-1] if rna else moves[:, 1:]         # RNA: the new event begins one sample after the move
    for a in (raw, kmer):
        changed = a[:, 1:] != a[:, :-1]
        assert not (changed & (starts == 0)).any(), f"{what}: a value changes inside an event"


def _all_four(b, L, S, dtype="f16", norm="medmad", **kw):
    return b.chunk_targets(L, S, dtype=dtype, norm=norm, clean=True, clean_raw=True, moves=True, kmer=True, **kw)


def _check(b, reads, mean, k, rna, meth, prof, L, S, settings, what, invariants=True):
    tg = None
    for dtype, norm in settings:
        want = T.batch_targets(reads, mean, k, rna, meth, L, S, dtype, norm, prof.range, prof.digitisation)
        tg = _all_four(b, L, S, dtype, norm)
        _compare(tg, want, f"{what} L {L} S {S} {dtype} {norm}")
    if invariants:
        _invariants(b, tg, L, S, rna, what)
    return tg


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [api.MODE_EXACT, api.MODE_CERTIFIED], ids=["exact", "certified"])
@pytest.mark.parametrize("cid,cmd", CASES, ids=[c[0] for c in CASES])
def test_targets_of_the_reference_vectors(cid, cmd, mode):
    """the fixture's reads through the HIP path; all four outputs against targets_ref over the FIXTURE's seq / ss / offset (sig for med2 / mad4)"""
    assert len(CASES) == 18
    reads = _fixture_reads(cid)
    o, k, gen = _context(cmd, mode)
    rna, meth = bool(o.flags & profiles.SQ_RNA), bool(o.meth_freq)
    mean, _ = model.synthetic_model(k, meth=meth)
    with_chunk = 0
    for lo in range(0, len(reads), o.batch):
        part = reads[lo:lo + o.batch]
        b = gen.stage([r["seq"] for r in part]).run().wait()
        tg = _check(b, part, mean, k, rna, meth, o.profile, 2048, 1024, ALL_SETTINGS, f"{cid} reads {lo}..")
        with_chunk += int(np.count_nonzero(np.diff(tg.chunk_off)))
        if cid == "r9_t1":                                  # the reference's own --ideal-amp run of reads 0-2
            amp = _fixture_reads("r9_ideal_amp")
            raw = _cpu(tg.clean_raw, "clean_raw")
            for i in range(3):
                rows = raw[tg.chunk_off[i]:tg.chunk_off[i + 1]]
                assert len(rows) > 0
                for j, row in enumerate(rows):
                    np.testing.assert_array_equal(row, amp[i]["sig"][j * 1024:j * 1024 + 2048], err_msg=f"read {i} chunk {j} vs r9_ideal_amp.npz")
        b.free()
    gen.close()
    assert with_chunk >= 0.9 * len(reads), f"{cid}: only {with_chunk} of {len(reads)} reads have a chunk"


def _cut(sigs, off, L, S):
    rows = [s[j * S:j * S + L] for i, s in enumerate(sigs) for j in range(int(off[i + 1] - off[i]))]
    return np.stack(rows) if rows else np.zeros((0, L), np.int16)


TWINS = {  # name -> (profile, extra flags, workers, how the reads are made)
    "r9": ("dna-r9-prom", 0, 1, "seqs"), "r10": ("dna-r10-prom", 0, 1, "seqs"), "rna9": ("rna-r9-prom", 0, 1, "seqs"),
    "rna004": ("rna004-prom", 0, 1, "seqs"), "meth": ("dna-r9-prom", profiles.SQ_METH, 1, "seqs"),
    "r10_t4": ("dna-r10-prom", 0, 4, "seqs"), "r9_sampled": ("dna-r9-prom", 0, 3, "sample"),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TWINS))
def test_clean_raw_is_the_signal_of_an_ideal_amp_twin(name):
    """same reads, seed and workers through a second context with SQG_IDEAL_AMP -- on the HIP library and on the oracle: its signal, cut by
    the plan, is clean_raw; and its PA chunks are the PA clean rows, bit for bit"""
    pname, extra, workers, how = TWINS[name]
    prof, fl = profiles.get_profile(pname)
    fl |= extra
    k = profiles.default_kmer_size(fl)
    rna, meth = bool(fl & profiles.SQ_RNA), bool(fl & profiles.SQ_METH)
    mean, stdv = model.synthetic_model(k, meth=meth)
    rng = np.random.default_rng(len(name) + 90)
    letters = list(b"ACGT" + (b"M" if meth else b""))
    nread = 4 if workers > 1 else 7                         # T = K: one read per worker and batch
    seqs = [bytes(rng.choice(letters, int(m)).astype(np.uint8)) for m in rng.integers(150, 900, nread)]
    gens = [api.SignalGenerator(prof, f, k, mean, stdv, 42, num_workers=workers, mode=api.MODE_CERTIFIED) for f in (fl, fl | profiles.SQ_IDEAL_AMP)]
    orac = orc.Oracle(prof, fl | profiles.SQ_IDEAL_AMP, k, mean, stdv, 42, num_workers=workers, rlen=1500)
    if how == "sample":
        ref = orac.load_ref(NCOV)
        contigs = [bytes(ref.seqs[i][:ref.lengths[i]]) for i in range(ref.num_ref)]
        for g in gens:
            g.load_genome(contigs, 1500)
        want = orac.run_batch(24)
        assert {w.strand for w in want} == {"+", "-"}
        b, twin = (g.sample(24).run().wait() for g in gens)
    else:
        want = orac.run_batch_seqs(seqs)
        b, twin = (g.submit(seqs) for g in gens)
    np.testing.assert_array_equal(twin.signal(), np.concatenate([w.sig for w in want]), err_msg="the twin context against the oracle")
    assert not np.array_equal(b.signal(), twin.signal())
    np.testing.assert_array_equal(b.dwell(), twin.dwell())
    np.testing.assert_array_equal(np.array(b.offset), np.array(twin.offset), err_msg="the twin draws the same offsets")
    tsig = twin.signal()
    tsigs = [tsig[twin.sig_off[i]:twin.sig_off[i + 1]] for i in range(twin.n_reads)]
    for L, S in ((256, 128), (64, 8), (72, 200)):
        tg = _all_four(b, L, S)
        assert tg.n_chunks > 0
        np.testing.assert_array_equal(_cpu(tg.clean_raw, "clean_raw"), _cut(tsigs, tg.chunk_off, L, S), err_msg=f"{name} L {L} S {S}: HIP twin")
        np.testing.assert_array_equal(_cpu(tg.clean_raw, "clean_raw"), _cut([w.sig for w in want], tg.chunk_off, L, S), err_msg=f"{name} L {L} S {S}: oracle")
        _invariants(b, tg, L, S, rna, f"{name} L {L} S {S}")
        for d in ("f16", "f32"):                            # PA is a function of code and offset alone, one statement of it: clean IS the twin's noisy chunk
            clean = b.chunk_targets(L, S, dtype=d, norm="pa", clean=True, moves=False).clean.cpu().numpy()
            np.testing.assert_array_equal(R.bits(clean), R.bits(twin.chunks(L, S, 0, dtype=d, norm="pa", labels=False).signal.cpu().numpy()), err_msg=f"{name} L {L} S {S} {d}: PA clean")
    for x in (b, twin):
        x.free()
    for g in gens:
        g.close()
    orac.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c.name for c in LC.CASES])
def test_geometries_and_dwell_extremes(name, monkeypatch):
    """label_cases' matrix: dwells 1 .. 5000, event counts around 1024-event tiles, L 64 / S 8, L 72, S > L, L 65544 (tiles of a chunk, rows
    that are only 8-byte aligned), the constant-dwell contexts (SQG_IDEAL_TIME, SQG_IDEAL); expected values over the ORACLE's reads"""
    monkeypatch.delenv("SQG_TEST_CHUNK_GENERIC", raising=False)
    case = LC.BY_NAME[name]
    prof, fl, k, mean, stdv, rna, meth = LC.context_of(case)
    ref = LC.reference(name)
    gen = api.SignalGenerator(prof, fl, k, mean, stdv, LC.SEED, num_workers=case.T, mode=api.MODE_CERTIFIED)
    b = gen.submit(ref["seqs"])
    np.testing.assert_array_equal(b.dwell(), np.concatenate([r["ss"] for r in ref["reads"]]))
    for g, (L, S, W) in enumerate(case.lsw):
        _check(b, ref["reads"], mean, k, rna, meth, prof, L, S, [LC.setting_of(case, g)], name)
    b.free(); gen.close()


@pytest.mark.gpu
def test_strides_odd_addresses_and_no_chunk():
    cid, cmd = "r10_t1", dict(CASES)["r10_t1"]
    reads = _fixture_reads(cid)
    o, k, gen = _context(cmd, api.MODE_CERTIFIED)
    mean, _ = model.synthetic_model(k)
    b = gen.stage([r["seq"] for r in reads]).run().wait()
    assert any(int(x) & 1 for x in b.sig_off[:-1])          # reads (and so chunks) that start at odd sample addresses
    for L, S, dtype in ((2048, 2048, "f16"), (2048, 3072, "f32"), (64, 8, "f16"), (72, 8, "f32"), (4096, 37, "f16"), (8200, 4099, "f32")):
        _check(b, reads, mean, k, False, False, o.profile, L, S, [(dtype, "medmad")], cid)
    tg = _all_four(b, 1 << 20, 64)                          # longer than every read: empty tensors, no device call
    assert tg.n_chunks == 0 and all(tuple(getattr(tg, key).shape) == (0, 1 << 20) for key in KEYS)
    tg = b.chunk_targets(2048)                              # the defaults: clean and moves, stride = chunk length
    assert tg.clean_raw is None and tg.kmer is None and tg.clean.dtype == torch.float16 and tg.moves.dtype == torch.uint8
    _compare(tg, T.batch_targets(reads, mean, k, False, False, 2048, 2048, "f16", "medmad", o.profile.range, o.profile.digitisation), "defaults", keys=("clean", "moves"))
    b.free(); gen.close()


@pytest.mark.gpu
def test_pore_model_far_outside_the_adc_range():
    """levels around +-1e6 and a range that makes picoamperes overflow binary16: clean_raw wraps as the oracle's --ideal-amp signal does,
    F16 clean has the helper's infinities"""
    prof, fl = profiles.get_profile("dna-r9-prom")
    prof = dataclasses.replace(prof, range=prof.range * 40.0)
    k = 6
    mean, stdv = model.synthetic_model(k)
    far = np.where(np.arange(len(mean)) % 2 == 0, 1e6 + 300.0 * mean, -1e6 - 300.0 * mean).astype(np.float32)
    rng = np.random.default_rng(3)
    seqs = [bytes(rng.choice(list(b"ACGT"), int(m)).astype(np.uint8)) for m in rng.integers(200, 1200, 6)]
    orac = orc.Oracle(prof, fl | profiles.SQ_IDEAL_AMP, k, far, stdv, 42, num_workers=1)
    amp = orac.run_batch_seqs(seqs)
    orac.close()
    orac = orc.Oracle(prof, fl, k, far, stdv, 42, num_workers=1)
    reads = [dict(sig=w.sig, ss=w.ss, seq=s, offset=w.offset) for w, s in zip(orac.run_batch_seqs(seqs), seqs)]
    orac.close()
    gen = api.SignalGenerator(prof, fl, k, far, stdv, 42, num_workers=1, mode=api.MODE_EXACT)
    b = gen.submit(seqs)
    np.testing.assert_array_equal(b.signal(), np.concatenate([r["sig"] for r in reads]))
    L, S = 512, 256
    for dtype, norm in ALL_SETTINGS:
        want = T.batch_targets(reads, far, k, False, False, L, S, dtype, norm, prof.range, prof.digitisation)
        tg = _all_four(b, L, S, dtype, norm)
        _compare(tg, want, f"far model {dtype} {norm}")
        if (dtype, norm) == ("f16", "pa"):
            assert np.isinf(want["clean"]).any() and (want["clean"] == -np.inf).any() and (want["clean"] == np.inf).any()
    np.testing.assert_array_equal(_cpu(tg.clean_raw, "clean_raw"), _cut([w.sig for w in amp], tg.chunk_off, L, S))
    level = far.astype(np.float64) * prof.digitisation / prof.range
    assert np.abs(level).min() > 2 * 32768                  # every level is outside int16: all of them wrap
    b.free(); gen.close()


def _raw_call(b, L, S, dtype, norm, **ptrs):
    cfg = b._chunk_cfg(L, S, 0, dtype, norm)
    out = api.CChunkTargets(*[ptrs.get(key) for key in ("clean", "clean_raw", "moves", "kmer", "med2", "mad4")])
    torch.cuda.synchronize()
    return b.gen.L.sqg_batch_chunk_targets(b.gen.ctx, b.handle, C.byref(cfg), C.byref(out))


@pytest.mark.gpu
def test_statistics_passed_in_and_null_outputs():
    cid, cmd = "r9_tk16", dict(CASES)["r9_tk16"]
    reads = _fixture_reads(cid)[:16]
    o, k, gen = _context(cmd, api.MODE_CERTIFIED)
    mean, _ = model.synthetic_model(k)
    b = gen.stage([r["seq"] for r in reads]).run().wait()
    L, S = 1024, 512
    ch = b.chunks(L, S, 64)
    for dtype in ("f16", "f32"):
        own = _all_four(b, L, S, dtype)
        given = _all_four(b, L, S, dtype, chunks=ch)
        for key in KEYS:
            assert torch.equal(getattr(own, key), getattr(given, key)), key
        _compare(given, T.batch_targets(reads, mean, k, False, False, L, S, dtype, "medmad", o.profile.range, o.profile.digitisation), f"statistics passed in, {dtype}")
    # wrong statistics change clean (they ARE used) and nothing else
    wrong = api.Chunks(med2=ch.med2 + 100, mad4=ch.mad4)
    w = _all_four(b, L, S, "f32", chunks=wrong)
    assert not torch.equal(w.clean, own.clean) and torch.equal(w.clean_raw, own.clean_raw) and torch.equal(w.moves, own.moves)
    # NULL outputs: each output alone and in pairs, inside guard bytes; what is not passed is not written
    nc = own.n_chunks
    size = {"clean": 4, "clean_raw": 2, "moves": 1, "kmer": 4}
    dev = own.clean.device
    for wanted in (("clean",), ("clean_raw",), ("moves",), ("kmer",), ("clean_raw", "moves"), ("clean", "kmer"), ("moves", "kmer")):
        bufs = {key: torch.full((nc * L * size[key] + 512,), 0xA5, dtype=torch.uint8, device=dev) for key in KEYS}
        ptrs = {key: bufs[key].data_ptr() + 256 for key in wanted}
        assert all(p % 256 == 0 for p in ptrs.values())
        assert _raw_call(b, L, S, "f32", "medmad", **ptrs) == 0
        for key in KEYS:
            a = bufs[key].cpu().numpy()
            if key in wanted:
                assert (a[:256] == 0xA5).all() and (a[-256:] == 0xA5).all(), f"{wanted}: guard bytes of {key}"
                np.testing.assert_array_equal(a[256:-256], _cpu(getattr(own, key), key).reshape(-1).view(np.uint8), err_msg=f"{wanted}: {key}")
            else:
                assert (a == 0xA5).all(), f"{wanted}: {key} was written"
    b.free(); gen.close()


@pytest.mark.gpu
def test_lifetime_and_errors():
    cid, cmd = "r9_tk16", dict(CASES)["r9_tk16"]
    reads = _fixture_reads(cid)
    o, k, gen = _context(cmd, api.MODE_EXACT)
    mean, _ = model.synthetic_model(k)
    parts = [reads[0:16], reads[16:32], reads[32:40]]
    b0 = gen.stage([r["seq"] for r in parts[0]])
    with pytest.raises(api.SqgError) as e:                  # staged, not run
        b0.chunk_targets(2048, 1024)
    assert e.value.code == -4
    dummy = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    rc = b0.gen.L.sqg_batch_chunk_targets(gen.ctx, b0.handle, C.byref(api.CChunkCfg(64, 64, 0, 0, 0)),
                                          C.byref(api.CChunkTargets(None, None, dummy.data_ptr(), None, None, None)))
    assert rc == -4 and b"sqg_batch_chunk_targets" in gen.L.sqg_last_error(gen.ctx)
    b0.run().wait()
    first = _all_four(b0, 2048, 1024)
    _compare(first, T.batch_targets(parts[0], mean, k, False, False, 2048, 1024, "f16", "medmad", o.profile.range, o.profile.digitisation), "batch 0")
    for bad in (dict(chunk_len=63), dict(chunk_len=0), dict(chunk_len=64, stride=0), dict(chunk_len=64, dtype=7), dict(chunk_len=64, norm=2),
                dict(chunk_len=(1 << 20) + 8)):
        with pytest.raises(api.SqgError) as e:
            b0.chunk_targets(**bad)
        assert e.value.code == -1 and "sqg_" in str(e.value), bad
    p = dummy.data_ptr()
    assert _raw_call(b0, 64, 64, "f16", "medmad", moves=p + 4) == -1 and b"sqg_batch_chunk_targets" in gen.L.sqg_last_error(gen.ctx)
    assert _raw_call(b0, 64, 64, "f16", "medmad", clean_raw=p + 8) == -1
    assert _raw_call(b0, 64, 64, "f16", "medmad", clean=p + 2) == -1
    assert _raw_call(b0, 64, 64, "f16", "medmad", kmer=p + 8) == -1
    assert _raw_call(b0, 64, 64, "f16", "medmad", clean=first.clean.data_ptr(), med2=p) == -1
    assert b"med2" in gen.L.sqg_last_error(gen.ctx) and b"sqg_batch_chunk_targets" in gen.L.sqg_last_error(gen.ctx)
    assert _raw_call(b0, 64, 64, "f16", "medmad", clean=first.clean.data_ptr(), mad4=p) == -1
    assert gen.L.sqg_batch_chunk_targets(None, None, None, None) == -1
    assert gen.L.sqg_batch_chunk_targets(gen.ctx, b0.handle, C.byref(api.CChunkCfg(64, 64, 0, 0, 0)), None) == -1
    assert _raw_call(b0, 64, 64, "f16", "medmad") == 0      # nothing wanted: nothing done
    b1 = gen.stage([r["seq"] for r in parts[1]]).run().wait()
    again = _all_four(b0, 2048, 1024)                       # after batch 1 has been run: the same
    for key in KEYS:
        assert torch.equal(getattr(again, key), getattr(first, key)), key
    b2 = gen.stage([r["seq"] for r in parts[2]]).run().wait()
    with pytest.raises(api.SqgError) as e:                  # two more batches: slabs and dwells are batch 2's
        b0.chunk_targets(2048, 1024)
    assert e.value.code == -4 and "sqg_batch_chunk_targets" in str(e.value)
    _compare(_all_four(b1, 2048, 1024), T.batch_targets(parts[1], mean, k, False, False, 2048, 1024, "f16", "medmad", o.profile.range, o.profile.digitisation), "batch 1 after batch 2")
    _compare(_all_four(b2, 2048, 1024), T.batch_targets(parts[2], mean, k, False, False, 2048, 1024, "f16", "medmad", o.profile.range, o.profile.digitisation), "batch 2")
    for b in (b0, b1, b2):
        b.free()
    gen.close()
    o, k, gen = _context(dict(REFVEC_CASES)["r9_prefix"], api.MODE_EXACT)
    b = gen.submit([r["seq"] for r in _fixture_reads("r9_prefix")])
    with pytest.raises(api.SqgError) as e:
        b.chunk_targets(2048, 1024)
    assert e.value.code == -1 and "SQG_PREFIX" in str(e.value)
    dummy = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    assert _raw_call(b, 64, 64, "f16", "medmad", moves=dummy.data_ptr()) == -1
    assert b"sqg_batch_chunk_targets" in gen.L.sqg_last_error(gen.ctx) and b"SQG_PREFIX" in gen.L.sqg_last_error(gen.ctx)
    b.free(); gen.close()


@pytest.mark.gpu
def test_targets_while_the_generator_runs_ahead(monkeypatch):
    """batch i+2 staged, batch i+1 queued and not waited for, the targets of batch i: all three dwell sets are live"""
    monkeypatch.setenv("SQG_SPLIT_CHAINS", "7")
    prof, fl = profiles.get_profile("dna-r10-prom")
    k, L, S = 9, 1024, 512
    mean, stdv = model.synthetic_model(k)
    rng = np.random.default_rng(61)
    batches = [[bytes(rng.choice(list(b"ACGTacgtNRY"), int(m), p=[.22, .22, .22, .22, .02, .02, .02, .02, .02, .01, .01]).astype(np.uint8))
                for m in rng.choice([k - 1, 64, 300, 513, 1024, 1025, 1600, 2100], int(rng.integers(6, 14)))] + [b"ACGT" * 300] for _ in range(5)]
    orac = orc.Oracle(prof, fl, k, mean, stdv, 42, num_workers=1)
    want = []
    for bt in batches:
        reads = [dict(sig=w.sig, ss=w.ss, seq=s, offset=w.offset) for w, s in zip(orac.run_batch_seqs(bt), bt)]
        want.append(T.batch_targets(reads, mean, k, False, False, L, S, "f16", "medmad", prof.range, prof.digitisation))
    orac.close()
    gen = api.SignalGenerator(prof, fl, k, mean, stdv, 42, num_workers=1, mode=api.MODE_CERTIFIED)
    assert api.build_info(gen.L)["dev"] == "1"
    dev = torch.device("cuda", gen.device)
    cur = gen.stage(batches[0]).run()
    nxt = gen.stage(batches[1])
    old = []
    for bi in range(len(batches)):
        nn = gen.stage(batches[bi + 2]) if bi + 2 < len(batches) else None
        off, nc = cur.chunk_plan(L, S)                      # (waits for batch bi)
        assert nc > 0
        tg = api.Chunks(n_chunks=nc, chunk_off=off, clean=torch.empty((nc, L), dtype=torch.float16, device=dev),
                        clean_raw=torch.empty((nc, L), dtype=torch.int16, device=dev), moves=torch.empty((nc, L), dtype=torch.uint8, device=dev),
                        kmer=torch.empty((nc, L), dtype=torch.int32, device=dev))
        torch.cuda.synchronize(dev)
        if nxt is not None:
            nxt.run()                                       # batch bi+1 in flight, batch bi+2 staged
        cfg = cur._chunk_cfg(L, S, 0, "f16", "medmad")
        out = api.CChunkTargets(tg.clean.data_ptr(), tg.clean_raw.data_ptr(), tg.moves.data_ptr(), tg.kmer.data_ptr(), None, None)
        gen._chk(gen.L.sqg_batch_chunk_targets(gen.ctx, cur.handle, C.byref(cfg), C.byref(out)), "sqg_batch_chunk_targets")
        _compare(tg, want[bi], f"batch {bi}, its successor in flight")
        if old and nxt is not None:
            with pytest.raises(api.SqgError) as e:
                old[-1].chunk_targets(L, S)
            assert e.value.code == -4
        if nxt is not None:
            nxt.wait()
        _compare(_all_four(cur, L, S), want[bi], f"batch {bi}, its successor done")
        old.append(cur)
        cur, nxt = nxt, nn
    for b in old:
        b.free()
    gen.close()
