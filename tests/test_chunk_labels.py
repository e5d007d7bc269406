"""The label pass of sqg_batch_chunks (k_chunk_labels, include/sqg_chunks.h) pinned where nothing sampled it: dwells from 1 to 5000 samples,
RNA and methylation at every geometry, event counts around the scan's 1024-event tiles, the 64-bit divisions, sampled reads of both
strands, and a batch's chunks taken while the generator runs two batches ahead.

Expected values never come from the library: sig / ss / offset are the ORACLE's (orc.Oracle), the chunks are chunks_ref's over them, and
label_cases.labels_by_definition is a second statement of the label rule that shares no idea with chunks_ref.  Every comparison is bit
for bit."""
import ctypes as C
import os

import numpy as np
import pytest
import torch  # noqa: F401  (before the library is loaded: the HIP runtime torch brings is the one the library then uses)

import chunks_ref as R
import label_cases as LC
import orc
from chunk_support import _assert_equal
from squigulator_amd import api, build, model, profiles

INPUTS = os.path.join(os.path.dirname(__file__), "golden", "inputs")
NCOV = os.path.join(INPUTS, "nCoV-2019.reference.fasta")
MFREQ_DENSE = os.path.join(INPUTS, "mfreq_dense.tsv")
MODES = {"certified": api.MODE_CERTIFIED, "exact": api.MODE_EXACT}


# ---------------------------------------------------------------------------------------------------------- no GPU
def test_label_code_table_against_chunks_ref():
    """the table typed from the header and chunks_ref's table say the same for every byte"""
    for b in range(256):
        want = LC.LABEL_CODE.get(chr(b), 1)
        assert R._CODE[b] == want, chr(b)
        assert R._CODE_METH[b] == (5 if chr(b) == "M" else want), chr(b)
    assert {LC.LABEL_CODE[c] for c in "RYSKBU"} == {1, 2, 3, 4} and LC.LABEL_CODE["N"] == 1


def test_labels_by_definition_on_the_hand_worked_read():
    """the numbers of test_chunks.test_reference_helper_on_hand_worked_reads: k = 3, dwells 3 2 4 2, E = 0 3 5 9, n = 11"""
    seq, ss = b"AMGTCA", [3, 2, 4, 2]
    lab, ll = LC.labels_by_definition(ss, seq, 3, False, True, 4, 2, 2)
    np.testing.assert_array_equal(lab, [[1, 5], [5, 3], [3, 0], [4, 0]])
    np.testing.assert_array_equal(ll, [2, 2, 1, 1])
    lab, ll = LC.labels_by_definition(ss, seq, 3, True, True, 4, 2, 3)
    np.testing.assert_array_equal(lab, [[4, 0, 0], [3, 0, 0], [3, 5, 0], [5, 0, 0]])
    np.testing.assert_array_equal(ll, [1, 1, 2, 1])
    lab, ll = LC.labels_by_definition(ss, seq, 3, False, False, 4, 2, 1)
    np.testing.assert_array_equal(lab, [[1], [1], [3], [4]])
    assert LC.labels_by_definition(ss, b"AC", 3, False, False, 4, 2, 1)[1].shape == (0,)       # shorter than k: no chunks


def _check_case_on_the_cpu(case):
    """the case is what its name says (from the oracle's output alone), and the two yardsticks agree on each of its geometries"""
    prof, fl, k, mean, stdv, rna, meth = LC.context_of(case)
    ref = LC.reference(case.name)
    kind, const = case.regime[0], int(case.regime[1])
    assert rna == case.ctx.startswith("rna") and meth == (case.ctx == "meth")
    ss_all = np.concatenate([r["ss"] for r, ev in zip(ref["reads"], case.events) if ev])
    for r, ev in zip(ref["reads"], case.events):
        assert len(r["ss"]) == (ev or 5) and int(np.sum(r["ss"])) == len(r["sig"])          # (a read shorter than k: five events, gensig.c:242)
        if kind != "drawn" and ev:
            assert (r["ss"] == const).all() and len(r["sig"]) == ev * const
        if meth and ev > 20:
            assert b"M" in r["seq"]
    if kind == "drawn":
        dmean, dstd = case.regime[1], case.regime[2]
        assert abs(ss_all.mean() - dmean) < 0.25 * dmean + 0.5 and ss_all.min() >= 1, (ss_all.mean(), ss_all.min())
        assert len(np.unique(ss_all)) > 1 and ss_all.std() < 1.5 * dstd + 1
    else:
        assert const == {"1": 1, "2.7": 2, "100": 100, "5000": 5000, "13.5": 13}[str(case.regime[1])]
    if any(c in case.name for c in ("drawn2", "time1", "meth")):
        assert set(b"acgtNRYSKBU") <= set(b"".join(ref["seqs"])), "lower case, N and the IUPAC letters must occur"
    shown = set()
    for (L, S, W) in case.lsw:
        want = ref["want"][(L, S, W)]
        off = want["chunk_off"]
        assert off[-1] <= 200000, (case.name, L, S, W, off[-1])
        assert want["labels"].shape == (off[-1], W)
        for i, r in enumerate(ref["reads"]):
            lab, ll = LC.labels_by_definition(r["ss"], r["seq"], k, rna, meth, L, S, W)
            np.testing.assert_array_equal(want["label_len"][off[i]:off[i + 1]], ll, err_msg=f"{case.name} {(L, S, W)} read {i}: label_len")
            np.testing.assert_array_equal(want["labels"][off[i]:off[i + 1]], lab, err_msg=f"{case.name} {(L, S, W)} read {i}: labels")
            shown |= LC.witnesses(r["ss"], len(r["sig"]), rna, L, S, W, lab, ll)
    assert set(case.shows) <= shown, f"{case.name} no longer shows {set(case.shows) - shown}"
    if case.regime == ("time", 1) and "wide" not in case.name:                        # the reads with n == L, L - 1, L + S - 1, L + S
        lens = {len(r["sig"]) for r in ref["reads"]}
        for L, S in ((64, 8), (128, 33), (72, 200), (4096, 4096)):
            assert {L, L - 1, L + S - 1, L + S} <= lens, (L, S)


@pytest.mark.parametrize("name", [c.name for c in LC.CASES])
def test_case_is_what_it_says_and_the_two_yardsticks_agree(name):
    _check_case_on_the_cpu(LC.BY_NAME[name])


def test_the_matrix_holds_what_the_label_pass_must_be_shown():
    """the table itself: contexts, worker counts, regimes, geometries, event counts, and every witness for DNA and for RNA (each case's
    `shows` is asserted from the oracle's output by the test above)"""
    cases = LC.CASES
    assert {c.ctx for c in cases} == set(LC.CONTEXTS) and {c.T for c in cases} == {1, 4}
    for fam in (("r9", "r10"), ("rna9", "rna004")):
        mine = [c for c in cases if c.ctx in fam]
        assert {c.T for c in mine if c.ctx == fam[0]} == {1, 4} and {c.T for c in mine if c.ctx == fam[1]} == {1, 4}
        assert {c.regime for c in mine if c.regime[0] == "drawn"} == {("drawn", 2, 0.5), ("drawn", 13, 4), ("drawn", 120, 96), ("drawn", 600, 480)}
        assert {c.regime for c in mine if c.regime[0] == "time"} == {("time", 1), ("time", 2.7), ("time", 100), ("time", 5000)}
        assert any(c.regime[0] == "ideal" for c in mine)
        lsw = {g for c in mine for g in c.lsw}
        assert {(64, 8, 48), (64, 1, 3), (128, 33, 61), (72, 200, 7), (4096, 4096, 256), (4096, 2048, 1000), (64, 64, 0)} <= lsw
        assert any(W == 65535 for _, _, W in lsw)
        const_events = {e for c in mine if c.regime[0] != "drawn" for e in c.events}
        assert {1, 2, 1023, 1024, 1025, 2048, 2049, 4097} <= const_events
        for w in LC.WITNESSES:
            assert any(w in c.shows for c in mine), f"{fam}: no case shows {w}"
        assert any(c.div64 and c.regime == ("drawn", 600, 480) for c in mine)
    meth = [c for c in cases if c.ctx == "meth"]
    assert {c.T for c in meth} == {1, 4} and all(set(LC.METH_WITNESSES) <= set(c.shows) for c in meth)
    assert any(c.div64 and c.ctx.startswith("rna") for c in cases)


# ---------------------------------------------------------------------------------------------------------- GPU
def _run_matrix_case(case, mode):
    prof, fl, k, mean, stdv, rna, meth = LC.context_of(case)
    ref = LC.reference(case.name)
    gen = api.SignalGenerator(prof, fl, k, mean, stdv, LC.SEED, num_workers=case.T, mode=mode)
    b = gen.submit(ref["seqs"])
    np.testing.assert_array_equal(b.signal(), np.concatenate([r["sig"] for r in ref["reads"]]), err_msg=f"{case.name}: signal")
    np.testing.assert_array_equal(b.dwell(), np.concatenate([r["ss"] for r in ref["reads"]]), err_msg=f"{case.name}: dwells")
    np.testing.assert_array_equal(np.array(b.offset), [r["offset"] for r in ref["reads"]])
    for g, (L, S, W) in enumerate(case.lsw):
        dtype, norm = LC.setting_of(case, g)
        _assert_equal(b.chunks(L, S, W, dtype=dtype, norm=norm), ref["want"][(L, S, W)], f"{case.name} L {L} S {S} W {W} {dtype} {norm}")
    b.free(); gen.close()


MATRIX = [(c.name, m) for c in LC.CASES for m in (("certified", "exact") if c.regime[0] == "drawn" else ("certified",))]


@pytest.mark.gpu
@pytest.mark.parametrize("name,mode", MATRIX, ids=[f"{n}-{m}" for n, m in MATRIX])
def test_label_geometry_matrix(name, mode, monkeypatch):
    monkeypatch.delenv("SQG_TEST_CHUNK_GENERIC", raising=False)
    _run_matrix_case(LC.BY_NAME[name], MODES[mode])


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c.name for c in LC.CASES if c.div64])
def test_label_geometry_with_64_bit_divisions(name, monkeypatch):
    """the development build's SQG_TEST_CHUNK_GENERIC=3: chunk_div's 64-bit branch, which otherwise needs a read of 2^31 samples; same outputs"""
    monkeypatch.setenv("SQG_TEST_CHUNK_GENERIC", "3")
    assert os.environ.get("SQG_LIB") or api.default_library_path() == build.LIB_DEV
    _run_matrix_case(LC.BY_NAME[name], MODES["certified"])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
def test_sampled_methylated_reads_of_both_strands(mode):
    """load_genome + set_meth + sample: the reads are the sampler's ('-' strand: reverse complement, then 'M' for the methylated CpGs);
    chunks_ref is fed with the ORACLE's reads, signal and dwells for the same draws"""
    prof, fl = profiles.get_profile("dna-r9-prom")
    fl |= profiles.SQ_METH
    k, T, rlen = 6, 3, 1500
    mean, stdv = model.synthetic_model(k, meth=True)
    orac = orc.Oracle(prof, fl, k, mean, stdv, 42, num_workers=T, rlen=rlen)
    ref = orac.load_ref(NCOV, None, MFREQ_DENSE)
    contigs = [bytes(ref.seqs[i][:ref.lengths[i]]) for i in range(ref.num_ref)]
    names = [ref.names[i].decode() for i in range(ref.num_ref)]
    gen = api.SignalGenerator(prof, fl, k, mean, stdv, 42, num_workers=T, mode=MODES[mode])
    gen.load_genome(contigs, rlen)
    gen.set_meth(contigs, names, MFREQ_DENSE)
    strands, minus_with_m, fives = set(), 0, 0
    for nb in (20, 33):
        want = orac.run_batch(nb)
        reads = [dict(sig=w.sig, ss=w.ss, seq=w.seq, offset=w.offset) for w in want]
        strands |= {w.strand for w in want}
        minus_with_m += sum(1 for w in want if w.strand == "-" and b"M" in w.seq)
        b = gen.sample(nb).run().wait()
        np.testing.assert_array_equal(b.signal(), np.concatenate([r["sig"] for r in reads]))
        np.testing.assert_array_equal(b.dwell(), np.concatenate([r["ss"] for r in reads]))
        for (L, S, W), (dtype, norm) in (((2048, 1024, 256), ("f16", "medmad")), ((128, 33, 61), ("f32", "pa")), ((64, 8, 5), ("f16", "pa"))):
            ch_want = R.batch_chunks(reads, k, False, True, L, S, W, dtype, norm, prof.range, prof.digitisation)
            _assert_equal(b.chunks(L, S, W, dtype=dtype, norm=norm), ch_want, f"sampled meth, batch of {nb}, L {L} S {S} W {W}")
            off = ch_want["chunk_off"]
            fives += sum(int((ch_want["labels"][off[i]:off[i + 1]] == 5).sum()) for i, w in enumerate(want) if w.strand == "-")
        b.free()
    gen.close(); orac.close()
    assert strands == {"+", "-"} and minus_with_m >= 5, (strands, minus_with_m)
    assert fives > 0                                         # code 5 in label rows of '-' strand reads


def _prepare_chunks(b, L, S, W):
    """Batch.chunks in two halves: the tensors now (with the device-wide synchronisation torch's allocator needs), the call later --
    so that the call itself can be made while a later batch's kernels are in flight"""
    cfg = b._chunk_cfg(L, S, W, "f16", "medmad")
    off, nc = b.chunk_plan(L, S)
    dev = torch.device("cuda", b.gen.device)
    ch = api.Chunks(n_chunks=nc, chunk_off=off, signal=torch.empty((nc, L), dtype=torch.float16, device=dev),
                    labels=torch.empty((nc, W), dtype=torch.uint8, device=dev), label_len=torch.empty((nc,), dtype=torch.int32, device=dev),
                    chunk_read=torch.empty((nc,), dtype=torch.int32, device=dev), chunk_start=torch.empty((nc,), dtype=torch.int64, device=dev),
                    med2=torch.zeros(b.n_reads, dtype=torch.int32, device=dev), mad4=torch.zeros(b.n_reads, dtype=torch.int32, device=dev))
    assert nc > 0
    out = api.CChunkOut(*[getattr(ch, key).data_ptr() for key in ("signal", "labels", "label_len", "chunk_read", "chunk_start", "med2", "mad4")])
    torch.cuda.synchronize(dev)

    def call():
        b.gen._chk(b.gen.L.sqg_batch_chunks(b.gen.ctx, b.handle, C.byref(cfg), C.byref(out)), "sqg_batch_chunks")
        return ch
    return call


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["default", "order-free"])
def test_labels_while_the_generator_runs_ahead(variant, monkeypatch):
    """what a trainer does: batch i+2 staged, batch i+1 queued and NOT waited for, chunks() of batch i -- in the 9-mer one-worker regime
    with cut chains, where all three dwell sets are live and batch i+2's first event pass rides inside batch i+1's hand-out"""
    monkeypatch.setenv("SQG_SPLIT_CHAINS", "7")
    prof, fl = profiles.get_profile("dna-r10-prom")
    flags = fl | (profiles.SQ_ORDER_FREE if variant == "order-free" else 0)
    k, L, S, W = 9, 1024, 512, 128
    mean, stdv = model.synthetic_model(k)
    rng = np.random.default_rng(61)
    batches = [[bytes(rng.choice(list(b"ACGTacgtNRY"), int(m), p=[.22, .22, .22, .22, .02, .02, .02, .02, .02, .01, .01]).astype(np.uint8))
                for m in rng.choice([k - 1, 64, 300, 513, 1024, 1025, 1600, 2100], int(rng.integers(6, 14)))] + [b"ACGT" * 300] for _ in range(5)]
    orac = orc.Oracle(prof, fl, k, mean, stdv, 42, num_workers=1)
    want = []
    for bt in batches:
        reads = [dict(sig=w.sig, ss=w.ss, seq=s, offset=w.offset) for w, s in zip(orac.run_batch_seqs(bt), bt)]
        want.append(R.batch_chunks(reads, k, False, False, L, S, W))
    orac.close()
    for mode in MODES.values():
        gen = api.SignalGenerator(prof, flags, k, mean, stdv, 42, num_workers=1, mode=mode)
        assert api.build_info(gen.L)["dev"] == "1"
        cur = gen.stage(batches[0]).run()
        nxt = gen.stage(batches[1])
        old = []
        for bi in range(len(batches)):
            nn = gen.stage(batches[bi + 2]) if bi + 2 < len(batches) else None
            call = _prepare_chunks(cur, L, S, W)            # (waits for batch bi, which a trainer has done anyway before it asks for chunks)
            ahead = nxt is not None
            if ahead:
                nxt.run()                                   # batch bi+1 in flight, batch bi+2 staged
            first = call()
            _assert_equal(first, want[bi], f"{variant} mode {mode} batch {bi}, its successor in flight")
            if old and ahead:                               # two runs old: its slabs and dwells belong to the batch in flight
                with pytest.raises(api.SqgError) as e:
                    old[-1].chunks(L, S, W)
                assert e.value.code == -4
            if nxt is not None:
                nxt.wait()
            again = cur.chunks(L, S, W)
            _assert_equal(again, want[bi], f"{variant} mode {mode} batch {bi}, its successor done")
            for key in ("signal", "labels", "label_len", "chunk_read", "chunk_start", "med2", "mad4"):
                assert torch.equal(getattr(first, key), getattr(again, key)), key
            old.append(cur)
            cur, nxt = nxt, nn
        assert len(old) == len(batches) >= 4
        for b in old:
            b.free()
        gen.close()
