"""The device read sampler (k_sampler.h, h_sampler.h, k_copy_reads) on drawn contexts: tests/sampler_cases.py draws 60 of them -- DNA with
and without the prefix, methylation on genomes with N runs and lower case, genomes that reject most attempts, RNA, cDNA and truncated
transcripts of drawn transcriptomes -- and every read is the oracle's, bit for bit (test_sampler._run).  One test without the device holds
the table to what it was drawn for; beside the draw stand the planted cases: the abundance table's fall-back, the error returns and what
the context does after them.  Every expectation is the oracle's (oracle/sqg_oracle.c, gen_read of src/genread.c:125-370)."""
import time

import numpy as np
import pytest

import orc
import sampler_cases as SC
from squigulator_amd import api, model, profiles
from test_sampler import _compare, _contigs, _run

SEEDS = range(SC.N_SEEDS)


def test_the_table_holds_what_it_is_for(tmp_path):
    """from the oracle's reads and the genomes alone: the paths of the copy kernel, the N bookkeeping, the methylation edges and the
    transcript rules that the drawn cases are there to reach.  A draw that stops reaching one fails here, on the CPU"""
    clean = {(s, p): set() for s in "+-" for p in (False, True)}
    with_N, clipped = set(), set()
    tail_N = cross64 = M_first = M_last = 0
    rna_N = cdna_minus_N = trunc_pos = trunc_N = short_in_table = at_bound = 0
    slowest = (0.0, None)
    variants = set()
    for seed in SEEDS:
        cs = SC.case(seed)
        reads, dt = SC.oracle_reads(cs, tmp_path)
        slowest = max(slowest, (dt, seed))
        fc = SC.facts(cs, reads)
        variants.add((cs.f, cs.profile))
        assert not SC.missing_in_case(fc), f"{cs.describe()}: lacks {SC.missing_in_case(fc)}"
        if cs.rejecting:                                    # the genome's share, not the outcome: at most a fifth of the bases can start a read
            assert sum(len(c) for c in cs.contigs if len(c) >= 200) <= 0.2 * sum(len(c) for c in cs.contigs)
        for s, m in fc["clean_mod8"]:
            clean[(s, cs.prefix)].add(m)
        with_N |= {(s, cs.prefix) for s in fc["with_N"]}
        at_bound += fc["at_bound"]
        tail_N += fc["tail_N"]; cross64 += fc["cross64"]; M_first += fc["M_first"]; M_last += fc["M_last"]
        if cs.f < 5:
            clipped |= fc["clipped"]
        else:
            rna_N += bool(fc["with_N"])
            cdna_minus_N += fc["minus_N"] if cs.f in (8, 9) else 0
            trunc_pos += fc["trunc_pos"] if cs.f in (7, 9) else 0
            trunc_N += fc["trunc_N"] if cs.f in (7, 9) else 0
            short_in_table += fc["short_in_table"] and fc["n_reads"] > 0
    print(f"slowest case for the oracle: seed {slowest[1]}, {slowest[0]:.2f} s")
    assert {f for f, _ in variants} == set(range(10)) and (0, "dna-r10-prom") in variants and (1, "dna-r10-prom") in variants
    for key, mods in clean.items():
        assert mods == set(range(8)), f"reads without N, (strand, prefix) {key}: rlen % 8 takes {sorted(mods)} only"
    assert with_N == {(s, p) for s in "+-" for p in (False, True)}, with_N
    assert tail_N > 0 and cross64 > 0 and at_bound > 0
    assert clipped == {"+", "-"}
    assert rna_N > 0 and cdna_minus_N > 0 and trunc_pos > 0 and trunc_N > 0 and short_in_table > 0
    assert M_first > 0 and M_last > 0


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_drawn_contexts_match_the_oracle(seed, tmp_path):
    """a drawn context through test_sampler._run: coordinates, ref_len, sequence, every int16, every dwell, offset and median_before of every
    read.  On an MI355X, the oracle's share included: median 0.10 s, slowest 0.52 s (seed 37), 8 s for the 60 seeds"""
    cs = SC.case(seed)
    t0 = time.perf_counter()
    n = _run(**cs.files(tmp_path))
    print(f"{cs.describe()}: {n} reads, {time.perf_counter() - t0:.2f} s with the oracle")


# ---- planted cases ---------------------------------------------------------------------------------------------------------------------

def _write(path, contigs):
    path.write_text("".join(f">c{i}\n{c.decode()}\n" for i, c in enumerate(contigs)))
    return str(path)


def _clean(rng, n):
    return bytes(rng.choice(list(b"ACGT"), n).astype(np.uint8))


@pytest.mark.gpu
def test_a_draw_above_the_abundance_table_falls_back_to_the_first_transcript(tmp_path):
    """get_transcript_idx, src/genread.c:283-300: seq_i stays 0 where the uniform exceeds the table's last cumulative value.  The table is
    scaled to end at 0.6 and does not name transcript 0 at all: every read of transcript 0 is the fall-back"""
    rng = np.random.default_rng(5)
    contigs = [_clean(rng, n) for n in (300, 400, 260, 700, 210)]
    fa = _write(tmp_path / "t.fa", contigs)
    tc = tmp_path / "t.tsv"
    tc.write_text("c3\t10\nc1\t25\nc4\t10\nc2\t5\n")
    reads = []
    _run("rna004-prom", 9, fa, 3, [9, 60, 7], rlen=10000, mode=api.SAMPLE_RNA, trans_count=str(tc), trans_scale=0.6, reads_out=reads)
    idx = [w.ref_idx for bt in reads for w in bt]
    assert idx.count(0) >= 10, "the oracle's own reads: transcript 0 has no weight in the table, four draws in ten lie above it"


def _unusable(kind, rng):
    if kind == "short":                                        # every contig below 200 nt (src/genread.c:126)
        return [_clean(rng, int(n)) for n in rng.integers(150, 200, 9)]
    out = []                                                   # N at every fifth base or denser (src/genread.c:139-142)
    for n in (200, 450, 3000):
        a = np.frombuffer(_clean(rng, n), np.uint8).copy()
        a[int(rng.integers(0, 5))::5] = ord("N")
        a[rng.random(n) < 0.05] = ord("N")
        out.append(bytes(a))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("kind,T,n", [("short", 2, 2), ("short", 1, 16), ("dense_N", 2, 2), ("dense_N", 1, 16)],
                         ids=["short_contigs-chains_of_1", "short_contigs-chain_of_16", "dense_N-chains_of_1", "dense_N-chain_of_16"])
def test_an_unusable_genome_is_an_error_and_the_context_goes_on(kind, T, n, tmp_path):
    """100001 rejected attempts in a row: SQG_EINVAL naming them (k_sample; k_sample_try / k_sample_pick from 16 reads a worker on).  The
    error word is cleared and the workers' scalar streams are where they were: the same context, given a usable genome, makes the reads of
    an oracle that never saw the failed call"""
    rng = np.random.default_rng(17)
    prof, fl = profiles.get_profile("dna-r9-prom")
    mean, stdv = model.synthetic_model(6)
    good = [_clean(rng, 900), _clean(rng, 2500)]
    orac = orc.Oracle(prof, fl, 6, mean, stdv, 23, num_workers=T, rlen=400)
    good = _contigs(orac.load_ref(_write(tmp_path / "good.fa", good)))
    gen = api.SignalGenerator(prof, fl, 6, mean, stdv, 23, num_workers=T, mode=api.MODE_CERTIFIED)
    gen.load_genome(_unusable(kind, rng), 400)
    t0 = time.perf_counter()
    with pytest.raises(api.SqgError) as e:
        gen.sample(n)
    print(f"{kind}, T = {T}, {n} reads: the refused call took {time.perf_counter() - t0:.2f} s")
    assert e.value.code == -1 and "100000 attempts" in str(e.value)
    gen.load_genome(good, 400)
    for nb in (5, 20):
        b = gen.sample(nb).run().wait()
        _compare(b, orac.run_batch(nb))
        b.free()
    gen.close(); orac.close()


@pytest.mark.gpu
def test_full_contigs_go_on_after_the_refused_call(tmp_path):
    """--full-contigs: seven contigs, five handed out, sample(3) refused -- sample(2) then gives the two left, as the oracle's sixth and
    seventh read: full_next and the scalar streams were put back"""
    rng = np.random.default_rng(4)
    contigs = [bytes(rng.choice(list(b"ACGTacgtN"), n).astype(np.uint8)) for n in (700, 5, 2600, 64, 1300, 900, 3)]
    prof, fl = profiles.get_profile("dna-r9-prom")
    mean, stdv = model.synthetic_model(6)
    orac = orc.Oracle(prof, fl | profiles.SQ_FULL_CONTIG, 6, mean, stdv, 1, num_workers=2)
    contigs = _contigs(orac.load_ref(_write(tmp_path / "g.fa", contigs)))
    gen = api.SignalGenerator(prof, fl, 6, mean, stdv, 1, num_workers=2, mode=api.MODE_CERTIFIED)
    gen.load_genome(contigs, 10000, api.SAMPLE_FULL)
    b = gen.sample(5).run().wait()
    _compare(b, orac.run_batch(5))
    b.free()
    with pytest.raises(api.SqgError) as e:
        gen.sample(3)                                        # two contigs left
    assert e.value.code == -1 and "contigs left" in str(e.value)
    b = gen.sample(2).run().wait()
    want = orac.run_batch(2)
    assert [w.ref_idx for w in want] == [5, 6]
    _compare(b, want)
    b.free()
    gen.close(); orac.close()


@pytest.mark.gpu
def test_a_call_refused_for_its_arguments_between_good_ones(tmp_path):
    """two batches, a call whose `workers` names a worker outside the context, a third batch: the oracle's third"""
    rng = np.random.default_rng(8)
    prof, fl = profiles.get_profile("dna-r9-prom")
    mean, stdv = model.synthetic_model(6)
    T = 3
    orac = orc.Oracle(prof, fl, 6, mean, stdv, 77, num_workers=T, rlen=500)
    contigs = _contigs(orac.load_ref(_write(tmp_path / "g.fa", [_clean(rng, 3000), _clean(rng, 800)])))
    gen = api.SignalGenerator(prof, fl, 6, mean, stdv, 77, num_workers=T, mode=api.MODE_CERTIFIED)
    gen.load_genome(contigs, 500)
    for nb in (7, 51):
        b = gen.sample(nb).run().wait()
        _compare(b, orac.run_batch(nb))
        b.free()
    with pytest.raises(api.SqgError) as e:
        gen.sample(4, workers=np.array([0, 1, T, 2], np.int32))
    assert e.value.code == -1
    b = gen.sample(9).run().wait()
    _compare(b, orac.run_batch(9))
    b.free()
    gen.close(); orac.close()
