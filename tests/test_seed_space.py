"""Seeding and the Lehmer generator outside the canonical seed range [1, M), M = 2^31 - 1 (tests/seed_cases.py).

The library reduces `seed + w*(num_kmer + 10) + j` mod M in six places -- k_init_rows, canon() (seed_base / seed_step, the time and
methylation streams), the count rows of k_events, the bucketed hand-out of k_part.h, k_init_sampler, and the host draws of offset /
median_before, which keep the reference's uncorrected form -- and admits |seed| + T*(num_kmer + 10) <= 9.0e10.  Here every one of
them runs on seeds at and above M, negative seeds, rows that cross M in the middle, and the zero stream (a seed that is 0 mod M: the
state stays 0, u = 1.0, every draw is the mean exactly); bit for bit against the oracle, which tests/test_oracle_vs_ref.py pins to
the compiled reference on the seed_* vectors."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import orc
import seed_cases as sc
from refvec_cases import SEED_CASES
from squigulator_amd import api, model, profiles

MODES = ((api.MODE_CERTIFIED, "certified"), (api.MODE_EXACT, "exact"))


# ---- CPU: the bound, and the zero stream in the oracle ------------------------------------------------------------------------------

def _canonical_step(x):
    c = sc.LCG_A * x % sc.M
    return c if c else sc.M


def _all_table_seeds():
    out = set()
    for T, nk in ((1, 4 ** 6), (4, 4 ** 6), (3, 4 ** 9), (2, 4 ** 9), (2, 5 ** 6), (2, 5 ** 7)):
        out.update(s for _, s in sc.seed_table(T, nk))
    return sorted(out)


def test_schrage_step_is_canonical_exactly_below_the_bound():
    """rng() of src/rand.h:79-85 with C's truncating / and %: its corrected value is 16807 x mod M (0 written as M) for every seed of
    the table and up to |x| = 96 752 654 378; at 96 752 654 379 the uncorrected state leaves (-M, M) and it is not"""
    for x in _all_table_seeds():
        for d in (0, 1, 2, 6, 4 ** 9 - 1):                           # (the seed itself and streams of its first row)
            assert sc.ref_rng(x + d)[1] == _canonical_step(x + d), x + d
    assert sc.VALID_BELOW == 96752654379 and sc.ADMITTED < sc.VALID_BELOW
    for x in (sc.VALID_BELOW - 1, -(sc.VALID_BELOW - 1), sc.ADMITTED + 6, -(sc.ADMITTED + 6)):
        nx, pos = sc.ref_rng(x)
        assert -sc.M < nx < sc.M and pos == _canonical_step(x), x
    for x in (sc.VALID_BELOW, -sc.VALID_BELOW):
        assert sc.ref_rng(x)[1] != _canonical_step(x), x
    assert sc.ref_rng(sc.VALID_BELOW) == (-sc.M - 781, -781)        # the first state that one correction does not bring back
    # two steps: the uncorrected state of a valid seed is itself a valid input (|nx| < M)
    rng = np.random.default_rng(1)
    for x in rng.integers(-sc.ADMITTED, sc.ADMITTED, 2000):
        nx, pos = sc.ref_rng(int(x))
        assert sc.ref_rng(nx)[1] == _canonical_step(pos)


def test_oracle_rng_is_the_restated_step():
    L = orc.lib()
    for x in _all_table_seeds() + [sc.VALID_BELOW - 1, -(sc.VALID_BELOW - 1)]:
        st = C.c_int64(x)
        u = L.orc_rng(C.byref(st))
        nx, pos = sc.ref_rng(x)
        assert st.value == nx and u == pos / 2147483647


def test_helpers():
    assert sc.canon(-1) == sc.M - 1 and sc.canon(sc.M) == 0 and sc.canon(2 ** 33) == 4
    assert sc.zero_rank(-2, 0, 4096) == 2 and sc.zero_rank(sc.M, 0, 4096) == 0 and sc.zero_rank(sc.M + 5, 0, 4096) is None
    assert sc.zero_rank(42, 8191, 4 ** 9) == 180191 and sc.zero_rank(42, 8190, 4 ** 9) is None       # --seed 42, R10 table: worker 8191
    assert sc.zero_rank(-2147483648, 0, 4096) == 1
    assert sc.kmer_of(180191, 9, False) == model.kmer_string(180191, 9).encode()
    assert sc.kmer_of(3 * 25 + 4, 3, True) == b"MAT"
    L = orc.lib()
    rng = np.random.default_rng(0)
    for k, meth, rank in ((6, False, 1365), (9, False, 180191), (6, True, 5 ** 6 // 3), (7, True, 5 ** 7 // 2)):
        kmer = sc.kmer_of(rank, k, meth)
        assert (L.orc_meth_kmer_rank if meth else L.orc_kmer_rank)(kmer, k) == rank
        read, hits = sc.planted(k, kmer, 40 * (k + 3), rng)
        assert len(hits) >= 40 and all(read[h:h + k] == kmer for h in hits)
        placed = [h for h in hits if all(abs(h - g) >= k for g in hits if g != h)]
        assert len(placed) >= 40 or len(set(kmer)) < k            # (a k-mer with a period may also overlap a chance copy)
    for i, n, T in ((0, 11, 3), (4, 11, 3), (10, 11, 3), (5, 6, 1)):
        assert sc.worker_of(i, n, T) == L.orc_worker_of(i, n, T)


def _c_round(x):
    return math.floor(x + 0.5) if x >= 0 else -math.floor(-x + 0.5)


def test_oracle_zero_time_stream_draws_the_mean_dwell():
    """seed -2: worker 0's rand_time (s + 2) is the zero stream -- every dwell is round(dwell_mean); worker 1's is not"""
    prof, fl = profiles.get_profile("dna-r9-prom")
    prof = prof.replace(dwell_mean=8.6)
    mean, stdv = model.synthetic_model(6)
    rng = np.random.default_rng(2)
    seqs = [bytes(rng.choice(list(b"ACGT"), 400).astype(np.uint8)) for _ in range(2)]
    orac = orc.Oracle(prof, fl, 6, mean, stdv, -2, num_workers=2)
    for _ in range(2):
        r = orac.run_batch_seqs(seqs)
        assert (r[0].ss == 9).all() and _c_round(prof.dwell_mean) == 9
        assert len(set(r[1].ss.tolist())) > 3
    orac.close()


def _event_starts(ss):
    st = np.zeros(len(ss) + 1, np.int64)
    st[1:] = np.cumsum(ss)
    return st


def _assert_planted(sig, ss, hits, expect, rna, what):
    """every sample of the events `hits` is `expect`; -> how many samples that is.  sig: the read's stored samples (RNA: reversed)"""
    gen_order = sig[::-1] if rna else sig
    st = _event_starts(ss)
    n = 0
    for h in hits:
        got = gen_order[st[h]:st[h + 1]]
        assert (got == expect).all(), f"{what}: event {h} of the zero stream holds {got[:8]}, not {expect}"
        n += len(got)
    return n


@pytest.mark.parametrize("name,k,sflags,seed", [("dna-r9-prom", 6, 0, sc.M), ("dna-r9-prom", 6, 0, -(4 ** 6 // 3)), ("dna-r10-prom", 9, 0, sc.M - 4 ** 9 // 2),
                                                ("dna-r9-prom", 6, profiles.SQ_METH, -(5 ** 6 // 3)), ("rna004-prom", 9, profiles.SQ_PREFIX, -1)],
                         ids=["k6_M", "k6_-nk/3", "k9_M-nk/2", "meth_k6_-nk/3", "rna004_prefix_-1"])
def test_oracle_zero_kmer_stream_is_the_closed_form(name, k, sflags, seed):
    """every sample of an event on the zero k-mer stream is to_i16((double)level_mean * dig / range - offset): stated without the oracle"""
    prof, fl = profiles.get_profile(name)
    fl |= sflags
    meth = bool(sflags & profiles.SQ_METH)
    mean, stdv = model.synthetic_model(k, meth=meth)
    j0 = sc.zero_rank(seed, 0, len(mean))
    assert j0 is not None
    rng = np.random.default_rng(3)
    orac = orc.Oracle(prof, fl, k, mean, stdv, seed, num_workers=1)
    for _ in range(2):
        read, hits = sc.planted(k, sc.kmer_of(j0, k, meth), 40 * (k + 3), rng)
        r = orac.run_batch_seqs([read])[0]
        n = _assert_planted(r.sig, r.ss, hits, sc.zero_stream_sample(mean[j0], prof, r.offset), bool(fl & profiles.SQ_RNA), "oracle")
        assert n >= 40
    orac.close()


# ---- GPU: the signal path on every regime, against the oracle ------------------------------------------------------------------------

_JOBS = {}                      # the most recent cases: the regimes that differ in the library's path alone share the oracle's run


def _job(name, k, T, seed, n_reads, sflags=0, dwell_mean=None, n_batches=2, lens=(300, 2000)):
    """the batches of a case and the oracle's results, computed once per case and shared by the tests that run it.
    -> dict(prof, flags, mean, stdv, batches, want, plants); plants[b]: [(read index, rank, event indices)] of batch b"""
    key = (name, k, T, seed, n_reads, sflags, dwell_mean, n_batches, lens)
    if key in _JOBS:
        return _JOBS[key]
    prof, fl = profiles.get_profile(name)
    fl |= sflags
    if dwell_mean is not None:
        prof = prof.replace(dwell_mean=float(dwell_mean))
    meth = bool(sflags & profiles.SQ_METH)
    mean, stdv = model.synthetic_model(k, meth=meth)
    nk = len(mean)
    rng = np.random.default_rng([k, T, n_reads, sflags, abs(seed) % 1000003])
    letters = list(b"ACGTM" if meth else b"ACGT")
    batches, plants = [], []
    for _ in range(n_batches):
        bt = [bytes(rng.choice(letters, int(m)).astype(np.uint8)) for m in rng.integers(lens[0], lens[1], n_reads)]
        pl = []
        for w in range(T):
            j0 = sc.zero_rank(seed, w, nk)
            if j0 is None:
                continue
            i = next(i for i in range(n_reads) if sc.worker_of(i, n_reads, T) == w)      # the planted read goes to the worker that owns the stream
            bt[i], hits = sc.planted(k, sc.kmer_of(j0, k, meth), max(lens[0], 40 * (k + 3)), rng)
            pl.append((i, j0, hits))
        batches.append(bt)
        plants.append(pl)
    orac = orc.Oracle(prof, fl, k, mean, stdv, seed, num_workers=T)
    want = [orac.run_batch_seqs(bt) for bt in batches]
    orac.close()
    # a zero time stream: the worker's dwells are all round(dwell_mean) -- asserted on the oracle here, the HIP path must equal it
    if not (fl & (profiles.SQ_IDEAL | profiles.SQ_IDEAL_TIME)):
        for w in range(T):
            if sc.canon(sc.stream_seed(seed, w, nk, 2)) == 0:
                for wt in want:
                    for i, r in enumerate(wt):
                        if sc.worker_of(i, n_reads, T) == w:
                            assert (r.ss == _c_round(prof.dwell_mean)).all()
    job = dict(prof=prof, flags=fl, mean=mean, stdv=stdv, batches=batches, want=want, plants=plants, k=k, T=T, seed=seed)
    if dwell_mean is None:
        while len(_JOBS) >= 48:
            del _JOBS[next(iter(_JOBS))]
        _JOBS[key] = job
    return job


def _check_batch(job, b, bi, what, fallback=None):
    sig, dw = b.signal(), b.dwell()
    rna = bool(job["flags"] & profiles.SQ_RNA)
    for i, w in enumerate(job["want"][bi]):
        np.testing.assert_array_equal(dw[b.ev_off[i]:b.ev_off[i + 1]], w.ss, err_msg=f"{what} batch {bi} read {i} (dwell)")
        np.testing.assert_array_equal(sig[b.sig_off[i]:b.sig_off[i + 1]], w.sig, err_msg=f"{what} batch {bi} read {i}")
        assert b.offset[i] == w.offset and b.median_before[i] == w.median_before, f"{what} batch {bi} read {i}: offset / median_before"
    n_planted = 0
    for i, j0, hits in job["plants"][bi]:
        expect = sc.zero_stream_sample(job["mean"][j0], job["prof"], b.offset[i])
        n_planted += _assert_planted(sig[b.sig_off[i]:b.sig_off[i + 1]], dw[b.ev_off[i]:b.ev_off[i + 1]], hits, expect, rna, f"{what} batch {bi} read {i}")
    if fallback is not None and job["plants"][bi]:
        # the witness that the fp32 path met c1 = 0 (box_muller_fast(0) = +inf) and rejected it: every such sample went to the FP64 path
        assert fallback >= n_planted > 0, f"{what} batch {bi}: {fallback} samples fell back, the zero streams alone hold {n_planted}"


def _run(job, cfg_flags=0, streamed=False, what=""):
    prof, fl, k, T, seed = job["prof"], job["flags"] | cfg_flags, job["k"], job["T"], job["seed"]
    batches = job["batches"]
    for mode, mname in MODES:
        tag = f"{what} seed {seed} {mname}"
        gen = api.SignalGenerator(prof, fl, k, job["mean"], job["stdv"], seed, num_workers=T, mode=mode)
        if not streamed:
            for bi, bt in enumerate(batches):
                b = gen.submit(bt)
                fb = gen.timing()["fallback_samples"] if mode == api.MODE_CERTIFIED and not (fl & (profiles.SQ_IDEAL | profiles.SQ_IDEAL_AMP)) else None
                _check_batch(job, b, bi, tag, fb)
                b.free()
        else:
            # batch i+2 staged, batch i+1 queued, batch i consumed: every run finds its successor staged, whose count pass then rides
            # along with this batch's hand-out (k_part_hand_count)
            carried = 0
            cur = gen.stage(batches[0]).run()
            nxt = gen.stage(batches[1])
            for bi in range(len(batches)):
                nn = gen.stage(batches[bi + 2]) if bi + 2 < len(batches) else None
                if nxt is not None:
                    nxt.run()
                cur.wait()
                carried += gen.timing()["carried_first_pass"]
                _check_batch(job, cur, bi, tag + " streamed")
                cur.free()
                cur, nxt = nxt, nn
            assert carried >= 1, f"{tag}: no batch carried its successor's count pass"
        gen.close()


# (name, k, T, reads per batch, SQG_SPLIT_CHAINS or None, cfg flags, streamed, flags of the simulation); the few-worker 9-mer regimes
# run the same three batches, so that one oracle run serves the three of a seed
REGIMES = {
    "k6_tk": ("dna-r9-prom", 6, 4, 4, None, 0, False, 0),                     # k_events, rows as states (k_init_rows)
    "k6_t1_cut": ("dna-r9-prom", 6, 1, 5, "7", 0, False, 0),                  # cut chains, one partition
    "k6_t3_cut": ("dna-r9-prom", 6, 3, 11, "7", 0, False, 0),
    "k9_tk": ("dna-r10-prom", 9, 3, 3, None, 0, False, 0),                    # k_events, count rows
    "k9_t1": ("dna-r10-prom", 9, 1, 5, "7", 0, False, 0),                     # bucketed hand-out (k_part_hand_ord)
    "k9_t2": ("dna-r10-prom", 9, 2, 7, "7", 0, False, 0),
    "k9_t1_order_free": ("dna-r10-prom", 9, 1, 5, "7", profiles.SQ_ORDER_FREE, False, 0),
    "k9_t2_order_free": ("dna-r10-prom", 9, 2, 7, "7", profiles.SQ_ORDER_FREE, False, 0),
    "k9_t1_streamed": ("dna-r10-prom", 9, 1, 5, "7", 0, True, 0),             # k_part_hand_count carries the next batch's count pass
    "k9_t2_streamed": ("dna-r10-prom", 9, 2, 7, "7", 0, True, 0),
}
METH_REGIMES = {
    "meth_k6_tk": ("dna-r9-prom", 6, 3, 3, None, 0, False, profiles.SQ_METH),      # 5^6 > 4096 streams: count rows
    "meth_k6_t2": ("dna-r9-prom", 6, 2, 7, "7", 0, False, profiles.SQ_METH),       # 4 partitions
    "meth_k7_t2": ("dna-r10-prom", 7, 2, 7, "7", 0, False, profiles.SQ_METH),      # 20 partitions, the last one ragged
}
RNA_REGIME = ("rna004-prom", 9, 2, 5, "7", 0, False, profiles.SQ_PREFIX)


def _nk(k, sflags):
    return 5 ** k if sflags & profiles.SQ_METH else 4 ** k


def _table_cases():
    out = []
    for rid, (name, k, T, n, links, cfg, streamed, sflags) in REGIMES.items():
        seen = set()
        for sid, seed in sc.seed_table(T, _nk(k, sflags)):
            if seed in seen:                                     # (2147483647 is M: one run)
                continue
            seen.add(seed)
            out.append(pytest.param(rid, seed, id=f"{rid}-{sid}"))
    for rid, (name, k, T, n, links, cfg, streamed, sflags) in METH_REGIMES.items():
        nk = _nk(k, sflags)
        for sid, seed in (("M-nk/2", sc.M - nk // 2), ("-nk/3", -(nk // 3)), ("+admitted", sc.largest_admitted(T, nk))):
            out.append(pytest.param(rid, seed, id=f"{rid}-{sid}"))
    for sid, seed in (("M-nk/2", sc.M - 4 ** 9 // 2), ("-1", -1)):
        out.append(pytest.param("rna004_prefix_t2", seed, id=f"rna004_prefix_t2-{sid}"))
    return out


def _regime(rid):
    return RNA_REGIME if rid == "rna004_prefix_t2" else {**REGIMES, **METH_REGIMES}[rid]


@pytest.mark.gpu
@pytest.mark.parametrize("rid,seed", _table_cases())
def test_signal_path_matches_oracle_at_off_range_seeds(rid, seed, monkeypatch):
    """two or three batches per context (the carried states count), both arithmetic modes; where a worker owns a zero k-mer stream, a
    read planted on that k-mer goes to it: its events hold the closed form, and in certified mode they all fell back to FP64"""
    name, k, T, n, links, cfg, streamed, sflags = _regime(rid)
    if links:
        monkeypatch.setenv("SQG_SPLIT_CHAINS", links)
    job = _job(name, k, T, seed, n, sflags=sflags, n_batches=3 if rid.startswith(("k9_t1", "k9_t2")) else 2)
    _run(job, cfg_flags=cfg, streamed=streamed, what=rid)


def _zero_cases():
    """every (regime, seed) of the table in which some worker owns a zero k-mer stream; streamed runs excepted (their fall-back counts
    are gone by the time the batch is consumed, and the kernels are those of the plain run)"""
    out = []
    for p in _table_cases():
        rid, seed = p.values
        name, k, T, n, links, cfg, streamed, sflags = _regime(rid)
        if not streamed and any(sc.zero_rank(seed, w, _nk(k, sflags)) is not None for w in range(T)):
            out.append(pytest.param(rid, seed, id=p.id))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("rid,seed", _zero_cases())
def test_zero_streams_in_events_longer_than_512_samples(rid, seed, monkeypatch):
    """dwell_mean = 600: events longer than 512 samples go through k_samples<..., GENERIC>; the same three assertions"""
    name, k, T, n, links, cfg, streamed, sflags = _regime(rid)
    if links:
        monkeypatch.setenv("SQG_SPLIT_CHAINS", links)
    job = _job(name, k, T, seed, n, sflags=sflags, dwell_mean=600, lens=(300, 500))
    assert any(job["plants"][0])
    _run(job, cfg_flags=cfg, what=rid + " dwell 600")


@pytest.mark.gpu
def test_zero_time_stream_draws_the_mean_dwell_on_the_device():
    """seed -2: worker 0's dwells are all round(dwell_mean), with the chain walked by k_events (T = K) and cut into links (T = 1)"""
    for rid in ("k6_tk", "k9_tk"):
        name, k, T, n, links, cfg, streamed, sflags = REGIMES[rid]
        job = _job(name, k, T, -2, n)
        assert sc.canon(sc.stream_seed(-2, 0, 4 ** k, 2)) == 0
        for mode, mname in MODES:
            gen = api.SignalGenerator(job["prof"], job["flags"], k, job["mean"], job["stdv"], -2, num_workers=T, mode=mode)
            for bt in job["batches"]:
                b = gen.submit(bt)
                dw = b.dwell()
                d0 = dw[b.ev_off[0]:b.ev_off[1]]
                assert (d0 == _c_round(job["prof"].dwell_mean)).all(), f"{rid} {mname}: {np.unique(d0)}"
                assert len(np.unique(dw[b.ev_off[1]:b.ev_off[2]])) > 3
                b.free()
            gen.close()


@pytest.mark.gpu
def test_a_shard_far_up_the_worker_range_crosses_M():
    """--seed 42, the R10 table, T = K: worker 8191's stream 180191 has seed exactly M and every later worker's seeds are above it.
    Workers [8190, 8194) of a 300000-worker job equal a 4-worker oracle seeded 42 + 8190 * 262154; worker 8191's read is planted"""
    prof, fl = profiles.get_profile("dna-r10-prom")
    k, nk, lo = 9, 4 ** 9, 8190
    mean, stdv = model.synthetic_model(k)
    assert sc.zero_rank(42, 8191, nk) == 180191 and sc.stream_seed(42, 8191, nk, 180191) == sc.M
    rng = np.random.default_rng(8191)
    batches, plants = [], []
    for _ in range(2):
        bt = [bytes(rng.choice(list(b"ACGT"), int(m)).astype(np.uint8)) for m in rng.integers(300, 2000, 4)]
        bt[1], hits = sc.planted(k, sc.kmer_of(180191, k, False), 600, rng)
        batches.append(bt)
        plants.append([(1, 180191, hits)])
    orac = orc.Oracle(prof, fl, k, mean, stdv, 42 + lo * (nk + 10), num_workers=4)
    want = [orac.run_batch_assigned(bt, range(4)) for bt in batches]
    orac.close()
    job = dict(prof=prof, flags=fl, mean=mean, stdv=stdv, batches=batches, want=want, plants=plants)
    for mode, mname in MODES:
        gen = api.SignalGenerator(prof, fl, k, mean, stdv, 42, num_workers=300000, mode=mode, worker_lo=lo, worker_hi=lo + 4)
        for bi, bt in enumerate(batches):
            b = gen.submit(bt, workers=range(lo, lo + 4))
            _check_batch(job, b, bi, f"shard {mname}", gen.timing()["fallback_samples"] if mode == api.MODE_CERTIFIED else None)
            b.free()
        gen.close()


# ---- GPU: the sampler (k_init_sampler, the methylation stream's canon(s + 6)) and range sharding ------------------------------------
# No seed here makes a worker's s or s + 3 zero (mod M): see tests/refvec_cases.py

@pytest.mark.gpu
@pytest.mark.parametrize("seed", [sc.M + 5, -1, -4, 2 ** 33, sc.largest_admitted(2, 4 ** 6)], ids=["M+5", "-1", "-4", "2^33", "+admitted"])
def test_sampler_at_off_range_seeds(seed):
    import test_sampler
    test_sampler._run("dna-r9-prom", 6, test_sampler.NCOV, 2, [4, 4], rlen=1000, seed=seed)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [-6, sc.M - 3000], ids=["-6", "M-3000"])
def test_sampler_methylation_stream_at_off_range_seeds(seed):
    """-6: rand_meth (s + 6) of worker 0 is the zero stream -- u = 1.0, no CpG is ever methylated; M - 3000: the 5^6 row crosses M"""
    import test_sampler
    test_sampler._run("dna-r9-prom", 6, test_sampler.NCOV, 2, [4, 4], rlen=1000, seed=seed, meth_freq=test_sampler.MFREQ_DENSE)


@pytest.mark.gpu
def test_sampler_long_chain_jumps_from_an_off_range_origin():
    """k_sample_try / k_sample_pick: attempt a of a chain is the origin advanced by a fixed number of draws"""
    import test_sampler
    test_sampler._run("dna-r9-prom", 6, test_sampler.NCOV, 1, [40, 25], rlen=800, seed=-1000)


@pytest.mark.gpu
def test_range_sharding_on_a_row_that_crosses_M():
    """G = 2 ranks, the 9-mer table at M - nk/2: sqg_skip_reads and the count exchange on a wrapped row"""
    import test_range_sharding
    import test_sampler
    test_range_sharding._run("dna-r10-prom", test_sampler.NCOV, 1, 2, [6, 5], rlen=700, seed=sc.M - 4 ** 9 // 2)


# ---- GPU: the compiled reference's vectors at off-range seeds ------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("mode", [api.MODE_EXACT, api.MODE_CERTIFIED], ids=["exact", "certified"])
@pytest.mark.parametrize("cid,cmd", SEED_CASES, ids=[c[0] for c in SEED_CASES])
def test_hip_matches_reference_vectors_at_off_range_seeds(cid, cmd, mode):
    import hiprun
    import test_hip_parity as thp
    v = np.load(os.path.join(thp.VEC, cid + ".npz"))
    assert str(v["cmd"]) == cmd
    want = thp._fixture_reads(v)
    got = hiprun.run_hip_on_reads(cmd, [w["seq"] for w in want], mode=mode)
    thp._compare(got, want, cid)


# ---- GPU: what sqg_create admits ---------------------------------------------------------------------------------------------------------

def _create(seed, T, k=6, flags=0, mode=api.MODE_EXACT):
    prof, fl = profiles.get_profile("dna-r9-prom")
    mean, stdv = model.synthetic_model(k, meth=bool(flags & profiles.SQ_METH))
    return api.SignalGenerator(prof, fl | flags, k, mean, stdv, seed, num_workers=T, mode=mode, worker_lo=0, worker_hi=min(T, 2))


@pytest.mark.gpu
@pytest.mark.parametrize("k,flags,T", [(6, 0, 2), (9, 0, 300000), (6, profiles.SQ_METH, 7)], ids=["k6_t2", "k9_t300000", "meth_k6_t7"])
def test_create_admits_up_to_9e10_and_refuses_one_worker_row_more(k, flags, T):
    nk = _nk(k, flags)
    big = sc.largest_admitted(T, nk)
    assert big + T * (nk + 10) == sc.ADMITTED == 9.0e10
    for seed in (big, -big):
        _create(seed, T, k, flags).close()
        for s2, T2 in ((seed, T + 1), (seed + (nk + 10) * (1 if seed > 0 else -1), T), (seed + (1 if seed > 0 else -1), T)):
            with pytest.raises(api.SqgError) as e:
                _create(s2, T2, k, flags)
            assert e.value.code == -1, (s2, T2)


@pytest.mark.gpu
@pytest.mark.parametrize("sign", [1, -1], ids=["+", "-"])
def test_the_admitted_extreme_equals_the_oracle(sign, monkeypatch):
    """two small batches at |seed| + T * (nk + 10) = 9.0e10, few workers over cut chains: offset and median_before are drawn on the
    host in the reference's uncorrected form from s + 4 and s + 5, the streams nearest to the bound"""
    monkeypatch.setenv("SQG_SPLIT_CHAINS", "7")
    _run(_job("dna-r9-prom", 6, 2, sign * sc.largest_admitted(2, 4 ** 6), 7), what="admitted extreme")      # (k = 9: the k9_t2 cases of the table)


@pytest.mark.gpu
def test_seed_zero_is_a_seed_like_any_other():
    """include/sqg.h: cfg.seed = 0 is taken as it is (replacing 0 by the time of day is the reference CLI's business).  Worker 0's
    stream of rank 0 -- AAAAAA -- is then the zero stream"""
    assert sc.zero_rank(0, 0, 4 ** 6) == 0
    job = _job("dna-r9-prom", 6, 2, 0, 2)
    assert job["plants"][0] and job["plants"][0][0][:2] == (0, 0)
    _run(job, what="seed 0")
