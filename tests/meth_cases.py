"""Cases for the 5-letter (A C G M T) methylation tables on the cut-chain paths (tests/test_meth_paths.py): a seeded generator in
the style of test_fuzz_parity._few_case, one planted read per case, the witnesses of what a case covers -- computed on the CPU from
the reads alone --, and the harness that drives a job through whichever library and compares it with the oracle.  Not collected.

Under SQG_METH the table has 5^k rows: the bucketed hand-out (k_part.h) then runs over 4 partitions of 4096 streams at k = 6
(15625 = 3*4096 + 3337) and over 20 at k = 7 (78125 = 19*4096 + 301), the last one ragged; k = 5, 8, 9 take the per-link rows."""
import functools
import re
from collections import namedtuple

import numpy as np

import orc
from squigulator_amd import api, model, profiles

KS = (5, 6, 7, 8, 9)
# (the flag sets cycle with seed // 5, so that every k meets every one of them.  The last two switch the amplitude noise off: such a context
# has no k-mer streams to hand out, and the library leaves its chains uncut whatever is asked for -- has_streams())
FLAG_SETS = [0, profiles.SQ_PREFIX, profiles.SQ_IDEAL_TIME, profiles.SQ_PREFIX | profiles.SQ_IDEAL_TIME, profiles.SQ_IDEAL_AMP, profiles.SQ_IDEAL]
PART_SUB = 4096                                            # streams per partition of the bucketed hand-out (k_part.h)
DNA_PREFIX = 24 + 61                                       # --prefix=yes on DNA: stall + adaptor bases in front of the read (src/genread.c:38,110)
LENGTHS = lambda k: [1, k - 1, k, k + 1, 64, 65, 300, 511, 512, 513, 1023, 1024, 1025, 1600, 2100]   # noqa: E731
LETTERS = list(b"ACGTMacgtmNRY")
LETTER_P = [.2] * 4 + [.165] + [.004] * 4 + [.007] + [.004] * 3     # M about one base in six; a few percent of acgt, m, N, R, Y

Case = namedtuple("Case", "seed prof flags k T ctx_seed batches links")


def has_streams(flags):
    """amplitude noise on: the per-k-mer streams exist, and a few-worker batch's chains are cut so that they can be handed out"""
    return not flags & (profiles.SQ_IDEAL | profiles.SQ_IDEAL_AMP)


def n_part(k):
    return (5 ** k + PART_SUB - 1) // PART_SUB


# ---- ranks, stated here on their own: base-5 digits A C G M T, first base most significant; anything else counts as A
_DIGIT = np.zeros(256, np.int64)
for _d, _ch in enumerate(b"ACGMT"):
    _DIGIT[_ch] = _d


def ranks(read: bytes, k: int) -> np.ndarray:
    """the 5-letter rank of every k-mer of a read (empty for a read shorter than k)"""
    d = _DIGIT[np.frombuffer(read, np.uint8)]
    if len(d) < k:
        return np.zeros(0, np.int64)
    r = np.zeros(len(d) - k + 1, np.int64)
    for j in range(k):
        r = r * 5 + d[j:len(d) - k + 1 + j]
    return r


def planted_read(k: int) -> bytes:
    """k-mers every case must hold, one after the other (so each of them is the k-mer of one event): T*k (rank 5^k - 1, the last live stream
    of the last partition), A*k (rank 0), M first / M last, a lower-case m and an IUPAC letter inside a k-mer, and for k = 6, 7 a walk
    over every partition's first stream -- the last partition's sub-index 0 among them; T*k is its last live sub-index"""
    parts = ["T" * k, "A" * k, "M" + "C" * (k - 1), "G" * (k - 1) + "M", "C" + "m" * (k - 1), "T" * (k - 1) + "R"]
    if k in (6, 7):
        parts += [model.meth_kmer_string(p * PART_SUB, k) for p in range(n_part(k))]
    return "".join(parts).encode()


def n_events(length: int, k: int, prefix: bool) -> int:
    """events of a DNA read (src/gensig.c:242-249): one per k-mer of the read with its prefix; five for a read shorter than k"""
    l0 = length + (DNA_PREFIX if prefix else 0)
    return 5 if l0 < k else l0 - k + 1


def worker_chains(lengths, k, T, prefix):
    """the events of every read, worker chain by worker chain in batch order (workers without a read have no chain)"""
    n = len(lengths)
    L = orc.lib()
    chains = {}
    for i, m in enumerate(lengths):
        chains.setdefault(0 if T <= 1 else L.orc_worker_of(i, n, T), []).append(n_events(m, k, prefix))
    return [chains[w] for w in sorted(chains)]


def expected_links(lengths, k, T, prefix, target):
    """(links, worker chains) of a batch whose chains are cut into links of whole reads with `target` links asked for: a chain gets its share
    of the target, at most one link per read, and a link closes once it holds its share of the chain's events.  Used to choose cases in
    which the cut really happens; what the library did is read off its own SQG_VERBOSE lines."""
    chains = worker_chains(lengths, k, T, prefix)
    nev = sum(map(sum, chains))
    links = 0
    for ch in chains:
        cev = sum(ch)
        lq = max(1, min(-(-target * cev // nev), len(ch)))
        per = -(-cev // lq)
        acc = 0
        for j, e in enumerate(ch):
            acc += e
            if j + 1 == len(ch) or acc >= per:
                links += 1
                acc = 0
    return links, len(chains)


@functools.lru_cache(maxsize=None)
def meth_case(seed: int) -> Case:
    """profile, dwell regime, flag set, k (cycling through 5 ... 9), T in 1 ... 4, 2-3 ragged batches of T+1 ... 3T+8 reads holding M, the
    forced link target; the planted read goes behind the first batch.  A batch that the link target would leave uncut is drawn again."""
    rng = np.random.default_rng(7000 + seed)
    base, _ = profiles.get_profile(["dna-r9-prom", "dna-r10-prom"][seed % 2])
    dwell_mean = float(rng.choice([2.0, 9.0, 13.0, 31.0, 120.0, 600.0]))
    dwell_std = float(rng.choice([0.0, 0.5, 4.0, dwell_mean * 0.8]))
    prof = base.replace(dwell_mean=dwell_mean, dwell_std=dwell_std, range=base.range * float(rng.uniform(0.6, 1.8)))
    flags = profiles.SQ_METH | FLAG_SETS[seed // len(KS) % len(FLAG_SETS)]
    k = KS[seed % len(KS)]
    T = int(rng.integers(1, 5))
    links = int(rng.choice([2, 7, 40, 100000] if k <= 7 else [2, 7, 40]))
    prefix = bool(flags & profiles.SQ_PREFIX)
    batches = []
    for bi in range(int(rng.integers(2, 4))):
        while True:
            n = int(rng.integers(T + 1, 3 * T + 8))
            lens = [int(m) for m in rng.choice(LENGTHS(k), n)]
            reads = [bytes(rng.choice(LETTERS, m, p=LETTER_P).astype(np.uint8)) for m in lens]
            if bi == 0:
                reads.append(planted_read(k))
            got, chains = expected_links([len(r) for r in reads], k, T, prefix, links)
            if got > chains:
                break
        batches.append(reads)
    return Case(seed, prof, flags, k, T, int(rng.integers(1, 1 << 30)), batches, links)


def witnesses(case: Case) -> dict:
    """what the reads of a case cover, from the reads alone (a read shorter than k is replaced by a fixed sequence: its own k-mers do not occur)"""
    k = case.k
    w = dict(parts=set(), last_sub=set(), rank0=False, rank_top=False, m_first=False, m_last=False, lower_m=False, iupac=False,
             max_chain_ev=0, short_read=False)
    top = 5 ** k - 1
    for bt in case.batches:
        for r in bt:
            if len(r) < k:
                w["short_read"] = True
                continue
            rk = ranks(r, k)
            w["parts"] |= set((rk // PART_SUB).tolist())
            w["last_sub"] |= set((rk[rk // PART_SUB == n_part(k) - 1] % PART_SUB).tolist())
            w["rank0"] |= bool((rk == 0).any())
            w["rank_top"] |= bool((rk == top).any())
            w["m_first"] |= bool((rk // 5 ** (k - 1) == 3).any())
            w["m_last"] |= bool((rk % 5 == 3).any())
            w["lower_m"] |= b"m" in r
            w["iupac"] |= any(c in r for c in (b"N", b"R", b"Y"))
        ch = worker_chains([len(r) for r in bt], k, case.T, bool(case.flags & profiles.SQ_PREFIX))
        w["max_chain_ev"] = max(w["max_chain_ev"], max(map(sum, ch)))
    return w


# ---- the matrix of tests/test_meth_paths.py, section "cut chains": (variant, seed); k = KS[seed % 5], the flag set FLAG_SETS[seed // 5 % 6],
# and odd seeds run the 256-thread k_events (SQG_EVENTS_WIDE_MAX=0): every k meets every variant at both widths.  The default variant
# takes every flag set; the others differ only in how streams are handed out, and take seeds whose flag set keeps the streams
VARIANTS = {
    "default": {},                                         # k 6, 7: k_events<PART> + the ordered hand-out over 4 / 20 partitions; k 5, 8, 9: per-link rows
    "order-free": {"cfg": profiles.SQ_ORDER_FREE},         # the hand-out by claims over the ragged partitions
    "claims": {"env": {"SQG_PART_CLAIMS": "1"}},           # the same through the development switch
    "per-link-rows": {"env": {"SQG_NO_PART": "1"}},        # k 6, 7 on k_events<HIST> + k_link_prefix with 5^k-wide rows
}
MATRIX = [("default", s) for s in range(0, 30)] + [("order-free", s) for s in range(30, 40)] + [("claims", s) for s in range(40, 50)] + \
         [("per-link-rows", s) for s in range(60, 70)]


# ---- the harness: one job through a library, both orders, against the oracle
def oracle_run(case: Case, level_mean, level_stdv):
    orac = orc.Oracle(case.prof, case.flags & ~profiles.SQ_ORDER_FREE, case.k, level_mean, level_stdv, case.ctx_seed, num_workers=case.T)
    want = [orac.run_batch_seqs(bt) for bt in case.batches]
    orac.close()
    return want


def check(b, want, tag):
    """signal, dwell, offset and median_before of a batch, bit for bit; the message names the read and the first differing sample"""
    sig, dw = b.signal(), b.dwell()
    assert b.n_reads == len(want), f"{tag}: {b.n_reads} reads, {len(want)} expected"
    for i, w in enumerate(want):
        got = sig[b.sig_off[i]:b.sig_off[i + 1]]
        if len(got) != len(w.sig):
            where = f"{len(got)} samples, {len(w.sig)} expected"
        else:
            bad = np.nonzero(got != w.sig)[0]
            where = f"first differing sample {bad[0]}: {got[bad[0]]} vs {w.sig[bad[0]]}, {bad.size} differ" if bad.size else ""
        np.testing.assert_array_equal(dw[b.ev_off[i]:b.ev_off[i + 1]], w.ss, err_msg=f"{tag} read {i}: dwell")
        np.testing.assert_array_equal(got, w.sig, err_msg=f"{tag} read {i}: {where}")
        assert b.offset[i] == w.offset and b.median_before[i] == w.median_before, f"{tag} read {i}: offset / median_before"


def describe(case: Case, variant="default"):
    return (f"seed {case.seed} k={case.k} T={case.T} flags={case.flags:#x} links={case.links} {variant} "
            f"dwell={case.prof.dwell_mean}/{case.prof.dwell_std}")


def run_submit(gen, case, want, tag):
    """batch by batch"""
    for bi, bt in enumerate(case.batches):
        b = gen.submit(bt)
        check(b, want[bi], f"{tag} submit batch {bi}")
        b.free()


def run_streamed(gen, case, want, tag):
    """batch i+2 staged, batch i+1 queued, batch i consumed"""
    batches = case.batches
    cur = gen.stage(batches[0]).run()
    nxt = gen.stage(batches[1]) if len(batches) > 1 else None
    for bi in range(len(batches)):
        nn = gen.stage(batches[bi + 2]) if bi + 2 < len(batches) else None
        if nxt is not None:
            nxt.run()
        cur.wait()
        check(cur, want[bi], f"{tag} streamed batch {bi}")
        cur.free()
        cur, nxt = nxt, nn


def run_case(case: Case, level_mean, level_stdv, want, modes, variant="default", lib_path=None, after_job=None):
    """every arithmetic mode x both orders, a fresh context each; after_job(tag, case) is called behind every one of them"""
    flags = case.flags | VARIANTS[variant].get("cfg", 0)
    for mode in modes:
        for how in (run_submit, run_streamed):
            tag = f"{describe(case, variant)} mode {mode}"
            gen = api.SignalGenerator(case.prof, flags, case.k, level_mean, level_stdv, case.ctx_seed, num_workers=case.T, mode=mode, lib_path=lib_path)
            how(gen, case, want, tag)
            gen.close()
            if after_job:
                after_job(f"{tag} {how.__name__}", case)


# ---- the path a batch took, from the library's SQG_VERBOSE lines (h_run.h: one per batch, the first eight batches of a context)
_BATCH_LINE = re.compile(r"\[sqg\] batch (\d+): (\d+) reads, (\d+) events, (\d+) links in (\d+) worker chains, (\d+) pieces, (\d+) slices")


def batch_lines(stderr_text: str):
    """[(batch, reads, events, links, worker chains, pieces, slices)] in the order printed; slices: the bound on the slices of the bucketed
    hand-out, at least one per (worker chain, partition) -- 0 for a batch that does not take it (per-link rows, or no cut at all)"""
    return [tuple(int(x) for x in m.groups()) for m in _BATCH_LINE.finditer(stderr_text)]
