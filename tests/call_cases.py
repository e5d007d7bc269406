"""The cases of tests/test_call.py: reads that hold what can go wrong in sqg_call_plan / sqg_batch_call, made-up rows and models, and the
drawn cases -- on the CPU from a generator of their own, on the GPU from tests/consumer_cases.py's drawing (imported, not edited).
Not collected."""
import numpy as np

import call_ref as R

LOAD, WAVE, TILE = 16, 1024, 4096          # k_call.h: bytes of a thread's load, of a wavefront's 64 loads, of a workgroup's tile
I64_MIN = -(1 << 63)


def small_reads(k):
    """reads of k - 1 (no sites), k and k + 1 bases; a site at p = 0 and at p = len - 2; a 'C' ending one read in front of a 'G' beginning
    the next; lower-case cg; IUPAC letters inside a span; CG runs, so that every k-mer holds several candidates; reads without a site
    between reads with sites; and -- the lengths before them being odd -- reads whose first base sits anywhere in its 16-byte load.  The
    two long reads put a CpG across every 16-byte load, every wavefront's 1024 bytes and the workgroup's 4096-byte tile whatever the
    alignment of the batch: "CG" repeated has a candidate at every even p, "ACG" repeated at every residue modulo 16"""
    pad = b"ATTAGACAT" * 3
    return [
        (b"CG" + pad)[:k - 1],                      # shorter than a k-mer: its stand-in events, no site
        (b"CG" + pad)[:k],                          # p = 0, one event
        (pad[:k - 1] + b"CG"),                      # k + 1 bases, p = len - 2
        pad[:k] + b"AC",                            # ends in C ...
        b"G" + pad[:k + 2],                         # ... begins with G: no candidate
        b"ATcgTAcGTACgTT" + pad,                    # lower case: no site
        b"TTAGA" + pad + b"TTA",                    # no site at all, between reads with sites
        b"ANCGRYTTMGNNACGKSCGW" + pad,              # IUPAC letters inside the spans: digit 0
        b"CGCGCGMGCGCGMGMGCG" + b"T" + b"CG" * 9,   # runs
        b"MG" + b"A" * (2 * k) + b"MG",             # p = 0 and p = len - 2, both 'M'
        b"CG" * (TILE // 2 + WAVE // 2 + 37),       # across every load, wavefront and tile boundary
        b"T" + b"ACG" * (TILE // 3 + 300) + b"C",   # the same at every residue; ends in a 'C' that has no 'G'
        b"G" + b"ACMGT" * 7,
    ]


def barren_reads(k):
    """a batch with no site at all: candidates only across reads, in lower case, or in a read shorter than a k-mer"""
    return [b"ATTACATTAC", b"GTTAGGACCAT" * 4, b"cgcg" * 7, b"CG", b"AAGCTTGCAAGC" * 3]


def drawn_reads(rng, n, k, hi=120):
    letters, p = list(b"ACGTMacgtNRY"), np.array([.2, .2, .22, .18, .08, .02, .02, .02, .02, .02, .01, .01])
    return [bytes(rng.choice(letters, int(m), p=p).astype(np.uint8)) for m in rng.choice([k - 1, k, k + 1, 2 * k, 40, 97, hi], n)] if n else []


def ev_offsets(reads, k):
    """the batch's ev_off: len - k + 1 events, five stand-in events for a read shorter than a k-mer"""
    return np.concatenate(([0], np.cumsum([len(r) - k + 1 if len(r) >= k else 5 for r in reads]))).astype(np.int64)


TERM_CAPS, LLR_MINS, MIN_OBS = [0, 1, 300, 256 * 50, 1 << 26], [0, 1, 512, 40000], [0, 1, 3, 12]


def drawn_cfg(rng):
    return (int(rng.integers(0, 2)), int(rng.choice(TERM_CAPS)), int(rng.choice(LLR_MINS)), int(rng.choice(MIN_OBS)))


def drawn_rows(rng, n_events, level_raw=None, wild=True):
    """made-up rows: lengths with zeros and negatives among them, sums around a level (the true one where it is given), a few of any size"""
    lens = rng.integers(1, 40, n_events)
    lens = np.where(rng.random(n_events) < 0.15, rng.integers(-2, 1, n_events), lens)
    centre = rng.integers(-500, 1500, n_events) if level_raw is None else np.asarray(level_raw, np.int64) + rng.integers(-30, 30, n_events)
    sums = centre * np.maximum(lens, 1) + rng.integers(-20, 20, n_events)
    if wild:
        sums = np.where(rng.random(n_events) < 0.05, rng.integers(I64_MIN, (1 << 63) - 1, n_events), sums)
    return sums.astype(np.int64), lens.astype(np.int64)


def drawn_model(rng, k, wild=True):
    n = 5 ** k
    w = rng.integers(0, 1 << 22, n)
    c = rng.integers(-3000, 3000, n)
    if wild:
        w = np.where(rng.random(n) < 0.05, rng.integers(-(1 << 31), (1 << 31) - 1, n), w)
        c = np.where(rng.random(n) < 0.05, rng.integers(-(1 << 31), (1 << 31) - 1, n), c)
    return w.astype(np.int32), c.astype(np.int32)


def drawn_scale(rng, n):
    gain = rng.integers(40000, 90000, n)
    shift = rng.integers(-20000, 20000, n)
    gain = np.where(rng.random(n) < 0.2, rng.choice([-5, 0, 1, 1 << 20, (1 << 20) + 1, (1 << 31) - 1], n), gain)
    shift = np.where(rng.random(n) < 0.2, rng.choice([-(1 << 31), -(1 << 26) - 1, 1 << 26, (1 << 30)], n), shift)
    return gain.astype(np.int32), shift.astype(np.int32)


def drawn_origin(rng, n, span=400, base=(1 << 40) + 77):
    """a caller's origin: all three steps, keys past 32 bits, the reads laid over one another"""
    step = ((np.arange(n) + int(rng.integers(0, 3))) % 3 - 1).astype(np.int8)
    return base + rng.integers(0, span, n).astype(np.int64), step


def cpu_case(seed):
    """a whole made-up case for the two statements alone -> (args, kwargs) of call_ref.by_site / vectorised"""
    rng = np.random.default_rng(500 + seed)
    k = 5 + seed % 3 if seed % 7 else 9
    reads = drawn_reads(rng, int(rng.integers(0, 7)), k)
    ev_off = ev_offsets(reads, k)
    ne = int(ev_off[-1])
    level_mean = rng.uniform(40, 160, 5 ** k).astype(np.float32)
    if seed % 5 == 0:
        level_mean[::7] = np.float32(1e12)                    # levels outside int32: the conversion's INT32_MIN
    offsets = rng.normal(10, 30, len(reads))
    rng_, dig = float(rng.uniform(700, 2900)), float(rng.choice([2048.0, 8192.0]))
    sums, lens = drawn_rows(rng, ne, wild=seed % 2 == 0)
    w, c = drawn_model(rng, k, wild=seed % 3 == 0)
    kw = {}
    if seed % 2:
        kw["scale"] = drawn_scale(rng, len(reads))
    if seed % 4 != 1:
        kw["origin"] = drawn_origin(rng, len(reads))
        if seed % 4 != 2:
            lo = (1 << 40) + 77 + int(rng.integers(-50, 200))
            kw["window"] = (lo, lo + int(rng.integers(0, 400)))
    return (reads, k, drawn_cfg(rng), sums, lens, ev_off, level_mean, offsets, rng_, dig, w, c), kw


GPU_SEEDS = [s for s in range(100) if s % 10 in (8, 9)]       # consumer_cases.FLAG_SETS 8 and 9: SQ_METH, and SQ_METH | SQ_IDEAL_TIME
assert R.DEFAULT == (1, 12800, 512, 1)
