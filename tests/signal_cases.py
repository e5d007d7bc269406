"""The adversarial int16 arrays that test_injected_signals.py puts into a batch (inject.py), and the read lengths they need.

Every builder takes the batch's sig_off and returns int16 [sig_off[-1]].  test_signal_cases.py shows without a GPU, with the references
alone (orc.svb_zd and slow5lib's committed bytes, the host BLOW5 encoder, chunks_ref), that each array does what its name says.

Two facts that shape these arrays:
  * a read's first svb-zd value is the delta to 0, so it never takes three bytes (|delta| <= 32768 -> z <= 65535): an array of
    alternating -32768 / 32767 has 3 n - 1 data bytes, not 3 n;
  * mad4 is even for every read: the two middle deviations |2 v - med2| both have med2's parity.  The smallest MAD above 0 is therefore
    mad4 = 2 (mad' = 0.5), and float16 MEDMAD output overflows only where mad4 = 2 and the median sits at an end of the int16 range
    ((v - med) / (1.4826 * 0.5) reaches +-88 406; with mad4 = 0, mad' = 1, it stays below 44 204 < 65 504).
"""
import os

import numpy as np

import chunks_ref as R

GOLD_SVB = os.path.join(os.path.dirname(__file__), "golden", "svb", "svb_cases.npz")


def svb_goldens():
    """[(int16 array, slow5lib's svb-zd bytes of it)] of tests/golden/svb/svb_cases.npz"""
    d = np.load(GOLD_SVB)
    so = np.concatenate(([0], np.cumsum(d["lens"])))
    eo = np.concatenate(([0], np.cumsum(d["enc_lens"])))
    return [(d["sig"][so[i]:so[i + 1]], d["enc"][eo[i]:eo[i + 1]]) for i in range(len(d["lens"]))]


# ---- the read lengths (samples) ----------------------------------------------------------------------------------------------------
# "exact1" (SQ_IDEAL_TIME, dwell 1): every golden array's length, so that a read IS that array; n mod 4 = 0 1 2 3; nine reads below 8
# samples; around one and two passes of k_svb_encode (256 quads = 1024 samples); above 70 000
EXACT1_LENGTHS = ([100003, 1, 2, 3, 4, 5, 6, 7, 8, 9, 1000, 85, 4099, 68999, 117490] + list(range(1020, 1029)) + list(range(2044, 2053))
                  + [70001, 3, 1])
# "exact2" (dwell 2): even reads that hold all 65 536 codes and enough more samples to put the median and the MAD anywhere
EXACT2_LENGTHS = [132000] * 6 + [64, 2, 4098]
# "drawn" (the profile's dwells): bases; the lengths are what the run gives
DRAWN_BASES = [3000, 12, 6, 700, 7, 8000, 250, 1500, 9000, 64]


def check_svb_geometry(lens):
    """what the svb / BLOW5 cases need of the batch they are injected into (asserted on the GPU about the batch the run gave)"""
    lens = np.asarray(lens, np.int64)
    assert set((lens % 4).tolist()) == {0, 1, 2, 3}
    assert np.count_nonzero(lens < 8) >= 4 and lens.min() == 1
    assert all(np.any(lens == c + e) for c in (1024, 2048) for e in range(-4, 5))
    assert lens.max() > 70000
    have = set(lens.tolist())
    assert all(len(s) in have for s, _ in svb_goldens() if len(s)), "a golden array has no read of its length"


def _reads(sig_off, f, seed=17):
    """f(i, n, rng) -> the samples of read i"""
    rng = np.random.default_rng(seed)
    out = np.zeros(int(sig_off[-1]), np.int16)
    for i in range(len(sig_off) - 1):
        n = int(sig_off[i + 1] - sig_off[i])
        v = np.asarray(f(i, n, rng))
        assert v.shape == (n,) and v.min(initial=0) >= -32768 and v.max(initial=0) <= 32767, (i, n, v.shape)
        out[sig_off[i]:sig_off[i + 1]] = v
    return out


# ---- svb-zd ------------------------------------------------------------------------------------------------------------------------
def slow5lib_goldens(sig_off):
    """a read whose length is a golden array's is that array; the others hold the goldens back to back, cut to length"""
    gold = [s for s, _ in svb_goldens() if len(s)]
    by_len = {len(s): s for s in gold}
    tile = np.concatenate(gold)
    return _reads(sig_off, lambda i, n, rng: by_len[n] if n in by_len else np.resize(np.roll(tile, -7 * i), n))


# deltas whose zig-zag values are 65535, 131070, 65535, 256, 255, 0, 65536, 65535, 2: the walk 0 -> -32768 -> 32767 -> -1 -> 127 -> -1
# -> -1 -> 32767 -> -1 -> 0 closes after 9 steps, and 9 is odd: every delta comes to every place of a quad
CLASS_DELTAS = np.array([-32768, 65535, -32768, 128, -128, 0, 32768, -32768, 1], np.int64)
CLASS_Z = (0, 255, 256, 65535, 65536, 131070)


def svb_classes(sig_off):
    return _reads(sig_off, lambda i, n, rng: np.cumsum(np.resize(CLASS_DELTAS, n)))


def svb_wrap(sig_off):
    return _reads(sig_off, lambda i, n, rng: np.resize(np.array([-32768, 32767]), n))


def border_steps(n):
    """where svb_borders steps: the first sample of every wavefront's first quad (256 m; 1024 m starts a pass of 256 quads) and the last"""
    return np.unique(np.concatenate((np.arange(256, n, 256), [n - 1]))) if n > 1 else np.zeros(0, np.int64)


def svb_borders(sig_off):
    """two levels 40 000 apart (-20 000 / 20 000: zig-zag 80 000 or 79 999, three bytes), flat between the steps"""
    def f(i, n, rng):
        lvl = np.zeros(n, np.int64)
        lvl[border_steps(n)] = 1
        return np.where(np.cumsum(lvl) & 1, 20000, -20000)
    return _reads(sig_off, f)


def uniform(sig_off):
    return _reads(sig_off, lambda i, n, rng: rng.integers(-32768, 32768, n))


def all_equal(sig_off):
    """a constant per read: 600, and the two ends of the range"""
    return _reads(sig_off, lambda i, n, rng: np.full(n, (600, -32768, 32767)[i % 3]))


def one_value_but_one(sig_off):
    def f(i, n, rng):
        v = np.full(n, 600)
        v[n // 2] = 601
        return v
    return _reads(sig_off, f)


def fib_counts(n):
    """Fibonacci numbers 34, 55, 89, ... while their sum stays within n.  The record's trailer (31 bytes + end of block) stands in for the
    terms below 34: a Huffman tree stays a chain only while what has been merged so far weighs less than the next leaf but one, and 32
    < 55 keeps it so; with the terms from 1 up the trailer's bytes would break the chain at the bottom and halve the depth"""
    f, a, b = [], 34, 55
    while sum(f) + a <= n:
        f.append(a)
        a, b = b, a + b
    return f


def fibonacci_encoding(n):
    """a VALID svb-zd encoding of n samples: the count, all-zero keys (one byte per value) and n data bytes whose counts are Fibonacci
    numbers (fib_counts) -- byte 0 the largest (+ what is left of n), then bytes 2, 1 (deltas +1, -1), 3, 4 (-2, +2), 6, 5, ... in falling counts,
    the heavier of each pair on alternating sides; ordered so that the decoded walk stays inside int16"""
    f = sorted(fib_counts(n), reverse=True)
    cnt = {0: n - sum(f) + (f[0] if f else 0)}
    flip = False
    for j in range(1, len(f), 2):
        mag = (j + 1) // 2                                  # deltas +mag (byte 2 mag) and -mag (byte 2 mag - 1)
        pair = (2 * mag - 1, 2 * mag) if flip else (2 * mag, 2 * mag - 1)
        cnt[pair[0]] = f[j]
        if j + 1 < len(f):
            cnt[pair[1]] = f[j + 1]
        flip = not flip
    assert max(cnt) < 256 and sum(cnt.values()) == n
    pos = np.concatenate([np.full(c, z, np.uint8) for z, c in sorted(cnt.items()) if z and z % 2 == 0] + [np.zeros(0, np.uint8)])
    neg = np.concatenate([np.full(c, z, np.uint8) for z, c in sorted(cnt.items()) if z % 2 == 1] + [np.zeros(0, np.uint8)])
    # merge: a step down whenever the walk is above 0 and steps down are left
    data, s, ip, im = np.zeros(n, np.uint8), 0, 0, 0
    for q in range(len(pos) + len(neg)):
        if (s > 0 and im < len(neg)) or ip == len(pos):
            z = int(neg[im]); im += 1
        else:
            z = int(pos[ip]); ip += 1
        data[q] = z
        s += (z >> 1) ^ -(z & 1)
        assert -32768 <= s <= 32767
    return np.concatenate((np.array([n], "<u4").view(np.uint8), np.zeros((n + 3) // 4, np.uint8), data)), cnt


def fibonacci(sig_off):
    import orc

    def f(i, n, rng):
        sig, used = orc.svb_zd_decode(fibonacci_encoding(n)[0])
        assert used == 4 + (n + 3) // 4 + n
        return sig
    return _reads(sig_off, f)


# ---- chunk statistics --------------------------------------------------------------------------------------------------------------
def _span(n, lo, span, rng):
    v = rng.integers(lo, lo + span, n)
    v[rng.choice(n, 2, replace=False)] = (lo, lo + span - 1)
    return v


def _stats_edge(i, n, rng):
    """-> (samples, (med2, mad4, span) as far as stated: None = whatever it comes to)"""
    if n == 1:
        return np.array([32767 if i % 2 else -32768]), ((65534 if i % 2 else -65536), 0, 1)
    if n == 2:
        return np.array([-32768, 32767]), (-1, 2 * 65535, 65536)              # |2 v + 1| = 65535 twice: the fold's largest value
    if n in (1000, 1020, 1021, 1022):                                         # the LDS histogram holds CHUNK_HIST = 4096 bins
        lo, span = {1000: (-2000, 4096), 1020: (-2000, 4097), 1021: (-32768, 4096), 1022: (32767 - 4096, 4097)}[n]
        return _span(n, lo, span, rng), (None, None, span)
    if n == 1024:                                                             # even n, the middle samples 1 and 30002: med2 odd
        v = np.concatenate((rng.integers(-100, 2, n // 2), rng.integers(30002, 30100, n // 2)))
        v[0], v[-1] = 1, 30002
        return rng.permutation(v), (30003, None, None)
    if n == 2048:                                                             # the smallest MAD above 0: mad4 = 2 (mad' = 0.5)
        v = np.concatenate((np.full(700, 500), np.full(700, 501), rng.integers(-3000, 400, 324), rng.integers(600, 1000, 324)))
        return rng.permutation(v), (1001, 2, None)
    if n == 2050:                                                             # half the samples one value: one LDS address
        v = np.concatenate((np.full(1025, 777), rng.integers(778, 1500, 1025)))
        v[-1] = 778
        return rng.permutation(v), (777 + 778, None, None)
    if n == 2052:                                                             # ... and one word of the global histogram
        v = np.concatenate((np.full(1027, -32768), rng.integers(-32768, 32768, 1025)))
        return rng.permutation(v), (-65536, 0, None)
    if n == 70001:
        return _span(n, -32768, 65536, rng), (None, None, 65536)
    if n > 60000:                                                             # natural: a narrow walk
        return 500 + np.clip(np.cumsum(rng.integers(-40, 41, n)), -400, 400), (None, None, None)
    return rng.integers(200, 1300, n), (None, None, None)


def stats_edges(sig_off):
    return _reads(sig_off, lambda i, n, rng: _stats_edge(i, n, rng)[0])


def stats_edges_expect(sig_off):
    """read -> (med2, mad4, span) as the case states them (None: not stated)"""
    rng = np.random.default_rng(17)
    return {i: _stats_edge(i, int(sig_off[i + 1] - sig_off[i]), rng)[1] for i in range(len(sig_off) - 1)}


# every_code: all 65 536 codes in a seeded order, then n - 65 536 samples that pin (med2, mad4).  n is even and >= 131 072.
#   ("typical", c, h): median c, MAD h: n/2 - 2 h samples of c itself (the codes have 2 h - 1 values nearer than h), the rest 20 000 off
#   ("pair", a):       median a + 1/2, mad4 = 2: the samples split over a and a + 1 so that the middle falls between them
#   ("top",):          median 32767, mad4 = 0
EVERY_CODE_TARGETS = [("typical", 0, 370), ("pair", -1), ("pair", 32766), ("pair", -32768), ("top",), ("typical", 700, 75)]
EVERY_CODE_STATS = [(0, 1480), (-1, 2), (65533, 2), (-65535, 2), (65534, 0), (1400, 300)]


def _every_code(i, n, rng):
    if i >= len(EVERY_CODE_TARGETS):
        return rng.integers(-32768, 32768, n)
    assert n % 2 == 0 and n >= 131072, n
    m, t = n - 65536, EVERY_CODE_TARGETS[i]
    codes = rng.permutation(np.arange(-32768, 32768))
    if t[0] == "typical":
        c, h = t[1], t[2]
        y = n // 2 - 2 * h
        x = m - y
        assert x >= 0
        rest = np.concatenate((np.full(y, c), np.full(x // 2, c - 20000), np.full(x - x // 2, c + 20000)))
    elif t[0] == "pair":
        a = t[1]
        below = a + 32768                                    # codes under a
        lo = n // 2 - below - 1                              # extra samples of a: codes under a + a's own + these = n / 2
        assert 0 <= lo <= m
        rest = np.concatenate((np.full(lo, a), np.full(m - lo, a + 1)))
    else:
        rest = np.full(m, 32767)
    return np.concatenate((codes, rng.permutation(rest)))


def every_code(sig_off):
    return _reads(sig_off, _every_code)


SVB_CASES = {"slow5lib_goldens": slow5lib_goldens, "svb_classes": svb_classes, "svb_wrap": svb_wrap, "svb_borders": svb_borders,
             "uniform": uniform, "all_equal": all_equal, "one_value_but_one": one_value_but_one, "fibonacci": fibonacci,
             "stats_edges": stats_edges}
CASES = dict(SVB_CASES, every_code=every_code)


def offsets(lens):
    return np.concatenate(([0], np.cumsum(lens))).astype(np.int64)


def medmad_two_ways(codes, med2, mad4):
    """float16 MEDMAD of int16 codes: (float32 product, then float16 -- the rule of include/sqg_chunks.h; one rounding of the exact
    product to float16 -- what a fused multiply-convert gives)"""
    madp = mad4 / 4.0 if mad4 > 0 else 1.0
    inv = np.float32(1.0 / (1.4826 * madp))
    diff = codes.astype(np.float32) - np.float32(med2 / 2.0)                  # exact: both are multiples of 1/2 below 2^17
    with np.errstate(over="ignore"):
        return R.bits((diff * inv).astype(np.float16)), R.bits((diff.astype(np.float64) * np.float64(inv)).astype(np.float16))
