"""Seeds outside the canonical range [1, M) of the Lehmer generator, M = 2^31 - 1: helpers and the case table of
tests/test_seed_space.py.

Every stream of the signal path is MINSTD.  The reference keeps its state uncorrected in an int64_t (src/rand.h:79-85) and seeds
stream j of worker w with seed + w*(num_kmer + 10) + j (src/sim.c:238-257), whatever that number is; the library keeps the state
canonical and reduces the seed mod M.  A seed that is 0 (mod M) stays 0: the reference's corrected value is then M, u = 1.0 on every
draw, sqrt(-2 log u) = 0, and the draw is the mean exactly -- the ZERO STREAM."""
import numpy as np

from squigulator_amd import model

M = 2 ** 31 - 1
LCG_A, LCG_Q, LCG_R = 16807, 127773, 2836        # a, M / a, M % a
# One Schrage step stays within (-M, M) -- the canonical form is valid -- exactly for |x| < 757223 * 127773: at that x the reference's
# corrected value is -781, not 16807 x mod M
VALID_BELOW = 757223 * 127773                     # 96 752 654 379
ADMITTED = 90_000_000_000                         # sqg_create: |seed| + T * (num_kmer + 10) <= 9.0e10 (csrc/h_context.h)


def stream_seed(seed, w, nk, j):
    """the number the reference seeds stream j of worker w with (kmer_gen[j]: rank j; the scalar streams: j = 0 ref_pos, 1 strand,
    2 time, 3 rlen, 4 offset, 5 median_before, 6 meth)"""
    return seed + w * (nk + 10) + j


def canon(x):
    """the canonical state, in [0, M)"""
    return x % M                                  # (Python's %: the sign of the divisor)


def zero_rank(seed, w, nk):
    """the rank j0 < nk whose k-mer stream of worker w is the zero stream, or None"""
    j0 = (-stream_seed(seed, w, nk, 0)) % M
    return j0 if j0 < nk else None


def c_div(a, b):
    """C's truncating division"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def ref_rng(x):
    """rng() of src/rand.h:79-85 in Python integers: (the new uncorrected state, the corrected value the uniform is made of)"""
    nx = LCG_A * (x - LCG_Q * c_div(x, LCG_Q)) - LCG_R * c_div(x, LCG_Q)          # a * (x % q) - r * (x / q), C's % and /
    return nx, (nx if nx > 0 else nx + M)


def kmer_of(rank, k, meth):
    """the bases of a rank: over A C G T, or over the 5-letter alphabet A C G M T of SQG_METH (src/seq.h:31-74)"""
    return (model.meth_kmer_string(rank, k) if meth else model.kmer_string(rank, k)).encode()


def planted(k, kmer, n, rng):
    """a read of n random bases that holds `kmer` at least 40 times, never overlapping itself, and the indices of ALL events whose
    k-mer is `kmer` (a k-mer such as AAAAAA also turns up next to a planted copy)"""
    copies = 40
    stride = n // copies
    assert len(kmer) == k and stride >= k + 1, "the read is too short for 40 copies"
    a = rng.choice(list(b"ACGT"), n).astype(np.uint8)
    km = np.frombuffer(kmer, np.uint8)
    for i in range(copies):
        p = i * stride + int(rng.integers(0, stride - k))     # (copy i within [i stride, (i + 1) stride - 1): a base between two copies)
        a[p:p + k] = km
    read = bytes(a)
    hits = [i for i in range(n - k + 1) if read[i:i + k] == kmer]
    assert len(hits) >= copies
    return read, hits


def to_i16(v):
    """(int16_t)double as gcc / x86-64 lowers it (cvttsd2si r32, low half): src/gensig.c:270"""
    t = int(v) if -2147483649.0 < v < 2147483648.0 else -(2 ** 31)
    t &= 0xffff
    return t - 0x10000 if t >= 0x8000 else t


def zero_stream_sample(level_mean, prof, offset):
    """every sample of a zero k-mer stream: nrng returns 0 * s + m = m, so raw = (double)level_mean * dig / range - offset"""
    return to_i16(float(np.float32(level_mean)) * prof.digitisation / prof.range - offset)


def worker_of(i, n, T):
    """the worker of read i of a batch of n (src/thread.c:80-99, the static partition)"""
    return 0 if T <= 1 else i // ((n + T - 1) // T)


def largest_admitted(T, nk):
    return ADMITTED - T * (nk + 10)


def seed_table(T, nk):
    """(id, seed).  2147483647 is M itself; -2147483648 = -(M + 1); both ends of what atoi returns (src/sim.c:940)"""
    big = largest_admitted(T, nk)
    return [("M-nk/2", M - nk // 2), ("M", M), ("M+5", M + 5), ("-1", -1), ("-2", -2), ("-4", -4), ("-5", -5), ("-6", -6),
            ("-nk/3", -(nk // 3)), ("int32_max", 2147483647), ("int32_min", -2147483648), ("2^33", 2 ** 33),
            ("+admitted", big), ("-admitted", -big)]
