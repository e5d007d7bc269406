"""numpy statement of include/sqg_targets.h: what sqg_batch_chunk_targets must produce, bit for bit.  Written from the rules of the
header; no call into the library.  The normalisation is chunks_ref's (the header refers to sqg_chunks.h for it)."""
import numpy as np

import chunks_ref as R

_BASE = np.zeros(256, np.int64)                     # src/seq.h:14-27
for _letters, _c in ((b"CcYB", 1), (b"GgSK", 2), (b"TtU", 3)):
    for _b in _letters:
        _BASE[_b] = _c
_METH = np.zeros(256, np.int64)                     # src/seq.h:45-60: A C G M T, upper case only
for _b, _c in zip(b"CGMT", (1, 2, 3, 4)):
    _METH[_b] = _c


def kmer_ranks(seq, k, meth):
    """the pore-table row of read[e .. e+k) for every event e"""
    d = (_METH if meth else _BASE)[np.frombuffer(bytes(seq), np.uint8)]
    ne = len(d) - k + 1
    rank = np.zeros(ne, np.int64)
    for q in range(k):
        rank = rank * (5 if meth else 4) + d[q:q + ne]
    return rank.astype(np.uint32)


def to_i16(v):
    """(int16_t)double as gcc / x86-64 lowers it: truncation to int32 (INT32_MIN when it does not fit), then the low half"""
    v = np.asarray(v, np.float64)
    fits = (v > -2147483649.0) & (v < 2147483648.0)
    t = np.where(fits, np.trunc(np.where(fits, v, 0.0)), -2147483648.0).astype(np.int64)
    return (t & 0xffff).astype(np.uint16).view(np.int16)


def read_samples(seq, ss, offset, level_mean, k, rna, meth, rng, dig):
    """one read -> (clean_raw, moves, kmer) for all of its samples AS STORED (RNA: reversed)"""
    ss = np.asarray(ss, np.int64)
    assert (ss >= 1).all()
    E = np.cumsum(ss) - ss
    n = int(ss.sum())
    g = np.arange(n, dtype=np.int64)
    e = np.searchsorted(E, g, "right") - 1                                   # E[e] <= g < E[e] + dwell[e]
    rank = kmer_ranks(seq, k, meth)
    assert len(rank) == len(ss)
    level = np.asarray(level_mean, np.float32)[rank].astype(np.float64)
    code = to_i16(level * np.float64(dig) / np.float64(rng) - np.float64(offset))     # src/gensig.c:270
    clean_raw, moves, kmer = code[e], (g == E[e]).astype(np.uint8), rank[e]
    if rna:
        clean_raw, moves, kmer = clean_raw[::-1], moves[::-1], kmer[::-1]
    return np.ascontiguousarray(clean_raw), np.ascontiguousarray(moves), np.ascontiguousarray(kmer)


def read_targets(sig, seq, ss, offset, level_mean, k, rna, meth, L, S, dtype="f16", norm="medmad", rng=1.0, dig=1.0):
    """one read -> dict(clean, clean_raw, moves, kmer), each [nc, L].  sig: the NOISY stored samples (for med2 / mad4 only)"""
    n = int(np.sum(ss))
    nc = R.n_chunks_of(n, L, S) if len(seq) >= k else 0
    fdt = np.float16 if dtype == "f16" else np.float32
    if nc == 0:
        return dict(clean=np.zeros((0, L), fdt), clean_raw=np.zeros((0, L), np.int16), moves=np.zeros((0, L), np.uint8), kmer=np.zeros((0, L), np.uint32))
    clean_raw, moves, kmer = read_samples(seq, ss, offset, level_mean, k, rna, meth, rng, dig)
    med2, mad4 = R.stats(np.asarray(sig, np.int16)) if norm == "medmad" else (0, 0)
    x = R.normalise(clean_raw, med2, mad4, norm, offset, rng, dig)
    if dtype == "f16":
        with np.errstate(over="ignore"):
            x = x.astype(np.float16)
    idx = (np.arange(nc, dtype=np.int64) * S)[:, None] + np.arange(L, dtype=np.int64)[None, :]
    return dict(clean=x[idx], clean_raw=clean_raw[idx], moves=moves[idx], kmer=kmer[idx])


def batch_targets(reads, level_mean, k, rna, meth, L, S, dtype, norm, rng, dig):
    """reads: list of dict(sig, ss, seq, offset) -> the batch's outputs as sqg_chunk_targets_t lays them out, and chunk_off"""
    per = [read_targets(r["sig"], r["seq"], r["ss"], r.get("offset", 0.0), level_mean, k, rna, meth, L, S, dtype, norm, rng, dig) for r in reads]
    out = {key: np.concatenate([p[key] for p in per]) for key in ("clean", "clean_raw", "moves", "kmer")}
    out["chunk_off"] = np.concatenate(([0], np.cumsum([len(p["moves"]) for p in per]))).astype(np.int64)
    return out
