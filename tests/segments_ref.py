"""numpy statement of include/sqg_segments.h: the segments of a read with an attached prefix, the level-shift range, and the trimmed
chunks / targets (the insert's slices handed to chunks_ref / targets_ref, the shift rule added).  Written from the rules of the header;
no call into the library."""
import numpy as np

import chunks_ref as R
import targets_ref as T

# the attached sequences are data (src/genread.c:37-39, 88, 110)
STALL_DNA = b"TTTTTTTTTTTTTTTTTTAATCAA"
ADAPTOR_DNA = b"GGCGTCTGCTTGGGTGTTTAACCTTTTTTTTTTAATGTACTTCGTTCAGTTACGTATTGCT"
POLYA = b"A" * 158
ADAPTOR_RNA = b"TGATGATGAGGGATAGACGATGGTTGTTTCTGTTGGTGCTGATATTGCTTTTTTTTTTTTTATGATGCAAGATACGCAC"
STALL_RNA = b"AAAAAGAAAAAACCCCCCCCCCCCCCCCCC"
SHORT_HACK = b"ACGTACGTACGT\0"                        # src/gensig.c:242-245: five k-mers of this, NUL included
assert (len(STALL_DNA), len(ADAPTOR_DNA), len(ADAPTOR_RNA), len(STALL_RNA)) == (24, 61, 79, 30)


def chains(seq, k, rna, prefix):
    """(chain 0, chain 1): the base sequences the signal is generated from, in generation order; short: chain 0 is the stand-in"""
    if not prefix:
        c0, c1 = bytes(seq), b""
    elif rna:
        c0, c1 = bytes(seq) + POLYA + ADAPTOR_RNA, STALL_RNA
    else:
        c0, c1 = STALL_DNA + ADAPTOR_DNA + bytes(seq), b""
    if len(c0) < k:
        c0 = SHORT_HACK[:5 + k - 1]
    return c0, c1


def segments(ss, length, k, rna, prefix, sps):
    """one read -> dict(seg [5], shift [2], events: the [lo, hi) ranges of ss of stall, adaptor, poly-A, insert, win: the part of the
    shift window inside the insert, generation order relative to the insert).  ss: the dwells as the reference writes them (chain 0,
    then chain 1); length: the read's own bases; sps: (int)dwell_mean"""
    ss = np.asarray(ss, np.int64)
    n = int(ss.sum())
    whole = dict(seg=np.array([0, 0, 0, 0, n], np.int64), shift=np.zeros(2, np.int64),
                 events=[(0, 0), (0, 0), (0, 0), (0, len(ss))], win=(0, 0))
    if not prefix:
        return whole                                          # (a read shorter than a k-mer included)
    E = np.concatenate(([0], np.cumsum(ss)))                  # E[e] for e in 0 .. len(ss)
    if not rna:
        ne0 = length + 85 - k + 1
        assert ne0 == len(ss)
        a, b = min(24, ne0), min(85, ne0)
        return dict(seg=np.array([0, E[a], E[b], E[b], n], np.int64), shift=np.zeros(2, np.int64),
                    events=[(0, a), (a, b), (b, b), (b, ne0)], win=(0, 0))
    ne0, ne1 = length + 237 - k + 1, 30 - k + 1
    assert ne0 + ne1 == len(ss)
    i1, i2 = min(length, ne0), min(length + 158, ne0)
    n0, g1, g2 = int(E[ne0]), int(E[i1]), int(E[i2])
    wl = max(0, n0 - 79 * sps)
    return dict(seg=np.array([0, n - n0, n - g2, n - g1, n], np.int64), shift=np.array([n - n0, n - wl], np.int64),
                events=[(ne0, ne0 + ne1), (i2, ne0), (i1, i2), (0, i1)], win=(min(wl, g1), g1))


def shift_code(rng, dig):
    """(int16)(30 digitisation / range), src/genread.c:83"""
    return int(T.to_i16(30 * np.float64(dig) / np.float64(rng)))


def lower(raw, by):
    """int16 - int16 stored into int16: wraps"""
    return ((np.asarray(raw, np.int16).astype(np.int32) - by) & 0xffff).astype(np.uint16).view(np.int16)


def read_level(seq, ss, offset, level_mean, k, rna, meth, prefix, rng, dig):
    """the noise-free ADC code of every sample of the WHOLE read as stored, WITHOUT the level shift: both chains by src/gensig.c:270"""
    c0, c1 = chains(seq, k, rna, prefix)
    ne0 = len(c0) - k + 1
    parts = [T.read_samples(c0, ss[:ne0], offset, level_mean, k, False, meth, rng, dig)[0]]
    if c1:
        parts.append(T.read_samples(c1, ss[ne0:], offset, level_mean, k, False, meth, rng, dig)[0])
    raw = np.concatenate(parts)
    return np.ascontiguousarray(raw[::-1]) if rna else raw


def insert_of(read, k, rna, prefix, sps):
    """a read dict(sig, ss, seq, offset) -> (its segments, the same dict for the insert alone: sig, ss, and seq as it was in the pore)"""
    sg = segments(read["ss"], len(read["seq"]), k, rna, prefix, sps)
    lo, hi = sg["events"][3]
    s3, s4 = int(sg["seg"][3]), int(sg["seg"][4])
    seq = bytes(read["seq"])
    if prefix and rna:
        seq += POLYA[:k - 1]                                  # the last k-1 insert events reach into the poly-A
    return sg, dict(sig=np.asarray(read["sig"], np.int16)[s3:s4], ss=np.asarray(read["ss"])[lo:hi], seq=seq, offset=read.get("offset", 0.0))


def read_chunks_trimmed(read, k, rna, meth, prefix, sps, L, S, W, dtype="f16", norm="medmad", rng=1.0, dig=1.0):
    _, ins = insert_of(read, k, rna, prefix, sps)
    return R.read_chunks(ins["sig"], ins["ss"], ins["seq"], k, rna, meth, L, S, W, dtype, norm, ins["offset"], rng, dig)


def read_targets_trimmed(read, level_mean, k, rna, meth, prefix, sps, L, S, dtype="f16", norm="medmad", rng=1.0, dig=1.0):
    sg, ins = insert_of(read, k, rna, prefix, sps)
    d = T.read_targets(ins["sig"], ins["seq"], ins["ss"], ins["offset"], level_mean, k, rna, meth, L, S, dtype, norm, rng, dig)
    w0, w1 = sg["win"]
    if w1 > w0 and len(d["moves"]):                           # the shift rule: generation samples [w0, w1) of the insert, stored n-1-g
        n = len(ins["sig"])
        raw = T.read_samples(ins["seq"], ins["ss"], ins["offset"], level_mean, k, rna, meth, rng, dig)[0].copy()
        raw[n - w1:n - w0] = lower(raw[n - w1:n - w0], shift_code(rng, dig))
        med2, mad4 = R.stats(ins["sig"]) if norm == "medmad" else (0, 0)
        x = R.normalise(raw, med2, mad4, norm, ins["offset"], rng, dig)
        if dtype == "f16":
            with np.errstate(over="ignore"):
                x = x.astype(np.float16)
        idx = (np.arange(len(d["moves"]), dtype=np.int64) * S)[:, None] + np.arange(L, dtype=np.int64)[None, :]
        d["clean_raw"], d["clean"] = raw[idx], x[idx]
    return d


def batch_segments(reads, k, rna, prefix, sps):
    """reads: list of dict(sig, ss, seq, offset) -> (seg [n, 5], shift [n, 2]) as sqg_segments_t lays them out"""
    per = [segments(r["ss"], len(r["seq"]), k, rna, prefix, sps) for r in reads]
    return (np.stack([p["seg"] for p in per]) if per else np.zeros((0, 5), np.int64),
            np.stack([p["shift"] for p in per]) if per else np.zeros((0, 2), np.int64))


def batch_chunks_trimmed(reads, k, rna, meth, prefix, sps, L, S, W, dtype="f16", norm="medmad", rng=1.0, dig=1.0):
    """the batch's outputs as sqg_chunk_out_t lays them out (chunks_ref.batch_chunks over the inserts)"""
    ins = [insert_of(r, k, rna, prefix, sps)[1] for r in reads]
    return R.batch_chunks(ins, k, rna, meth, L, S, W, dtype, norm, rng, dig)


def batch_targets_trimmed(reads, level_mean, k, rna, meth, prefix, sps, L, S, dtype, norm, rng, dig):
    per = [read_targets_trimmed(r, level_mean, k, rna, meth, prefix, sps, L, S, dtype, norm, rng, dig) for r in reads]
    out = {key: np.concatenate([p[key] for p in per]) for key in ("clean", "clean_raw", "moves", "kmer")}
    out["chunk_off"] = np.concatenate(([0], np.cumsum([len(p["moves"]) for p in per]))).astype(np.int64)
    return out
