"""numpy statement of include/sqg_pileup.h: what sqg_batch_pileup must add, bit for bit.  Written from the rules of the header; no call
into the library.  It takes the per-event columns of include/sqg_events.h -- events_ref.batch_events' or Batch.events()' -- and the
reads' origins and lengths; the sums are np.add.at in wrapping integer arithmetic."""
import numpy as np

OUTPUTS = ("n", "dwell", "dwell_sq", "mean_sum", "mean_sq", "sd_sum")
BY_REF, BY_KMER = 0, 1
SPLIT_STRAND, SPLIT_METH = 1, 2
PREFIX_DNA, PREFIX_RNA = 24 + 61, 158 + 79          # bases attached in front of a DNA read / behind an RNA read (segments_ref.py)


def q(x):
    """(int64)rint((double)x * 4096): ties to even; the product is exact"""
    return np.rint(np.asarray(x, np.float32).astype(np.float64) * 4096.0).astype(np.int64)


def sampler_origin(contig_off, ref_idx, ref_pos, rlen, strand, k):
    """(key0, step) of sampled reads: the leftmost forward-strand coordinate of the k-mer at the read's base 0, and the direction"""
    minus = np.frombuffer(bytes(strand), np.uint8) == ord("-")
    key0 = np.asarray(contig_off, np.int64)[np.asarray(ref_idx)] + np.asarray(ref_pos, np.int64) + np.where(minus, np.asarray(rlen, np.int64) - k, 0)
    return key0, np.where(minus, -1, 1).astype(np.int8)


def first_insert_base(rna, prefix):
    """where the insert starts in chain 0: behind the stall and the adaptor of a DNA read, at base 0 otherwise"""
    return PREFIX_DNA if prefix and not rna else 0


def has_m(kmer, k):
    """the k-mer of base-5 rank `kmer` has an 'M': a digit 3"""
    x = np.asarray(kmer, np.int64).copy()
    m = np.zeros(x.shape, bool)
    for _ in range(k):
        m |= x % 5 == 3
        x //= 5
    return m


def eligible_and_key(ev, ev_off, key0, step, lens, k, rna, prefix, by=BY_REF, segs=0):
    """per event: (counts before the window is looked at, key, the read's step).  ev: dict of per-event columns (ev_read, and kmer / seg
    for BY_KMER); lens: the reads' own bases; chain 0 of read r holds max(lens[r] + attached - k + 1, 5) events"""
    r = np.asarray(ev["ev_read"], np.int64)
    ev_off = np.asarray(ev_off, np.int64)
    st = np.asarray(step, np.int64)[r]
    if by == BY_KMER:
        mask = segs if segs else 8
        return (st != 0) & (((mask >> np.asarray(ev["seg"], np.int64)) & 1) == 1), np.asarray(ev["kmer"]).astype(np.int64), st
    L = np.asarray(lens, np.int64)
    att = L + (0 if not prefix else PREFIX_RNA if rna else PREFIX_DNA)
    ne0 = np.where(att < k, 5, att - k + 1)
    e = np.arange(len(r), dtype=np.int64) - ev_off[r]
    j = e - first_insert_base(rna, prefix)
    ok = (st != 0) & (e < ne0[r]) & (j >= 0) & (j <= L[r] - k)
    return ok, np.asarray(key0, np.int64)[r] + st * j, st


def pileup(ev, ev_off, key0, step, lens, k, rna, prefix, by=BY_REF, split=0, segs=0, lo=0, hi=0, into=None):
    """-> (dict of the six arrays [planes, hi - lo], counted, outside).  ev: per-event columns ev_read, ev_len, mean, sd (made with the
    cfg's norm and trim) and, where the key or a split needs them, kmer and seg.  into: arrays to add to (copied), default zeros"""
    ok, key, st = eligible_and_key(ev, ev_off, key0, step, lens, k, rna, prefix, by, segs)
    S = 2 if split & SPLIT_STRAND else 1
    planes = S * (2 if split & SPLIT_METH else 1)
    plane = np.zeros(len(key), np.int64)
    if split & SPLIT_STRAND:
        plane += st < 0
    if split & SPLIT_METH:
        plane += S * has_m(np.asarray(ev["kmer"]).astype(np.int64), k)
    inside = ok & (key >= lo) & (key < hi)
    width = hi - lo
    at = (plane * width + key - lo)[inside]
    ln = np.asarray(ev["ev_len"], np.int64)[inside]
    some = ln > 0                                              # an event without a sample adds to n only
    with np.errstate(over="ignore", invalid="ignore"):
        qm, qs = q(np.asarray(ev["mean"])[inside][some]), q(np.asarray(ev["sd"])[inside][some])
        add = dict(dwell=ln[some], dwell_sq=ln[some] * ln[some], mean_sum=qm, mean_sq=qm * qm, sd_sum=qs)
        out = {}
        for name in OUTPUTS:
            dt = np.uint32 if name == "n" else np.int64
            flat = np.zeros(planes * width, dt) if into is None or into.get(name) is None else np.array(into[name], dt).reshape(-1)
            if name == "n":
                np.add.at(flat, at, np.uint32(1))
            else:
                np.add.at(flat, at[some], add[name])
            out[name] = flat.reshape(planes, width)
    return out, int(inside.sum()), int((ok & ~inside).sum())
