"""numpy statement of include/sqg_events.h: what sqg_batch_events must produce, bit for bit.  Written from the rules of the header; no
call into the library.  The statistics and inv are chunks_ref's, the k-mer rank and the level code targets_ref's, the chains and the
event ranges of the segments segments_ref's (the headers those rules belong to)."""
import numpy as np

import chunks_ref as R
import segments_ref as G
import targets_ref as T

PER_EVENT = ("ev_read", "ev_start", "ev_len", "sum", "sumsq", "vmin", "vmax", "kmer", "level_raw", "seg", "mean", "sd")
PER_READ = ("med2", "mad4")
DTYPES = dict(ev_read=np.int32, ev_start=np.int64, ev_len=np.int32, sum=np.int64, sumsq=np.int64, vmin=np.int16, vmax=np.int16, kmer=np.uint32,
              level_raw=np.int16, seg=np.uint8, mean=np.float32, sd=np.float32, med2=np.int32, mad4=np.int32)


def read_events(read, level_mean, k, rna, meth, prefix, sps, norm="pa", trim=False, rng=1.0, dig=1.0, index=0):
    """one read dict(sig, ss, seq, offset) -> dict of its rows (PER_EVENT) and med2 / mad4.  ss: the dwells of chain 0, then chain 1, as
    the reference writes them (a read shorter than a k-mer: those of its five stand-in events); sps: (int)dwell_mean"""
    raw = np.asarray(read["sig"], np.int16).astype(np.int64)
    d = np.asarray(read["ss"], np.int64)
    n, ne = len(raw), len(d)
    offset = np.float64(read.get("offset", 0.0))
    c0, c1 = G.chains(read["seq"], k, rna, prefix)
    ne0 = len(c0) - k + 1
    ne1 = len(c1) - k + 1 if c1 else 0
    assert ne == ne0 + ne1 and int(d.sum()) == n, (ne, ne0, ne1, int(d.sum()), n)
    E = np.cumsum(d) - d                                                          # over both chains, generation order
    start = n - E - d if rna else E
    # sum, sumsq, vmin, vmax over raw[start, start + len): stated event by event
    s1, s2 = np.zeros(ne, np.int64), np.zeros(ne, np.int64)
    lo, hi = np.zeros(ne, np.int16), np.zeros(ne, np.int16)
    for e in range(ne):
        x = raw[start[e]:start[e] + d[e]]
        s1[e], s2[e], lo[e], hi[e] = x.sum(), (x * x).sum(), x.min(), x.max()
    rank = np.concatenate([T.kmer_ranks(c0, k, meth)] + ([T.kmer_ranks(c1, k, meth)] if c1 else []))
    level = np.asarray(level_mean, np.float32)[rank].astype(np.float64)
    level_raw = T.to_i16(level * np.float64(dig) / np.float64(rng) - offset)       # sqg_targets.h's clean_raw, no level shift
    sg = G.segments(d, len(read["seq"]), k, rna, prefix, sps)
    seg = np.full(ne, 255, np.uint8)
    for q, (a, b) in enumerate(sg["events"]):
        seg[a:b] = q
    assert (seg <= 3).all()
    span = np.asarray(read["sig"], np.int16)[int(sg["seg"][3]):int(sg["seg"][4])] if trim else np.asarray(read["sig"], np.int16)
    med2, mad4 = R.stats(span)
    with np.errstate(invalid="ignore", divide="ignore"):
        ln = d.astype(np.float64)
        m = s1.astype(np.float64) / ln
        v = (s2.astype(np.float64) - s1.astype(np.float64) * m) / ln
        v = np.where(v < 0, np.float64(0), v)
        s = np.sqrt(v)
        if norm == "pa":
            mean = (((m + offset) * np.float64(rng)) / np.float64(dig)).astype(np.float32)
            sd = ((s * np.float64(rng)) / np.float64(dig)).astype(np.float32)
        else:
            madp = mad4 / 4.0 if mad4 > 0 else 1.0
            inv = np.float64(np.float32(1.0 / (1.4826 * madp)))
            mean = ((m - np.float64(med2) * 0.5) * inv).astype(np.float32)
            sd = (s * inv).astype(np.float32)
    return dict(ev_read=np.full(ne, index, np.int32), ev_start=start.astype(np.int64), ev_len=d.astype(np.int32), sum=s1, sumsq=s2, vmin=lo, vmax=hi,
                kmer=rank.astype(np.uint32), level_raw=level_raw, seg=seg, mean=mean, sd=sd, med2=med2, mad4=mad4, segments=sg["seg"])


def batch_events(reads, level_mean, k, rna, meth, prefix, sps, norm="pa", trim=False, rng=1.0, dig=1.0):
    """reads: list of dict(sig, ss, seq, offset) -> the batch's outputs as sqg_event_out_t lays them out, and ev_off"""
    per = [read_events(r, level_mean, k, rna, meth, prefix, sps, norm, trim, rng, dig, i) for i, r in enumerate(reads)]
    out = {key: (np.concatenate([p[key] for p in per]) if per else np.zeros(0)).astype(DTYPES[key]) for key in PER_EVENT}
    for key in PER_READ:
        out[key] = np.array([p[key] for p in per], DTYPES[key])
    out["ev_off"] = np.concatenate(([0], np.cumsum([len(p["ev_len"]) for p in per]))).astype(np.int64)
    return out
