"""A second, vectorised statement of the sample-derived columns of include/sqg_events.h (sum, sumsq, vmin, vmax, mean, sd) and of the
rows' places (ev_read, ev_start, ev_len), for batches of millions of events: events_ref.read_events walks the events in Python.  The
sample reduction is independent of events_ref's: differences of np.cumsum over the int64 samples and their squares, np.minimum.reduceat /
np.maximum.reduceat over the events' starts, on the signal put into generation order (an RNA read is stored reversed).  mean / sd are
the header's FP64 formulas.  test_event_grids.py proves it bit-equal to events_ref.batch_events on the committed reference vectors."""
import numpy as np

SAMPLE_KEYS = ("sum", "sumsq", "vmin", "vmax", "mean", "sd")
PLACE_KEYS = ("ev_read", "ev_start", "ev_len")


def stats_fast(raw):
    """chunks_ref.stats by selection instead of sorting: (med2, mad4) of an int16 array"""
    raw = np.asarray(raw, np.int16)
    n = len(raw)
    if n == 0:
        return 0, 0
    mid = sorted({(n - 1) // 2, n // 2})
    s = np.partition(raw, mid)
    med2 = int(s[(n - 1) // 2]) + int(s[n // 2])
    d = np.partition(np.abs(2 * raw.astype(np.int32) - med2), mid)                  # (|2 v - med2| < 2^17)
    return med2, int(d[(n - 1) // 2]) + int(d[n // 2])


def batch_rows(sig, sig_off, dwell, ev_off, offset, rna, norm="pa", rng=1.0, dig=1.0, stats=None, reuse=None):
    """sig: int16 [n_samples], the batch's slab as stored; dwell: [n_events] in the order of the rows (generation order, both chains);
    offset: [n_reads]; stats: [(med2, mad4)] per read for "medmad" (default: stats_fast of the whole read); reuse: the result of an
    earlier call on the same batch, whose places and integer sums are taken (they do not depend on norm).
    -> dict of PLACE_KEYS + SAMPLE_KEYS (+ med2, mad4 [n_reads] for "medmad"), typed as sqg_event_out_t"""
    sig = np.asarray(sig, np.int16)
    sig_off, ev_off = np.asarray(sig_off, np.int64), np.asarray(ev_off, np.int64)
    d = np.asarray(dwell, np.int64)
    n_reads, ne = len(sig_off) - 1, len(d)
    assert len(sig) == sig_off[-1] and ne == ev_off[-1] and (d >= 1).all()          # (reduceat has no empty segment)
    ev_read = np.repeat(np.arange(n_reads, dtype=np.int64), np.diff(ev_off))
    ends = np.concatenate(([0], np.cumsum(d)))
    assert np.array_equal(ends[ev_off], sig_off), "a read's dwells do not add up to its samples"
    E = ends[:-1]                                                                   # first sample of every event, generation order, whole batch
    x = sig.astype(np.int64) if reuse is None else None
    if rna and reuse is None:                                                                         # generation order: every read turned round
        for r in range(n_reads):
            x[sig_off[r]:sig_off[r + 1]] = x[sig_off[r]:sig_off[r + 1]][::-1].copy()
    within = E - sig_off[ev_read]
    ev_start = (np.diff(sig_off)[ev_read] - within - d) if rna else within
    out = dict(ev_read=ev_read.astype(np.int32), ev_start=ev_start.astype(np.int64), ev_len=d.astype(np.int32))
    if reuse is not None:
        out.update({key: reuse[key] for key in ("sum", "sumsq", "vmin", "vmax")})
    elif ne == 0:
        z = np.zeros(0, np.int64)
        out.update(sum=z, sumsq=z, vmin=z.astype(np.int16), vmax=z.astype(np.int16), mean=z.astype(np.float32), sd=z.astype(np.float32))
    else:
        out["vmin"] = np.minimum.reduceat(x, E).astype(np.int16)
        out["vmax"] = np.maximum.reduceat(x, E).astype(np.int16)
        c = np.concatenate(([0], np.cumsum(x)))
        out["sum"] = c[E + d] - c[E]
        np.multiply(x, x, out=x)
        np.cumsum(x, out=c[1:])
        out["sumsq"] = c[E + d] - c[E]
        del c, x
    if norm != "pa":
        if stats is None:
            stats = [stats_fast(sig[sig_off[r]:sig_off[r + 1]]) for r in range(n_reads)]
        out["med2"] = np.array([s[0] for s in stats], np.int32).reshape(n_reads)
        out["mad4"] = np.array([s[1] for s in stats], np.int32).reshape(n_reads)
    if ne:
        # include/sqg_events.h, one rounding per operation in FP64, then one to float32
        with np.errstate(invalid="ignore", divide="ignore"):
            ln, s1 = d.astype(np.float64), out["sum"].astype(np.float64)
            m = s1 / ln
            v = (out["sumsq"].astype(np.float64) - s1 * m) / ln
            v = np.where(v < 0, np.float64(0), v)
            s = np.sqrt(v)
            if norm == "pa":
                off = np.asarray(offset, np.float64)[ev_read]
                out["mean"] = (((m + off) * np.float64(rng)) / np.float64(dig)).astype(np.float32)
                out["sd"] = ((s * np.float64(rng)) / np.float64(dig)).astype(np.float32)
            else:
                mad4 = out["mad4"].astype(np.float64)
                madp = np.where(mad4 > 0, mad4 / 4.0, 1.0)
                inv = (1.0 / (1.4826 * madp)).astype(np.float32).astype(np.float64)[ev_read]
                out["mean"] = ((m - out["med2"].astype(np.float64)[ev_read] * 0.5) * inv).astype(np.float32)
                out["sd"] = (s * inv).astype(np.float32)
    return out
