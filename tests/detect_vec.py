"""A second, vectorised statement of the rows of include/sqg_detect.h for batches of millions of rows: detect_ref.read_rows walks the
rows in Python.  The boundaries stay detect_ref.boundaries' (the peak machine, sample by sample); what is stated again is everything
between them: the rows' places, the sample-derived columns -- events_vec.batch_rows with the rows' lengths where it takes the dwells: a
detected row is a run of stored samples as an event of a DNA read is -- and true_ev by one np.searchsorted over the first stored sample
of every true event.  DNA only (stored order is generation order).  test_event_grids.py proves it bit-equal to detect_ref.batch_rows.
batch_rows_of_reads takes what detect_ref.batch_rows takes, any chemistry: the rows' columns the same vectorised way, true_ev and the
statistics read by read as detect_ref states them; test_sharded_consumers.py proves it bit-equal on RNA, prefix, trimmed and short reads."""
import numpy as np

import chunks_ref as R
import detect_ref as D
import events_vec as VEC
import segments_ref as G

PER_ROW = ("dt_read", "dt_start", "dt_len", "sum", "sumsq", "vmin", "vmax", "mean", "sd", "true_ev")


def batch_rows(sig, sig_off, starts, dwell, ev_off, offset, norm="pa", rng=1.0, dig=1.0, reuse=None):
    """sig: int16 [n_samples], the batch's slab; starts: per read the first sample of every row, [0] + detect_ref.boundaries(read);
    dwell: [n_events] of the true events, every one at least 1; reuse: the result of an earlier call on the same batch and starts.
    -> dict of PER_ROW, det_off (+ med2, mad4 [n_reads] over the whole reads for "medmad"), typed as sqg_detect_out_t"""
    sig_off, ev_off = np.asarray(sig_off, np.int64), np.asarray(ev_off, np.int64)
    d = np.asarray(dwell, np.int64)
    n_reads = len(sig_off) - 1
    assert len(starts) == n_reads and all(len(s) and s[0] == 0 for s in starts) and (d >= 1).all()
    det_off = np.concatenate(([0], np.cumsum([len(s) for s in starts]))).astype(np.int64)
    dt_start = np.concatenate([np.asarray(s, np.int64) for s in starts])
    dt_read = np.repeat(np.arange(n_reads, dtype=np.int64), np.diff(det_off))
    at = sig_off[dt_read] + dt_start                                                # the row's first sample in the slab
    nxt = np.concatenate((at[1:], sig_off[-1:]))                                    # a read's last row ends where the next read starts
    dt_len = nxt - at
    assert (dt_len >= 1).all() and np.array_equal(nxt[det_off[1:] - 1], sig_off[1:])
    w = VEC.batch_rows(sig, sig_off, dt_len, det_off, offset, False, norm, rng, dig, reuse=reuse)
    assert np.array_equal(w["ev_start"], dt_start) and np.array_equal(w["ev_read"], dt_read)
    first = np.cumsum(d) - d                                                        # the true events' first samples in the slab: ascending, distinct
    assert np.array_equal(first[ev_off[:-1]], sig_off[:-1]) and int(d.sum()) == sig_off[-1]
    out = dict(dt_read=w["ev_read"], dt_start=w["ev_start"], dt_len=w["ev_len"], true_ev=(np.searchsorted(first, at, side="right") - 1).astype(np.int64), det_off=det_off)
    out.update({key: w[key] for key in VEC.SAMPLE_KEYS + (("med2", "mad4") if norm != "pa" else ())})
    return out


def batch_rows_of_reads(reads, cfg, k, rna, prefix, sps, norm="pa", trim=False, rng=1.0, dig=1.0, info=None):
    """detect_ref.batch_rows(the same arguments), the rows' sample-derived columns by events_vec instead of a walk over the rows.  A
    detected row is a run of STORED samples whatever the chemistry, so events_vec is asked for a DNA batch whose "dwells" are the rows'
    lengths; the boundaries, true_ev (detect_ref.true_events) and the statistics' span (segments_ref) are detect_ref's own, per read"""
    n_reads = len(reads)
    if n_reads == 0:
        return D.batch_rows(reads, cfg, k, rna, prefix, sps, norm, trim, rng, dig, info)
    sigs = [np.asarray(r["sig"], np.int16) for r in reads]
    sig_off = np.concatenate(([0], np.cumsum([len(x) for x in sigs]))).astype(np.int64)
    ev_off = np.concatenate(([0], np.cumsum([len(r["ss"]) for r in reads]))).astype(np.int64)
    starts = [np.array([0] + D.boundaries(x, cfg, info), np.int64) for x in sigs]
    det_off = np.concatenate(([0], np.cumsum([len(s) for s in starts]))).astype(np.int64)
    dt_len = np.concatenate([np.diff(np.concatenate((s, [len(x)]))) for s, x in zip(starts, sigs)])
    stats = []
    for r, x in zip(reads, sigs):
        span = x
        if trim:
            sg = G.segments(np.asarray(r["ss"], np.int64), len(r["seq"]), k, rna, prefix, sps)["seg"]
            span = x[int(sg[3]):int(sg[4])]
        stats.append(R.stats(span))
    w = VEC.batch_rows(np.concatenate(sigs), sig_off, dt_len, det_off, [r.get("offset", 0.0) for r in reads], False, norm, rng, dig, stats=stats)
    assert np.array_equal(w["ev_start"], np.concatenate(starts))
    true_ev = np.concatenate([ev_off[i] + D.true_events(r["ss"], len(x), rna, s) for i, (r, x, s) in enumerate(zip(reads, sigs, starts))])
    out = dict(dt_read=w["ev_read"], dt_start=w["ev_start"], dt_len=w["ev_len"], true_ev=true_ev.astype(np.int64), det_off=det_off,
               med2=np.array([s[0] for s in stats], np.int32), mad4=np.array([s[1] for s in stats], np.int32))
    out.update({key: w[key] for key in VEC.SAMPLE_KEYS})
    return out
