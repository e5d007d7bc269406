"""numpy statement of include/sqg_collapse.h: what sqg_batch_collapse must write and sqg_batch_pileup_rows must add, bit for bit.
Written from the rules of the header; no call into the library.  The sums are np.add.at in wrapping integer arithmetic, mean / sd the
formulas of events_ref on the summed columns, eligibility, key and plane pileup_ref's."""
import numpy as np

import pileup_ref as PR

OUTPUTS = ("ob_rows", "ob_len", "ob_sum", "ob_sumsq", "mean", "sd", "rd_dropped")


def _wrap(x):
    """int64 values as the uint64 of the same bits: sums of those wrap modulo 2^64 without a warning"""
    return np.asarray(x, np.int64).view(np.uint64)


def collapse(row_off, ev, sum, sumsq, len, ev_off, norm="pa", offset=None, rng=1.0, dig=1.0, med2=None, mad4=None):      # noqa: A002  (the header's names)
    """-> dict of OUTPUTS.  row_off [n_reads+1]: the rows of every read; ev, sum, sumsq, len [n_rows] (sumsq None: zeros); ev_off
    [n_reads+1]: the batch's events.  norm "pa": offset [n_reads], rng, dig; "medmad": med2, mad4 [n_reads] of the span trim selects"""
    row_off, ev_off = np.asarray(row_off, np.int64), np.asarray(ev_off, np.int64)
    n_reads, n_rows, n_events = row_off.size - 1, int(row_off[-1]), int(ev_off[-1])
    ev, ln = np.asarray(ev, np.int64)[:n_rows], np.asarray(len, np.int64)[:n_rows]
    s1 = np.asarray(sum, np.int64)[:n_rows]
    s2 = np.zeros(n_rows, np.int64) if sumsq is None else np.asarray(sumsq, np.int64)[:n_rows]
    rd = np.repeat(np.arange(n_reads), np.diff(row_off))                                   # the read of every row
    counts = (ev >= ev_off[rd]) & (ev < ev_off[rd + 1])
    dropped = np.bincount(rd[~counts], minlength=n_reads).astype(np.int32)
    at = ev[counts]
    some = ln[counts] >= 1                                                                 # a row with len < 1 adds to ob_rows only
    rows = np.zeros(n_events, np.uint32)
    np.add.at(rows, at, np.uint32(1))
    ob = {}
    for name, col in (("ob_len", ln), ("ob_sum", s1), ("ob_sumsq", s2)):
        acc = np.zeros(n_events, np.uint64)
        np.add.at(acc, at[some], _wrap(col[counts][some]))
        ob[name] = acc.view(np.int64)
    # mean / sd: events_ref's expressions on (double)ob_len, (double)ob_sum, (double)ob_sumsq of the event's read
    er = np.repeat(np.arange(n_reads), np.diff(ev_off))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        dl, ds, dq = ob["ob_len"].astype(np.float64), ob["ob_sum"].astype(np.float64), ob["ob_sumsq"].astype(np.float64)
        m = ds / dl
        v = (dq - ds * m) / dl
        v = np.where(v < 0, np.float64(0), v)
        s = np.sqrt(v)
        if norm == "pa":
            off = np.asarray(offset, np.float64)[er]
            mean = (((m + off) * np.float64(rng)) / np.float64(dig)).astype(np.float32)
            sd = ((s * np.float64(rng)) / np.float64(dig)).astype(np.float32)
        else:
            md2, md4 = np.asarray(med2, np.int64), np.asarray(mad4, np.int64)
            madp = np.where(md4 > 0, md4 / 4.0, 1.0)
            inv = (1.0 / (1.4826 * madp)).astype(np.float32).astype(np.float64)[er]
            mean = ((m - md2.astype(np.float64)[er] * 0.5) * inv).astype(np.float32)
            sd = (s * inv).astype(np.float32)
    none = ob["ob_len"] <= 0
    mean, sd = np.where(none, np.float32(0), mean).astype(np.float32), np.where(none, np.float32(0), sd).astype(np.float32)
    return dict(ob_rows=rows, mean=mean, sd=sd, rd_dropped=dropped, **ob)


def pileup_rows(ob, ev, ev_off, key0, step, lens, k, rna, prefix, by=PR.BY_REF, split=0, segs=0, lo=0, hi=0, into=None):
    """-> (dict of the six arrays [planes, hi - lo], counted, outside, unseen, dropped).  ob: collapse()'s result under the cfg's norm and
    trim; ev: the per-event columns pileup_ref.eligible_and_key takes (ev_read, and kmer / seg where the key or a split needs them)"""
    ok, key, st = PR.eligible_and_key(ev, ev_off, key0, step, lens, k, rna, prefix, by, segs)
    S = 2 if split & PR.SPLIT_STRAND else 1
    planes = S * (2 if split & PR.SPLIT_METH else 1)
    plane = np.zeros(key.size, np.int64)
    if split & PR.SPLIT_STRAND:
        plane += st < 0
    if split & PR.SPLIT_METH:
        plane += S * PR.has_m(np.asarray(ev["kmer"]).astype(np.int64), k)
    seen = ob["ob_rows"] != 0
    inside = ok & seen & (key >= lo) & (key < hi)
    width = hi - lo
    at = (plane * width + key - lo)[inside]
    ln = ob["ob_len"][inside]
    some = ln > 0                                              # an observed event without a sample adds to n only
    with np.errstate(over="ignore", invalid="ignore"):
        qm, qs = PR.q(ob["mean"][inside][some]), PR.q(ob["sd"][inside][some])
        add = dict(dwell=ln[some], dwell_sq=(_wrap(ln[some]) * _wrap(ln[some])).view(np.int64), mean_sum=qm, mean_sq=qm * qm, sd_sum=qs)
        out = {}
        for name in PR.OUTPUTS:
            dt = np.uint32 if name == "n" else np.int64
            flat = np.zeros(planes * width, dt) if into is None or into.get(name) is None else np.array(into[name], dt).reshape(-1)
            if name == "n":
                np.add.at(flat, at, np.uint32(1))
            else:
                np.add.at(flat, at[some], add[name])
            out[name] = flat.reshape(planes, width)
    return out, int(inside.sum()), int((ok & seen & ~inside).sum()), int((ok & ~seen).sum()), int(ob["rd_dropped"].sum())
