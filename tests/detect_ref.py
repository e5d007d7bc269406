"""Plain statement of include/sqg_detect.h: what sqg_detect_plan and sqg_batch_detect must produce, bit for bit.  Written from the rules
of the header; no call into the library.  The t-statistic is stated twice (cumulative sums, direct window slices), the peak machine
sample by sample in plain Python; sum .. sd follow sqg_events.h's formulas with len = dt_len, the statistics are chunks_ref's and the
insert's span segments_ref's."""
import math

import numpy as np

import chunks_ref as R
import segments_ref as G

DNA = (3, 6, 1.4, 9.0, 0.2)           # SQG_DETECT_DNA
RNA = (7, 14, 2.5, 9.0, 1.0)          # SQG_DETECT_RNA
PER_ROW = ("dt_read", "dt_start", "dt_len", "sum", "sumsq", "vmin", "vmax", "mean", "sd", "true_ev")
PER_READ = ("med2", "mad4")
DTYPES = dict(dt_read=np.int32, dt_start=np.int64, dt_len=np.int32, sum=np.int64, sumsq=np.int64, vmin=np.int16, vmax=np.int16,
              mean=np.float32, sd=np.float32, true_ev=np.int64, med2=np.int32, mad4=np.int32)


def tstat(x, w):
    """t_w[0..n) of the samples x as float64, by cumulative sums in exact integers"""
    x = np.asarray(x, np.int16).astype(np.int64)
    n = len(x)
    t = np.zeros(n, np.float64)
    if n < 2 * w:
        return t
    c1 = np.concatenate(([0], np.cumsum(x)))
    c2 = np.concatenate(([0], np.cumsum(x * x)))
    i = np.arange(w, n - w + 1)
    s1, s2, q = c1[i] - c1[i - w], c1[i + w] - c1[i], c2[i + w] - c2[i - w]
    N = w * (s2 - s1) ** 2
    D = w * q - s1 * s1 - s2 * s2
    assert (D >= 0).all() and (N < 1 << 51).all() and (D < 1 << 44).all()
    t[i] = np.sqrt(N.astype(np.float64) / np.where(D > 0, D, 1).astype(np.float64))
    return t


def tstat_slices(x, w):
    """the same by direct window slices in Python integers: true division of two integers below 2^53 is the IEEE quotient of their doubles"""
    x = [int(v) for v in x]
    n = len(x)
    t = [0.0] * n
    for i in range(n):
        if i < w or i > n - w:
            continue
        a, b = x[i - w:i], x[i:i + w]
        s1, s2, q = sum(a), sum(b), sum(v * v for v in a + b)
        N = w * (s2 - s1) ** 2
        D = w * q - s1 * s1 - s2 * s2
        t[i] = math.sqrt(N / (D if D > 0 else 1))
    return np.array(t, np.float64)


def boundaries(x, cfg, info=None):
    """the peak machine of the header over the samples x, sample by sample -> the recorded boundaries in order of recording.  info: a dict
    that gets how often either detector recorded ("short", "long"), how often the short one masked the long one ("masks") and how often
    the `pos > last` guard dropped a peak ("dropped")"""
    W, TH, h = (int(cfg[0]), int(cfg[1])), (float(cfg[2]), float(cfg[3])), float(cfg[4])
    n = len(x)
    t = (tstat(x, W[0]).tolist(), tstat(x, W[1]).tolist())
    pos, val, valid, masked, last = [-1, -1], [math.inf, math.inf], [False, False], [0, 0], 0
    out, seen = [], dict(short=0, long=0, masks=0, dropped=0)
    for i in range(n):
        for k in (0, 1):
            if masked[k] >= i:
                continue
            cur = t[k][i]
            if pos[k] < 0:
                if cur < val[k]:
                    val[k] = cur
                elif cur - val[k] > h:
                    val[k] = cur; pos[k] = i
            else:
                if cur > val[k]:
                    val[k] = cur; pos[k] = i
                if k == 0 and val[0] > TH[0]:
                    masked[1] = pos[0] + W[0]; pos[1] = -1; val[1] = math.inf; valid[1] = False
                    seen["masks"] += 1
                if val[k] - cur > h and val[k] > TH[k]:
                    valid[k] = True
                if valid[k] and i - pos[k] > W[k] // 2:
                    if pos[k] > last:
                        out.append(pos[k]); last = pos[k]
                        seen["long" if k else "short"] += 1
                    else:
                        seen["dropped"] += 1
                    pos[k] = -1; val[k] = cur; valid[k] = False
    if info is not None:
        for key, v in seen.items():
            info[key] = info.get(key, 0) + v
    return out


def true_events(ss, n, rna, starts):
    """the index within the read of the event with at least one sample whose stored samples hold each of `starts`"""
    d = np.asarray(ss, np.int64)
    E = np.cumsum(d) - d
    ev_start = n - E - d if rna else E
    some = np.flatnonzero(d >= 1)
    order = some[np.argsort(ev_start[some], kind="stable")]
    e = order[np.searchsorted(ev_start[order], starts, side="right") - 1]
    assert ((ev_start[e] <= starts) & (starts < ev_start[e] + d[e])).all()
    return e


def read_rows(read, cfg, k, rna, prefix, sps, norm="pa", trim=False, rng=1.0, dig=1.0, index=0, ev_off=0, info=None):
    """one read dict(sig, ss, seq, offset) -> dict of its rows (PER_ROW) and med2 / mad4.  ev_off: the read's first row of sqg_batch_events"""
    sig = np.asarray(read["sig"], np.int16)
    raw = sig.astype(np.int64)
    n = len(raw)
    b = boundaries(sig, cfg, info)
    assert all(0 < p < n for p in b) and all(q > p for p, q in zip(b, b[1:]))
    start = np.array([0] + b, np.int64)
    ln = np.diff(np.concatenate((start, [n])))
    m_rows = len(start)
    s1, s2 = np.zeros(m_rows, np.int64), np.zeros(m_rows, np.int64)
    lo, hi = np.zeros(m_rows, np.int16), np.zeros(m_rows, np.int16)
    for j in range(m_rows):
        x = raw[start[j]:start[j] + ln[j]]
        s1[j], s2[j], lo[j], hi[j] = x.sum(), (x * x).sum(), x.min(), x.max()
    span = sig
    if trim:
        sg = G.segments(np.asarray(read["ss"], np.int64), len(read["seq"]), k, rna, prefix, sps)["seg"]
        span = sig[int(sg[3]):int(sg[4])]
    med2, mad4 = R.stats(span)
    offset = np.float64(read.get("offset", 0.0))
    with np.errstate(invalid="ignore", divide="ignore"):
        dl, ds = ln.astype(np.float64), s1.astype(np.float64)
        m = ds / dl
        v = (s2.astype(np.float64) - ds * m) / dl
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
    return dict(dt_read=np.full(m_rows, index, np.int32), dt_start=start, dt_len=ln.astype(np.int32), sum=s1, sumsq=s2, vmin=lo, vmax=hi, mean=mean, sd=sd,
                true_ev=(ev_off + true_events(read["ss"], n, rna, start)).astype(np.int64), med2=med2, mad4=mad4)


def batch_rows(reads, cfg, k, rna, prefix, sps, norm="pa", trim=False, rng=1.0, dig=1.0, info=None):
    """reads: list of dict(sig, ss, seq, offset) -> the batch's outputs as sqg_detect_out_t lays them out, and det_off"""
    ev_off = np.concatenate(([0], np.cumsum([len(r["ss"]) for r in reads]))).astype(np.int64)
    per = [read_rows(r, cfg, k, rna, prefix, sps, norm, trim, rng, dig, i, int(ev_off[i]), info) for i, r in enumerate(reads)]
    out = {key: (np.concatenate([p[key] for p in per]) if per else np.zeros(0)).astype(DTYPES[key]) for key in PER_ROW}
    for key in PER_READ:
        out[key] = np.array([p[key] for p in per], DTYPES[key])
    out["det_off"] = np.concatenate(([0], np.cumsum([len(p["dt_len"]) for p in per]))).astype(np.int64)
    return out
