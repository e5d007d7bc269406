"""numpy statement of include/sqg_sites.h: what sqg_site_plan and sqg_batch_sites must produce, bit for bit.  Written from the rules of
the header; no call into the library.  The normalisation, the statistics and the label codes are chunks_ref's (the header refers to
sqg_chunks.h for them)."""
from collections import namedtuple

import numpy as np

import chunks_ref as R

# L win_len, before, f focus, B ctx_len, cb ctx_before; dtype "f16" | "f32", norm "medmad" | "pa"
Cfg = namedtuple("Cfg", "L before f B cb dtype norm", defaults=(0, 0, "f16", "medmad"))
KEYS = ("signal", "label", "site_read", "site_pos", "win_start", "context", "ctx_start")


def cfg(L, before=None, f=None, B=0, cb=None, dtype="f16", norm="medmad", k=None):
    """the defaults of Batch.sites: before = L / 2, focus = k / 2, ctx_before = B / 2"""
    return Cfg(L, L // 2 if before is None else before, k // 2 if f is None else f, B, B // 2 if cb is None else cb, dtype, norm)


def candidates(seq, meth):
    """every base position p with p + 1 < len, read[p+1] == 'G' and read[p] == 'C' (or 'M' in a methylation context): upper case only"""
    s = np.frombuffer(bytes(seq), np.uint8)
    if len(s) < 2:
        return np.zeros(0, np.int64)
    first = (s[:-1] == ord("C")) | ((s[:-1] == ord("M")) if meth else False)
    return np.flatnonzero(first & (s[1:] == ord("G"))).astype(np.int64)


def read_sites(sig, ss, seq, k, meth, c, offset=0.0, rng=1.0, dig=1.0):
    """one read -> dict(med2, mad4, dropped, signal [ns, L], label, site_pos, win_start [ns], context [ns, B], ctx_start [ns, B + 1]);
    dropped: the candidates that are no sites"""
    raw = np.asarray(sig, np.int16)
    med2, mad4 = R.stats(raw)
    L, B = c.L, c.B
    fdt = np.float16 if c.dtype == "f16" else np.float32
    s = np.frombuffer(bytes(seq), np.uint8)
    ln = len(s)
    pos, w0s = [], []
    dropped = 0
    if ln >= k:
        d = np.asarray(ss, np.int64)
        ne = ln - k + 1
        assert len(d) == ne, f"{len(d)} dwells for {ne} events"
        E = np.cumsum(d) - d
        n = int(d.sum())
        assert n == len(raw), f"{n} samples of dwell for {len(raw)} stored"
        for p in candidates(seq, meth):
            a = int(p) - c.f
            w0 = int(E[a]) - c.before if 0 <= a < ne else -1
            if 0 <= a < ne and w0 >= 0 and w0 + L <= n:
                pos.append(int(p)); w0s.append(w0)
            else:
                dropped += 1
    ns = len(pos)
    x = R.normalise(raw, med2, mad4, c.norm, offset, rng, dig)
    if c.dtype == "f16":
        with np.errstate(over="ignore"):
            x = x.astype(np.float16)
    out = dict(med2=med2, mad4=mad4, dropped=dropped, signal=np.zeros((ns, L), fdt), label=np.zeros(ns, np.uint8),
               site_pos=np.array(pos, np.int32), win_start=np.array(w0s, np.int64),
               context=np.zeros((ns, B), np.uint8), ctx_start=np.zeros((ns, B + 1), np.int32))
    codes = (R._CODE_METH if meth else R._CODE)[s]
    for j, (p, w0) in enumerate(zip(pos, w0s)):
        out["signal"][j] = x[w0:w0 + L]
        out["label"][j] = 1 if s[p] == ord("M") else 0
        for i in range(B + 1):
            q = p - c.cb + i                                # the base; its event is q - f
            if i < B and 0 <= q < ln:
                out["context"][j, i] = codes[q]
            e = q - c.f
            X = 0 if e <= 0 else n if e >= ne else int(E[e])
            out["ctx_start"][j, i] = min(max(X - w0, 0), L)
    return out


def batch_sites(reads, k, meth, c, rng=1.0, dig=1.0):
    """reads: list of dict(sig, ss, seq, offset) -> the batch's outputs as sqg_site_out_t lays them out, site_off, and dropped per read"""
    per = [read_sites(r["sig"], r["ss"], r["seq"], k, meth, c, r.get("offset", 0.0), rng, dig) for r in reads]
    fdt = np.float16 if c.dtype == "f16" else np.float32
    empty = dict(signal=np.zeros((0, c.L), fdt), label=np.zeros(0, np.uint8), site_pos=np.zeros(0, np.int32), win_start=np.zeros(0, np.int64),
                 context=np.zeros((0, c.B), np.uint8), ctx_start=np.zeros((0, c.B + 1), np.int32))
    out = {key: np.concatenate([p[key] for p in per]) if per else empty[key] for key in empty}
    out["site_read"] = np.concatenate([np.full(len(p["label"]), i, np.int32) for i, p in enumerate(per)]) if per else np.zeros(0, np.int32)
    out["med2"] = np.array([p["med2"] for p in per], np.int32)
    out["mad4"] = np.array([p["mad4"] for p in per], np.int32)
    out["site_off"] = np.concatenate(([0], np.cumsum([len(p["label"]) for p in per]))).astype(np.int64)
    out["dropped"] = np.array([p["dropped"] for p in per], np.int64)
    return out


def moves_in_window(ctx_start_row, L):
    """the move table ctx_start implies inside its window: 1 at every boundary in [0, L) where a new context base begins.  Boundaries
    clamped to 0 by the window's left edge are no event starts unless the event really starts there -- the caller compares only rows whose
    context covers the window"""
    m = np.zeros(L, np.uint8)
    b = np.asarray(ctx_start_row, np.int64)
    m[b[(b >= 0) & (b < L)]] = 1
    return m
