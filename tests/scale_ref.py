"""Plain statements of include/sqg_scale.h: what sqg_batch_scale and sqg_batch_align_scaled must produce, bit for bit.  The rule of
sqg_batch_scale is written twice, from the header, and the two share no code:

  by_read(...)      read by read, row by row, in Python integers -- exact at any size, wrapped to 64 bits where the header says the sums
                    wrap -- and np.float64 scalars, one operation per line.
  vectorised(...)   the whole batch at once: np.add.at on wrapping int64, the derived values on float64 arrays.

Both take row_off / ev_off [n_reads+1], sums / lens [n_rows], level_raw [n_events] as sqg_batch_events gives it, the mode and, for FIT,
ev [n_rows]; both return a dict of OUTPUTS, [n_reads] each, in the dtypes of the device's.

The scaled aligner is align_ref's: row_values -> the header's clamp and scaling (scaled_values) -> align_ref.banded / full unchanged."""
import numpy as np

import align_ref as A

MOMENTS, FIT = 0, 1
OUTPUTS = ("n", "nx", "sy", "syy", "sx", "sxx", "sxy", "gain", "shift", "rd_dropped")
DTYPES = {k: (np.int32 if k in ("gain", "shift", "rd_dropped") else np.int64) for k in OUTPUTS}
Y_MAX, Q_MAX, GAIN_MAX = 1 << 20, 1 << 26, 1 << 20


def _wrap(v):
    """a Python integer as the int64 of its low 64 bits"""
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >> 63 else v


def row_value(s, n):
    """y = clamp(floor(16 * sum / max(len, 1)), -2^20, 2^20), the product modulo 2^64"""
    return min(max(_wrap(16 * int(s)) // max(int(n), 1), -Y_MAX), Y_MAX)


def estimate(mode, n, nx, sy, syy, sx, sxx, sxy):
    """(gain, shift) from one read's sums (int64 values as Python integers): the header's lines, one rounding each"""
    if n == 0 or nx == 0:
        return 65536, 0
    f = np.float64
    my = f(sy) / f(n)
    mx = f(sx) / f(nx)
    ey = f(syy) / f(n)
    ex = f(sxx) / f(nx)
    vy = ey - my * my
    vx = ex - mx * mx
    g = f(1.0)
    if mode == FIT:
        exy = f(sxy) / f(n)
        cxy = exy - mx * my
        if vy > 0:
            g = cxy / vy
    elif vy > 0 and vx > 0:
        g = np.sqrt(vx / vy)
    g = min(max(g, f(2.0 ** -16)), f(16.0))
    s = mx - g * my
    gain = int(np.rint(g * f(65536.0)))
    shift = int(min(max(np.rint(s * f(16.0)), f(-2.0 ** 26)), f(2.0 ** 26)))
    return gain, shift


def by_read(row_off, sums, lens, ev_off, level_raw, mode, ev=None):
    nr = len(row_off) - 1
    out = {k: np.zeros(nr, DTYPES[k]) for k in OUTPUTS}
    if nr and int(row_off[-1]) == 0:                        # the header's n_rows == 0: no target is read either
        out["gain"][:] = 65536
        return out
    for r in range(nr):
        a, z, e0, e1 = int(row_off[r]), int(row_off[r + 1]), int(ev_off[r]), int(ev_off[r + 1])
        n = nx = sy = syy = sx = sxx = sxy = dropped = 0
        if mode == MOMENTS:
            for i in range(a, z):
                y = row_value(sums[i], lens[i])
                n, sy, syy = n + 1, sy + y, syy + y * y
            for j in range(e0, e1):
                x = 16 * int(level_raw[j])
                nx, sx, sxx = nx + 1, sx + x, sxx + x * x
        else:
            for i in range(a, z):
                e = int(ev[i])
                if not e0 <= e < e1:
                    dropped += 1
                    continue
                y, x = row_value(sums[i], lens[i]), 16 * int(level_raw[e])
                n, sy, syy, sx, sxx, sxy = n + 1, sy + y, syy + y * y, sx + x, sxx + x * x, sxy + x * y
            nx = n
        vals = [_wrap(v) for v in (n, nx, sy, syy, sx, sxx, sxy)]
        for k, v in zip(OUTPUTS[:7], vals):
            out[k][r] = v
        out["gain"][r], out["shift"][r] = estimate(mode, *vals)
        out["rd_dropped"][r] = dropped
    return out


def vectorised(row_off, sums, lens, ev_off, level_raw, mode, ev=None):
    row_off, ev_off = np.asarray(row_off, np.int64), np.asarray(ev_off, np.int64)
    nr, n_rows = len(row_off) - 1, int(row_off[-1])
    out = {k: np.zeros(nr, DTYPES[k]) for k in OUTPUTS}
    out["gain"][:] = 65536
    if nr == 0 or n_rows == 0:
        return out
    s, ln = np.asarray(sums, np.int64)[:n_rows], np.maximum(np.asarray(lens, np.int64)[:n_rows], 1)
    y = np.clip((s.view(np.uint64) << np.uint64(4)).view(np.int64) // ln, -Y_MAX, Y_MAX)
    x_all = 16 * np.asarray(level_raw, np.int64)
    rd = np.repeat(np.arange(nr), np.diff(row_off))
    with np.errstate(over="ignore"):
        if mode == MOMENTS:
            out["n"][:], out["nx"][:] = np.diff(row_off), np.diff(ev_off)
            np.add.at(out["sy"], rd, y); np.add.at(out["syy"], rd, y * y)
            er = np.repeat(np.arange(nr), np.diff(ev_off))
            np.add.at(out["sx"], er, x_all); np.add.at(out["sxx"], er, x_all * x_all)
        else:
            e = np.asarray(ev, np.int64)[:n_rows]
            ok = (e >= ev_off[rd]) & (e < ev_off[rd + 1])
            np.add.at(out["rd_dropped"], rd[~ok], 1)
            rd, y, x = rd[ok], y[ok], x_all[e[ok]]
            np.add.at(out["n"], rd, 1)
            out["nx"] = out["n"].copy()
            for k, v in (("sy", y), ("syy", y * y), ("sx", x), ("sxx", x * x), ("sxy", x * y)):
                np.add.at(out[k], rd, v)
    have = (out["n"] != 0) & (out["nx"] != 0)
    with np.errstate(all="ignore"):
        dn, dnx = out["n"].astype(np.float64), out["nx"].astype(np.float64)
        my, mx = out["sy"].astype(np.float64) / dn, out["sx"].astype(np.float64) / dnx
        vy = out["syy"].astype(np.float64) / dn - my * my
        vx = out["sxx"].astype(np.float64) / dnx - mx * mx
        if mode == FIT:
            cxy = out["sxy"].astype(np.float64) / dn - mx * my
            g = np.where(vy > 0, cxy / vy, 1.0)
        else:
            g = np.where((vy > 0) & (vx > 0), np.sqrt(vx / vy), 1.0)
        g = np.minimum(np.maximum(g, 2.0 ** -16), 16.0)
        sh = np.minimum(np.maximum(np.rint((mx - g * my) * 16.0), -2.0 ** 26), 2.0 ** 26)
        out["gain"] = np.where(have, np.rint(g * 65536.0), 65536).astype(np.int32)
        out["shift"] = np.where(have, sh, 0).astype(np.int32)
    return out


def scaled_values(sums, lens, gain, shift):
    """q of one read's rows under (gain, shift): q0 clamped, scaled with a floor, clamped; gain and shift clamped into their ranges"""
    g, s = min(max(int(gain), 1), GAIN_MAX), min(max(int(shift), -Q_MAX), Q_MAX)
    q0 = [min(max(q, -Q_MAX), Q_MAX) for q in A.row_values(sums, lens)]
    return [min(max(((g * q) >> 16) + s, -Q_MAX), Q_MAX) for q in q0]       # (Python's >> of a negative integer is a floor)


def align_scaled(row_off, sums, lens, ev_off, level_raw, rna, cfg, gain, shift, one=A.banded):
    """align_ref.batch with every read's row values scaled"""
    n = len(row_off) - 1
    al_ev = np.zeros(int(row_off[-1]), np.int64)
    al_cost, al_edge = np.zeros(n, np.int64), np.zeros(n, np.int32)
    for r in range(n):
        a, z, e0, e1 = int(row_off[r]), int(row_off[r + 1]), int(ev_off[r]), int(ev_off[r + 1])
        lv = np.asarray(level_raw[e0:e1]).astype(np.int64) * 256
        if rna:
            lv = lv[::-1]
        js, cost, edge = one(scaled_values(sums[a:z], lens[a:z], gain[r], shift[r]), [int(v) for v in lv], cfg)
        al_ev[a:z] = np.where(js < 0, -1, (e1 - 1 - js) if rna else (e0 + js))
        al_cost[r], al_edge[r] = cost, edge
    return dict(al_ev=al_ev, al_cost=al_cost, al_edge=al_edge)
