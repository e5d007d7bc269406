"""Plain statements of include/sqg_align.h: what sqg_batch_align must produce, bit for bit.  Written from the rule in the header, twice:

  banded(q, Lv, cfg)   (a) the banded recurrence as the header writes it: a band of 64 cells that moves with the path, the move codes,
                       the end, the traceback, the rim count.
  full(q, Lv, cfg)     (b) the same programme over the whole matrix, no band, cell by cell in Python integers.  Valid for T <= 32:
                       there a_i <= 31, so lo never moves and the band holds every target.  It shares no code with (a).

Both take one read: q the row values (Python integers), Lv the targets' levels 256 * level_raw in stored-sample order, cfg = (stay_pen,
skip_pen, cost_cap); both return (j [m] target of every row or -1, cost, edge).  batch() maps the targets to event indices."""
import numpy as np

INF = 1 << 62
BAND = 64


def row_values(sums, lens):
    """q[i] = floor(256 * sum[i] / max(len[i], 1)) in Python integers (// floors toward minus infinity)"""
    return [(256 * int(s)) // max(int(n), 1) for s, n in zip(sums, lens)]


def _cost(q, lv, cap):
    return min(abs(int(q) - int(lv)), cap)


def banded(q, Lv, cfg):
    stay_pen, skip_pen, cap = (int(v) for v in cfg)
    m, T = len(q), len(Lv)
    if m == 0:
        return np.zeros(0, np.int64), -1, 0
    if T == 0:
        return np.full(m, -1, np.int64), -1, 0
    lanes = np.arange(BAND)
    levels = np.concatenate((np.asarray(Lv, np.int64), np.zeros(BAND, np.int64)))      # (past the read: never a finite cell)
    outside = np.full(2, INF, np.int64)
    los, codes = [], []
    lo, prev, prev_lo = 0, None, 0
    for i in range(m):                                      # one row: the band's 64 cells at once, every value below 2^63
        j = lo + lanes
        lv = levels[lo:lo + BAND]
        if abs(q[i]) < 1 << 61:
            c = np.minimum(np.abs(np.int64(q[i]) - lv), cap)
        else:                                               # (a q that int64 differences cannot hold)
            c = np.array([_cost(q[i], v, cap) for v in lv], np.int64)
        if i == 0:
            D, code = np.where(j < T, c + j * skip_pen, INF), np.full(BAND, 3)
        else:
            ext = np.concatenate((outside, prev, outside))  # ext[k + 2] = D[i-1][prev_lo + k]: INF outside the band of the row before
            k = j - prev_lo + 2
            cands = np.stack((ext[k - 1], ext[k] + stay_pen, ext[k - 2] + skip_pen))
            best, code = cands.min(axis=0), cands.argmin(axis=0)      # argmin: the first of the smallest
            dead = (best >= INF) | (j >= T)
            D, code = np.where(dead, INF, best + c), np.where(dead, 3, code)
        los.append(lo); codes.append(code)
        a = lo + int(np.argmin(D))                          # the lowest j of the smallest D; lo if the whole row is INF
        prev, prev_lo = D, lo
        lo = lo + min(2, max(0, a - lo - 31))
    lo = prev_lo
    ends = [(int(prev[l]) + (T - 1 - (lo + l)) * skip_pen, lo + l) for l in range(BAND) if prev[l] < INF]
    if not ends:
        return np.full(m, -1, np.int64), -1, 0
    cost, e = min(ends)                                     # the lowest j among the smallest
    js = np.zeros(m, np.int64)
    j, edge = e, 0
    for i in range(m - 1, -1, -1):
        js[i] = j
        edge += int(j == los[i] + BAND - 1 or (j == los[i] and los[i] > 0))
        j -= (1, 0, 2, 0)[codes[i][j - los[i]]]
    return js, cost, edge


def full(q, Lv, cfg):
    stay_pen, skip_pen, cap = (int(v) for v in cfg)
    m, T = len(q), len(Lv)
    assert T <= 32, "the full matrix is the banded programme only while the band never moves"
    if m == 0:
        return np.zeros(0, np.int64), -1, 0
    if T == 0:
        return np.full(m, -1, np.int64), -1, 0
    D = {(0, j): _cost(q[0], Lv[j], cap) + j * skip_pen for j in range(T)}
    back = {}
    for i in range(1, m):
        for j in range(T):
            best, move = D.get((i - 1, j - 1), INF), 1
            if D.get((i - 1, j), INF) + stay_pen < best:
                best, move = D[(i - 1, j)] + stay_pen, 0
            if D.get((i - 1, j - 2), INF) + skip_pen < best:
                best, move = D[(i - 1, j - 2)] + skip_pen, 2
            if best < INF:
                D[(i, j)] = best + _cost(q[i], Lv[j], cap)
                back[(i, j)] = move
    cost, e = None, -1
    for j in range(T):
        if (m - 1, j) in D:
            v = D[(m - 1, j)] + (T - 1 - j) * skip_pen
            if cost is None or v < cost:
                cost, e = v, j
    if cost is None:
        return np.full(m, -1, np.int64), -1, 0
    js = np.zeros(m, np.int64)
    for i in range(m - 1, -1, -1):
        js[i] = e
        if i:
            e -= back[(i, e)]
    return js, cost, 0                                      # lo stays 0 and no target is 63: no row on the rim


def batch(row_off, sums, lens, ev_off, level_raw, rna, cfg, one=banded):
    """al_ev [n_rows], al_cost [n_reads], al_edge [n_reads] of a batch: row_off / ev_off [n_reads+1], sums / lens [n_rows], level_raw
    [n_events] as sqg_batch_events gives it"""
    n = len(row_off) - 1
    al_ev = np.zeros(int(row_off[-1]), np.int64)
    al_cost, al_edge = np.zeros(n, np.int64), np.zeros(n, np.int32)
    for r in range(n):
        a, z = int(row_off[r]), int(row_off[r + 1])
        e0, e1 = int(ev_off[r]), int(ev_off[r + 1])
        lv = level_raw[e0:e1].astype(np.int64) * 256
        if rna:
            lv = lv[::-1]
        js, cost, edge = one(row_values(sums[a:z], lens[a:z]), [int(v) for v in lv], cfg)
        ev = np.where(js < 0, -1, (e1 - 1 - js) if rna else (e0 + js))
        al_ev[a:z] = ev
        al_cost[r], al_edge[r] = cost, edge
    return dict(al_ev=al_ev, al_cost=al_cost, al_edge=al_edge)
