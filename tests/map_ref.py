"""Plain statements of include/sqg_map.h: what sqg_map_track and sqg_batch_map must produce, bit for bit.  The programme is written from
the rule in the header, twice:

  by_rows(q, Lv, cfg)   (a) row by row, vectorised over u, the start of the path carried with the cell (S).
  by_matrix(q, Lv, cfg) (b) the full matrix cell by cell in Python integers with stored move codes, then a traceback from the end.  It
                        shares no code with (a) and is used for m * W <= 2 * 10^5.

Both take one read on one strand: q the row values, Lv the strand's levels in u order (NONE where there is none), cfg = (stay_pen,
skip_pen, cost_cap); both return (cost, e, S) -- the end cost, the end and the start in u -- or None for m == 0 or W == 0.
strand_levels() turns the track into a strand's Lv, read_rows() a read's rows into q, batch() the per-read outputs, track() the track."""
import numpy as np

NONE = -(1 << 31)
I64_MIN = -(1 << 63)
OUTPUTS = ("map_cost", "map_step", "map_key0", "map_key1", "map_cost_other")
DTYPES = dict(map_cost=np.int32, map_step=np.int8, map_key0=np.int64, map_key1=np.int64, map_cost_other=np.int32)
DEFAULT = (4096, 4096, 65536, 0, 256, 3)
Q_MAX, LV_MAX, GAIN_MAX = 1 << 26, 1 << 23, 1 << 20
BIG = 1 << 40               # an absent candidate: above every D, which stays below 2^30
ABSENT = np.int32(1 << 30)  # the same in (a)'s 32-bit rows


# ------------------------------------------------------------------------------------------------ the rows
def _wrap(v):
    """two's complement of v modulo 2^64"""
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >> 63 else v


def row_values(sums, lens, gain=None, shift=None):
    """q of rows: sqg_scale.h's q0 (the product modulo 2^64, a floor, the clamp) and, under a scale, its q"""
    out = []
    for s, n in zip(sums, lens):
        q = _wrap(256 * int(s)) // max(int(n), 1)           # (// floors toward minus infinity)
        q = min(max(q, -Q_MAX), Q_MAX)
        if gain is not None:
            g, sh = min(max(int(gain), 1), GAIN_MAX), min(max(int(shift), -Q_MAX), Q_MAX)
            q = min(max(((g * q) >> 16) + sh, -Q_MAX), Q_MAX)
        out.append(q)
    return out


def read_rows(r, row_off, sums, lens, cfg, scale=None):
    """q of the rows read r maps: m = clamp(rows - row_first, 0, row_count) from row_off[r] + row_first on"""
    first, count = cfg[3], cfg[4]
    m = min(max(int(row_off[r + 1]) - int(row_off[r]) - first, 0), count)
    a = int(row_off[r]) + first
    g, sh = (None, None) if scale is None else (scale[0][r], scale[1][r])
    return row_values(sums[a:a + m], lens[a:a + m], g, sh)


def strand_levels(fwd, rev, minus):
    """Lv in u order, clamped: '+' fwd[u], '-' rev[W - 1 - u]"""
    lv = np.asarray(rev if minus else fwd, np.int64)
    lv = lv[::-1] if minus else lv
    return np.where(lv == NONE, NONE, np.clip(lv, -LV_MAX, LV_MAX))


# ------------------------------------------------------------------------------------------------ (a)
def by_rows(q, Lv, cfg):
    stay, skip, cap = (int(v) for v in cfg[:3])
    m, W = len(q), len(Lv)
    if m == 0 or W == 0:
        return None
    Lv = np.asarray(Lv, np.int64)
    none = Lv == NONE
    lv = np.where(none, 0, Lv).astype(np.int32)             # (32 bits hold every value: |q| <= 2^26, |Lv| <= 2^23, D < 2^30, ABSENT + a penalty < 2^31)

    def cost(qi):
        return np.where(none, np.int32(cap), np.minimum(np.abs(np.int32(qi) - lv), np.int32(cap)))
    D, S = cost(int(q[0])), np.arange(W, dtype=np.int32)
    a, aS, c, cS = (np.empty(W, np.int32) for _ in range(4))
    for i in range(1, m):
        a[:1] = ABSENT; a[1:] = D[:-1]; aS[:1] = 0; aS[1:] = S[:-1]                    # step
        b, bS = D + np.int32(stay), S                                                     # stay
        c[:2] = ABSENT; c[2:] = D[:-2] + np.int32(skip); cS[:2] = 0; cS[2:] = S[:-2]   # skip
        t = b < a
        w, wS = np.where(t, b, a), np.where(t, bS, aS)
        t = c < w
        D, S = np.where(t, c, w) + cost(int(q[i])), np.where(t, cS, wS)
    e = int(np.argmin(D))                                   # (the first of the smallest: the lowest u)
    return int(D[e]), e, int(S[e])


# ------------------------------------------------------------------------------------------------ (b)
def by_matrix(q, Lv, cfg):
    stay, skip, cap = (int(v) for v in cfg[:3])
    m, W = len(q), len(Lv)
    if m == 0 or W == 0:
        return None
    assert m * W <= 200000
    D = [[0] * W for _ in range(m)]
    mv = [[3] * W for _ in range(m)]
    for i in range(m):
        for u in range(W):
            lv = int(Lv[u])
            c = cap if lv == NONE else min(abs(int(q[i]) - lv), cap)
            if i == 0:
                D[i][u] = c
                continue
            best, code = None, 3
            for k, (du, pen) in enumerate(((1, 0), (0, stay), (2, skip))):       # step, stay, skip: the FIRST smallest wins
                if u - du >= 0:
                    v = D[i - 1][u - du] + pen
                    if best is None or v < best:
                        best, code = v, k
            D[i][u], mv[i][u] = best + c, code
    e = min(range(W), key=lambda u: (D[m - 1][u], u))
    u = e
    for i in range(m - 1, 0, -1):
        u -= (1, 0, 2)[mv[i][u]]
    return D[m - 1][e], e, u


def has_tie(q, Lv, cfg):
    """whether some cell of the programme has two candidates of the same smallest value, or the last row two smallest cells: (b)'s matrix again"""
    stay, skip, cap = (int(v) for v in cfg[:3])
    m, W = len(q), len(Lv)
    if m == 0 or W == 0:
        return False
    Lv = np.asarray(Lv, np.int64)
    D = np.where(Lv == NONE, cap, np.minimum(np.abs(int(q[0]) - Lv), cap))
    for i in range(1, m):
        a = np.full(W, BIG, np.int64); a[1:] = D[:-1]
        b = D + stay
        c = np.full(W, BIG, np.int64); c[2:] = D[:-2] + skip
        w = np.minimum(np.minimum(a, b), c)
        if (((a == w).astype(int) + (b == w) + (c == w)) > 1).any():
            return True
        D = w + np.where(Lv == NONE, cap, np.minimum(np.abs(int(q[i]) - Lv), cap))
    return int((D == D.min()).sum()) > 1


# ------------------------------------------------------------------------------------------------ the reads
def one_read(q, lo, hi, fwd, rev, cfg, one=by_rows):
    """the five outputs of one read from its q"""
    strands = int(cfg[5])
    W = hi - lo
    if len(q) == 0 or W == 0:
        return -1, 0, I64_MIN, I64_MIN, -1
    res = {}
    for minus in (0, 1):
        if strands >> minus & 1:
            res[minus] = one(q, strand_levels(fwd, rev, minus), cfg)
    win = 1 if (len(res) == 2 and res[1][0] < res[0][0]) else min(res)      # a tie goes to '+'
    cost, e, s = res[win]
    other = res[1 - win][0] if len(res) == 2 else -1
    if win:
        return cost, -1, hi - 1 - s, hi - 1 - e, other
    return cost, 1, lo + s, lo + e, other


def batch(row_off, sums, lens, lo, hi, fwd, rev, cfg, scale=None, one=by_rows):
    n = len(row_off) - 1
    out = {k: np.zeros(n, DTYPES[k]) for k in OUTPUTS}
    for r in range(n):
        v = one_read(read_rows(r, row_off, sums, lens, cfg, scale), lo, hi, fwd, rev, cfg, one)
        for k, x in zip(OUTPUTS, v):
            out[k][r] = x
    return out


# ------------------------------------------------------------------------------------------------ the track
_CODE2 = {c: v for v, cs in enumerate(("Aa", "Cc", "Gg", "Tt")) for c in cs.encode()}          # without SQG_METH: either case
_CODE5 = {ord("A"): 0, ord("C"): 1, ord("G"): 2, ord("T"): 4}                                  # with: upper case only, anything else 0
_COMP = {c: t for cs, t in (("Aa", "T"), ("Cc", "G"), ("Gg", "C"), ("Tt", "A")) for c in cs.encode()}


def track(genome, contig_off, k, meth, lo, hi, levels):
    """(fwd, rev) of [lo, hi): genome the contigs' bytes end to end, contig_off [n_contigs+1]"""
    total = int(contig_off[-1])
    levels = np.clip(np.asarray(levels, np.int64), -LV_MAX, LV_MAX)
    fwd, rev = np.full(hi - lo, NONE, np.int64), np.full(hi - lo, NONE, np.int64)
    ends = np.asarray(contig_off[1:], np.int64)
    for g in range(lo, hi):
        end = int(ends[np.searchsorted(ends, g, side="right")])         # the end of the contig that holds base g
        kmer = genome[g:g + k]
        if g + k > end or g + k > total or any(c not in _COMP for c in kmer):
            continue
        if meth:
            rf = 0
            for c in kmer:
                rf = rf * 5 + _CODE5.get(c, 0)
            rr = 0
            for c in reversed(kmer):
                rr = rr * 5 + _CODE5[ord(_COMP[c])]
        else:
            rf = 0
            for c in kmer:
                rf = rf * 4 + _CODE2[c]
            rr = 0
            for c in reversed(kmer):
                rr = rr * 4 + _CODE2[ord(_COMP[c])]
        fwd[g - lo], rev[g - lo] = levels[rf], levels[rr]
    return fwd.astype(np.int32), rev.astype(np.int32)
