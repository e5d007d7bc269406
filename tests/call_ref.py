"""Plain statements of include/sqg_call.h: what sqg_call_plan and sqg_batch_call must produce, bit for bit.  The rule is written twice,
from the header, and the two share no code:

  by_site(...)      read by read, candidate by candidate, event by event and digit by digit, in Python integers and Python floats (doubles,
                    one rounding per operation).
  vectorised(...)   a read's events at once: the hypothesis ranks of every event from digit arrays, the row values and terms on int64
                    arrays, the sites gathered from them.

Both take the reads' bytes, k, cfg = (neigh, term_cap, llr_min, min_obs), the rows sums / lens [n_events] with ev_off [n_reads+1] (the
batch's: a read shorter than a k-mer has stand-in events and no site), the pore model's level_mean (float32, [5^k]), the reads' offsets,
the profile's range and digitisation, the model tables w / c (int32, [5^k]) and optionally scale = (gain, shift), origin = (key0, step)
and window = (lo, hi).  Both return a dict of site_off [n_reads+1] and OUTPUTS [n_sites] in the device's dtypes (site_key only with an
origin), freq: {cov, truth, called, meth} [hi - lo] of uint32 -- what the call ADDS -- with a window, and stat = (sites, outside, called,
agree).  No call into the library."""
import numpy as np

NEIGH_READ, NEIGH_SAME = 0, 1
DEFAULT = (NEIGH_SAME, 256 * 50, 256 * 2, 1)
OUTPUTS = ("site_read", "site_pos", "label", "site_key", "n_obs", "nll_c", "nll_m", "llr", "call")
DTYPES = dict(site_read=np.int32, site_pos=np.int32, label=np.uint8, site_key=np.int64, n_obs=np.int32, nll_c=np.int32, nll_m=np.int32,
              llr=np.int32, call=np.uint8)
FREQ = ("cov", "truth", "called", "meth")
I64_MIN = -(1 << 63)
Q_MAX, D_MAX, W_MAX, C_MAX, GAIN_MAX = 1 << 26, 1 << 19, 1 << 24, 1 << 20, 1 << 20


def _pack(cols, site_off, origin, window, freq, stat):
    out = {n: np.asarray(cols[n], DTYPES[n]) for n in OUTPUTS if n != "site_key" or origin is not None}
    out["site_off"] = np.asarray(site_off, np.int64)
    out["stat"] = tuple(int(v) for v in stat)
    if window is not None:
        out["freq"] = freq
    return out


# ------------------------------------------------------------------------------------------------------------------ the plain loop
def _wrap(v):
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >> 63 else v


def _clamp(v, lo, hi):
    return lo if v < lo else hi if v > hi else v


def _digit(byte):
    """sqg_targets.h's kmer rule in an SQG_METH context: A C G M T -> 0 1 2 3 4, upper case only, anything else 0"""
    return {65: 0, 67: 1, 71: 2, 77: 3, 84: 4}.get(byte, 0)


def _is_candidate(read, j):
    return j + 1 < len(read) and read[j + 1] == 71 and read[j] in (67, 77)


def _level_raw(mean32, offset, rng, dig):
    """sqg_targets.h's clean_raw: (int16)((double)level_mean * digitisation / range - offset), the conversion as on x86-64"""
    v = float(np.float32(mean32)) * float(dig) / float(rng) - float(offset)
    t = int(v) if -2147483649.0 < v < 2147483648.0 else -(1 << 31)
    t &= 0xffff
    return t - 65536 if t >= 32768 else t


def row_value(s, L, gain=None, shift=None):
    """q of an observed event (L >= 1): q0 = clamp(floor(256 sum / L), +-2^26), the product modulo 2^64; under a scaling
    clamp((gain q0 >> 16) + shift, +-2^26) with gain and shift clamped into 1 .. 2^20 and +-2^26"""
    q = _clamp(_wrap(256 * int(s)) // int(L), -Q_MAX, Q_MAX)
    if gain is not None:
        q = _clamp(((_clamp(int(gain), 1, GAIN_MAX) * q) >> 16) + _clamp(int(shift), -Q_MAX, Q_MAX), -Q_MAX, Q_MAX)
    return q


def term(q, lv, w, c, term_cap):
    """Cc + t of one event under one row"""
    d = _clamp(q - 256 * lv, -D_MAX, D_MAX)
    return _clamp(int(c), -C_MAX, C_MAX) + min((_clamp(int(w), 0, W_MAX) * d * d) >> 32, term_cap)


def by_site(reads, k, cfg, sums, lens, ev_off, level_mean, offsets, rng, dig, w, c, scale=None, origin=None, window=None):
    neigh, term_cap, llr_min, min_obs = cfg
    cols = {n: [] for n in OUTPUTS}
    site_off = [0]
    freq = {n: np.zeros(window[1] - window[0], np.uint32) for n in FREQ} if window is not None else None
    outside = called = agree = 0
    for r, read in enumerate(reads):
        read = bytes(read)
        ln = len(read)
        ne = ln - k + 1
        for p in range(ln - 1 if ln >= k else 0):
            if not _is_candidate(read, p):
                continue
            n_obs, nll = 0, {1: 0, 3: 0}
            for e in range(max(0, p - k + 1), min(p, ne - 1) + 1):
                x = int(ev_off[r]) + e
                L = int(lens[x])
                if L < 1:
                    continue
                q = row_value(sums[x], L, *((scale[0][r], scale[1][r]) if scale is not None else ()))
                for h in (1, 3):
                    R = 0
                    for i in range(k):
                        j = e + i
                        takes = _is_candidate(read, j) if neigh == NEIGH_SAME else j == p
                        R += (h if takes else _digit(read[j])) * 5 ** (k - 1 - i)
                    nll[h] += term(q, _level_raw(level_mean[R], offsets[r], rng, dig), w[R], c[R], term_cap)
                n_obs += 1
            llr = nll[1] - nll[3]
            call = 0 if (n_obs < min_obs or abs(llr) < llr_min) else 2 if llr > 0 else 1
            label = int(read[p] == 77)
            key = I64_MIN
            if origin is not None:
                step = int(origin[1][r])
                if step > 0:
                    key = int(origin[0][r]) + p
                elif step < 0:
                    key = int(origin[0][r]) + k - 2 - p
            if window is not None:
                if origin is not None and int(origin[1][r]) != 0 and window[0] <= key < window[1]:
                    at = key - window[0]
                    freq["cov"][at] += 1; freq["truth"][at] += label; freq["called"][at] += int(call != 0); freq["meth"][at] += int(call == 2)
                else:
                    outside += 1
            called += int(call != 0)
            agree += int(call != 0 and (call == 2) == (label == 1))
            for n, v in (("site_read", r), ("site_pos", p), ("label", label), ("site_key", key), ("n_obs", n_obs), ("nll_c", nll[1]), ("nll_m", nll[3]),
                         ("llr", llr), ("call", call)):
                cols[n].append(v)
        site_off.append(len(cols["site_read"]))
    return _pack(cols, site_off, origin, window, freq, (len(cols["site_read"]), outside, called, agree))


# ------------------------------------------------------------------------------------------------------------------ vectorised
_DIGITS = np.zeros(256, np.int64)
for _i, _ch in enumerate(b"ACGMT"):
    _DIGITS[_ch] = _i


def _levels(mean64, offset, rng, dig):
    v = mean64 * np.float64(dig) / np.float64(rng) - np.float64(offset)
    fits = (v > -2147483649.0) & (v < 2147483648.0)
    t = np.where(fits, np.trunc(np.where(fits, v, 0.0)), -2147483648.0).astype(np.int64)
    return (t & 0xffff).astype(np.uint16).view(np.int16).astype(np.int64)


def _ranks(d, k):
    """the base-5 rank of d[e .. e+k) for every e"""
    ne = len(d) - k + 1
    rank = np.zeros(ne, np.int64)
    for i in range(k):
        rank = rank * 5 + d[i:i + ne]
    return rank


def vectorised(reads, k, cfg, sums, lens, ev_off, level_mean, offsets, rng, dig, w, c, scale=None, origin=None, window=None):
    neigh, term_cap, llr_min, min_obs = cfg
    sums, lens, ev_off = np.asarray(sums, np.int64), np.asarray(lens, np.int64), np.asarray(ev_off, np.int64)
    mean64 = np.asarray(level_mean, np.float32).astype(np.float64)
    W = np.clip(np.asarray(w, np.int64), 0, W_MAX)
    C = np.clip(np.asarray(c, np.int64), -C_MAX, C_MAX)
    parts = {n: [] for n in OUTPUTS}
    site_off = [0]
    for r, read in enumerate(reads):
        s = np.frombuffer(bytes(read), np.uint8)
        ln = len(s)
        if ln < k:
            site_off.append(site_off[-1])
            continue
        ne = ln - k + 1
        cand = np.zeros(ln, bool)
        cand[:-1] = ((s[:-1] == ord("C")) | (s[:-1] == ord("M"))) & (s[1:] == ord("G"))
        P = np.flatnonzero(cand)
        own = _DIGITS[s]
        # the rows' values, every event of the read
        x = ev_off[r] + np.arange(ne)
        L = lens[x]
        seen = L >= 1
        q = np.clip(np.floor_divide((sums[x].view(np.uint64) << np.uint64(8)).view(np.int64), np.maximum(L, 1)), -Q_MAX, Q_MAX)
        if scale is not None:
            g = min(max(int(scale[0][r]), 1), GAIN_MAX)
            sh = min(max(int(scale[1][r]), -Q_MAX), Q_MAX)
            q = np.clip(((g * q) >> 16) + sh, -Q_MAX, Q_MAX)
        lev = _levels(mean64, offsets[r], rng, dig)             # every row's level_raw under this read's offset
        # the span: column t is event p - k + 1 + t
        E = P[:, None] - k + 1 + np.arange(k)[None, :]
        inside = (E >= 0) & (E <= ne - 1)
        Ec = np.clip(E, 0, ne - 1)
        used = inside & seen[Ec]
        nll = {}
        for h in (1, 3):
            if neigh == NEIGH_SAME:
                R = _ranks(np.where(cand, h, own), k)[Ec]
            else:
                R = _ranks(own, k)[Ec] + (h - own[P])[:, None] * 5 ** np.clip(k - 1 - (P[:, None] - Ec), 0, k - 1)      # (base p is digit p - e of event e)
            R = np.where(inside, R, 0)
            d = np.clip(q[Ec] - 256 * lev[R], -D_MAX, D_MAX)
            t = np.minimum((W[R] * d * d) >> 32, term_cap)
            nll[h] = np.where(used, C[R] + t, 0).sum(axis=1)
        n_obs = used.sum(axis=1)
        llr = nll[1] - nll[3]
        call = np.where((n_obs < min_obs) | (np.abs(llr) < llr_min), 0, np.where(llr > 0, 2, 1))
        key = np.full(len(P), I64_MIN, np.int64)
        if origin is not None and int(origin[1][r]) != 0:
            key = int(origin[0][r]) + (P if int(origin[1][r]) > 0 else k - 2 - P)
        for n, v in (("site_read", np.full(len(P), r)), ("site_pos", P), ("label", s[P] == ord("M")), ("site_key", key), ("n_obs", n_obs), ("nll_c", nll[1]),
                     ("nll_m", nll[3]), ("llr", llr), ("call", call)):
            parts[n].append(np.asarray(v).astype(DTYPES[n]))
        site_off.append(site_off[-1] + len(P))
    cols = {n: np.concatenate(parts[n] + [np.zeros(0, DTYPES[n])]) for n in OUTPUTS}
    freq, outside = None, 0
    if window is not None:
        lo, hi = window
        step = np.asarray(origin[1], np.int64)[cols["site_read"]] if origin is not None else np.zeros(len(cols["site_read"]), np.int64)
        ok = (step != 0) & (cols["site_key"] >= lo) & (cols["site_key"] < hi)
        at = (cols["site_key"][ok] - lo).astype(np.int64)
        freq = {}
        for n, v in (("cov", np.ones(len(ok), bool)), ("truth", cols["label"] == 1), ("called", cols["call"] != 0), ("meth", cols["call"] == 2)):
            freq[n] = np.bincount(at[v[ok]], minlength=hi - lo).astype(np.uint32)
        outside = int((~ok).sum())
    called = cols["call"] != 0
    agree = called & ((cols["call"] == 2) == (cols["label"] == 1))
    return _pack(cols, site_off, origin, window, freq, (len(called), outside, int(called.sum()), int(agree.sum())))


def both(*a, what="", **kw):
    """the two statements on one batch: they agree on every output -> the first one's"""
    u, v = by_site(*a, **kw), vectorised(*a, **kw)
    assert set(u) == set(v), what
    for n in u:
        if n == "freq":
            for f in FREQ:
                assert u[n][f].dtype == v[n][f].dtype == np.uint32
                np.testing.assert_array_equal(u[n][f], v[n][f], err_msg=f"{what}: the two statements differ in freq.{f}")
        elif n == "stat":
            assert u[n] == v[n], f"{what}: the two statements differ in stat: {u[n]} {v[n]}"
        else:
            assert u[n].dtype == v[n].dtype, (what, n)
            np.testing.assert_array_equal(u[n], v[n], err_msg=f"{what}: the two statements differ in {n}")
    return u


def call_model(level_stdv, rng, dig):
    """the recommended tables of the header: sdc = (double)level_stdv * digitisation / range, w = clip(rint(2^24 / (2 sdc sdc)), 0, 2^24),
    c = clip(rint(256 ln(sdc)), +-2^20)"""
    sdc = np.asarray(level_stdv, np.float32).astype(np.float64) * np.float64(dig) / np.float64(rng)
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.clip(np.rint(np.float64(1 << 24) / (2.0 * sdc * sdc)), 0, W_MAX)
        c = np.clip(np.rint(256.0 * np.log(sdc)), -C_MAX, C_MAX)
    return np.nan_to_num(w, nan=0.0).astype(np.int32), np.nan_to_num(c, nan=0.0, neginf=-C_MAX).astype(np.int32)
