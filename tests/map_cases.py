"""Cases for include/sqg_map.h: drawn (q, Lv, cfg) triples for the two statements of map_ref.py, and synthetic tracks and rows for the device."""
import numpy as np

import map_ref as R

NONE = R.NONE


def drawn(rng, i):
    """case i of the statements' comparison -> (q, Lv, cfg, kind).  Kinds cycle: two-level tracks without jitter (most costs tie),
    penalties of 0, a constant track, tracks with NONE runs, tiny m and W, and ordinary noisy ones"""
    kind = ("two-level", "zero-pen", "constant", "none-runs", "tiny", "noisy", "two-level-none", "coarse")[i % 8]
    W = int(rng.integers(1, 60))
    m = int(rng.integers(1, 40))
    stay, skip, cap = (int(rng.choice([0, 1, 7, 256, 4096, 1 << 17])) for _ in range(3))
    cap = max(cap, 1)
    Lv = rng.integers(-30000, 30000, W)
    if kind in ("two-level", "two-level-none"):
        Lv = rng.choice([1000, 5000], W)
    if kind == "zero-pen":
        stay = skip = 0
    if kind == "constant":
        Lv = np.full(W, 777)
    if kind == "coarse":
        Lv = rng.integers(0, 4, W) * 100
        stay, skip = int(rng.choice([0, 100])), int(rng.choice([0, 100, 200]))
    if kind == "tiny":
        W, m = int(rng.integers(0, 4)), int(rng.integers(0, 3))
        Lv = rng.integers(-500, 500, W)
    Lv = np.asarray(Lv, np.int64)
    if kind in ("none-runs", "two-level-none") and W:
        for _ in range(int(rng.integers(1, 4))):
            a = int(rng.integers(0, W)); Lv[a:a + int(rng.integers(1, 6))] = NONE
    # the rows: a walk along the track with stays and skips, exact or jittered
    q, u = [], int(rng.integers(0, max(W, 1)))
    for _ in range(m):
        lv = int(Lv[u]) if W and Lv[u] != NONE else 0
        q.append(lv + (0 if kind in ("two-level", "two-level-none", "constant", "coarse") else int(rng.integers(-300, 300))))
        u = min(u + int(rng.choice([0, 1, 1, 1, 2])), max(W - 1, 0))
    return q, Lv, (stay, skip, cap), kind


def rows_of(q, rng=None, lens=None):
    """(sum, len) whose row values are exactly q: len drawn in 1 .. 9, sum = q * len / 256 needs q a multiple of 256 -- so len = 256 k"""
    q = np.asarray(q, np.int64)
    ln = np.full(len(q), 256, np.int64) if rng is None else 256 * rng.integers(1, 4, len(q))
    return q * (ln // 256), ln.astype(np.int32)


def walk(rng, Lv, at, m, jitter=40, moves=(0, 1, 1, 1, 1, 2)):
    """m row values that follow Lv from position `at` on with the given moves (ending inside the track), and where the walk ended"""
    q, u = [], at
    for i in range(m):
        q.append(int(Lv[u]) + int(rng.integers(-jitter, jitter + 1)))
        if i + 1 < m:
            u = min(u + int(rng.choice(moves)), len(Lv) - 1)
    return q, u


def track_of(rng, W, none_runs=0):
    """a random track of W levels in +-2^15 (fwd) and an unrelated one (rev), with NONE runs"""
    f, r = rng.integers(-32768, 32768, W).astype(np.int32), rng.integers(-32768, 32768, W).astype(np.int32)
    for t in (f, r):
        for _ in range(none_runs):
            a = int(rng.integers(0, max(W, 1))); t[a:a + int(rng.integers(1, 9))] = NONE
    return f, r
