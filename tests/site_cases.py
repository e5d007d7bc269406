"""Hand-built reads for include/sqg_sites.h (tests/test_sites.py).  Constant dwell: with SQG_IDEAL_TIME on dna-r9-prom every event has
SPS = (int)dwell_mean = 9 samples, so E[e] = 9 e and a read of len bases has ne = len - 5 events and n = 9 ne samples: every expected
value below is worked by inspection.  k = 6; the focus is 3 unless a case says otherwise.  Not collected."""
from sites_ref import Cfg

K, SPS = 6, 9
FILL = b"ATTAAT"                                            # no C, G or M: a filler base is never part of a candidate


def planted(length, pairs):
    """a read of `length` filler bases with the two letters of `pair` at p, p + 1 for every (p, pair) of pairs"""
    s = bytearray((FILL * (length // len(FILL) + 1))[:length])
    for p, pair in pairs:
        s[p:p + len(pair)] = pair
    return bytes(s)


def const_ss(seq, sps=SPS):
    """the dwells of a constant-dwell context (none for a read shorter than a k-mer: its stand-in events are not the read's)"""
    return [sps] * (len(seq) - K + 1) if len(seq) >= K else []


# 40 bases: ne = 35, n = 315.  First event: p = 3.  Last event a = 34: p = 37, E[34] = 306.
FIRST = planted(40, [(3, b"CG")])
LAST = planted(40, [(37, b"CG")])
LETTERS = planted(40, [(10, b"cg"), (14, b"Cg"), (18, b"MG"), (22, b"YG"), (26, b"CG")])

# name -> (reads, cfg, sites without SQG_METH [(read, p, w0)], sites with it, dropped candidates without / with)
CASES = {
    # a = 0: w0 = -before
    "first_event_before_0_w0_0": ([FIRST], Cfg(16, 0, 3), [(0, 3, 0)], [(0, 3, 0)], 0, 0),
    "first_event_one_sample_off": ([FIRST], Cfg(16, 1, 3), [], [], 1, 1),
    # a = ne - 1 = 34: w0 = 306 - before; w0 + 16 <= 315 iff before >= 7
    "last_event_before_L_minus_1": ([LAST], Cfg(16, 15, 3), [(0, 37, 291)], [(0, 37, 291)], 0, 0),
    "last_event_window_ends_at_n": ([LAST], Cfg(16, 7, 3), [(0, 37, 299)], [(0, 37, 299)], 0, 0),
    "last_event_one_sample_off": ([LAST], Cfg(16, 6, 3), [], [], 1, 1),
    # before = 18 = E[2]: the site of event 2 (p = 5) starts at w0 = 0, that of event 1 (p = 4) at -9
    "w0_zero_inside": ([planted(40, [(5, b"CG")]), planted(40, [(4, b"CG")])], Cfg(24, 18, 3), [(0, 5, 0)], [(0, 5, 0)], 1, 1),
    # anchors outside [0, ne): p = 1 -> a = -2, p = 38 -> a = 35 = ne (p + 1 = 39 < 40: a candidate); focus 0: p = 38 -> a = 38
    "anchor_outside_the_events": ([planted(40, [(1, b"CG"), (38, b"CG")])], Cfg(16, 0, 3), [], [], 2, 2),
    "anchor_outside_focus_0": ([planted(40, [(1, b"CG"), (38, b"CG")])], Cfg(16, 0, 0), [(0, 1, 9)], [(0, 1, 9)], 1, 1),
    # cg, Cg, YG: never; MG: a site (label 1) under SQG_METH only; CG: always.  a = 15 -> w0 = 127, a = 23 -> w0 = 199
    "letters": ([LETTERS], Cfg(16, 8, 3), [(0, 26, 199)], [(0, 18, 127), (0, 26, 199)], 0, 0),
    # a C that ends one read and a G that begins the next; the second read's own CG at p = 20: a = 17, w0 = 145
    "read_border": ([planted(40, [(39, b"C")]), planted(40, [(0, b"G"), (20, b"CG")])], Cfg(16, 8, 3), [(1, 20, 145)], [(1, 20, 145)], 0, 0),
    # a read shorter than a k-mer has no sites, whatever its letters
    "short_read": ([b"ACGCG", planted(40, [(20, b"CG")])], Cfg(16, 8, 3), [(1, 20, 145)], [(1, 20, 145)], 0, 0),
    # the window is longer than the read: every candidate is dropped
    "all_dropped": ([planted(40, [(10, b"CG"), (20, b"CG")])], Cfg(320, 8, 3), [], [], 2, 2),
    "no_candidate": ([planted(40, []), planted(17, [])], Cfg(16, 8, 3), [], [], 0, 0),
}

# context rows that reach outside the read, B = 9, cb = 4 (codes A 1, C 2, G 3, T 4): name -> (context row, ctx_start row) of the case's one site
CONTEXT = {
    # bases -1 .. 7 of ATTCGTATT...: the first is outside.  Events -4 .. 5: E = 0 for e <= 0, E[1] = 9, E[2] = 18 -> L
    "first_event_before_0_w0_0": ([0, 1, 4, 4, 2, 3, 4, 1, 4], [0, 0, 0, 0, 0, 9, 16, 16, 16, 16]),
    # bases 33 .. 41 of ...AATACGA: the last two are outside.  Events 30 .. 39 against w0 = 291: 270 279 288 -> 0, 297 -> 6, 306 -> 15 = before,
    # e >= 35 = ne -> n - w0 = 24 -> L
    "last_event_before_L_minus_1": ([1, 1, 4, 1, 2, 3, 1, 0, 0], [0, 0, 0, 6, 15, 16, 16, 16, 16, 16]),
}


def long_read():
    """2100 bases (ne = 2095, n = 18855 at 9 samples per event) with a CG every 50 bases from p = 3 on: event 1024, the edge of the
    4 x 256-event scan tile, lies between two of them"""
    return planted(2100, [(p, b"CG") for p in range(3, 2090, 50)])


def tile_edge_reads():
    """anchor events 1023 and 1025 in one read (p = 1026, 1028: CGCG), 1024 in another (p = 1027): the sites on either side of the scan's tile edge"""
    return [planted(2100, [(1026, b"CG"), (1028, b"CG"), (100, b"CG")]), planted(2100, [(1027, b"CG"), (2000, b"MG")])]
