"""The label geometries of test_chunk_labels.py: which reads, under which dwells, cut into which (L, S, W) -- and what each case shows.

The labels of sqg_batch_chunks (include/sqg_chunks.h) are a function of the per-event dwells, the read's bases, the RNA flag, the
methylation flag and (L, S, W); k_chunk_labels computes them with a tiled scan over the events and interval arithmetic per event.  A case
here is a context, a dwell regime, a worker count, the event counts of its reads and its geometries.  reference() runs the ORACLE for
the reads and chunks_ref over the oracle's output: nothing in this module loads the HIP library.

Two yardsticks: chunks_ref.read_chunks (searchsorted over the event starts) and labels_by_definition below (a boolean mask over all events
per chunk, codes from a table typed out of the header).  test_chunk_labels.py shows without a GPU that they agree on every geometry, and
that every case shows what its `shows` says (witnesses(), from the oracle's output alone), so a case cannot decay silently.
"""
import collections
import functools
import zlib

import numpy as np

import chunks_ref as R
import inject
import orc
from squigulator_amd import model, profiles

SEED = 42

# include/sqg_chunks.h, "Codes": rank 0/1/2/3 -> 1/2/3/4, the IUPAC letters as the kernels rank them, anything else 1; 'M' -> 5 under SQG_METH
LABEL_CODE = {"A": 1, "a": 1, "R": 1, "W": 1, "M": 1, "D": 1, "H": 1, "V": 1, "N": 1,
              "C": 2, "c": 2, "Y": 2, "B": 2,
              "G": 3, "g": 3, "S": 3, "K": 3,
              "T": 4, "t": 4, "U": 4}


def labels_by_definition(ss, seq, k, rna, meth, L, S, W):
    """one read -> (labels [nc, W], label_len [nc]) by the header's rule, stated as dumbly as it can be: E[e] by a running sum, per chunk
    the mask g0 <= E[e] < g1 over ALL events (reversed for RNA), the codes letter by letter from LABEL_CODE"""
    E, n = [], 0
    for d in ss:
        E.append(n)
        n += int(d)
    E = np.array(E, np.int64)
    nc = ((n - L) // S + 1) if (n >= L and len(seq) >= k) else 0
    lab = np.zeros((nc, W), np.uint8)
    ll = np.zeros(nc, np.int32)
    text = bytes(seq).decode("latin-1")
    for j in range(nc):
        g0, g1 = (n - j * S - L, n - j * S) if rna else (j * S, j * S + L)
        mask = (g0 <= E) & (E < g1)
        events = np.flatnonzero(mask)
        if rna:
            events = events[::-1]
        ll[j] = len(events)
        for x, e in enumerate(events[:W]):
            b = text[e]
            lab[j, x] = 5 if (meth and b == "M") else LABEL_CODE.get(b, 1)
    return lab, ll


# ---- the matrix ----------------------------------------------------------------------------------------------------------------------
CONTEXTS = {  # name -> (profile, extra flags); none has SQ_PREFIX
    "r9": ("dna-r9-prom", 0),                    # k 6
    "r10": ("dna-r10-prom", 0),                  # k 9
    "rna9": ("rna-r9-prom", 0),                  # k 5
    "rna004": ("rna004-prom", 0),                # k 9
    "meth": ("dna-r9-prom", profiles.SQ_METH),   # k 6, the 5-letter model
}

Case = collections.namedtuple("Case", "name ctx T regime events lsw shows div64")
# regime: ("drawn", mean, std) | ("time", mean) under SQ_IDEAL_TIME | ("ideal", mean) under SQ_IDEAL; constant dwell = (int)mean
# events: events per read (bases - k + 1); 0 stands for a read of k - 1 bases, which has samples and no chunks
# lsw: the geometries; shows: the witnesses this case must show in at least one of them; div64: also run under SQG_TEST_CHUNK_GENERIC=3

TILE = [1, 2, 1023, 1024, 1025, 2048, 2049, 4097]          # the scan's tiles are 4 * 256 events
SMALL = [(64, 8, 48), (64, 8, 32), (64, 1, 3), (128, 33, 61), (72, 200, 7), (64, 64, 0)]
BIG = [(4096, 4096, 256), (4096, 2048, 1000)]
# dwell 1: n = events, so these reads have n == L, L - 1, L + S - 1, L + S for (64, 8, .), (128, 33, .), (72, 200, .) and (4096, 4096, .)
EDGES = [64, 63, 71, 72, 128, 127, 160, 161, 71, 271, 272, 4096, 4095, 8191, 8192]


def _family(k56, k9):
    """the regimes for a pair of contexts: the 6-mer / 5-mer one and the 9-mer one of DNA, or of RNA"""
    return [
        Case(f"{k56}_drawn2", k56, 1, ("drawn", 2, 0.5), TILE + [40, 0], SMALL, ("Wm1", "W", "Wp1", "on_event", "inside", "e0_0"), True),
        Case(f"{k9}_drawn13", k9, 4, ("drawn", 13, 4), [1023, 1024, 1025, 2049, 300, 5], SMALL[:1] + SMALL[3:] + BIG, ("inside",), False),
        Case(f"{k56}_drawn120", k56, 4, ("drawn", 120, 96), [1, 2, 60, 500, 1025], [(64, 8, 48), (128, 33, 61), (72, 200, 7)] + BIG, ("empty",), False),
        Case(f"{k9}_drawn600", k9, 1, ("drawn", 600, 480), [1, 2, 30, 300], [(64, 8, 48), (128, 33, 61), (64, 64, 0), (4096, 2048, 1000)],
             ("empty", "span50"), True),
        Case(f"{k56}_time1", k56, 1, ("time", 1), TILE + EDGES + [0], SMALL + BIG, ("long", "tile", "e0_0", "g1_n", "on_event"), True),
        Case(f"{k56}_time1_wide", k56, 4, ("time", 1), [70000, 65544, 65543], [(65544, 4096, 65535)] + BIG, ("long", "g1_n"), False),
        Case(f"{k9}_time2.7", k9, 4, ("time", 2.7), [1, 2, 32, 1023, 1024, 1025, 2049, 4097], SMALL + BIG[:1], ("on_event", "inside", "tile"), False),
        Case(f"{k56}_time100", k56, 1, ("time", 100), [1, 2, 41, 1023, 1025, 2049], [(64, 8, 48), (128, 33, 61), (72, 200, 7)] + BIG,
             ("empty", "inside"), False),
        Case(f"{k9}_time5000", k9, 4, ("time", 5000), [1, 2, 10], [(64, 1, 3), (64, 8, 48), (72, 200, 7), (4096, 2048, 1000)],
             ("empty", "span50"), True),
        Case(f"{k56}_ideal13", k56, 1, ("ideal", 13.5), [1, 5, 1024, 1025, 2500], SMALL[:1] + SMALL[3:] + BIG[:1], ("inside",), False),
    ]


CASES = _family("r9", "r10") + _family("rna9", "rna004") + [
    Case("meth_drawn13", "meth", 1, ("drawn", 13, 4), [1024, 1025, 300, 77, 0], SMALL[:1] + SMALL[3:] + BIG[:1], ("meth_first", "meth_last"), True),
    Case("meth_drawn2", "meth", 4, ("drawn", 2, 0.5), [2049, 40, 500], SMALL, ("meth_first", "meth_last", "Wm1", "W", "Wp1"), False),
    Case("meth_time2.7", "meth", 1, ("time", 2.7), [1, 2, 1025, 333], SMALL, ("meth_first", "meth_last"), False),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# every witness must occur somewhere in the matrix, for DNA and for RNA (the two meth ones: in the meth context)
WITNESSES = ("empty", "long", "on_event", "inside", "tile", "e0_0", "g1_n", "span50", "Wm1", "W", "Wp1")
METH_WITNESSES = ("meth_first", "meth_last")


def context_of(case):
    """-> (profile, flags, k, mean, stdv, rna, meth)"""
    name, extra = CONTEXTS[case.ctx]
    prof, fl = profiles.get_profile(name)
    assert not (fl | extra) & profiles.SQ_PREFIX
    kind, dmean = case.regime[0], case.regime[1]
    prof = prof.replace(dwell_mean=float(dmean), dwell_std=float(case.regime[2]) if kind == "drawn" else 0.0)
    fl |= extra | {"drawn": 0, "time": profiles.SQ_IDEAL_TIME, "ideal": profiles.SQ_IDEAL}[kind]
    k = profiles.default_kmer_size(fl)
    meth = bool(fl & profiles.SQ_METH)
    mean, stdv = model.synthetic_model(k, meth=meth)
    return prof, fl, k, mean, stdv, bool(fl & profiles.SQ_RNA), meth


def seqs_of(case, k, meth):
    """the case's reads: mostly A C G T, one base in twelve lower case, N or an IUPAC letter; the meth context has 'M' one base in six"""
    rng = np.random.default_rng(zlib.crc32(case.name.encode()))
    letters = list(b"ACGT" + (b"M" if meth else b"") + b"acgtNRYSKBU")
    p = np.array([.23 - .05 * meth] * 4 + ([.2] if meth else []) + [.08 / 11] * 11)
    const = int(case.regime[1]) if case.regime[0] != "drawn" else 1
    out = []
    for ev in case.events:
        m = k - 1 if ev == 0 else inject.bases_for([ev * const], k, const)[0]          # (constant dwell: exactly ev * const samples)
        out.append(bytes(rng.choice(letters, m, p=p / p.sum()).astype(np.uint8)))
    return out


def witnesses(ss, n, rna, L, S, W, lab, ll):
    """what one read's chunks of one geometry show; from the oracle's dwells and the reference's rows alone"""
    out = set()
    nc = len(ll)
    if nc == 0:
        return out
    ss = np.asarray(ss, np.int64)
    E = np.cumsum(ss) - ss
    j = np.arange(nc, dtype=np.int64)
    g0 = n - j * S - L if rna else j * S
    g1 = g0 + L
    if (ll == 0).any():
        out.add("empty")
    if W >= 1 and (ll > 10 * W).any():
        out.add("long")
    starts = set(E.tolist())
    on = np.array([int(g) in starts for g in g0])
    if (on & (g0 > 0)).any():
        out.add("on_event")
    if (~on).any():
        out.add("inside")
    tiles = set(E[1024::1024].tolist())
    if any(int(g) in tiles for g in g0) or any(int(g) in tiles for g in g1):
        out.add("tile")
    if (g0 == 0).any():
        out.add("e0_0")                                     # g0 = 0 = E[0]: the chunk starts with event 0
    last = g1 == n
    if last.any() and E[-1] < n:
        out.add("g1_n")                                     # g1 = n > E[last]: the chunk ends with the last event, e1 = n_events
    cover = np.searchsorted(E, g0, "right") - 1             # the event that holds the chunk's first sample
    inside_one = (cover == np.searchsorted(E, g1 - 1, "right") - 1)
    run = best = 0
    for a in range(nc):
        run = run + 1 if (inside_one[a] and a and inside_one[a - 1] and cover[a] == cover[a - 1]) else int(inside_one[a])
        best = max(best, run)
    if best >= 50:
        out.add("span50")
    if W >= 2:
        out |= {name for name, v in (("Wm1", W - 1), ("W", W), ("Wp1", W + 1)) if (ll == v).any()}
    kept = np.minimum(ll, W)
    has = kept > 0
    if has.any():
        if (lab[has, 0] == 5).any():
            out.add("meth_first")
        if (lab[np.flatnonzero(has), kept[has] - 1] == 5).any():
            out.add("meth_last")
    return out


SETTINGS = [("f16", "medmad"), ("f32", "pa"), ("f32", "medmad"), ("f16", "pa")]


def setting_of(case, g):
    """the one dtype x norm the signal is checked at for the case's g-th geometry (the signal side is test_injected_signals' job)"""
    return SETTINGS[(zlib.crc32(case.name.encode()) + g) % 4]


@functools.lru_cache(maxsize=2)
def reference(name):
    """the oracle's reads of the case and chunks_ref's outputs for each of its geometries:
    -> dict(seqs, reads [dict(sig, ss, seq, offset)], want {(L, S, W): batch_chunks(...)})"""
    case = BY_NAME[name]
    prof, fl, k, mean, stdv, rna, meth = context_of(case)
    seqs = seqs_of(case, k, meth)
    orac = orc.Oracle(prof, fl, k, mean, stdv, SEED, num_workers=case.T)
    reads = [dict(sig=w.sig, ss=w.ss, seq=s, offset=w.offset) for w, s in zip(orac.run_batch_seqs(seqs), seqs)]
    orac.close()
    want = {}
    for g, (L, S, W) in enumerate(case.lsw):
        dtype, norm = setting_of(case, g)
        want[(L, S, W)] = R.batch_chunks(reads, k, rna, meth, L, S, W, dtype, norm, prof.range, prof.digitisation)
    return dict(seqs=seqs, reads=reads, want=want)
