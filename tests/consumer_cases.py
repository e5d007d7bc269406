"""The drawn cases of tests/test_fuzz_consumers.py: draw(seed) -> a shard_cases.Setup made from explicit values -- a profile, a flag set,
k, a model, batches of staged reads and the cfg of every consumer call -- drawn in strata of the seed, so that what the test asserts of the
table holds by construction; and facts(su): what the oracle and the numpy references alone say of such a case.  Not collected."""
import numpy as np

import call_cases as CS
import call_ref as CL
import chunks_ref as R
import shard_cases as SC
import sites_ref as S
from squigulator_amd import profiles as P

# seed % 10 -> (the flags beside the profile's own, the profile's family)
FLAG_SETS = ((0, "dna"), (P.SQ_PREFIX, "dna"), (0, "rna"), (P.SQ_PREFIX, "rna"), (P.SQ_IDEAL_TIME, "dna"), (P.SQ_IDEAL_AMP, "dna"), (P.SQ_IDEAL, "dna"),
             (P.SQ_PREFIX | P.SQ_IDEAL_TIME, "rna"), (P.SQ_METH, "dna"), (P.SQ_METH | P.SQ_IDEAL_TIME, "dna"))
FAMILY = dict(dna=("dna-r9-prom", "dna-r9-min", "dna-r10-prom"), rna=("rna-r9-prom", "rna004-prom"))
IDEAL_FLAGS = P.SQ_IDEAL | P.SQ_IDEAL_TIME | P.SQ_IDEAL_AMP
DWELL_MEANS = (2.0, 5.0, 9.0, 13.0, 31.0, 43.0, 120.0, 600.0)
SHAPES = ("empty batch", "one-read batch", "batch of short reads", "short read first", "short read last")
CHUNK_LENS = (64, 72, 256, 512, 4096)
LABEL_WIDTHS = (0, 1, 7, 128, 65535)
SITE_LENS = (16, 64, 256, 1024)
SITE_CTX = ((0, 0), (1, 0), (21, 10), (255, 254), (255, 0))
W_SHORT = (1, 2, 3, 7, 31, 63)
THRESHOLDS = (0.0, 1.4, 4.0, 9.0)
PEAKS = (0.0, 0.2, 1.0)
PENALTIES = (0, 256, 1024, 4096, 1 << 24)
COST_CAPS = (1, 4096, 65536, 1 << 24)
LETTERS = b"ACGTacgtNRY"
LETTER_P = (.22, .22, .22, .22, .02, .02, .02, .02, .02, .01, .01)
# The size conditions of a case.  MAX_SAMPLES bounds the samples of all its batches together, MAX_ELEMENTS the output elements of one
# chunk, target or site call.  draw() holds an estimate -- events times dwell_mean, known before the oracle runs -- HEADROOM below
# either; facts() asserts the bounds themselves of what the oracle then made
MAX_SAMPLES = 1_500_000
MAX_ELEMENTS = 1 << 22
HEADROOM = 0.8
COLLAPSE_SHIFTS = (0, 0, 0, 0, 2, -3)                       # (mostly the aligner's own answer: the call conditions are about that one)
CFG_BASE = 17000                                           # draw()'s second generator is default_rng(CFG_BASE + seed)


def n_events(m, k, rna, prefix):
    """the events of a read of m bases: both chains, the stand-in of a read shorter than a k-mer included (segments_ref.chains)"""
    if not prefix:
        return m - k + 1 if m >= k else 5
    return m + 85 - k + 1 if not rna else (m + 237 - k + 1) + (30 - k + 1)


def estimate(batches, k, rna, prefix, dwell_mean, chunk):
    """-> (the samples of the case, the largest element count of a chunk call and of a target call of one batch), with every event taken
    to last dwell_mean samples"""
    L, St, W = chunk
    total, chunk_el, target_el = 0, 0, 0
    for bt in batches:
        nc = 0
        for m in bt:
            n = int(n_events(m, k, rna, prefix) * dwell_mean)
            total += n
            nc += R.n_chunks_of(int(m * dwell_mean) if prefix else n, L, St)        # (with a prefix the insert alone is cut: at most m events)
        chunk_el, target_el = max(chunk_el, nc * (L + W + 3)), max(target_el, nc * 4 * L)
    return total, chunk_el, target_el


def shrink(lens, k, rna, prefix, dwell_mean, chunk):
    """the size conditions, enforced on the drawn lengths `lens` (a list of lists, changed in place): the longest read of the case loses a
    quarter of its bases until the estimate fits; reads that are down to k + 1 bases stay, and a read from the middle of the largest batch
    goes instead -- the first and the last read of a batch, which the planted shapes are about, never go"""
    def fits():
        total, chunk_el, target_el = estimate(lens, k, rna, prefix, dwell_mean, chunk)
        return total <= HEADROOM * MAX_SAMPLES and max(chunk_el, target_el) <= HEADROOM * MAX_ELEMENTS
    while not fits():
        bi, i = max(((bi, i) for bi, bt in enumerate(lens) for i in range(len(bt))), key=lambda at: lens[at[0]][at[1]])
        if lens[bi][i] > k + 1:
            lens[bi][i] = max(k + 1, lens[bi][i] * 3 // 4)
            continue
        bi = max(range(len(lens)), key=lambda b: len(lens[b]))
        assert len(lens[bi]) >= 3, "the case does not fit the size conditions with two reads a batch"
        del lens[bi][len(lens[bi]) // 2]


def draw(seed):
    """the case of a seed, deterministic.  f = seed % 10 picks the flag set and q = seed // 10 the k; the choices that the table's conditions
    are about go by strata of (f, q), the others by the seed's generator"""
    f, q = seed % 10, seed // 10
    rng = np.random.default_rng(7000 + seed)
    extra, family = FLAG_SETS[f]
    base, fl = P.get_profile(FAMILY[family][(q + f // 2) % len(FAMILY[family])])
    flags = fl | extra
    rna, prefix, meth = bool(flags & P.SQ_RNA), bool(flags & P.SQ_PREFIX), bool(flags & P.SQ_METH)
    k = 5 + q % 5
    dwell_mean = DWELL_MEANS[(f + 3 * q) % 8]
    dwell_std = (0.0, 0.5, 4.0, 0.8 * dwell_mean)[(f + 2 * q) % 4]
    prof = base.replace(dwell_mean=dwell_mean, dwell_std=dwell_std, offset_mean=base.offset_mean + float(rng.normal(0, 30)),
                        offset_std=float(rng.choice([0.0, 5.0, 20.0])), range=base.range * float(rng.uniform(0.5, 2.0)))
    T = int(rng.integers(1, 5))
    amp = float(rng.choice([1.0, 1.0, 0.3, 2.5]))
    # ---- the cfgs
    L = CHUNK_LENS[(f // 2 + q) % 5]
    si = (f + 2 * q) % 5
    St = (8, L // 2, L, L + 8, 3 * L)[si]
    W = LABEL_WIDTHS[(si + 2 + 3 * (q // 5)) % 5]           # (the widest rows go with a stride of L or 3 L: the element bound leaves them reads)
    norms = ("medmad", "pa") if (f + q) % 2 else ("pa", "medmad")
    Lw = SITE_LENS[(f + q) % 4]
    before = (0, Lw // 2, Lw - 1)[(f // 2 + 2 * q) % 3]
    focus = (0, (k + 1) // 2, k - 1)[(f + q // 2) % 3]
    w_short = W_SHORT[(f + 5 * q) % 6]
    w_long = 64 if (f + q) % 4 == 0 else int(rng.integers(w_short + 1, 65))
    detect_b = (w_short, w_long, float(rng.choice(THRESHOLDS)), float(rng.choice(THRESHOLDS)), float(rng.choice(PEAKS)))
    triple = lambda: (int(rng.choice(PENALTIES)), int(rng.choice(PENALTIES)), int(rng.choice(COST_CAPS)))      # noqa: E731
    cfgs = dict(chunk=(L, St, W), chunk_settings=(("f16", norms[0]), ("f32", norms[1])), site_geometries=((Lw, before),), focus=focus,
                site_ctx=SITE_CTX[(f + 3 * q) % 5], detect_b=detect_b, align_detected=triple(), align_rows=("detect A", "detect B"), align_truth=triple(),
                pile_kmer=True)
    # ---- the batches: lengths first, the planted shape, the size conditions, then the letters
    choice = [1, 3, k - 1, k, k + 1, 63, 64, 65, 200, 511, 700]
    lens = [[int(m) for m in rng.choice(choice, int(rng.integers(0, 10)))] for _ in range(int(rng.integers(2, 4)))]
    shape = SHAPES[(f + q) % 5]
    few = lambda n: [int(m) for m in rng.choice([1, 3, k - 1], n)]          # noqa: E731  (lengths below k)
    body = lambda n: [int(m) for m in rng.choice(choice[3:], n)]           # noqa: E731  (lengths of at least k)
    if shape == "empty batch":
        lens[q % len(lens)] = []
    elif shape == "one-read batch":
        lens[q % len(lens)] = body(1)
    elif shape == "batch of short reads":
        lens[q % len(lens)] = few(int(rng.integers(2, 5)))
    elif shape == "short read first":
        lens[q % len(lens)] = few(1) + body(int(rng.integers(2, 6)))
    else:
        lens[q % len(lens)] = body(int(rng.integers(2, 6))) + few(1)
    if all(len(bt) < 3 for bt in lens):                     # (a batch of three reads or more: the caller's origin then has all three steps)
        lens[(q + 1) % len(lens)] = body(4)
    shrink(lens, k, rna, prefix, dwell_mean, cfgs["chunk"])
    letters, p = (LETTERS + b"M", [v * 0.93 for v in LETTER_P] + [0.07]) if meth else (LETTERS, LETTER_P)
    batches = [[bytes(rng.choice(list(letters), m, p=p).astype(np.uint8)) for m in bt] for bt in lens]
    # ---- the cfgs of the calls added since the table was drawn, from a generator of their own: every value above stays what it was
    rng2 = np.random.default_rng(CFG_BASE + seed)
    cfgs["call_observed"] = (CL.NEIGH_READ, int(rng2.choice(CS.TERM_CAPS)), int(rng2.choice(CS.LLR_MINS)), int(rng2.choice(CS.MIN_OBS)))
    cfgs["collapse_shift"] = int(rng2.choice(COLLAPSE_SHIFTS))
    su = SC.Setup.of(f"drawn {seed}", prof, flags, k, seed, T, batches, amp_noise=amp, seed=int(rng.integers(1, 1 << 30)), **cfgs)
    su.drawn = dict(seed=seed, flag_set=f, shape=shape, dwell=(dwell_mean, dwell_std))
    return su


def describe(su):
    d = su.drawn
    return (f"seed {d['seed']}: flags {su.flags:#x} k {su.k} T {su.T} dwell {d['dwell'][0]}/{d['dwell'][1]} {d['shape']}, reads {[[len(r) for r in bt] for bt in su.batches]}, "
            f"chunk {su.chunk} {su.chunk_settings}, sites {su.site_geometries} focus {su.focus} ctx {su.site_ctx}, detect B {su.detect_b}, "
            f"align {su.align_detected} / {su.align_truth}, call observed {su.call_observed}, collapse shift {su.collapse_shift}")


def site_facts(su, reads):
    """of one batch, from the header's rule alone: (candidates, dropped at the front, dropped at the back, ctx_start clamped to 0, to L)"""
    (L, before), f, (B, cb), k = su.site_geometries[0], su.focus, su.site_ctx, su.k
    cand = front = back = low = high = 0
    for r in reads:
        m = len(r["seq"])
        if m < k:
            continue
        d = np.asarray(r["ss"], np.int64)
        E, n, ne = np.cumsum(d) - d, int(d.sum()), m - k + 1
        for p in S.candidates(r["seq"], su.meth):
            cand += 1
            a = int(p) - f
            if a < 0 or (a < ne and E[a] - before < 0):
                front += 1
            elif a >= ne or E[a] - before + L > n:
                back += 1
            else:
                e = int(p) - cb + np.arange(B + 1) - f
                X = np.where(e <= 0, 0, np.where(e >= ne, n, E[np.clip(e, 0, ne - 1)])) - (E[a] - before)
                low += int((X < 0).any()); high += int((X > L).any())
    return cand, front, back, low, high


def chain_facts(su, w, o=None):
    """of one batch, from the chained references' groups w (Setup.expected) and the oracle's batch o: what the scale, collapse and call
    groups hold of what can go wrong in them; w None: the figures of no batch.  Counts add up and flags are or-ed over a case's batches"""
    out = dict(unseen_beside_summed=False, rd_dropped=0, fit_gain=False, fit_shift=False, fit_fallback=False, part_obs=0, no_obs=0, calls=set(), labels=set(),
               call_outside=0, called=0, agree=0, site_steps=set(), two_in_kmer=False, site_first=False, site_last=False)
    if w is None:
        return out
    co, ev_off = w["collapse pa 0"], w["collapse pa 0"]["off"]
    for r in range(len(ev_off) - 1):
        rows, ln = (co["rows"][key][ev_off[r]:ev_off[r + 1]] for key in ("ob_rows", "ob_len"))
        out["unseen_beside_summed"] |= bool((ln == 0).any() and (rows >= 2).any())
    out["rd_dropped"] = int(co["per_read"]["rd_dropped"].sum())
    fit = w["scale fit"]["per_read"]
    out["fit_gain"], out["fit_shift"] = bool((fit["gain"] != 65536).any()), bool((fit["shift"] != 0).any())
    out["fit_fallback"] = bool((fit["n"] < 2).any())          # no row or one: no variance to fit a gain to
    if not su.calls:
        return out
    k = su.k
    c, t = w["call observed"], w["call true"]
    lens = o["lens"][c["read"]]
    p = c["rows"]["site_pos"].astype(np.int64)
    span = np.minimum(p, lens - k) - np.maximum(0, p - k + 1) + 1
    n_obs = c["rows"]["n_obs"]
    out["part_obs"], out["no_obs"] = int(((n_obs > 0) & (n_obs < span)).sum()), int((n_obs == 0).sum())
    out["calls"], out["labels"] = set(c["rows"]["call"].tolist()), set(c["rows"]["label"].tolist())
    out["call_outside"], out["called"], out["agree"] = c["stat"][1:]
    out["site_steps"] = set(o["step"][c["read"]].tolist())
    a, kw = t["args"]
    other = CL.vectorised(a[0], a[1], (CL.NEIGH_READ,) + CL.DEFAULT[1:], *a[3:], **kw)
    out["two_in_kmer"] = bool((other["llr"] != t["rows"]["llr"]).any())
    tp = t["rows"]["site_pos"]
    out["site_first"], out["site_last"] = bool((tp == 0).any()), bool((tp == o["lens"][t["read"]] - 2).any())
    return out


def facts(su):
    """what the oracle and the references say of a case, the device nowhere: a dict of the figures test_fuzz_consumers.py's conditions are
    about.  Asserts the size conditions of the case"""
    job = su.oracle_job()
    k, (L, St, W) = su.k, su.chunk
    out = dict(su.drawn, k=k, flags=su.flags, prefix=su.prefix, sites=su.sites, stride=(St > L) - (St < L), W=W, shapes=set(), samples=0,
               no_chunk_beside=False, label_over=False, label1=0, front=0, back=0, barren=False, ctx_low=0, ctx_high=0, long=0, masks=0, brief=False,
               edge=False, more_rows=False, more_events=False, outside=0, steps=set(), shared=False, collapse_shift=su.collapse_shift, **chain_facts(su, None))
    keys, site_keys = [], []
    for o in job:
        reads = o["reads"]
        short = [len(r["seq"]) < k for r in reads]
        out["samples"] += sum(len(r["sig"]) for r in reads)
        if not reads:
            out["shapes"].add("empty batch")
        if len(reads) == 1:
            out["shapes"].add("one-read batch")
        if len(reads) >= 2 and all(short):
            out["shapes"].add("batch of short reads")
        if len(reads) >= 2 and not all(short):
            out["shapes"] |= ({"short read first"} if short[0] else set()) | ({"short read last"} if short[-1] else set())
        seen = {}
        w = su.expected(reads, seen=seen, origin=(o["key0"], o["step"]))
        for key, v in chain_facts(su, w, o).items():
            out[key] = out[key] | v if isinstance(v, (bool, set)) else out[key] + v
        if su.calls:
            sk, (lo, hi) = w["call observed"]["rows"]["site_key"], su.window()      # (a read without a step has INT64_MIN there: below the window)
            site_keys.append(set(sk[(sk >= lo) & (sk < hi)].tolist()))
        for name, g in w.items():                           # the element bound, of the outputs the references hold
            if name.split()[0] in ("chunks", "targets", "sites"):
                el = sum(a.size for a in g["rows"].values()) + len(g["read"])
                assert el <= MAX_ELEMENTS, f"{describe(su)}: {name} has {el} elements"
        ch = w[f"chunks {su.chunk_settings[0][0]} {su.chunk_settings[0][1]}"]
        per = np.diff(ch["off"])
        out["no_chunk_beside"] |= bool(len(per) and per.min() == 0 and per.max() > 0)
        out["label_over"] |= bool(W > 0 and len(ch["rows"]["label_len"]) and ch["rows"]["label_len"].max() > W)
        if su.sites:
            st = w[f"sites {su.site_geometries[0][0]}"]
            cand, front, back, low, high = site_facts(su, reads)
            assert cand - front - back == len(st["read"])
            out["label1"] += int(st["rows"]["label"].sum()); out["front"] += front; out["back"] += back
            out["barren"] |= cand > 0 and len(st["read"]) == 0
            out["ctx_low"] += low; out["ctx_high"] += high
        out["long"] += sum(s.get("long", 0) for s in seen.values()); out["masks"] += sum(s.get("masks", 0) for s in seen.values())
        for name, (cfg, _, _, _) in su.detect_settings().items():
            out["brief"] |= any(len(r["sig"]) < 2 * cfg[0] for r in reads)
        nev = np.diff(w["events pa 0"]["off"])
        for name in ("align detected", "align detected B", "align truth"):
            out["edge"] |= bool((w[name]["per_read"]["al_edge"] > 0).any())
            rows = np.diff(w[name]["off"])
            out["more_rows"] |= bool((rows > nev).any()); out["more_events"] |= bool((rows < nev).any())
        out["steps"] |= set(o["step"].tolist())
        keys.append(set(su.keys(o, np.arange(len(reads))).tolist()))
    assert out["samples"] <= MAX_SAMPLES, f"{describe(su)}: {out['samples']} samples"
    out["shared"] = any(keys[a] & keys[b] for a in range(len(keys)) for b in range(a + 1, len(keys)))
    out["site_shared"] = any(site_keys[a] & site_keys[b] for a in range(len(site_keys)) for b in range(a + 1, len(site_keys)))
    for c, (kw, norm, trim) in su.pile_cfgs().items():
        out["outside"] += su.expected_pileup(kw, norm, trim)[2]
    return out
