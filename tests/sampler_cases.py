"""The drawn cases of tests/test_sampler_fuzz.py: case(seed) -> a Case holding everything test_sampler._run needs -- a genome or a
transcriptome, the count and frequency files, the flags, workers, batches and read length -- drawn in strata of the seed from
np.random.default_rng; and facts(case, reads): what the oracle's reads and the genome alone say of such a case.  Not collected.

N_SEEDS = 60: the oracle's share of the slowest case stays below a second (the condition test prints it)."""
import os

import numpy as np

from squigulator_amd import api
from squigulator_amd import profiles as P

N_SEEDS = 60
LENS = (150, 199, 200, 210, 260, 400, 1500, 6000, 20000)
TRANS_LENS = (150, 199, 200, 210, 260, 400, 1500)       # (a transcript is read whole: 30 samples a base keep the oracle's second)
RLENS = (250, 600, 1500)
VARIANTS = ("dna", "dna prefix", "meth", "meth prefix", "meth rejecting", "rna uniform", "rna count", "rna count trunc", "cdna count", "cdna trunc")
RUN_LENS = (1, 1, 2, 3, 5, 8, 13, 30, 70, 120)
FREQS = tuple(f"{v / 10:.1f}" for v in range(11))
MAX_BATCH = 128                                         # (8 workers with a chain of 16 each: "about 120")
# seed -> how often the case was drawn again until the conditions of test_the_table_holds_what_it_is_for held (found on the CPU, from
# the oracle's reads; 0 where not listed)
REDRAWN = {2: 4, 14: 1, 23: 9, 52: 1}


def _letters(rng, n, sprinkle):
    p = [.2, .2, .2, .2, .04, .04, .04, .04, .01, .01, .02 if sprinkle else 0.0]
    p = np.array(p) / sum(p)
    return rng.choice(list(b"ACGTacgtRYN"), n, p=p).astype(np.uint8)


def _put(s, at, word):
    """word at s[at:], where it fits and covers no N"""
    if 0 <= at and at + len(word) <= len(s) and not (s[at:at + len(word)] == ord("N")).any():
        s[at:at + len(word)] = list(word)


def draw_genome(rng, lens, dense_cpg=False, rejecting=False, run_share=1.0):
    """contigs of the lengths `lens` (list of bytes): the letters, then the N runs planted three ways, then the CpGs beside them.
    Contig `clean` (the first of 260 nt or more, or the longest) takes neither sprinkled N nor a 10 % stretch: the genome stays usable.
    run_share: the share of the contigs that take N at all (a transcript is read whole: some have to stay without)"""
    clean = next((i for i, n in enumerate(lens) if n >= 260), int(np.argmax(lens)))
    contigs, off = [], 0
    for ci, n in enumerate(lens):
        with_N = rng.random() < run_share
        s = _letters(rng, n, sprinkle=with_N and ci != clean and not rejecting and rng.random() < 0.25)
        runs = []
        small = n < 1500 or rejecting

        def run(at, ln):
            at, ln = max(at, 0), min(ln, 8 if small else 120)
            if at < n and with_N:
                s[at:at + ln] = ord("N")
                runs.append((at, min(at + ln, n)))
        # (i) runs that straddle the 64-base blocks of the N-prefix table: they start at 64 j - r of the concatenated genome
        for _ in range(max(1, n // 800) if not rejecting else 0):
            j = int(rng.integers(off // 64 + 1, (off + n) // 64 + 1))
            run(64 * j - int(rng.integers(0, 7)) - off, int(rng.choice(RUN_LENS)))
        # (ii) at the contig's first and last bases
        if rng.random() < (0.8 if rejecting else 0.4):
            run(0, int(rng.integers(1, 4 if rejecting else 7)))
        if rng.random() < 0.4:
            ln = int(rng.integers(1, 7))
            run(n - ln, ln)
        # (iii) a stretch near 10 % density: every tenth base (a window of 10 m bases then holds m, exactly the bound), or one base in ten
        if n >= 1500 and ci != clean and with_N and rng.random() < 0.7:
            ln = int(rng.choice([400, 900]))
            at = n - ln if rng.random() < 0.5 else int(rng.integers(0, n - ln))
            if rng.random() < 0.6:
                s[at + int(rng.integers(0, 10)):at + ln:10] = ord("N")
            else:
                s[at:at + ln][rng.random(ln) < 0.1] = ord("N")
        # CpGs at the contig's ends and next to the runs, lower-case ones beside them
        if rng.random() < 0.7:
            _put(s, 0, b"CG"); _put(s, 2, [b"cG", b"Cg", b"cg"][int(rng.integers(0, 3))])
        if rng.random() < 0.7:
            _put(s, n - 2, b"CG"); _put(s, n - 4, [b"cG", b"Cg", b"cg"][int(rng.integers(0, 3))])
        for a, b in runs:
            how = int(rng.integers(0, 4))
            if how == 0:
                _put(s, b, b"CG"); _put(s, b + 2, b"cg")
            elif how == 1:
                _put(s, a - 2, b"CG"); _put(s, a - 4, b"Cg")
            elif how == 2:
                _put(s, a - 1, b"C"); _put(s, b, b"G")           # C N...N G: no CpG, whatever the N become
            else:
                _put(s, a - 2, b"cG"); _put(s, b, b"CG")
        if dense_cpg:
            for at in rng.integers(0, n - 1, n // 30):
                _put(s, int(at), b"CG")
            for at in rng.integers(0, n - 1, n // 100):
                _put(s, int(at), [b"cG", b"Cg", b"cg"][int(rng.integers(0, 3))])
        if rejecting and n >= 200:                                # the part a read can end in: CpGs for the read's last base to cut
            for at in range(198, n - 1, 2):
                if rng.random() < 0.6:
                    _put(s, at, b"CG")
        contigs.append(bytes(s))
        off += n
    return contigs


def upper_cpgs(c):
    a = np.frombuffer(c, np.uint8)
    return np.flatnonzero((a[:-1] == ord("C")) & (a[1:] == ord("G")))


def draw_freqs(rng, contigs, without=None):
    """the --meth-freq file's text and the contigs it names: every second upper-case CpG and a few lower-case c, frequencies 0 .. 1 in
    tenths; at least one contig of 200 nt or more stays without a line, at least one has lines"""
    long_ = [i for i, c in enumerate(contigs) if len(c) >= 200 and len(upper_cpgs(c)) >= 2]
    assert len(long_) >= 2
    order = [int(i) for i in rng.permutation(long_)]
    without = set(order[:max(1, len(order) // 3)]) if without is None else set(without)
    lines, named = [], []
    for i, c in enumerate(contigs):
        if i in without or (i not in long_ and rng.random() < 0.5):
            continue
        at = [int(p) for p in upper_cpgs(c)[int(rng.integers(0, 2))::2]]
        low = np.flatnonzero(np.frombuffer(c, np.uint8) == ord("c"))
        at += [int(p) for p in low[:: max(1, len(low) // 8)]]
        if not at:
            continue
        named.append(i)
        for p in sorted(at):
            lines.append(f"c{i}\t{p}\t{'1.0' if c[p:p + 1] == b'c' else FREQS[int(rng.integers(0, 11))]}\n")
    return "".join(lines), named, sorted(without)


def draw_batches(rng, T, rejecting=False):
    """short chains, long chains, short chains again (and, every other time, long ones once more): below 16 reads a worker, 16 or more,
    below 16; the second batch is larger than the first, a fourth larger than the second where there is room"""
    if rejecting:
        m = int(rng.integers(40, MAX_BATCH // T + 1))
        return [int(rng.integers(1, 15 * T + 1)), m * T, int(rng.integers(1, 15 * T + 1)), m * T]
    m = int(rng.integers(16, max(MAX_BATCH // T, 16) + 1))
    first = int(rng.integers(1, min(15 * T, m * T - 1) + 1))
    out = [first, m * T, int(rng.integers(1, 15 * T + 1))]
    if rng.random() < 0.5:
        m2 = int(rng.integers(16, max(MAX_BATCH // T, 16) + 1))
        out.append(m2 * T - int(rng.integers(0, T)) if m2 > 16 else m2 * T)
    return out


def chain_lengths(n, T):
    """reads of each worker in a batch of n (src/thread.c:80-99: step = ceil(n / T))"""
    if T <= 1:
        return [n]
    step = -(-n // T)
    return [max(0, min(step, n - w * step)) for w in range(T)]


class Case:
    """one drawn context.  files(dir) writes the FASTA, the count file and the frequency file and returns _run's arguments"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def files(self, d):
        fa = os.path.join(str(d), f"g{self.seed}.fa")
        with open(fa, "w") as f:
            f.write("".join(f">c{i} drawn\n{c.decode()}\n" for i, c in enumerate(self.contigs)))
        tc = mf = None
        if self.counts is not None:
            tc = os.path.join(str(d), f"g{self.seed}.count.tsv")
            with open(tc, "w") as f:
                f.write(self.counts)
        if self.freqs is not None:
            mf = os.path.join(str(d), f"g{self.seed}.mfreq.tsv")
            with open(mf, "w") as f:
                f.write(self.freqs)
        return dict(profile=self.profile, k=self.k, fasta=fa, T=self.T, batches=self.batches, rlen=self.rlen, oflags=self.oflags,
                    sflags=self.sflags, mode=self.mode, trans_count=tc, seed=self.sim_seed, meth_freq=mf)

    def describe(self):
        return (f"seed {self.seed} ({self.variant}): {self.profile} k {self.k} T {self.T} rlen {self.rlen} batches {self.batches} "
                f"prefix {self.prefix} contigs {[len(c) for c in self.contigs]}")


def case(seed):
    """the case of a seed, deterministic.  f = seed % 10 is the variant, q = seed // 10 the stratum"""
    f, q = seed % 10, seed // 10
    rng = np.random.default_rng(31000 + seed + 1000 * REDRAWN.get(seed, 0))
    variant = VARIANTS[f]
    meth, rejecting = f in (2, 3, 4), f == 4
    prefix = f in (1, 3) or (f in (5, 8) and q % 2 == 1)
    profile, k = ("rna004-prom", 9) if f in (5, 6, 7) else ("dna-r9-prom", 6)
    if f in (0, 1) and (q + f) % 5 == 4:                  # one stratum in five of the plain DNA variants: the 9-mer table
        profile, k = "dna-r10-prom", 9
    oflags = {7: P.SQ_TRANS_TRUNC, 8: P.SQ_CDNA, 9: P.SQ_CDNA | P.SQ_TRANS_TRUNC}.get(f, 0)
    mode = {5: api.SAMPLE_RNA, 6: api.SAMPLE_RNA, 7: api.SAMPLE_RNA | api.SAMPLE_TRUNC, 8: api.SAMPLE_CDNA,
            9: api.SAMPLE_CDNA | api.SAMPLE_TRUNC}.get(f, api.SAMPLE_DNA)
    counts = freqs = None
    named, without = [], []
    if f >= 5:
        # a transcriptome: one transcript of 400 nt or more stays clean, and the table (where there is one) gives it a count
        lens = [int(n) for n in rng.choice(TRANS_LENS, int(rng.integers(3, 13)))]
        lens[int(rng.integers(0, len(lens)))] = int(rng.choice([400, 1500]))
        if q % 3 == 0:
            lens[int(rng.integers(0, len(lens)))] = 6000
        if not any(n < 200 for n in lens):
            lens.append(int(rng.choice([150, 199])))
        contigs = draw_genome(rng, lens, run_share=0.5)
        clean = next(i for i, n in enumerate(lens) if n >= 260)
        if f in (6, 7, 8):
            short = next(i for i, n in enumerate(lens) if n < 200)
            rows = {clean: int(rng.choice([10, 25])), short: int(rng.choice([3, 10]))}
            for i in rng.permutation(len(lens))[:max(2, len(lens) * 2 // 3)]:
                rows.setdefault(int(i), int(rng.choice([0, 0, 3, 3, 7, 10, 10, 25])))
            if 0 not in rows.values():
                rows[next(i for i in rows if i not in (clean, short))] = 0
            counts = "".join(f"c{i}\t{rows[i]}\n" for i in (int(j) for j in rng.permutation(sorted(rows))))
            named = sorted(rows)
        rlen, T = 10000, int(rng.integers(1, 9))
        batches = draw_batches(rng, T)
    elif rejecting:
        # (two contigs a read can come from, 470 of at most 2460 bases: the one of 260 nt takes the frequencies, so that reads of it can end
        # inside it, the other has none)
        longs = (260, 210)
        shorts = [199] * 10
        for i in range(int(rng.integers(0, 3))):
            shorts[i] = 150
        lens = [int(n) for n in rng.permutation(list(longs) + shorts)]
        assert sum(n for n in lens if n >= 200) <= 0.2 * sum(lens)
        contigs = draw_genome(rng, lens, dense_cpg=True, rejecting=True)
        rlen, T = 250, int(rng.integers(1, 4))           # (the shortest: a longer read never ends inside a contig of 260 nt)
        batches = draw_batches(rng, T, rejecting=True)
    else:
        lens = [int(n) for n in rng.choice(LENS, int(rng.integers(2 if meth else 1, 13)))]
        if meth and sum(n >= 400 for n in lens) < 2:     # (a contig with frequencies and one without, both with room for reads)
            lens += [int(rng.choice([400, 1500])), int(rng.choice([400, 1500, 6000]))]
        if not any(n >= 260 for n in lens):
            lens[0] = int(rng.choice([260, 400, 1500]))
        lens = lens[:12]
        contigs = draw_genome(rng, lens, dense_cpg=meth)
        rlen, T = int(RLENS[(q + f) % 3]), int(rng.integers(1, 9))
        batches = draw_batches(rng, T)
    if meth:
        freqs, named, without = draw_freqs(rng, contigs, [lens.index(210)] if rejecting else None)
    assert 1 <= len(contigs) <= 12 + (f >= 5) and all(len(c) in LENS for c in contigs)
    assert 1 <= T <= 8 and 3 <= len(batches) <= 4 and max(batches) <= MAX_BATCH and batches[1] > batches[0]
    assert max(chain_lengths(batches[0], T)) < 16 <= max(chain_lengths(batches[1], T)) and max(chain_lengths(batches[2], T)) < 16
    assert not rejecting or min(n for n in chain_lengths(batches[1], T) if n) >= 40
    sflags = (P.SQ_PREFIX if prefix else 0)
    return Case(seed=seed, variant=variant, f=f, q=q, profile=profile, k=k, contigs=contigs, counts=counts, freqs=freqs, named=named,
                without=without, T=T, batches=batches, rlen=rlen, oflags=oflags, sflags=sflags, mode=mode, prefix=prefix, meth=meth,
                rejecting=rejecting, sim_seed=int(rng.integers(1, 1 << 20)))


def oracle_reads(cs, d):
    """the oracle's reads of a case, a list per batch, and the seconds they took: no device"""
    import time

    import orc
    from squigulator_amd import model
    kw = cs.files(d)
    prof, fl = P.get_profile(kw["profile"])
    mean, stdv = model.synthetic_model(cs.k, meth=cs.meth)
    t0 = time.perf_counter()
    orac = orc.Oracle(prof, fl | cs.oflags | cs.sflags | (P.SQ_METH if cs.meth else 0), cs.k, mean, stdv, cs.sim_seed, num_workers=cs.T, rlen=cs.rlen)
    ref = orac.load_ref(kw["fasta"], kw["trans_count"], kw["meth_freq"])
    assert [bytes(ref.seqs[i][:ref.lengths[i]]) for i in range(ref.num_ref)] == cs.contigs
    reads = [orac.run_batch(nb) for nb in cs.batches]
    orac.close()
    return reads, time.perf_counter() - t0


def missing_in_case(fc):
    """the conditions every methylation case meets (and every rejecting one), as the names of those that fc = facts(...) lacks"""
    if fc["f"] not in (2, 3, 4):
        return []
    want = dict(M_plus="+" in fc["M"], M_minus="-" in fc["M"], M_and_N=fc["M_and_N"] > 0, cut_plus="+" in fc["cut"], cut_minus="-" in fc["cut"],
                cut_front=fc["cut_front"] > 0, lower_cpg=fc["lower_cpg"] > 0, bare_between=fc["bare_between"] > 0,
                bare_between_long=fc["bare_between_long"] > 0)
    return [name for name, ok in want.items() if not ok]


def facts(cs, reads):
    """what the oracle's reads (a list per batch) and the genome say of a case, the device nowhere"""
    T = cs.T
    off = np.concatenate(([0], np.cumsum([len(c) for c in cs.contigs])))
    out = dict(seed=cs.seed, f=cs.f, prefix=cs.prefix, clean_mod8=set(), with_N=set(), tail_N=0, cross64=0, clipped=set(), trunc_pos=0, minus_N=0,
               short_in_table=any(len(cs.contigs[i]) < 200 for i in (cs.named if cs.counts is not None else range(len(cs.contigs)))),
               M=set(), M_and_N=0, cut=set(), lower_cpg=0, bare_between=0, M_first=0, M_last=0, n_reads=0, at_bound=0, trunc_N=0, cut_front=0,
               bare_between_long=0)
    for batch in reads:
        step = -(-len(batch) // T) if T > 1 else max(len(batch), 1)
        rows = []
        for i, w in enumerate(batch):
            g = cs.contigs[w.ref_idx]
            a, n = w.ref_pos_st, w.rlen
            span = np.frombuffer(g, np.uint8)[a:a + n]
            isN = span == ord("N")
            out["n_reads"] += 1
            assert n >= 200 and len(span) == n and len(w.seq) == n
            if not isN.any():
                out["clean_mod8"].add((w.strand, n % 8))
            else:
                out["with_N"].add(w.strand)
                out["tail_N"] += int(isN[n - n % 8:].any())
                at = np.flatnonzero(isN[1:] & isN[:-1]) + 1
                out["cross64"] += int(((off[w.ref_idx] + a + at) % 64 == 0).any())
                out["minus_N"] += w.strand == "-"
                out["at_bound"] += int(10 * int(isN.sum()) == n)           # as many N as the 10 % test lets through
                out["trunc_N"] += int(a > 0)
            if a + n == len(g):
                out["clipped"].add(w.strand)
            out["trunc_pos"] += int(a > 0)
            nM = w.seq.count(b"M")
            if cs.meth:
                has = w.ref_idx in cs.named
                assert has or nM == 0
                if nM:
                    out["M"].add(w.strand)
                    out["M_and_N"] += int(isN.any())
                    out["M_first"] += w.seq[0:1] == b"M"
                    out["M_last"] += w.seq[n - 2:n - 1] == b"M"
                if has and a + n < len(g) and g[a + n - 1:a + n + 1] == b"CG":
                    out["cut"].add(w.strand)
                out["cut_front"] += int(has and a > 0 and g[a - 1:a + 1] == b"CG")
                low = g[a:a + n]
                out["lower_cpg"] += int(any(x in low for x in (b"cg", b"cG", b"Cg")))
                rows.append((i // step if T > 1 else 0, has, nM > 0))
        for wk in set(r[0] for r in rows):                       # a read without frequencies between two of the worker's that carry M
            mine = [r for r in rows if r[0] == wk]
            for j, (_, has, _) in enumerate(mine):
                if not has and any(m for _, _, m in mine[:j]) and any(m for _, _, m in mine[j + 1:]):
                    out["bare_between"] += 1
                    out["bare_between_long"] += int(len(mine) >= 16)
    return out
