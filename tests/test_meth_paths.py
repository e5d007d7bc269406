"""The 5-letter methylation tables (SQG_METH, 5^k rows) on the paths only a few-worker batch reaches: chains cut into links in
front of the bucketed hand-out over 4 (k = 6) and 20 (k = 7) partitions with a ragged last one -- ordered and by claims --, the
per-link rows of k = 5, 8, 9 (12.5 KB to 7.8 MB a row), forced here on small batches and reached without a knob at 65536 events.
Signal, dwell, offset and median_before against the oracle, bit for bit, both arithmetic modes, batch by batch and streamed; the path
a batch took is read off the library's own SQG_VERBOSE lines.  Cases, witnesses and harness: tests/meth_cases.py."""
import os

import numpy as np
import pytest

import meth_cases as mc
import orc
from squigulator_amd import api, build, model, profiles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_LIB = os.path.join(ROOT, "oracle", "libsqg_cpu.so")
MODES = (api.MODE_CERTIFIED, api.MODE_EXACT)


# ---- 1. the cases and what they cover (CPU)
def test_ranks_stated_here_equal_the_oracles_and_the_table_writers():
    L = orc.lib()
    rng = np.random.default_rng(1)
    for k in range(1, 10):
        top = 5 ** k - 1
        for r in [0, top, top // 2] + [int(x) for x in rng.integers(0, top + 1, 40)]:
            s = model.meth_kmer_string(r, k).encode()
            assert mc.ranks(s, k).tolist() == [r] and L.orc_meth_kmer_rank(s, k) == r, (k, r)
        read = bytes(rng.choice(mc.LETTERS, 200 + k, p=mc.LETTER_P).astype(np.uint8))        # lower case, m, IUPAC: all rank as A
        assert mc.ranks(read, k).tolist() == [L.orc_meth_kmer_rank(read[i:i + k], k) for i in range(len(read) - k + 1)]
    assert mc.ranks(b"m" * 6, 6).tolist() == [0] and mc.ranks(b"M" * 6, 6).tolist() == [3 * (5 ** 6 - 1) // 4]
    assert [mc.n_part(k) for k in (6, 7)] == [4, 20] and 5 ** 6 - 3 * 4096 == 3337 and 5 ** 7 - 19 * 4096 == 301


def test_every_case_covers_what_it_claims():
    long_chain = short_read = False
    for variant, seed in mc.MATRIX:
        case = mc.meth_case(seed)
        k, w = case.k, mc.witnesses(case)
        assert case.flags & profiles.SQ_METH and not case.flags & profiles.SQ_RNA
        assert case.links in (2, 7, 40) or (case.links == 100000 and k <= 7), (seed, case.links)
        if k in (6, 7):
            assert w["parts"] == set(range(mc.n_part(k))), (seed, sorted(w["parts"]))
            assert {0, 5 ** k - 1 - (mc.n_part(k) - 1) * mc.PART_SUB} <= w["last_sub"], seed   # the ragged partition's first and last live stream
        assert w["rank0"] and w["rank_top"] and w["m_first"] and w["m_last"] and w["lower_m"] and w["iupac"], (seed, w)
        long_chain |= w["max_chain_ev"] >= 1024
        short_read |= w["short_read"]
        for bi, bt in enumerate(case.batches):                   # every batch has more reads than workers, and the forced cut takes place
            assert len(bt) > case.T
            links, chains = mc.expected_links([len(r) for r in bt], k, case.T, bool(case.flags & profiles.SQ_PREFIX), case.links)
            assert links > chains, (seed, bi, links, chains)
    assert long_chain and short_read


def test_no_cell_of_the_matrix_is_empty():
    """every (k, variant) pair at least twice with cut chains, at both widths of k_events; the flag sets without amplitude noise -- no
    streams, no cut -- under every k in the default variant"""
    cells, uncut = {}, set()
    for variant, seed in mc.MATRIX:
        case = mc.meth_case(seed)
        k = mc.KS[seed % len(mc.KS)]
        assert case.k == k
        if not mc.has_streams(case.flags):
            assert variant == "default"
            uncut.add((k, case.flags))
            continue
        cells[(k, variant)] = cells.get((k, variant), 0) + 1
        if seed % 2:
            cells[(k, "narrow-events")] = cells.get((k, "narrow-events"), 0) + 1
    assert len(mc.MATRIX) == len(set(mc.MATRIX)) == 60
    assert len(uncut) == 2 * len(mc.KS)
    assert {(mc.meth_case(s).k, mc.meth_case(s).flags) for s in range(30)} == {(k, profiles.SQ_METH | f) for k in mc.KS for f in mc.FLAG_SETS}
    for k in mc.KS:
        for variant in list(mc.VARIANTS) + ["narrow-events"]:
            assert cells.get((k, variant), 0) >= 2, (k, variant)
        for variant in mc.VARIANTS:                              # ... and every variant meets every k at both widths of k_events
            assert {s % 2 for v, s in mc.MATRIX if v == variant and s % len(mc.KS) == mc.KS.index(k) and mc.has_streams(mc.meth_case(s).flags)} == {0, 1}, (k, variant)


# ---- 2. generator, reads and comparison proven on the CPU backend (oracle/libsqg_cpu.so: the same C ABI on the oracle)
@pytest.mark.parametrize("seed", range(0, 30, 6), ids=[f"k{k}" for k in mc.KS])        # (five k, five flag sets)
def test_cases_through_the_cpu_backend_equal_the_oracle(seed):
    import subprocess
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "libsqg_cpu.so"], stdout=subprocess.DEVNULL)
    case = mc.meth_case(seed)
    mean, stdv = model.synthetic_model(case.k, salt=seed, meth=True)
    want = mc.oracle_run(case, mean, stdv)
    for bt, wt in zip(case.batches, want):                       # the event counts the link witnesses are built on
        assert [len(w.ss) for w in wt] == [mc.n_events(len(r), case.k, bool(case.flags & profiles.SQ_PREFIX)) for r in bt]
    mc.run_case(case, mean, stdv, want, (api.MODE_CERTIFIED,), lib_path=CPU_LIB)


# ---- 3. cut chains under the 5-letter table (forced on small batches: development library)
def _assert_cut(capfd, tag, case, variant):
    lines = mc.batch_lines(capfd.readouterr().err)
    assert len(lines) == len(case.batches), f"{tag}: {len(lines)} SQG_VERBOSE batch lines for {len(case.batches)} batches"
    bucketed = case.k in (6, 7) and variant != "per-link-rows" and mc.has_streams(case.flags)
    for bi, (_, reads, events, links, chains, pieces, slices) in enumerate(lines):
        if bucketed:                                             # the hand-out over 4 / 20 partitions ...
            assert slices >= chains * mc.n_part(case.k), f"{tag} batch {bi}: {slices} slices for {chains} worker chains x {mc.n_part(case.k)} partitions"
        else:                                                    # ... or the per-link rows
            assert slices == 0, f"{tag} batch {bi}: {slices} slices -- the bucketed hand-out where per-link rows were expected"
        assert reads == len(case.batches[bi]) > case.T
        if mc.has_streams(case.flags):
            assert links > chains, f"{tag} batch {bi}: {links} links in {chains} worker chains -- the chains were not cut"
        else:                                                    # --ideal / --ideal-amp: no k-mer streams, nothing to hand out, no cut
            assert links == chains, f"{tag} batch {bi}: {links} links in {chains} worker chains of a context without k-mer streams"
        assert pieces == 0, f"{tag} batch {bi}: {pieces} pieces -- a methylation context took the wavefront-per-link path"


@pytest.mark.gpu
@pytest.mark.parametrize("variant,seed", mc.MATRIX, ids=[f"{v}-{s}-k{mc.KS[s % 5]}" for v, s in mc.MATRIX])
def test_cut_chains_under_the_methylation_table(variant, seed, monkeypatch, capfd):
    case = mc.meth_case(seed)
    monkeypatch.setenv("SQG_SPLIT_CHAINS", str(case.links))
    monkeypatch.setenv("SQG_VERBOSE", "1")
    if seed % 2:                                                 # odd seeds: the 256-thread k_events
        monkeypatch.setenv("SQG_EVENTS_WIDE_MAX", "0")
    for name, val in mc.VARIANTS[variant].get("env", {}).items():
        monkeypatch.setenv(name, val)
    assert api.build_info(api.load_library())["dev"] == "1"      # (the release library would ignore every knob above)
    mean, stdv = model.synthetic_model(case.k, salt=seed, meth=True)
    want = mc.oracle_run(case, mean, stdv)
    capfd.readouterr()
    mc.run_case(case, mean, stdv, want, MODES, variant, after_job=lambda tag, c: _assert_cut(capfd, tag, c, variant))


# ---- 4. the natural threshold: no knob but SQG_VERBOSE, which both builds read
def _threshold_case(name, k, T):
    """over (48 reads of 1400 ... 1500 bases: some 69000 events), under (40 reads, 60000 events), over: the chains are cut from 65536
    events on, so one context goes from cut to uncut and back"""
    rng = np.random.default_rng(60 + k + T)
    prof, fl = profiles.get_profile(name)
    reads = lambda lens: [bytes(rng.choice(mc.LETTERS, int(m), p=mc.LETTER_P).astype(np.uint8)) for m in lens]   # noqa: E731
    batches = [reads(rng.integers(1400, 1501, 48)), reads([1500 + k - 1] * 40), reads(rng.integers(1400, 1501, 48))]
    return mc.Case(0, prof, fl | profiles.SQ_METH, k, T, 42, batches, None)


@pytest.mark.gpu
@pytest.mark.parametrize("lib", ["dev", "release"])
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("name,k", [("dna-r9-prom", 6), ("dna-r10-prom", 7)])
def test_chains_are_cut_from_65536_events_on_without_a_knob(name, k, T, lib, monkeypatch, capfd):
    for knob in api.DEV_KNOBS + ("SQG_LIB",):
        monkeypatch.delenv(knob, raising=False)
    monkeypatch.setenv("SQG_VERBOSE", "1")
    lib_path = {"dev": build.LIB_DEV, "release": build.LIB}[lib]
    assert api.build_info(api.load_library(lib_path))["dev"] == {"dev": "1", "release": "0"}[lib]
    case = _threshold_case(name, k, T)
    mean, stdv = model.synthetic_model(k, meth=True)
    want = mc.oracle_run(case, mean, stdv)

    def witness(tag, c):
        lines = mc.batch_lines(capfd.readouterr().err)
        assert len(lines) == 3, f"{tag}: {len(lines)} SQG_VERBOSE batch lines"
        for bi, (_, reads, events, links, chains, pieces, slices) in enumerate(lines):
            assert chains == T and pieces == 0, f"{tag} batch {bi}"
            if bi == 1:
                assert events == 60000 and links == chains and slices == 0, f"{tag} batch {bi}: {events} events, {links} links in {chains} worker chains"
            else:                                                # cut, and handed out over the 4 / 20 partitions
                assert events >= 65536 and links > chains, f"{tag} batch {bi}: {events} events, {links} links in {chains} worker chains"
                assert slices >= T * mc.n_part(k), f"{tag} batch {bi}: {slices} slices"
    capfd.readouterr()
    mc.run_case(case, mean, stdv, want, MODES, lib_path=lib_path, after_job=witness)
