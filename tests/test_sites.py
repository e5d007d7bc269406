"""include/sqg_sites.h: CpG-centred signal windows with their methylation labels (sqg_site_plan, sqg_batch_sites), against the numpy
statement of the header's rules (sites_ref.py), against the compiled reference's own methylated reads and against hand-worked reads
(site_cases.py).  Every comparison is bit for bit (floats as integers)."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (before the library is loaded: the HIP runtime torch brings is the one the library then uses)

import chunks_ref as R
import orc
import site_cases as SC
import sites_ref as S
import targets_ref as T
from chunk_support import ALL_SETTINGS, _context, _declared, _fixture_reads
from refvec_cases import REFVEC_CASES
from squigulator_amd import api, build, model, options, profiles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_LIB = os.path.join(ROOT, "oracle", "libsqg_cpu.so")
NCOV = os.path.join(ROOT, "tests", "golden", "inputs", "nCoV-2019.reference.fasta")
MFREQ_DENSE = os.path.join(ROOT, "tests", "golden", "inputs", "mfreq_dense.tsv")
METH_VECTORS = ("r9_meth", "r10_meth_dense", "r9_meth_dense", "r9_meth_tk4")
GEOMETRIES = ((64, 32), (256, 128), (1024, 100))            # (win_len, before)
OUT_KEYS = api.SITE_OUTPUTS


def _focus(k):
    """k / 2, the half rounded up: 3 at k = 6, 5 at k = 9.  (With 4 at k = 9 r10_meth_dense drops no candidate at (64, 32); with 5 every
    vector has sites of both labels and a dropped candidate at all three geometries, which is what the vector tests require.)"""
    return (k + 1) // 2


def _vector(cid):
    o = options.parse_args(dict(REFVEC_CASES)[cid])
    assert o.meth_freq and o.flags & profiles.SQ_METH and not o.flags & (profiles.SQ_RNA | profiles.SQ_PREFIX)
    return o, o.kmer_size_default, _fixture_reads(cid)


# ---------------------------------------------------------------------------------------------------------- no GPU
def test_header_declares_the_site_exports_and_the_libraries_have_them():
    assert _declared("sqg_sites.h") == set(api.EXPORTS_SITES) == {"sqg_site_plan", "sqg_batch_sites"}
    others = set(api.EXPORTS) | set(api.EXPORTS_CHUNKS) | set(api.EXPORTS_TARGETS) | set(api.EXPORTS_SEGMENTS)
    assert not set(api.EXPORTS_SITES) & others
    assert _declared("sqg_segments.h") == set(api.EXPORTS_SEGMENTS) and _declared("sqg.h") == set(api.EXPORTS)     # the other headers: unchanged
    build.build()
    for lib in (build.LIB, build.LIB_DEV):
        L = api.load_library(lib)
        for n in api.EXPORTS_SITES:
            assert hasattr(L, n), f"{n} not exported by {lib}"
    assert os.path.join(ROOT, "include", "sqg_sites.h") in build.headers()
    for h in ("k_sites.h", "h_sites.h"):
        assert os.path.join(ROOT, "squigulator_amd", "csrc", h) in build.headers()
    hdr = open(os.path.join(ROOT, "include", "sqg_sites.h")).read()
    for struct, ctype in (("sqg_site_cfg_t", api.CSiteCfg), ("sqg_site_out_t", api.CSiteOut)):
        body = hdr[:hdr.index("} " + struct)]
        body = body[body.rindex("typedef struct"):]
        fields = [f[0] for f in ctype._fields_]
        at = [body.index(name + ";") for name in fields]     # every field is declared, in the binding's order
        assert at == sorted(at), f"{struct}: {fields}"
    assert [f[0] for f in api.CSiteCfg._fields_] == ["win_len", "before", "focus", "ctx_len", "ctx_before", "dtype", "norm"]
    assert [f[0] for f in api.CSiteOut._fields_] == ["signal", "label", "site_read", "site_pos", "win_start", "context", "ctx_start", "med2", "mad4"]


def test_the_cpu_backend_has_no_sites_and_says_so():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "libsqg_cpu.so"])
    prof, fl = profiles.get_profile("dna-r9-prom")
    mean, stdv = model.synthetic_model(6)
    gen = api.SignalGenerator(prof, fl, 6, mean, stdv, 42, lib_path=CPU_LIB)
    for n in api.EXPORTS_SITES:
        assert not hasattr(gen.L, n)
    b = gen.submit([b"ACGTACGTACGTTTGACA" * 40])
    for call in (lambda: b.sites(64), lambda: b.site_plan(64)):
        with pytest.raises(api.SqgError) as e:
            call()
        assert e.value.code == -1 and "sqg_batch_sites" in str(e.value)
    b.free(); gen.close()


@pytest.mark.parametrize("L,before", GEOMETRIES)
@pytest.mark.parametrize("cid", METH_VECTORS)
def test_helper_against_the_reference_vectors(cid, L, before):
    """the compiled reference's own methylated reads, dwells and signal: every M is a candidate, label 1 sits on an M, and the moves
    ctx_start implies are targets_ref's move table inside the window"""
    o, k, reads = _vector(cid)
    mean, _ = model.synthetic_model(k, meth=True)
    c = S.Cfg(L, before, _focus(k), 255, 127, "f32", "medmad")
    n0 = n1 = dropped = covered = 0
    for i, r in enumerate(reads):
        seq = np.frombuffer(r["seq"], np.uint8)
        cand = S.candidates(r["seq"], True)
        assert set(np.flatnonzero(seq == ord("M"))) <= set(cand), f"{cid} read {i}: an M that is no candidate"
        assert len(S.candidates(r["seq"], False)) == len(cand) - int((seq == ord("M")).sum())     # without SQG_METH an M is no site
        w = S.read_sites(r["sig"], r["ss"], r["seq"], k, True, c, r["offset"], o.profile.range, o.profile.digitisation)
        ns = len(w["label"])
        assert ns + w["dropped"] == len(cand) and set(w["site_pos"]) <= set(cand)
        np.testing.assert_array_equal(w["label"], (seq[w["site_pos"]] == ord("M")).astype(np.uint8))
        n0 += int((w["label"] == 0).sum()); n1 += int((w["label"] == 1).sum()); dropped += w["dropped"]
        _, moves, _ = T.read_samples(r["seq"], r["ss"], r["offset"], mean, k, False, True, o.profile.range, o.profile.digitisation)
        E = np.cumsum(r["ss"]) - r["ss"]
        for j in range(ns):
            p, w0, cs = int(w["site_pos"][j]), int(w["win_start"][j]), w["ctx_start"][j].astype(np.int64)
            assert w0 == E[p - c.f] - before and cs[c.cb] == before and (np.diff(cs) >= 0).all()
            win = moves[w0:w0 + L]
            assert win[cs[(cs > 0) & (cs < L)]].all(), f"{cid} read {i} site {j}: a boundary that is no event start"
            if cs[0] == 0 and cs[-1] == L:                  # the row's events cover the window: its boundaries are all the event starts
                covered += 1
                np.testing.assert_array_equal(np.flatnonzero(win[1:]) + 1, np.unique(cs[(cs > 0) & (cs < L)]), err_msg=f"{cid} read {i} site {j}")
                assert win[0] == (w0 in E)
    print(f"{cid} L {L} before {before}: {n0} sites with label 0, {n1} with label 1, {dropped} dropped, {covered} rows cover their window")
    assert n0 >= 1 and n1 >= 1 and dropped >= 1, f"{cid} L {L} before {before}: {n0} / {n1} / {dropped}: the case must hold both labels and a dropped candidate"
    assert covered >= (n0 + n1) // 2
    if cid == "r9_meth":                                    # (focus 3 at k = 6 either way)
        assert (n0, n1, dropped) == {(64, 32): (154, 4, 1), (256, 128): (153, 4, 2), (1024, 100): (148, 2, 9)}[(L, before)]


def _hand_reads(seqs, sps=SC.SPS):
    """constant dwell: the signal is a ramp that differs from sample to sample, so that a window shifted by one sample shows"""
    out, at = [], 0
    for s in seqs:
        ss = SC.const_ss(s, sps)
        n = sum(ss) if ss else 5 * sps                      # (a read shorter than a k-mer: the five stand-in events)
        out.append(dict(sig=((np.arange(at, at + n) * 7) % 1000 - 500).astype(np.int16), ss=ss, seq=s, offset=3.0))
        at += n
    return out


@pytest.mark.parametrize("name", list(SC.CASES))
def test_helper_on_hand_worked_reads(name):
    seqs, c, plain, meth, dropped_plain, dropped_meth = SC.CASES[name]
    reads = _hand_reads(seqs)
    for m, sites, dropped in ((False, plain, dropped_plain), (True, meth, dropped_meth)):
        c9 = c._replace(B=9, cb=4, dtype="f32")
        w = S.batch_sites(reads, SC.K, m, c9)
        assert list(zip(w["site_read"], w["site_pos"], w["win_start"])) == sites, f"{name} meth {m}"
        assert int(w["dropped"].sum()) == dropped
        np.testing.assert_array_equal(w["site_off"], np.concatenate(([0], np.cumsum([sum(1 for s in sites if s[0] == i) for i in range(len(seqs))]))))
        np.testing.assert_array_equal(w["label"], [1 if seqs[r][p:p + 1] == b"M" else 0 for r, p, _ in sites])
        for j, (r, p, w0) in enumerate(sites):              # E[e] = 9 e: the window starts `before` samples in front of event p - f
            assert w0 == SC.SPS * (p - c.f) - c.before and 0 <= w0 <= len(reads[r]["sig"]) - c.L
            med2, mad4 = R.stats(reads[r]["sig"])
            np.testing.assert_array_equal(R.bits(w["signal"][j]), R.bits(R.normalise(reads[r]["sig"][w0:w0 + c.L], med2, mad4, "medmad", 0, 1, 1)))
            assert w["ctx_start"][j][4] == c.before
        if name in SC.CONTEXT:
            np.testing.assert_array_equal(w["context"][0], SC.CONTEXT[name][0])
            np.testing.assert_array_equal(w["ctx_start"][0], SC.CONTEXT[name][1])
    if name == "letters":                                   # under SQG_METH the M at p = 18 is code 5 in the row of the site at p = 18
        w = S.batch_sites(reads, SC.K, True, c._replace(B=3, cb=1))
        np.testing.assert_array_equal(w["context"], [[4, 5, 3], [4, 2, 3]])            # T M G, T C G


# ---------------------------------------------------------------------------------------------------------- GPU
def _cpu(t):
    return None if t is None else t.cpu().numpy()


def _assert_sites(st, want, what, keys=OUT_KEYS):
    assert st.n_sites == want["site_off"][-1], f"{what}: {st.n_sites} sites, expected {want['site_off'][-1]}"
    np.testing.assert_array_equal(st.site_off, want["site_off"], err_msg=f"{what}: site_off")
    for key in keys:
        got = _cpu(getattr(st, key))
        assert got is not None and got.shape == want[key].shape and got.dtype == want[key].dtype, f"{what}: {key} {got.shape} {got.dtype} vs {want[key].shape} {want[key].dtype}"
        np.testing.assert_array_equal(R.bits(got), R.bits(want[key]), err_msg=f"{what}: {key}")


def _own_reads(b, seqs, const_sps=None):
    """the batch's own fetched signal and dwells with the reads it was staged from, as sites_ref takes them"""
    sig = b.signal()
    dw = None if const_sps else b.dwell()
    out = []
    for i, s in enumerate(seqs):
        ss = SC.const_ss(s, const_sps) if const_sps else (dw[b.ev_off[i]:b.ev_off[i + 1]] if len(s) >= b.gen.kmer_size else [])
        out.append(dict(sig=sig[b.sig_off[i]:b.sig_off[i + 1]], ss=ss, seq=s, offset=float(b.offset[i])))
    return out


def _check(b, reads, k, meth, c, what, keys=OUT_KEYS):
    prof = b.gen.profile
    want = S.batch_sites(reads, k, meth, c, prof.range, prof.digitisation)
    st = b.sites(c.L, c.before, c.f, c.B, c.cb, dtype=c.dtype, norm=c.norm)
    _assert_sites(st, want, what, keys)
    off, ns = b.site_plan(c.L, c.before, c.f)
    assert ns == st.n_sites
    np.testing.assert_array_equal(off, want["site_off"])
    return st, want


@pytest.mark.gpu
@pytest.mark.parametrize("cid,mode", [(cid, api.MODE_CERTIFIED) for cid in METH_VECTORS] + [("r9_meth_tk4", api.MODE_EXACT)],
                         ids=[f"{cid}-certified" for cid in METH_VECTORS] + ["r9_meth_tk4-exact"])
def test_sites_of_the_methylation_vectors(cid, mode):
    """the fixture's reads through the HIP path: all outputs in all four settings and three geometries against sites_ref fed with the
    batch's own signal and dwells -- which are the fixture's; med2 / mad4 and the signal rows against Batch.chunks of the same batch"""
    o, k, reads = _vector(cid)
    _, _, gen = _context(dict(REFVEC_CASES)[cid], mode)
    for lo in range(0, len(reads), o.batch):
        part = reads[lo:lo + o.batch]
        b = gen.stage([r["seq"] for r in part]).run().wait()
        own = _own_reads(b, [r["seq"] for r in part])
        for r, w in zip(part, own):
            np.testing.assert_array_equal(w["sig"], r["sig"]); np.testing.assert_array_equal(w["ss"], r["ss"])
        labels = set()
        for (dtype, norm), (L, before) in zip(ALL_SETTINGS, GEOMETRIES + GEOMETRIES[:1]):
            c = S.Cfg(L, before, _focus(k), 21, 10, dtype, norm)
            st, want = _check(b, own, k, True, c, f"{cid} reads {lo}.. L {L} {dtype} {norm}")
            labels |= set(want["label"])
            ch = b.chunks(2048, 2048, 0, labels=False, signal=False)
            assert torch.equal(st.med2, ch.med2) and torch.equal(st.mad4, ch.mad4)
        if lo == 0:
            assert labels == {0, 1} or cid == "r9_meth_tk4"     # (four reads of the -K 4 vector need not hold an M)
        # the same bits through two paths: the rows of the first read against its chunks at stride 1 (chunk j starts at sample j)
        c = S.Cfg(64, 13, _focus(k), 0, 0, "f16", "medmad")
        st = b.sites(c.L, c.before, c.f, outputs=("signal", "site_read", "win_start"))
        one = b.chunks(64, 1, 0, labels=False)
        rd, w0 = _cpu(st.site_read), _cpu(st.win_start)
        first = np.flatnonzero(rd == 0)
        assert len(first) > 0
        rows = one.signal[torch.as_tensor(one.chunk_off[0] + w0[first], device=one.signal.device)]
        assert torch.equal(rows.view(torch.int16), st.signal[torch.as_tensor(first, device=st.signal.device)].view(torch.int16))
        b.free()
    gen.close()


def _ideal_time_context(meth):
    prof, fl = profiles.get_profile("dna-r9-prom")
    fl |= profiles.SQ_IDEAL_TIME | (profiles.SQ_METH if meth else 0)
    assert profiles.default_kmer_size(fl) == SC.K and int(prof.dwell_mean) == SC.SPS
    mean, stdv = model.synthetic_model(SC.K, meth=meth)
    return api.SignalGenerator(prof, fl, SC.K, mean, stdv, 42, mode=api.MODE_CERTIFIED)


@pytest.mark.gpu
@pytest.mark.parametrize("meth", [False, True], ids=["plain", "meth"])
def test_hand_built_reads_with_constant_dwell(meth):
    """the reads of test_helper_on_hand_worked_reads in an SQG_IDEAL_TIME context: the sites worked by hand, every output against sites_ref"""
    gen = _ideal_time_context(meth)
    for name, (seqs, c, plain, with_meth, _, _) in SC.CASES.items():
        b = gen.submit(seqs)
        own = _own_reads(b, seqs, SC.SPS)
        c9 = c._replace(B=9, cb=4, dtype="f32")
        st, want = _check(b, own, SC.K, meth, c9, f"{name} meth {meth}")
        sites = with_meth if meth else plain
        assert list(zip(_cpu(st.site_read), _cpu(st.site_pos), _cpu(st.win_start))) == sites, name
        if name in SC.CONTEXT:
            np.testing.assert_array_equal(_cpu(st.context)[0], SC.CONTEXT[name][0])
            np.testing.assert_array_equal(_cpu(st.ctx_start)[0], SC.CONTEXT[name][1])
        b.free()
    # the shortest and a long window on a 2100-base read; L = 4096 is 8 steps of a wavefront's 512 samples
    seqs = [SC.long_read(), SC.planted(40, [(20, b"CG")])]
    b = gen.submit(seqs)
    own = _own_reads(b, seqs, SC.SPS)
    for L, before, B, cb, dtype, norm in ((16, 0, 21, 10, "f16", "medmad"), (16, 15, 255, 254, "f32", "pa"), (4096, 2048, 255, 0, "f16", "pa"), (4096, 1, 64, 63, "f32", "medmad")):
        st, want = _check(b, own, SC.K, meth, S.Cfg(L, before, 3, B, cb, dtype, norm), f"long read L {L} before {before}")
        assert st.n_sites >= 20 and (L == 16 or int(want["dropped"].sum()) >= 10)
    b.free(); gen.close()


@pytest.mark.gpu
def test_scan_tile_edge_dropped_candidates_and_batches_without_sites():
    """real dwells: sites whose anchor events are 1023, 1024 and 1025 -- the edge of the scan's 1024-event tile --, a read whose candidates
    are all dropped, a read shorter than a k-mer (whose stand-in sequence holds CG), a batch without sites, an empty batch"""
    prof, fl = profiles.get_profile("dna-r9-prom")
    fl |= profiles.SQ_METH
    k = 6
    mean, stdv = model.synthetic_model(k, meth=True)
    gen = api.SignalGenerator(prof, fl, k, mean, stdv, 7, mode=api.MODE_CERTIFIED)
    seqs = SC.tile_edge_reads() + [SC.planted(30, [(8, b"CG"), (20, b"MG")]), b"ACGCG", SC.planted(1500, [(p, b"CG") for p in range(0, 1490, 7)])]
    b = gen.submit(seqs)
    own = _own_reads(b, seqs)
    assert int(np.asarray(own[0]["ss"]).max()) > int(np.asarray(own[0]["ss"]).min())       # the dwells are drawn
    for c in (S.Cfg(512, 256, 3, 21, 10, "f16", "medmad"), S.Cfg(512, 511, 3, 255, 127, "f32", "pa"), S.Cfg(1024, 0, 0, 1, 0, "f16", "pa")):
        st, want = _check(b, own, k, True, c, f"tile edge L {c.L}")
        got = set(zip(_cpu(st.site_read), _cpu(st.site_pos)))
        if c.f == 3:
            assert {(0, 1026), (0, 1028), (1, 1027), (1, 2000)} <= got                      # anchors 1023, 1025, 1024
        off = want["site_off"]
        assert off[3] == off[2] == off[4] and want["dropped"][2] == 2 and want["dropped"][3] == 0      # all dropped; shorter than a k-mer
        assert off[5] - off[4] > 100
    b.free()
    seqs = [SC.planted(300, []), b"ACG", SC.planted(40, [(10, b"CG")])]
    b = gen.submit(seqs)
    own = _own_reads(b, seqs)
    st, want = _check(b, own, k, True, S.Cfg(512, 256, 3, 21, 10, "f16", "medmad"), "no site")
    assert st.n_sites == 0 and tuple(st.signal.shape) == (0, 512) and want["dropped"].sum() == 1
    assert (_cpu(st.med2) != 0).any()                       # med2 / mad4 are written all the same
    b.free()
    b = gen.submit([])
    st = b.sites(64, ctx_len=5)
    assert st.n_sites == 0 and list(st.site_off) == [0] and tuple(st.ctx_start.shape) == (0, 6) and tuple(st.med2.shape) == (0,)
    assert b.site_plan(64)[1] == 0
    b.free(); gen.close()


def _raw_call(gen, b, cfg, ptrs):
    return gen.L.sqg_batch_sites(gen.ctx, b.handle, C.byref(cfg), C.byref(api.CSiteOut(*[ptrs.get(n) for n in OUT_KEYS])))


@pytest.mark.gpu
def test_nothing_but_the_rows_is_written():
    """caller arrays at odd addresses inside one guarded buffer: the bytes of every output are sites_ref's, every other byte keeps its
    fill; context rows of 1 and 255 bases; every subset of the outputs with the others NULL"""
    prof, fl = profiles.get_profile("dna-r9-prom")
    fl |= profiles.SQ_METH
    k = 6
    mean, stdv = model.synthetic_model(k, meth=True)
    gen = api.SignalGenerator(prof, fl, k, mean, stdv, 11, mode=api.MODE_CERTIFIED)
    seqs = [SC.planted(90, [(p, b"CG") for p in range(4, 80, 9)] + [(31, b"MG")]), SC.planted(61, [(p, b"MG") for p in range(2, 55, 11)]), b"ACGCG"]
    b = gen.submit(seqs)
    own = _own_reads(b, seqs)
    buf = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
    base = buf.data_ptr()
    assert base % 16 == 0

    wants = {}

    def run(c, names):
        if c not in wants:
            wants[c] = S.batch_sites(own, k, True, c, prof.range, prof.digitisation)
        want = wants[c]
        ns = int(want["site_off"][-1])
        assert ns >= 10
        at, place = 48, {}
        for name in OUT_KEYS:                                # 16-byte aligned signal; the byte arrays at odd addresses; the rest at their natural alignment
            align = {"signal": 16, "label": 1, "context": 1, "win_start": 8}.get(name, 4)
            at = (at + align - 1) // align * align
            if align == 1 and at % 2 == 0:
                at += 1
            place[name] = at
            at += want[name].nbytes + 24
        assert at < buf.numel()
        buf.fill_(0xA5)
        torch.cuda.synchronize()
        cfg = api.CSiteCfg(c.L, c.before, c.f, c.B, c.cb, api.CHUNK_F32 if c.dtype == "f32" else api.CHUNK_F16, api.CHUNK_PA if c.norm == "pa" else api.CHUNK_MEDMAD)
        assert _raw_call(gen, b, cfg, {n: base + place[n] for n in names}) == 0, gen.L.sqg_last_error(gen.ctx)
        got = buf.cpu().numpy()
        expect = np.full(buf.numel(), 0xA5, np.uint8)
        for n in names:
            expect[place[n]:place[n] + want[n].nbytes] = np.ascontiguousarray(want[n]).view(np.uint8).reshape(-1)
        bad = np.flatnonzero(got != expect)
        assert len(bad) == 0, f"{c} {names}: byte {bad[0]} of the buffer ({[n for n in OUT_KEYS if place[n] <= bad[0]][-1]} is at {place})"

    for B, cb in ((1, 0), (255, 0), (255, 254), (0, 0)):
        for dtype, norm in (("f16", "medmad"), ("f32", "pa")):
            run(S.Cfg(16, 5, 3, B, cb, dtype, norm), OUT_KEYS)
    c = S.Cfg(24, 23, 2, 5, 2, "f16", "medmad")
    for m in range(len(OUT_KEYS) + 1):
        for names in itertools.combinations(OUT_KEYS, m):
            run(c, names)
    b.free(); gen.close()


@pytest.mark.gpu
def test_sampled_methylated_reads_of_both_strands():
    """load_genome + set_meth + sample: the reads are the sampler's, taken back with Batch.reads(); sites_ref is fed with them and with
    the batch's own signal and dwells"""
    prof, fl = profiles.get_profile("dna-r9-prom")
    fl |= profiles.SQ_METH
    k, T_, rlen = 6, 3, 1500
    mean, stdv = model.synthetic_model(k, meth=True)
    orac = orc.Oracle(prof, fl, k, mean, stdv, 42, num_workers=T_, rlen=rlen)
    ref = orac.load_ref(NCOV, None, MFREQ_DENSE)
    contigs = [bytes(ref.seqs[i][:ref.lengths[i]]) for i in range(ref.num_ref)]
    names = [ref.names[i].decode() for i in range(ref.num_ref)]
    gen = api.SignalGenerator(prof, fl, k, mean, stdv, 42, num_workers=T_, mode=api.MODE_CERTIFIED)
    gen.load_genome(contigs, rlen)
    gen.set_meth(contigs, names, MFREQ_DENSE)
    b = gen.sample(24).run().wait()
    seqs = b.reads()
    assert set(b.sampled["strand"]) == set(b"+-")
    assert any(b"M" in s for s, sd in zip(seqs, b.sampled["strand"]) if sd == ord("-")) and any(b"M" in s for s, sd in zip(seqs, b.sampled["strand"]) if sd == ord("+"))
    own = _own_reads(b, seqs)
    st, want = _check(b, own, k, True, S.Cfg(256, 128, 3, 21, 10, "f16", "medmad"), "sampled")
    assert set(want["label"]) == {0, 1} and st.n_sites > 200 and want["dropped"].sum() > 0
    _check(b, own, k, True, S.Cfg(1024, 100, 2, 64, 0, "f32", "pa"), "sampled L 1024")
    b.free(); gen.close(); orac.close()


@pytest.mark.gpu
def test_errors():
    dummy = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    for name, extra, seq in (("rna-r9-prom", 0, b"ACGUACGUCGCG" * 30), ("dna-r9-prom", profiles.SQ_PREFIX, b"ACGTACGTCGCG" * 30)):
        prof, fl = profiles.get_profile(name)
        fl |= extra
        k = profiles.default_kmer_size(fl)
        mean, stdv = model.synthetic_model(k)
        gen = api.SignalGenerator(prof, fl, k, mean, stdv, 42)
        b = gen.submit([seq])
        for call in (lambda: b.sites(64), lambda: b.site_plan(64)):
            with pytest.raises(api.SqgError) as e:
                call()
            assert e.value.code == -1 and ("SQG_RNA" if fl & profiles.SQ_RNA else "SQG_PREFIX") in str(e.value)
        b.free(); gen.close()
    o, k, reads = _vector("r9_meth_dense")
    _, _, gen = _context(dict(REFVEC_CASES)["r9_meth_dense"], api.MODE_CERTIFIED)
    b = gen.stage([r["seq"] for r in reads])
    for call in (lambda: b.sites(64), lambda: b.site_plan(64)):
        with pytest.raises(api.SqgError) as e:              # staged, not run: an error, not a hang
            call()
        assert e.value.code == -4
    b.run().wait()
    good = dict(win_len=64, before=32, focus=3, ctx_len=21, ctx_before=10)
    assert b.sites(**good).n_sites > 0
    for bad in (dict(win_len=8), dict(win_len=60), dict(win_len=65544), dict(win_len=0), dict(before=-1), dict(before=64), dict(focus=-1), dict(focus=6),
                dict(ctx_len=-1), dict(ctx_len=256), dict(ctx_before=-1), dict(ctx_before=21), dict(ctx_len=0, ctx_before=1), dict(dtype=7), dict(norm=2)):
        with pytest.raises(api.SqgError) as e:
            b.sites(**{**good, **bad})
        assert e.value.code == -1 and "sqg_" in str(e.value), bad
        what = next(iter(bad)) if len(bad) == 1 else "ctx_before"
        assert what in str(e.value), f"{bad}: {e.value}"
    Lb, cfg, ns = gen.L, api.CSiteCfg(64, 32, 3, 21, 10, 0, 0), C.c_int64()
    assert Lb.sqg_batch_sites(None, None, None, None) == -1 and Lb.sqg_site_plan(None, None, None, None, None) == -1
    assert Lb.sqg_batch_sites(gen.ctx, None, C.byref(cfg), C.byref(api.CSiteOut())) == -1
    assert Lb.sqg_batch_sites(gen.ctx, b.handle, None, C.byref(api.CSiteOut())) == -1
    assert Lb.sqg_batch_sites(gen.ctx, b.handle, C.byref(cfg), None) == -1
    assert b"sqg_batch_sites" in Lb.sqg_last_error(gen.ctx) and b"out" in Lb.sqg_last_error(gen.ctx)
    out = api.CSiteOut(dummy.data_ptr() + 8, *[None] * 8)
    assert Lb.sqg_batch_sites(gen.ctx, b.handle, C.byref(cfg), C.byref(out)) == -1 and b"16-byte" in Lb.sqg_last_error(gen.ctx)
    assert not dummy.any()
    assert Lb.sqg_site_plan(gen.ctx, b.handle, C.byref(cfg), None, None) == -1 and b"n_sites" in Lb.sqg_last_error(gen.ctx)
    assert Lb.sqg_site_plan(gen.ctx, b.handle, C.byref(cfg), None, C.byref(ns)) == 0 and ns.value == b.sites(**good).n_sites
    assert Lb.sqg_batch_sites(gen.ctx, b.handle, C.byref(cfg), C.byref(api.CSiteOut())) == 0          # nothing wanted: nothing written
    b.free(); gen.close()


@pytest.mark.gpu
def test_lifetime_and_sites_while_the_generator_runs_ahead():
    """a batch keeps its sites until two more batches have been run; taken while two later batches are staged and one is running they
    are what they were when the generator was quiet"""
    o, k, reads = _vector("r9_meth_tk4")
    _, _, gen = _context(dict(REFVEC_CASES)["r9_meth_tk4"], api.MODE_EXACT)
    parts = [[r["seq"] for r in reads[0:4]], [r["seq"] for r in reads[4:8]], [r["seq"] for r in reads[0:4]], [r["seq"] for r in reads[4:8]]]
    kw = dict(win_len=256, before=100, focus=3, ctx_len=21, ctx_before=10)
    b0 = gen.stage(parts[0]).run().wait()
    quiet = b0.sites(**kw)
    _assert_sites(quiet, S.batch_sites(_own_reads(b0, parts[0]), k, True, S.Cfg(256, 100, 3, 21, 10), o.profile.range, o.profile.digitisation), "quiet")
    assert quiet.n_sites > 0
    b1, b2, b3 = (gen.stage(p) for p in parts[1:])
    b1.run()                                                # one running, two staged
    for turn in range(2):                                   # with the plan of the quiet call in the scratch, then with another made in between
        busy = b0.sites(**kw)
        assert busy.n_sites == quiet.n_sites and b0.site_plan(64, 32, 3)[1] >= quiet.n_sites
        for key in OUT_KEYS:
            assert torch.equal(getattr(busy, key), getattr(quiet, key)), key
    b1.wait()
    again = b0.sites(**kw)                                  # after one more batch has run: the same
    for key in OUT_KEYS:
        assert torch.equal(getattr(again, key), getattr(quiet, key)), key
    b2.run().wait()
    for call in (lambda: b0.sites(**kw), lambda: b0.site_plan(256, 100, 3)):
        with pytest.raises(api.SqgError) as e:              # two more batches: slabs and dwells are batch 2's
            call()
        assert e.value.code == -4 and "sqg_" in str(e.value)
    st = b1.sites(**kw)
    _assert_sites(st, S.batch_sites(_own_reads(b1, parts[1]), k, True, S.Cfg(256, 100, 3, 21, 10), o.profile.range, o.profile.digitisation), "batch 1 after batch 2")
    for b in (b0, b1, b2, b3):
        b.free()
    gen.close()
