"""svb-zd, BLOW5 framing / Huffman coding and the chunk kernels on signals the generator never makes.

Everything behind the sample kernel is a function of an int16 array, and natural signal is all alike: 213 ... 1315, never negative, no
three-byte svb-zd value, at most 878 codes in a read.  Here a batch is run for its geometry, its samples are overwritten on the device
(inject.py) with the arrays of signal_cases.py -- each shown on the CPU to be what its name says (test_signal_cases.py) -- and the
library's outputs are compared bit for bit with the plain references over the same array: orc.svb_zd and slow5lib's committed bytes,
the host BLOW5 writer fed with the oracle's encodings and read back by the deflate reader of test_blow5_huffman.py, chunks_ref."""
import os
import struct

import numpy as np
import pytest
import torch  # noqa: F401  (before the library is loaded: the HIP runtime torch brings is the one the library then uses)

import chunks_ref as R
import inject
import orc
import signal_cases as SC
from squigulator_amd import api, build, model, profiles
from test_blow5 import parse_blow5
from test_blow5_huffman import huffman_records
import chunk_support as TC

ALL_SETTINGS, _assert_equal, _cpu = TC.ALL_SETTINGS, TC._assert_equal, TC._cpu

pytestmark = pytest.mark.gpu


def _exact1():
    """the svb / BLOW5 geometry: a batch whose reads have exactly SC.EXACT1_LENGTHS samples -- asserted, not hoped for"""
    gen, prof, fl, k = inject.context("exact1")
    b = inject.run_geometry(gen, inject.seqs_for(inject.bases_for(SC.EXACT1_LENGTHS, k, 1)))
    lens = np.diff(b.sig_off)
    np.testing.assert_array_equal(lens, SC.EXACT1_LENGTHS)
    SC.check_svb_geometry(lens)
    assert len({int(o) % 8 for o in b.sig_off[:-1]}) >= 6             # the reads start at all kinds of addresses
    return gen, prof, fl, k, b


@pytest.mark.parametrize("case", list(SC.SVB_CASES))
def test_svb_zd(case):
    """compress() == orc.svb_zd read by read, the offsets, the round trip; slow5lib's own bytes where a read is a golden array"""
    assert api.dev_knobs_set() == []
    gen, prof, fl, k, b = _exact1()
    arr = SC.SVB_CASES[case](b.sig_off)
    inject.inject(b, arr)
    enc, off = b.compress()
    assert off[0] == 0 and off[-1] == len(enc)
    gold = {len(s): e for s, e in SC.svb_goldens() if len(s)}
    seen = 0
    for i in range(b.n_reads):
        s = arr[b.sig_off[i]:b.sig_off[i + 1]]
        got = enc[off[i]:off[i + 1]]
        np.testing.assert_array_equal(got, orc.svb_zd(s), err_msg=f"{case}: read {i} ({len(s)} samples)")
        dec, used = orc.svb_zd_decode(got)
        np.testing.assert_array_equal(dec, s)
        assert used == len(got)
        if case == "slow5lib_goldens" and len(s) in gold:
            np.testing.assert_array_equal(got, gold[len(s)], err_msg=f"slow5lib's bytes of the array of {len(s)} samples")
            seen += 1
    assert case != "slow5lib_goldens" or seen >= 15
    enc2, off2 = b.compress()                                           # always recomputed: the same again
    np.testing.assert_array_equal(off2, off)
    np.testing.assert_array_equal(enc2, enc)
    b.free(); gen.close()


def _samples_of(raw):
    """the int16 samples a raw BLOW5 record carries"""
    (idl,) = struct.unpack_from("<H", raw, 0)
    q = 2 + idl + 4 + 32
    (nb,) = struct.unpack_from("<Q", raw, q)
    dec, used = orc.svb_zd_decode(np.frombuffer(raw, np.uint8, nb, q + 8))
    assert used == nb
    return dec, idl, nb


@pytest.mark.parametrize("case", list(SC.SVB_CASES))
def test_blow5_records(case, tmp_path):
    """both device modes, through blow5_records and through write_batch, with and without the ONT trailer: the host writer's bytes (the
    host side coded from the ORACLE's svb-zd), valid two-block streams with codes of at most 15 bits, the injected samples inside"""
    assert api.dev_knobs_set() == []
    gen, prof, fl, k, b = _exact1()
    assert api.LOADED_PATH == os.path.abspath(build.LIB)                # the product library, no knob
    arr = SC.SVB_CASES[case](b.sig_off)
    inject.inject(b, arr)
    b.compress()                                                        # (inject.py: before any BLOW5 call)
    n = b.n_reads
    ids = inject.read_ids(n)
    assert {1, 15, 16, 17, 4096} <= {len(x) for x in ids}
    for ont in (0, profiles.SQ_ONT):
        for mode, mflag in (("huffman", api.BLOW5_HUFFMAN), ("stored", 0)):
            tag = f"{mode}{'_ont' if ont else ''}"
            host, hs = inject.host_blow5(str(tmp_path / f"host_{tag}.blow5"), prof, fl | ont, ids, b.offset, b.median_before, b.sig_off, arr,
                                         **{mode: True})
            recs, ro = b.blow5_records(prof, ont | mflag, ids)
            assert ro[-1] == len(recs) and recs == host[68 + hs:-5], f"{case} {tag}: sqg_batch_blow5_records"
            p_dev = str(tmp_path / f"dev_{tag}.blow5")
            w = api.Blow5Writer(p_dev, prof, fl | ont, **{mode: True})
            w.write_batch(b, ids)
            nbytes = w.close()
            dev = open(p_dev, "rb").read()
            assert nbytes == len(dev) and dev == host, f"{case} {tag}: sqg_blow5_write_batch"
            if mode == "huffman":                                       # either trailer: every record through parse_record
                parsed = huffman_records(dev)                           # two BTYPE-10 blocks, the cut, lengths <= 15, Adler-32, zlib.decompress
                raws = [r[0] for r in parsed]
                assert raws == parse_blow5(dev)[1]
                if case == "fibonacci":                                 # the length limiter at deflate's own limit, on the device
                    deep = [max(lb) for (_, _, lb), m in zip(parsed, SC.EXACT1_LENGTHS) if m > 60000]
                    assert len(deep) >= 4 and set(deep) == {15}
            else:
                raws = parse_blow5(dev)[1]
            assert len(raws) == n
            for i, raw in enumerate(raws):
                dec, idl, nb = _samples_of(raw)
                assert idl == len(ids[i]) and len(raw) == 2 + idl + 4 + 32 + 8 + nb + 30 + (1 if ont else 0)
                np.testing.assert_array_equal(dec, arr[b.sig_off[i]:b.sig_off[i + 1]], err_msg=f"{case} {tag}: record {i}")
    b.free(); gen.close()


# ---- chunks ------------------------------------------------------------------------------------------------------------------------
CHUNK_CASES = [("stats_edges", "exact1"), ("every_code", "exact2"), ("slow5lib_goldens", "exact1"), ("svb_classes", "exact1"),
               ("svb_wrap", "drawn"), ("svb_borders", "drawn"), ("uniform", "drawn"), ("all_equal", "drawn"), ("one_value_but_one", "drawn"),
               ("fibonacci", "drawn")]
LS = [(64, 8), (4096, 4096), (128, 33)]                                 # stride 33: chunks start at odd 2-byte addresses (k_chunk_emit's `odd`)


def _chunk_batch(geometry, range_div=1.0, lib_path=None):
    # (a range 2^14 times smaller makes the generator's own samples absurd, too many for the certified mode's FP64 list: the exact mode there;
    # the samples are overwritten anyway)
    gen, prof, fl, k = inject.context(geometry, range_div, lib_path=lib_path, mode=api.MODE_CERTIFIED if range_div == 1.0 else api.MODE_EXACT)
    if geometry == "drawn":
        seqs = inject.seqs_for(SC.DRAWN_BASES)
    else:
        lens, dwell = (SC.EXACT1_LENGTHS, 1) if geometry == "exact1" else (SC.EXACT2_LENGTHS, 2)
        seqs = inject.seqs_for(inject.bases_for(lens, k, dwell))
    b = inject.run_geometry(gen, seqs)
    lens_got = np.diff(b.sig_off)
    if geometry == "drawn":
        assert lens_got.max() > 70000 and lens_got.min() < 8 and {int(x) & 1 for x in lens_got} == {0, 1}
        assert len(set(b.dwell().tolist())) > 8                         # irregular event boundaries
    else:
        np.testing.assert_array_equal(lens_got, lens)
    return gen, prof, fl, k, b, seqs


def _ref_reads(b, arr, seqs):
    dw = b.dwell()
    return [dict(sig=arr[b.sig_off[i]:b.sig_off[i + 1]], ss=dw[b.ev_off[i]:b.ev_off[i + 1]], seq=seqs[i], offset=b.offset[i])
            for i in range(b.n_reads)]


def _check_chunks(case, geometry, div, W=48):
    """one context at range / div: the injected batch's chunks against chunks_ref, setting by setting"""
    gen, prof, fl, k, b, seqs = _chunk_batch(geometry, div)
    arr = SC.CASES[case](b.sig_off)
    labels_before = b.chunks(64, 8, W) if div == 1.0 else None          # the generator's own samples: the labels must come out the same
    inject.inject(b, arr)
    reads = _ref_reads(b, arr, seqs)
    stats = [R.stats(r["sig"]) for r in reads]
    if case == "every_code":
        assert stats[:len(SC.EVERY_CODE_STATS)] == SC.EVERY_CODE_STATS
    if case == "stats_edges":
        for i, want in SC.stats_edges_expect(b.sig_off).items():
            assert all(w is None or w == g for w, g in zip(want[:2], stats[i]))
    settings = ALL_SETTINGS if div == 1.0 else [("f16", "pa"), ("f32", "pa")]
    for L, S in (LS if div == 1.0 else LS[:1]):
        for dtype, norm in settings:
            with np.errstate(over="ignore"):
                want = R.batch_chunks(reads, k, False, False, L, S, W, dtype, norm, prof.range, prof.digitisation)
            ch = b.chunks(L, S, W, dtype=dtype, norm=norm)
            _assert_equal(ch, want, f"{case} L {L} S {S} {dtype} {norm} range / {div:g}")
            if (L, S) == (64, 8) and labels_before is not None:
                np.testing.assert_array_equal(_cpu(ch.labels), _cpu(labels_before.labels))
                np.testing.assert_array_equal(_cpu(ch.label_len), _cpu(labels_before.label_len))
    if case == "every_code":                                            # what the case is for, seen in the device's own output
        got = R.bits(_cpu(b.chunks(64, 64, 0, dtype="f16", norm=("medmad" if div == 1.0 else "pa")).signal))
        if div == 1.0:
            assert (got == 0x7c00).any() and (got == 0xfc00).any()      # +inf, -inf
        elif div == 2.0 ** 14:
            assert np.count_nonzero(((got & 0x7fff) > 0) & ((got & 0x7fff) < 0x0400)) >= 4
        else:
            assert (got == 0x8000).any() and (got == 0).any()           # -0, +0
    b.free(); gen.close()


@pytest.mark.parametrize("case,geometry", CHUNK_CASES, ids=[c for c, _ in CHUNK_CASES])
def test_injected_chunks(case, geometry, monkeypatch):
    """chunks() == chunks_ref over the injected array with the batch's own dwells and reads: every dtype x norm, three L / S, labels too"""
    monkeypatch.delenv("SQG_TEST_CHUNK_GENERIC", raising=False)
    assert api.dev_knobs_set() == []
    _check_chunks(case, geometry, 1.0)


@pytest.mark.parametrize("div", [2.0 ** 14, 2.0 ** 24], ids=["subnormal", "signed_zero"])
def test_every_code_in_small_picoamperes(div, monkeypatch):
    """PA with the profile's range / 2^14 (float16 subnormals) and / 2^24 (the smallest values round to +0 and -0)"""
    monkeypatch.delenv("SQG_TEST_CHUNK_GENERIC", raising=False)
    _check_chunks("every_code", "exact2", div)


@pytest.mark.parametrize("force", ["1", "2"], ids=["wide", "long"])
@pytest.mark.parametrize("case,geometry", CHUNK_CASES, ids=[c for c, _ in CHUNK_CASES])
def test_injected_statistics_by_the_generic_paths(case, geometry, force, monkeypatch):
    """the development library's SQG_TEST_CHUNK_GENERIC: the same med2 / mad4 whichever path counts them"""
    monkeypatch.delenv("SQG_TEST_CHUNK_GENERIC", raising=False)
    gen, prof, fl, k, b, seqs = _chunk_batch(geometry, lib_path=build.LIB_DEV)
    arr = SC.CASES[case](b.sig_off)
    inject.inject(b, arr)
    monkeypatch.setenv("SQG_TEST_CHUNK_GENERIC", force)
    ch = b.chunks(64, 64, 0, signal=False, labels=False)
    want = [R.stats(arr[b.sig_off[i]:b.sig_off[i + 1]]) for i in range(b.n_reads)]
    np.testing.assert_array_equal(_cpu(ch.med2), [w[0] for w in want], err_msg=f"{case}: med2")
    np.testing.assert_array_equal(_cpu(ch.mad4), [w[1] for w in want], err_msg=f"{case}: mad4")
    if case == "every_code":
        with np.errstate(over="ignore"):
            want = R.batch_chunks(_ref_reads(b, arr, seqs), k, False, False, 4096, 4096, 48, "f16", "medmad")
            _assert_equal(b.chunks(4096, 4096, 48), want, f"{case} forced {force}")
    b.free(); gen.close()


def test_the_generator_is_unharmed_by_an_injection():
    """the stream states carried from batch to batch do not live in the signal slab: after an injected batch has been used and freed, the
    context's next batches still equal the oracle"""
    name, extra, _, _ = inject.GEOMETRIES["drawn"]
    prof, fl = profiles.get_profile(name)
    k = profiles.default_kmer_size(fl)
    mean, stdv = model.synthetic_model(k)
    batches = [inject.seqs_for(SC.DRAWN_BASES, seed=s) for s in (3, 4, 5)]
    orac = orc.Oracle(prof, fl, k, mean, stdv, inject.SEED, num_workers=1)
    want = [orac.run_batch_seqs(bt) for bt in batches]
    orac.close()
    gen, prof2, fl2, k2 = inject.context("drawn")
    assert (prof2, fl2, k2) == (prof, fl, k)
    for bi, bt in enumerate(batches):
        b = inject.run_geometry(gen, bt)
        sig = b.signal()
        for i, w in enumerate(want[bi]):
            np.testing.assert_array_equal(sig[b.sig_off[i]:b.sig_off[i + 1]], w.sig, err_msg=f"batch {bi} read {i}")
        if bi == 0:
            arr = SC.uniform(b.sig_off)
            inject.inject(b, arr)
            enc, off = b.compress()
            np.testing.assert_array_equal(enc[off[-2]:off[-1]], orc.svb_zd(arr[b.sig_off[-2]:b.sig_off[-1]]))
            b.blow5_records(prof, api.BLOW5_HUFFMAN, inject.read_ids(b.n_reads))
            b.chunks(64, 8, 16)
        b.free()
    gen.close()
