"""signal_cases.py proven without a GPU: every adversarial array does what its name says, shown with the references alone -- orc.svb_zd
and slow5lib's committed bytes, the host BLOW5 encoder with the deflate reader of test_blow5_huffman.py, chunks_ref.  The arrays are
built over the read lengths the GPU tests run (test_injected_signals.py asserts that the batch it got has them)."""
import os
import struct

import numpy as np
import pytest

import chunks_ref as R
import inject
import orc
import signal_cases as SC
from squigulator_amd import profiles
from test_blow5_huffman import cut_of, huffman_depth, huffman_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFF1 = SC.offsets(SC.EXACT1_LENGTHS)
OFF2 = SC.offsets(SC.EXACT2_LENGTHS)


def _reads(arr, off):
    return [arr[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def _svb_parts(enc):
    """-> (count, 2-bit codes [count], data bytes)"""
    count = int(enc[:4].view(np.uint32)[0])
    nkey = (count + 3) // 4
    codes = ((enc[4:4 + nkey, None] >> (2 * np.arange(4, dtype=np.uint8))) & 3).reshape(-1)[:count]
    return count, codes, enc[4 + nkey:]


def _zigzag(sig):
    d = np.diff(np.concatenate(([0], sig.astype(np.int64))))
    return (d << 1) ^ (d >> 63)


def test_the_planned_lengths_meet_the_conditions():
    SC.check_svb_geometry(SC.EXACT1_LENGTHS)
    assert all(n % 2 == 0 and n >= 131072 for n in SC.EXACT2_LENGTHS[:len(SC.EVERY_CODE_TARGETS)])
    assert min(SC.EXACT2_LENGTHS[:len(SC.EVERY_CODE_TARGETS)]) >= 65536 + 4096
    with pytest.raises(AssertionError):
        SC.check_svb_geometry([n for n in SC.EXACT1_LENGTHS if n != 1027])


@pytest.mark.parametrize("geometry,lens,dwell", [("exact1", SC.EXACT1_LENGTHS, 1), ("exact2", SC.EXACT2_LENGTHS, 2)])
def test_ideal_time_gives_exactly_these_lengths(geometry, lens, dwell):
    """the same context and reads through the CPU backend (the oracle behind the C ABI): n = (bases - k + 1) * dwell"""
    import subprocess
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "libsqg_cpu.so"])
    gen, prof, fl, k = inject.context(geometry, lib_path=os.path.join(ROOT, "oracle", "libsqg_cpu.so"))
    b = inject.run_geometry(gen, inject.seqs_for(inject.bases_for(lens, k, dwell)))
    np.testing.assert_array_equal(b.sig_off, SC.offsets(lens))
    assert set(b.dwell().tolist()) == {dwell}
    b.free(); gen.close()


def test_every_case_fills_the_batch_and_is_deterministic():
    for name, build in SC.SVB_CASES.items():
        a = build(OFF1)
        assert a.dtype == np.int16 and len(a) == OFF1[-1], name
        if name in ("uniform", "stats_edges"):
            np.testing.assert_array_equal(a, build(OFF1), err_msg=name)


def test_slow5lib_goldens():
    arr = SC.slow5lib_goldens(OFF1)
    gold = {len(s): (s, e) for s, e in SC.svb_goldens() if len(s)}
    seen = 0
    for r in _reads(arr, OFF1):
        if len(r) in gold:
            s, e = gold[len(r)]
            np.testing.assert_array_equal(r, s)
            np.testing.assert_array_equal(orc.svb_zd(r), e, err_msg=f"array of {len(r)} samples")
            seen += 1
    assert seen >= len(gold) == 15
    assert arr.min() == -32768 and arr.max() == 32767


def test_svb_classes():
    arr = SC.svb_classes(OFF1)
    for r in _reads(arr, OFF1):
        if len(r) < 36:
            continue
        count, codes, _ = _svb_parts(orc.svb_zd(r))
        assert count == len(r)
        for j in range(4):                                  # every field of the key bytes holds 1-, 2- and 3-byte codes, none holds 4
            assert set(codes[j::4].tolist()) == {0, 1, 2}, (len(r), j)
        z = _zigzag(r)
        for j in range(4):
            assert set(SC.CLASS_Z) <= set(z[j::4].tolist()), (len(r), j)
        np.testing.assert_array_equal(codes, np.where(z < 256, 0, np.where(z < 65536, 1, 2)))


def test_svb_wrap():
    for r in _reads(SC.svb_wrap(OFF1), OFF1):
        count, codes, data = _svb_parts(orc.svb_zd(r))
        # the first value is the delta to 0 (-32768: z = 65535, two bytes); every other one is +-65535: three bytes
        assert codes[0] == 1 and (codes[1:] == 2).all() and len(data) == 3 * len(r) - 1
        assert set(_zigzag(r)[1:].tolist()) <= {131070, 131069}


def test_svb_borders():
    for r in _reads(SC.svb_borders(OFF1), OFF1):
        n = len(r)
        count, codes, data = _svb_parts(orc.svb_zd(r))
        steps = SC.border_steps(n)
        big = np.flatnonzero(codes == 2)
        np.testing.assert_array_equal(big, steps)
        inner = steps[steps < n - 1] if n - 1 not in np.arange(256, n, 256) else steps
        assert (inner % 256 == 0).all()                     # quad 64 m: lane 0 of a wavefront, whose predecessor is fetched, not shuffled
        if n > 1024:
            assert 1024 in steps                            # quad 256: the first of the second pass
        assert (codes[np.setdiff1d(np.arange(1, n), steps)] == 0).all() and codes[0] == 1


CPU_LIB = os.path.join(ROOT, "oracle", "libsqg_cpu.so")


def _host_records(arr, off, tmp_path, ont=False):
    """the host encoder's Huffman records (parsed) and the sizes of its Huffman and stored records; the CPU backend's writer is the product's
    (csrc/h_blow5.h), so this needs no HIP library"""
    import subprocess
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "libsqg_cpu.so"])
    prof, fl = profiles.get_profile("dna-r9-prom")
    fl |= profiles.SQ_ONT if ont else 0
    n = len(off) - 1
    ids = inject.read_ids(n)
    out = {}
    for mode in ("huffman", "stored"):
        buf, hs = inject.host_blow5(str(tmp_path / (mode + ".blow5")), prof, fl, ids, np.linspace(1, 2, n), np.linspace(180, 220, n), off, arr,
                                    lib_path=CPU_LIB, **{mode: True})
        out[mode] = buf
    sizes = []
    for buf in (out["huffman"], out["stored"]):
        p, sz = 68 + struct.unpack_from("<I", buf, 64)[0], []
        while buf[p:] != b"5WOLB":
            sz.append(struct.unpack_from("<Q", buf, p)[0])
            p += 8 + sz[-1]
        sizes.append(np.array(sz))
    return huffman_records(out["huffman"]), sizes[0], sizes[1]


@pytest.mark.parametrize("ont", [False, True], ids=["plain", "ont"])
def test_uniform(ont, tmp_path):
    arr = SC.uniform(OFF1)
    recs, nh, ns = _host_records(arr, OFF1, tmp_path, ont=ont)
    assert (nh <= 1.01 * ns + 300).all()                    # incompressible: every record at most 1 % + 300 B over stored blocks
    raw, la, lb = recs[0]                                   # the longest read: block B uses every byte value, none is rare
    counts = np.bincount(np.frombuffer(raw[cut_of(raw):], np.uint8), minlength=256)
    assert counts.min() > 0.5 * np.median(counts) and max(lb[:256]) <= 10 and np.median(lb[:256]) >= 8, (counts.min(), np.median(counts), set(lb))
    z = _zigzag(_reads(arr, OFF1)[0])
    assert (z >= 65536).mean() > 0.2 and (z < 256).any()


def test_constant_reads(tmp_path):
    for name in ("all_equal", "one_value_but_one"):
        arr = SC.CASES[name](OFF1)
        for i, r in enumerate(_reads(arr, OFF1)):
            med2, mad4 = R.stats(r)
            assert (mad4 == 0 and med2 == 2 * int(r[0])) or len(r) == 2        # (600, 601 alone: med2 = 1201, mad4 = 2)
        recs, _, _ = _host_records(arr, OFF1, tmp_path)
        raw = recs[0][0]                                    # 100 003 samples
        (idl,) = struct.unpack_from("<H", raw, 0)
        h = 2 + idl + 4 + 32 + 8
        keys = np.frombuffer(raw[h + 4:cut_of(raw)], np.uint8)
        nb = struct.unpack_from("<Q", raw, h - 8)[0]
        data = np.frombuffer(raw[cut_of(raw):h + nb], np.uint8)
        # the first value's two bytes and zeros; the odd sample adds a step up and a step down (bytes 2 and 1)
        assert len(set(keys.tolist())) == 2 and 2 <= len(set(data.tolist())) <= (3 if name == "all_equal" else 5), name


@pytest.mark.parametrize("ont", [False, True], ids=["plain", "ont"])
def test_fibonacci(ont, tmp_path):
    arr = SC.fibonacci(OFF1)
    for r in _reads(arr, OFF1):
        enc, cnt = SC.fibonacci_encoding(len(r))
        np.testing.assert_array_equal(orc.svb_zd(r), enc)
        f = sorted(SC.fib_counts(len(r)), reverse=True)
        assert sorted(cnt.values(), reverse=True)[1:] == f[1:]
    recs, _, _ = _host_records(arr, OFF1, tmp_path, ont=ont)
    deep = 0
    for (raw, la, lb), n in zip(recs, SC.EXACT1_LENGTHS):
        counts = np.bincount(np.frombuffer(raw[cut_of(raw):], np.uint8), minlength=256).tolist() + [1]
        assert max(lb) <= 15 and max(la) <= 15
        if n > 60000:
            assert huffman_depth(counts) > 15 and max(lb) == 15, n      # the limiter at deflate's own limit had work to do
            deep += 1
    assert deep >= 4


def test_stats_edges():
    arr = SC.stats_edges(OFF1)
    np.testing.assert_array_equal(arr, SC.stats_edges(OFF1))
    expect = SC.stats_edges_expect(OFF1)
    stated = set()
    for i, r in enumerate(_reads(arr, OFF1)):
        med2, mad4 = R.stats(r)
        span = int(r.max()) - int(r.min()) + 1
        assert mad4 % 2 == 0
        for got, want, what in zip((med2, mad4, span), expect[i], ("med2", "mad4", "span")):
            if want is not None:
                assert got == want, (i, len(r), what, got, want)
                stated.add((what, want))
    assert {("span", 4096), ("span", 4097), ("span", 65536), ("mad4", 2), ("mad4", 131070), ("med2", 30003), ("med2", -1), ("span", 1)} <= stated
    r = _reads(arr, OFF1)[SC.EXACT1_LENGTHS.index(2050)]
    assert np.count_nonzero(r == 777) == 1025


def test_mad4_is_always_even():
    rng = np.random.default_rng(2)
    for _ in range(300):
        r = rng.integers(-40, 40, int(rng.integers(1, 30))).astype(np.int16)
        assert R.stats(r)[1] % 2 == 0


def test_every_code():
    arr = SC.every_code(OFF2)
    reads = _reads(arr, OFF2)
    prof, _ = profiles.get_profile("dna-r9-prom")
    inf_pos = inf_neg = ties = 0
    for i, want in enumerate(SC.EVERY_CODE_STATS):
        r = reads[i]
        np.testing.assert_array_equal(np.sort(r[:65536]), np.arange(-32768, 32768))
        assert R.stats(r) == want, (i, R.stats(r), want)
        with np.errstate(over="ignore"):
            x = R.normalise(r, want[0], want[1], "medmad", 0.0, 1.0, 1.0).astype(np.float16)
        inf_pos += int(np.count_nonzero(np.isposinf(x[:65536])))
        inf_neg += int(np.count_nonzero(np.isneginf(x[:65536])))
        assert not np.isnan(x).any()
        two, one = SC.medmad_two_ways(np.arange(-32768, 32768).astype(np.int16), *want)
        differ = np.flatnonzero(two != one) - 32768
        if want == (0, 1480):
            assert len(differ) == 10 and {-16624, -8312, -4156, -2078, -1039} <= set(differ.tolist())
        if want == (1400, 300):
            assert len(differ) == 4
        ties += len(differ)
    # (v - med) / 0.7413 reaches 65520, where float16 rounds to infinity, 48 570.5 codes from the median: the 65 535 - 48 570 = 16 965
    # farthest codes of the read whose median sits at the other end of the range
    assert inf_neg == 16965 and inf_pos == 16965 and ties >= 14
    # picoamperes at range / 2^14: float16 subnormals; at range / 2^24 the smallest values round to +0 and -0
    offset = -237.4102
    for div, what in ((2.0 ** 14, "subnormal"), (2.0 ** 24, "zero")):
        x = R.bits(R.normalise(reads[0][:65536], 0, 0, "pa", offset, prof.range / div, prof.digitisation).astype(np.float16))
        mag = x & 0x7fff
        if what == "subnormal":
            assert np.count_nonzero((mag > 0) & (mag < 0x0400)) >= 4
        else:
            assert (x == 0x8000).any() and (x == 0).any()
