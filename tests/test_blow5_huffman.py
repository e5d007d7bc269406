"""SQG_BLOW5_HUFFMAN (include/sqg.h, squigulator_amd/csrc/kh_huff.h): the BLOW5 writer's records in zlib streams of two dynamic-Huffman
blocks -- block A the head, the svb-zd count and the key bytes, block B (final) the data bytes and the trailer.

CPU: the host encoder (sqg_blow5_write) against the reference's files (tests/golden/blow5): the same header, the same records once
inflated, every stream parsed here bit by bit (78 01, two BTYPE-10 blocks split where the format says, code lengths within deflate's
limits, Adler-32), and about as small as the reference's zlib.  GPU: the records coded on the device (k_blow5_huff_size / _encode)
are the host encoder's bytes."""
import heapq
import os
import struct
import zlib

import numpy as np
import pytest

import orc
from blow5_cases import BLOW5_CASES
from squigulator_amd import api, build, model, profiles
from test_blow5 import DUMP, GOLD, INPUTS, _case, parse_blow5, ref_dump

CPU_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "libsqg_cpu.so")
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


# ---- a deflate reader for exactly this format ------------------------------------------------------------------------------------
class _Bits:
    def __init__(self, b):
        self.b, self.p = bytes(b) + b"\0" * 8, 0

    def get(self, n):
        q = self.p >> 3
        v = (int.from_bytes(self.b[q:q + 4], "little") >> (self.p & 7)) & ((1 << n) - 1)
        self.p += n
        return v


def _decoder(lens):
    """canonical Huffman code of `lens` (RFC 1951 3.2.2) -> (table indexed by the next maxlen bits, maxlen); the code must be complete"""
    m = max(lens)
    assert sum(2.0 ** -l for l in lens if l) == 1.0, "incomplete or over-subscribed code"
    count = [0] * (m + 1)
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, c = [0] * (m + 2), 0
    for b in range(1, m + 1):
        c = (c + count[b - 1]) << 1
        nxt[b] = c
    table = [None] * (1 << m)
    for s, l in enumerate(lens):
        if l:
            code = nxt[l]
            nxt[l] += 1
            rev = int(format(code, "0%db" % l)[::-1], 2)
            table[rev::1 << l] = [(s, l)] * (1 << (m - l))
    return table, m


def _sym(bits, dec):
    table, m = dec
    q = bits.p >> 3
    v = (int.from_bytes(bits.b[q:q + 4], "little") >> (bits.p & 7)) & ((1 << m) - 1)
    s, l = table[v]
    bits.p += l
    return s


def _block(bits, want_final):
    """one BTYPE-10 block, literals only: -> (bytes, literal code lengths)"""
    assert bits.get(1) == want_final and bits.get(2) == 2
    hlit, hdist, hclen = bits.get(5), bits.get(5), bits.get(4)
    assert hlit == 0 and hdist == 1                     # 257 literal/length codes, two distance codes
    cl = [0] * 19
    for j in range(hclen + 4):
        cl[CL_ORDER[j]] = bits.get(3)
    assert max(cl) <= 7
    cdec = _decoder(cl)
    lens = []
    while len(lens) < 259:
        s = _sym(bits, cdec)
        if s < 16:
            lens.append(s)
        elif s == 16:
            lens += [lens[-1]] * (3 + bits.get(2))
        elif s == 17:
            lens += [0] * (3 + bits.get(3))
        else:
            lens += [0] * (11 + bits.get(7))
    assert len(lens) == 259 and lens[257:] == [1, 1]
    lit = lens[:257]
    assert max(lit) <= 15 and lit[256] > 0
    dec = _decoder(lit)
    out = bytearray()
    while True:
        s = _sym(bits, dec)
        if s == 256:
            return bytes(out), lit
        assert s < 256                                   # literals only: no length codes
        out.append(s)


def cut_of(raw):
    """where block A ends in a raw record: head + svb-zd count + key bytes"""
    (idl,) = struct.unpack_from("<H", raw, 0)
    h = 2 + idl + 4 + 32 + 8
    (S,) = struct.unpack_from("<Q", raw, h - 8)
    if S < 4:
        return h + S
    (cnt,) = struct.unpack_from("<I", raw, h)
    return h + min(S, 4 + (cnt + 3) // 4)


def parse_record(z):
    """78 01 | block A | final block B | Adler-32, nothing else -> (raw record, lengths of A, lengths of B)"""
    assert z[:2] == b"\x78\x01"
    bits = _Bits(z[2:])
    a, la = _block(bits, 0)
    b, lb = _block(bits, 1)
    end = (bits.p + 7) // 8
    assert bits.p == end * 8 or (z[2 + end - 1] >> (bits.p & 7)) == 0      # zero padding up to the byte
    assert 2 + end + 4 == len(z)
    raw = a + b
    assert struct.unpack(">I", z[-4:])[0] == zlib.adler32(raw)
    assert len(a) == cut_of(raw)
    assert zlib.decompress(z) == raw
    return raw, la, lb


def huffman_records(buf):
    """every record of a BLOW5 file parsed as above -> [(raw, lengths A, lengths B)]"""
    hs = struct.unpack_from("<I", buf, 64)[0]
    p, out = 68 + hs, []
    while buf[p:] != b"5WOLB":
        (n,) = struct.unpack_from("<Q", buf, p)
        out.append(parse_record(buf[p + 8:p + 8 + n]))
        p += 8 + n
    return out


def huffman_depth(counts):
    """the deepest leaf of an unlimited Huffman code over the nonzero counts"""
    h = [(c, 0) for c in counts if c]
    heapq.heapify(h)
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        heapq.heappush(h, (a[0] + b[0], max(a[1], b[1]) + 1))
    return h[0][1]


def _write_case(cid, path, threads, lib_path=None, **mode):
    o, ids, offset, median, so, sig = _case(cid)
    encs = [orc.svb_zd(sig[so[i]:so[i + 1]]) for i in range(len(ids))]
    w = api.Blow5Writer(path, o.profile, o.flags, threads=threads, lib_path=lib_path, **mode)
    done = 0
    while done < len(ids):
        nb = min(o.batch, len(ids) - done)
        e = encs[done:done + nb]
        eo = np.concatenate(([0], np.cumsum([len(x) for x in e]))).astype(np.int64)
        w.write(ids[done:done + nb], offset[done:done + nb], median[done:done + nb], so[done:done + nb + 1] - so[done], np.concatenate(e), eo)
        done += nb
    return w, w.close()


# ---- 1. the golden cases ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c[0] for c in BLOW5_CASES])
@pytest.mark.parametrize("threads", [1, 3])
def test_huffman_mode_holds_the_reference_records(cid, threads, tmp_path):
    """host encoder: the reference file's header and records (inflated), valid two-block streams, the reference's slow5lib reads it to
    the same text, and the file is at most 3 % larger than the reference's zlib file and at least 22 % smaller than the stored-block one"""
    gold = os.path.join(GOLD, cid + ".blow5")
    path, ps = str(tmp_path / "h.blow5"), str(tmp_path / "s.blow5")
    _, n = _write_case(cid, path, threads, huffman=True)
    _, ns = _write_case(cid, ps, threads, stored=True)
    got = open(path, "rb").read()
    assert n == len(got)
    assert parse_blow5(got) == parse_blow5(open(gold, "rb").read())
    recs = huffman_records(got)
    assert [r[0] for r in recs] == parse_blow5(got)[1]
    d = ref_dump(path)
    if d is not None:
        assert d == ref_dump(gold)
    assert n <= 1.03 * os.path.getsize(gold) and n <= 0.78 * ns, (n, os.path.getsize(gold), ns)


def test_records_continue_over_batches(tmp_path):
    """r9_two_batches (-K 3): read_number and start_time carry over the writer's calls in the Huffman mode as in the others"""
    path = str(tmp_path / "h.blow5")
    _write_case("r9_two_batches", path, 2, huffman=True)
    o, ids, offset, median, so, sig = _case("r9_two_batches")
    recs = [r[0] for r in huffman_records(open(path, "rb").read())]
    assert len(recs) == len(ids) > o.batch
    for i, r in enumerate(recs):
        (idl,) = struct.unpack_from("<H", r, 0)
        q = 2 + idl + 4 + 32
        (nb,) = struct.unpack_from("<Q", r, q)
        _, rn, _, st = struct.unpack_from("<diBQ", r, q + 8 + nb + 9)
        assert (rn, st) == (i, int(so[i]))


# ---- 2. degenerate inputs --------------------------------------------------------------------------------------------------------
def _fib_svb():
    """an svb-zd field of count 0 (block B: these bytes + the trailer) whose block B counts are 1, 1, 2, 3, 5, ... 6765: end of block and
    the trailer's 0x01 the two 1s, the trailer's 0x30 and 0x00 (28 of them with a median of 0) topped up to 2 and 34 -- an unlimited Huffman
    code for it is 19 bits deep"""
    f = [1, 1]
    while len(f) < 20:
        f.append(f[-1] + f[-2])
    own = {0x30: 1, 0x00: 34 - 28}                       # what the data adds to the trailer's bytes
    syms = iter(range(0x80, 0x100))
    data = bytes([0x30]) * own[0x30]
    for c in f[3:]:
        data += bytes([0x00]) * own[0x00] if c == 34 else bytes([next(syms)]) * c
    return np.frombuffer(b"\0\0\0\0" + data, np.uint8)


def _degenerate_cases():
    rng = np.random.default_rng(11)
    sigs = {
        "one_sample": [np.array([517], np.int16)],
        "all_equal": [np.full(40000, 600, np.int16)],
        "uniform_random": [rng.integers(-32768, 32768, 120000).astype(np.int16)],
        "long_records": [np.cumsum(rng.integers(-40, 41, m)).astype(np.int16) + 500 for m in (70000, 300000)],
    }
    cases = {k: ([b"r%d" % i for i in range(len(v))], [orc.svb_zd(x) for x in v]) for k, v in sigs.items()}
    walk = (np.cumsum(rng.integers(-6, 7, 3000)) + 450).astype(np.int16)
    cases["id_lengths"] = ([b"a", b"L" * 65535, b"m" * 4097], [orc.svb_zd(walk)] * 3)
    cases["fibonacci"] = ([b"fib"], [_fib_svb()])
    return cases


@pytest.mark.parametrize("case", ["one_sample", "all_equal", "uniform_random", "long_records", "id_lengths", "fibonacci"])
def test_degenerate_records(case, tmp_path):
    """round trip through any inflate, code lengths within deflate's limits, the stored-mode records; incompressible data costs at most
    1 % + 300 B over stored blocks"""
    ids, encs = _degenerate_cases()[case]
    prof, fl = profiles.get_profile("dna-r9-prom")
    n = len(ids)
    lens = np.array([struct.unpack_from("<I", e.tobytes(), 0)[0] for e in encs], np.int64)
    so = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    eo = np.concatenate(([0], np.cumsum([len(x) for x in encs]))).astype(np.int64)
    out = {}
    for mode in ("huffman", "stored"):
        path = str(tmp_path / (mode + ".blow5"))
        w = api.Blow5Writer(path, prof, fl, threads=2, **{mode: True})
        w.write(ids, np.linspace(1, 2, n), np.zeros(n), so, np.concatenate(encs), eo)
        out[mode] = (w.close(), open(path, "rb").read())
    recs = huffman_records(out["huffman"][1])
    assert [r[0] for r in recs] == parse_blow5(out["stored"][1])[1]
    for raw, la, lb in recs:
        assert max(la) <= 15 and max(lb) <= 15
    if case == "fibonacci":
        raw, _, lb = recs[0]
        counts = np.bincount(np.frombuffer(raw[cut_of(raw):], np.uint8), minlength=256).tolist() + [1]
        assert huffman_depth(counts) > 15 and max(lb) == 15             # the limiter had work to do
    if case == "uniform_random":
        assert out["huffman"][0] <= 1.01 * out["stored"][0] + 300
    d = ref_dump(str(tmp_path / "huffman.blow5"), "hash")
    assert d is None or d.strip().endswith("records\t%d" % n)


def test_length_cap_of_the_development_build(tmp_path, monkeypatch):
    """SQG_TEST_B5_MAXBITS=9 (development build only): the golden records through a 9-bit limit -- still valid, and limited"""
    monkeypatch.setenv("SQG_TEST_B5_MAXBITS", "9")
    path = str(tmp_path / "h9.blow5")
    _write_case("r10_t1", path, 2, lib_path=build.LIB_DEV, huffman=True)
    got = open(path, "rb").read()
    assert parse_blow5(got) == parse_blow5(open(os.path.join(GOLD, "r10_t1.blow5"), "rb").read())
    recs = huffman_records(got)
    assert max(max(la + lb) for _, la, lb in recs) == 9
    raw = recs[0][0]
    counts = np.bincount(np.frombuffer(raw[cut_of(raw):], np.uint8), minlength=256).tolist() + [1]
    assert huffman_depth(counts) > 9


# ---- 3. flags and several files --------------------------------------------------------------------------------------------------
def test_stored_and_huffman_together_are_rejected(tmp_path):
    prof, fl = profiles.get_profile("dna-r9-prom")
    with pytest.raises(api.SqgError):
        api.Blow5Writer(str(tmp_path / "x.blow5"), prof, fl, stored=True, huffman=True)
    assert not os.path.exists(tmp_path / "x.blow5")


def _records_in_order(paths, parse):
    hdrs, recs = [], []
    for pth in paths:
        h, r = parse_blow5(open(pth, "rb").read())
        hdrs.append(h)
        recs += r
        if parse:
            huffman_records(open(pth, "rb").read())
    assert all(h == hdrs[0] for h in hdrs)

    def read_number(rec):
        (idl,) = struct.unpack_from("<H", rec, 0)
        q = 2 + idl + 4 + 32
        (nb,) = struct.unpack_from("<Q", rec, q)
        return struct.unpack_from("<i", rec, q + 8 + nb + 9 + 8)[0]
    return hdrs[0], sorted(recs, key=read_number)


@pytest.mark.parametrize("cid", ["r9_t1", "r9_two_batches", "r9_ont"])
@pytest.mark.parametrize("shards", [2, 3])
def test_sharded_huffman_files(cid, shards, tmp_path):
    """SQG_BLOW5_HUFFMAN | SQG_BLOW5_SHARDS(n): n files whose records are the stored-mode shards' (and the reference file's)"""
    wh, nh = _write_case(cid, str(tmp_path / "h.blow5"), 2, huffman=True, shards=shards)
    ws, _ = _write_case(cid, str(tmp_path / "s.blow5"), 2, stored=True, shards=shards)
    assert nh == sum(os.path.getsize(q) for q in wh.paths)
    for qh, qs in zip(wh.paths, ws.paths):
        assert parse_blow5(open(qh, "rb").read()) == parse_blow5(open(qs, "rb").read())
    hdr, recs = _records_in_order(wh.paths, parse=True)
    assert (hdr, recs) == parse_blow5(open(os.path.join(GOLD, cid + ".blow5"), "rb").read())
    if os.path.exists(DUMP):
        assert sum(int(ref_dump(q, "hash").strip().splitlines()[-1].split("\t")[1]) for q in wh.paths) == len(recs)


# ---- 4. the CPU backend ----------------------------------------------------------------------------------------------------------
def test_cpu_backend_batch_records(tmp_path):
    """oracle/libsqg_cpu.so's sqg_batch_blow5_records with the flag (its framing is h_blow5.h's) == the host writer's bytes"""
    import bench
    prof, fl = profiles.get_profile("dna-r10-prom")
    mean, stdv = model.synthetic_model(9)
    gen = api.SignalGenerator(prof, fl, 9, mean, stdv, 42, num_workers=2, mode=api.MODE_CERTIFIED, lib_path=CPU_LIB)
    gen.load_genome(bench.synthetic_genome_host(1.0), 1500, api.SAMPLE_DNA)
    b = gen.sample(7).run().wait()
    ids = [b"S1_%d" % i for i in range(b.n_reads)]
    mflags = (fl & (profiles.SQ_RNA | profiles.SQ_R10 | profiles.SQ_ONT)) | api.BLOW5_HUFFMAN
    recs, ro = b.blow5_records(prof, mflags, ids)
    enc, eo = b.compress()
    path = str(tmp_path / "h.blow5")
    w = api.Blow5Writer(path, prof, fl, threads=3, huffman=True)
    w.write(ids, b.offset, b.median_before, b.sig_off, enc, eo)
    w.close()
    host = open(path, "rb").read()
    hs = struct.unpack_from("<I", host, 64)[0]
    assert recs == host[68 + hs:-5] and ro[-1] == len(recs)
    assert len(huffman_records(host)) == b.n_reads
    b.free()
    gen.close()


# ---- 5-8. the device's records -----------------------------------------------------------------------------------------------------
def _device_and_host(cid, tmp_path, lib_path=None):
    o, ids, offset, median, so, sig = _case(cid)
    import bench
    contigs = bench.load_contigs(os.path.join(INPUTS, o.ref))
    k = o.kmer_size_default
    mean, stdv = model.synthetic_model(k)
    gen = api.SignalGenerator(o.profile, o.flags, k, mean, stdv, o.seed, num_workers=o.threads, mode=api.MODE_CERTIFIED, lib_path=lib_path)
    gen.load_genome(contigs, o.rlen, api.SAMPLE_RNA if (o.flags & profiles.SQ_RNA) else api.SAMPLE_DNA)
    p_dev, p_host = str(tmp_path / "dev.blow5"), str(tmp_path / "host.blow5")
    w = api.Blow5Writer(p_dev, o.profile, o.flags, threads=2, huffman=True, lib_path=lib_path)
    wh = api.Blow5Writer(p_host, o.profile, o.flags, threads=1, huffman=True, lib_path=lib_path)
    done = 0
    while done < len(ids):
        nb = min(o.batch, len(ids) - done)
        b = gen.sample(nb).run().wait()
        w.write_batch(b, ids[done:done + nb])
        enc, eo = b.compress()
        wh.write(ids[done:done + nb], b.offset, b.median_before, b.sig_off, enc, eo)
        b.free()
        done += nb
    w.close(); wh.close()
    gen.close()
    return p_dev, open(p_dev, "rb").read(), open(p_host, "rb").read()


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ["r9_t1", "r10_t1", "rna004_prefix", "r9_two_batches", "r9_ont"])
def test_device_huffman_records_equal_the_host_encoder(cid, tmp_path):
    """fixture reads -> kernels -> svb-zd -> k_blow5_huff_size / _encode -> file: the host encoder's bytes, the reference's records"""
    p_dev, dev, host = _device_and_host(cid, tmp_path)
    assert dev == host
    gold = os.path.join(GOLD, cid + ".blow5")
    assert parse_blow5(dev) == parse_blow5(open(gold, "rb").read())
    huffman_records(dev)
    d = ref_dump(p_dev)
    assert d is None or d == ref_dump(gold)


@pytest.mark.gpu
def test_device_huffman_records_under_a_lowered_length_cap(tmp_path, monkeypatch):
    """SQG_TEST_B5_MAXBITS=9 in the development build: natural records go through the length limiter on the device, the same bytes"""
    monkeypatch.setenv("SQG_TEST_B5_MAXBITS", "9")
    _, dev, host = _device_and_host("r10_t1", tmp_path, lib_path=build.LIB_DEV)
    assert dev == host
    assert max(max(la + lb) for _, la, lb in huffman_records(dev)) == 9


@pytest.mark.gpu
def test_device_huffman_of_a_bench_sized_batch(tmp_path):
    """2048 reads of 10 kb: the device's records are the host encoder's, decode to the batch's signals, within 2 % of zlib level 6 (on
    every 16th record: zlib in Python is slow) and at least 22 % smaller than stored blocks"""
    import bench
    prof, fl = profiles.get_profile("dna-r10-prom")
    mean, stdv = model.synthetic_model(9)
    gen = api.SignalGenerator(prof, fl, 9, mean, stdv, 42, num_workers=1, mode=api.MODE_CERTIFIED)
    gen.load_genome(bench.synthetic_genome_host(8.0), 10000, api.SAMPLE_DNA)
    b = gen.sample(2048).run().wait()
    ids = [b"S1_%d!c!0!1!+" % (i + 1) for i in range(b.n_reads)]
    mflags = (fl & (profiles.SQ_RNA | profiles.SQ_R10 | profiles.SQ_ONT)) | api.BLOW5_HUFFMAN
    recs, ro = b.blow5_records(prof, mflags, ids)
    enc, eo = b.compress()
    ph = str(tmp_path / "h.blow5")
    wh = api.Blow5Writer(ph, prof, fl, threads=8, huffman=True)
    wh.write(ids, b.offset, b.median_before, b.sig_off, enc, eo)
    wh.close()
    host = open(ph, "rb").read()
    hs = struct.unpack_from("<I", host, 64)[0]
    assert recs == host[68 + hs:-5] and ro[-1] == len(recs)
    sig = b.signal()
    raws = []
    for i in range(0, b.n_reads, 16):
        z = recs[ro[i] + 8:ro[i + 1]]
        raw = zlib.decompress(z)
        raws.append(raw)
        assert len(z) <= 1.02 * len(zlib.compress(raw, 6)) + 64
        (idl,) = struct.unpack_from("<H", raw, 0)
        q = 2 + idl + 4 + 32
        (nb,) = struct.unpack_from("<Q", raw, q)
        dec, used = orc.svb_zd_decode(np.frombuffer(raw, np.uint8, nb, q + 8))
        np.testing.assert_array_equal(dec, sig[b.sig_off[i]:b.sig_off[i + 1]])
    ours = sum(int(ro[i + 1] - ro[i]) - 8 for i in range(0, b.n_reads, 16))
    assert ours <= 1.02 * sum(len(zlib.compress(r, 6)) for r in raws)
    for i in (0, 1, b.n_reads - 1):
        parse_record(recs[ro[i] + 8:ro[i + 1]])
    stored = sum(8 + 2 + 5 * ((len(r) + 65534) // 65535) + len(r) + 4 for r in raws)
    assert sum(int(ro[i + 1] - ro[i]) for i in range(0, b.n_reads, 16)) <= 0.78 * stored
    b.free(); gen.close()


@pytest.mark.gpu
def test_device_huffman_on_four_files_and_the_host_fallback(tmp_path):
    """write_batch with SQG_BLOW5_SHARDS(4): four files that hold the one-file writer's records; a batch with a read id over 4096 bytes is
    coded on the host (the same bytes as the all-host file), and the writer outlives its context"""
    import bench
    prof, fl = profiles.get_profile("dna-r10-prom")
    mean, stdv = model.synthetic_model(9)
    gen = api.SignalGenerator(prof, fl, 9, mean, stdv, 42, num_workers=1, mode=api.MODE_CERTIFIED)
    gen.load_genome(bench.synthetic_genome_host(8.0), 4000, api.SAMPLE_DNA)
    w4 = api.Blow5Writer(str(tmp_path / "q.blow5"), prof, fl, huffman=True, shards=4)
    w1 = api.Blow5Writer(str(tmp_path / "one.blow5"), prof, fl, huffman=True)
    wh = api.Blow5Writer(str(tmp_path / "host.blow5"), prof, fl, threads=2, huffman=True)
    nread = 0
    for bi, n in enumerate((301, 64, 3)):
        b = gen.sample(n).run().wait()
        ids = [b"S1_%d!c!0!1!+" % (nread + i + 1) for i in range(n)]
        if bi == 1:
            ids[7] = b"L" * 5000                                      # > 4096: this batch is coded on the host
        w4.write_batch(b, ids); w1.write_batch(b, ids)
        enc, eo = b.compress()
        wh.write(ids, b.offset, b.median_before, b.sig_off, enc, eo)
        nread += n
        b.free()
    gen.close()                                                       # before the writers: their last background writes drain first
    n4, n1 = w4.close(), w1.close()
    wh.close()
    one = open(w1.paths[0], "rb").read()
    assert one == open(str(tmp_path / "host.blow5"), "rb").read() and n1 == len(one)
    assert len(huffman_records(one)) == nread
    hdr4, rec4 = _records_in_order(w4.paths, parse=False)
    assert (hdr4, rec4) == parse_blow5(one)
    assert n4 == n1 + 3 * (68 + len(hdr4) + 5)
