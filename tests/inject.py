"""Injected signals: run a batch for its geometry, overwrite its samples on the device, then ask the library for everything it
derives from them.

svb-zd (k_svb.h), the BLOW5 framing and Huffman coding (k_blow5.h, kh_huff.h) and the chunk kernels (k_chunks.h) are functions of an
int16 array and of nothing else the generator made.  Natural signal is all alike (213 ... 1315 on the committed fixtures, no negative
sample, no three-byte svb-zd value), so the arrays of signal_cases.py are put where the generator's samples were:

    gen, prof, flags, k = inject.context("exact1")
    b = inject.run_geometry(gen, inject.seqs_for(lengths, k))        # sig_off, dwells, reads: the run's own
    inject.inject(b, arr)                                              # arr: int16 [b.n_samples]
    enc, off = b.compress()                                            # ... and blow5_records(), write_batch(), chunks()

This is a TEST DEVICE, not API: sqg_result_t.d_signal is `const` in include/sqg.h and stays so; Batch.signal_tensor() hands out a
writable torch view of it (zero copy) because torch has no read-only tensors, and only this module writes through it.

The one trap: sqg_batch_blow5_records (and sqg_blow5_write_batch, which calls it) reuses the batch's earlier svb-zd encoding while
the context's compress_seq still matches the batch's (csrc/h_results.h, `b->compress_seq != c->compress_seq`).  After an injection
call compress() BEFORE any BLOW5 call; sqg_batch_compress itself always recomputes.

Read lengths are what the run gave.  Under SQ_IDEAL_TIME with dwell_std = 0 a read of m bases has exactly (m - k + 1) * (int)dwell_mean
samples, which is how the case tables get the lengths they need; they assert them, they do not hope for them.
"""
import numpy as np

from squigulator_amd import api, model, profiles

SEED = 42

# name -> (profile, extra flags, dwell_mean or None (the profile's dwells, drawn), dwell_std)
GEOMETRIES = {
    "exact1": ("dna-r9-prom", profiles.SQ_IDEAL_TIME, 1.0, 0.0),       # n = bases - k + 1
    "exact2": ("dna-r9-prom", profiles.SQ_IDEAL_TIME, 2.0, 0.0),       # n = 2 (bases - k + 1): always even
    "exact15": ("dna-r9-prom", profiles.SQ_IDEAL_TIME, 15.0, 0.0),     # n = 15 (bases - k + 1): few events under many samples, reads that start at odd samples too
    "drawn": ("dna-r9-prom", 0, None, None),                           # ordinary dwells (9 +- 4): the labels' event boundaries are irregular
}


def context(geometry, range_div=1.0, lib_path=None, mode=api.MODE_CERTIFIED):
    """-> (generator, profile, flags, k) of one of GEOMETRIES; range_div: the profile's range divided by it (picoampere scale of chunks)"""
    name, extra, dmean, dstd = GEOMETRIES[geometry]
    prof, fl = profiles.get_profile(name)
    if dmean is not None:
        prof = prof.replace(dwell_mean=dmean, dwell_std=dstd)
    if range_div != 1.0:
        prof = prof.replace(range=prof.range / range_div)
    fl |= extra
    k = profiles.default_kmer_size(fl)
    mean, stdv = model.synthetic_model(k)
    gen = api.SignalGenerator(prof, fl, k, mean, stdv, SEED, num_workers=1, mode=mode, lib_path=lib_path)
    return gen, prof, fl, k


def seqs_for(n_bases, seed=3):
    """random reads of the given numbers of bases"""
    rng = np.random.default_rng(seed)
    return [bytes(rng.choice(list(b"ACGT"), int(m)).astype(np.uint8)) for m in n_bases]


def bases_for(n_samples, k, dwell=1):
    """bases of a read that has n_samples samples under SQ_IDEAL_TIME with that constant dwell"""
    out = []
    for n in n_samples:
        assert n > 0 and n % dwell == 0, (n, dwell)
        out.append(n // dwell + k - 1)
    return out


def run_geometry(gen, seqs):
    """a batch of the given reads (list of bytes), run and waited for: its sig_off / ev_off / dwells are the geometry the injected samples
    live in.  Reads only: a batch sampled from a genome (gen.sample(n)) works the same way, but no case here needs one"""
    return gen.stage(seqs).run().wait()


def inject(batch, arr):
    """overwrite the batch's samples on the device with arr (int16, len == batch.n_samples) and prove it: a test that failed to inject
    must not be able to pass"""
    import torch
    arr = np.ascontiguousarray(arr)
    assert arr.dtype == np.int16 and arr.ndim == 1 and len(arr) == batch.n_samples, (arr.dtype, arr.shape, batch.n_samples)
    t = batch.signal_tensor()
    assert t.data_ptr() == batch.res.d_signal and t.numel() == len(arr)
    t.copy_(torch.from_numpy(arr))
    torch.cuda.synchronize(t.device)                        # (the library works on streams of its own)
    del t
    np.testing.assert_array_equal(batch.signal(), arr, err_msg="the injected samples did not arrive")
    return batch


def read_ids(n):
    """ids of 1, 15, 16, 17 and 4096 bytes among ordinary ones: the record head's end moves across the 16-byte steps of the coders"""
    ids = [b"S1_%d!c!0!1!+" % (i + 1) for i in range(n)]
    for i, m in zip((0, 1, 2, 3, n - 1, n // 2), (1, 15, 16, 17, 4096, 4096)):
        ids[i] = bytes(65 + (i + j) % 26 for j in range(m))
    return ids


def host_blow5(path, prof, flags, ids, offset, median, sig_off, arr, lib_path=None, **mode):
    """the reference side of a BLOW5 comparison: the HOST writer (sqg_blow5_write) fed with the ORACLE's svb-zd encodings of arr --
    never with the device's compress() output, or an svb-zd error would cancel out.  lib_path: the library whose host writer is used (the
    CPU backend has the same one).  -> (file bytes, header size)"""
    import struct
    import orc
    encs = [orc.svb_zd(arr[sig_off[i]:sig_off[i + 1]]) for i in range(len(ids))]
    eo = np.concatenate(([0], np.cumsum([len(e) for e in encs]))).astype(np.int64)
    w = api.Blow5Writer(path, prof, flags, threads=4, lib_path=lib_path, **mode)
    w.write(ids, offset, median, sig_off, np.concatenate(encs), eo)
    w.close()
    buf = open(path, "rb").read()
    return buf, struct.unpack_from("<I", buf, 64)[0]
