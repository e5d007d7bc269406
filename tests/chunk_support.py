"""What the chunk test modules share: the cases, a fixture's reads, a context for a case's command line, Chunks against chunks_ref bit for bit."""
import os
import re

import numpy as np

import chunks_ref as R
from refvec_cases import LIVE_CMD, LIVE_SEEDS, REFVEC_CASES
from squigulator_amd import api, model, options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(cid, cmd) for cid, cmd in REFVEC_CASES if "--prefix" not in cmd] + [(f"live_seed{s}", LIVE_CMD.format(seed=s)) for s in LIVE_SEEDS]
ALL_SETTINGS = [("f16", "medmad"), ("f32", "medmad"), ("f16", "pa"), ("f32", "pa")]


def _declared(header):
    hdr = open(os.path.join(ROOT, "include", header)).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return set(re.findall(r"\b(sqg_[a-z0-9_]+)\s*\(", hdr))


def _fixture_reads(cid):
    v = np.load(os.path.join(ROOT, "tests", "golden", "refvec", cid + ".npz"))
    meta = v["meta"]
    so = go = eo = 0
    out = []
    for i in range(len(meta)):
        rlen, nsig, nss = int(meta[i][4]), int(meta[i][7]), int(meta[i][8])
        out.append(dict(seq=v["seq"][so:so + rlen].tobytes(), sig=v["sig"][go:go + nsig], ss=v["ss"][eo:eo + nss], offset=float(v["offset"][i])))
        so += rlen; go += nsig; eo += nss
    return out


def _context(cmd, mode):
    o = options.parse_args(cmd)
    k = o.kmer_size_default
    mean, stdv = model.synthetic_model(k, meth=bool(o.meth_freq))
    gen = api.SignalGenerator(o.profile, o.flags, k, mean, stdv, o.seed, num_workers=o.threads, amp_noise=o.amp_noise, mode=mode)
    return o, k, gen


def _cpu(t):
    return None if t is None else t.cpu().numpy()


def _assert_equal(ch, want, what, keys=("signal", "labels", "label_len", "chunk_read", "chunk_start", "med2", "mad4")):
    assert ch.n_chunks == len(want["chunk_read"]), f"{what}: {ch.n_chunks} chunks, expected {len(want['chunk_read'])}"
    np.testing.assert_array_equal(ch.chunk_off, want["chunk_off"], err_msg=f"{what}: chunk_off")
    for key in keys:
        got = _cpu(getattr(ch, key))
        if got is None:
            continue
        assert got.shape == want[key].shape and got.dtype == want[key].dtype, f"{what}: {key} {got.shape} {got.dtype} vs {want[key].shape} {want[key].dtype}"
        np.testing.assert_array_equal(R.bits(got), R.bits(want[key]), err_msg=f"{what}: {key}")
