#!/usr/bin/env python3
"""The BLOW5 writer's record compression modes on the headline workload (-x dna-r10-prom, 10 kb reads, -t 1): SQG_BLOW5_STORED against
SQG_BLOW5_HUFFMAN, into one file and into four (SQG_BLOW5_SHARDS(4)) of /dev/shm, timed as bench.py's e2e legs are (one host thread:
batch i+1 sampled and queued before batch i is written; the encoder first, the next batch's kernels behind it), `--reps` rounds of the
four legs, interleaved.  A zlib leg (the default mode: the reference's bytes, host deflate) on one small batch, for its size only, next to
the other two modes' sizes of the same batch.  Prints one JSON line.

    python tools/blow5_modes.py [--reads 8192] [--seconds 2] [--reps 3] [--genome-mb 64]
    tools/kstats.sh tools/blow5_modes.py --kernels     # per-batch time of k_blow5_frame against k_blow5_huff_size + k_blow5_huff_encode:
                                                       # --kernels frames --batches batches each way (sqg_batch_blow5_records), no files
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (first: the HIP runtime torch brings is the one the library then uses)

import bench  # noqa: E402
from squigulator_amd import api, model, profiles  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=8192, help="reads per batch (bench.py's e2e_fast_batch_reads)")
ap.add_argument("--seconds", type=float, default=2.0, help="per leg")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--genome-mb", type=float, default=64.0)
ap.add_argument("--zlib-reads", type=int, default=256, help="reads of the one batch the size comparison (zlib included) writes")
ap.add_argument("--kernels", action="store_true", help="only frame --batches batches each way, for tools/kstats.sh")
ap.add_argument("--batches", type=int, default=8)
args = ap.parse_args()

torch.zeros(1, device="cuda")
prof, fl = profiles.get_profile("dna-r10-prom")
mflags = fl & (profiles.SQ_RNA | profiles.SQ_R10 | profiles.SQ_ONT)
mean, stdv = model.synthetic_model(9)
seq, lens = bench.synthetic_genome_device(args.genome_mb, torch.device("cuda", 0))
gen = api.SignalGenerator(prof, fl, 9, mean, stdv, 42, num_workers=1, mode=api.MODE_CERTIFIED)
gen.load_genome_device(seq.data_ptr(), lens, 10000, api.SAMPLE_DNA)
workers = np.zeros(args.reads, np.int32)
ids = [b"S1_%d!c0!0!10000!+" % i for i in range(args.reads)]
shm = "/dev/shm" if os.path.isdir("/dev/shm") else "/tmp"

if args.kernels:
    for flags in (mflags | api.BLOW5_STORED, mflags | api.BLOW5_HUFFMAN):
        for _ in range(args.batches):
            b = gen.sample(args.reads, workers).run().wait()
            b.blow5_records(prof, flags, ids)
            b.free()
    gen.close()
    print(json.dumps({"kernels": True, "batches_per_mode": args.batches, "reads_per_batch": args.reads}))
    sys.exit(0)


def leg(mode, shards):
    """samples/s and bytes/sample of one timed leg (bench.py's e2e_legs loop)"""
    path = os.path.join(shm, f"sqg_modes_{os.getpid()}.blow5")
    w = api.Blow5Writer(path, prof, fl, threads=0, shards=shards, **{mode: True})
    paths = list(w.paths)
    samples = nb = 0
    try:
        cur = gen.sample(args.reads, workers).run()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        while True:
            last = nb >= 1 and time.perf_counter() - t0 >= args.seconds
            cur.compress(fetch=False)
            nxt = None if last else gen.sample(args.reads, workers).run()
            cur.wait()
            w.write_batch(cur, ids)
            samples += cur.n_samples; nb += 1
            cur.free()
            if nxt is None:
                break
            cur = nxt
        nbytes = w.close(); w = None
        dt = time.perf_counter() - t0
    finally:
        if w is not None:
            w.close()
        for q in paths:
            try:
                os.unlink(q)
            except OSError:
                pass
    return {"samples_per_s": samples / dt, "bytes_per_sample": nbytes / samples, "GBps": nbytes / dt / 1e9, "batches": nb}


legs = [("stored", 1), ("huffman", 1), ("stored", 4), ("huffman", 4)]
runs = {f"{m}_{s}file{'s' if s > 1 else ''}": [] for m, s in legs}
leg("huffman", 1)                                        # warm-up: buffers of both modes allocated, files system warm
for _ in range(args.reps):
    for m, s in legs:
        runs[f"{m}_{s}file{'s' if s > 1 else ''}"].append(leg(m, s))

# sizes of one batch in all three modes (zlib: host deflate, seconds per batch -- hence a small one)
b = gen.sample(args.zlib_reads, workers[:args.zlib_reads]).run().wait()
sizes = {}
for mode in ("zlib", "stored", "huffman"):
    path = os.path.join(shm, f"sqg_modes_{os.getpid()}_{mode}.blow5")
    w = api.Blow5Writer(path, prof, fl, threads=0, **({} if mode == "zlib" else {mode: True}))
    w.write_batch(b, ids[:b.n_reads])
    sizes[mode] = w.close() / b.n_samples
    os.unlink(path)
b.free()
gen.close()

out = {"workload": "dna-r10-prom, 10 kb reads, -t 1", "reads_per_batch": args.reads, "seconds_per_leg": args.seconds, "reps": args.reps,
       "bytes_per_sample_one_batch": sizes, "zlib_batch_reads": args.zlib_reads}
for k, v in runs.items():
    out[k] = {"samples_per_s_median": statistics.median(r["samples_per_s"] for r in v),
              "samples_per_s": [round(r["samples_per_s"], -6) for r in v],
              "bytes_per_sample": statistics.median(r["bytes_per_sample"] for r in v),
              "GBps_median": statistics.median(r["GBps"] for r in v), "batches": [r["batches"] for r in v]}
print(json.dumps(out))
