#!/usr/bin/env python3
"""Rate of sqg_batch_chunks (include/sqg_chunks.h) on the headline workload's shape: K sampled 10-kb reads, -x dna-r10-prom, -t 1.
Per setting: the blocking call's wall-clock milliseconds (median of the timed calls, after a warm-up call), next to the same batch's
generation time (sqg_timing_t.total_ms), and the bytes the call must move (2 N + dtype_bytes L n_chunks + W n_chunks) over that time,
next to the streaming-store rate sqg_probe_store_bandwidth reports in the same run.  Prints a markdown table (profiles/chunks.md).
Then the same for sqg_batch_chunk_targets (include/sqg_targets.h) on the same batch: clean + moves, all four outputs, each with and
without the statistics of an earlier Batch.chunks passed in; bytes = what the call writes per sample (F16 clean 2, clean_raw 2, moves 1, kmer 4).  The milliseconds are the whole blocking
Batch.chunk_targets call (tensor allocation, plan and synchronisation included); per-kernel times come from running this tool under
tools/kstats.sh (profiles/chunk_targets.md).
--workload sequin-rna004: K whole sequin transcripts, -x rna004-prom --prefix=yes, -t 1 (BASELINE.json configs[4]; K defaults to 8192, a
step well under a second); --no-prefix: the same reads without the prefix.  --trim: the calls of include/sqg_segments.h (Batch.segments,
trim=True), the only chunk calls a --prefix=yes context takes; the table then starts with the blocking Batch.segments call
(profiles/segments.md).
usage: python tools/chunks_rate.py [reads_per_batch=32768] [timed_calls=5] [genome_mb] [--workload hg38-r10|sequin-rna004] [--no-prefix] [--trim]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (first: the HIP runtime torch brings is the one the library then uses)

torch.zeros(1, device="cuda")
import bench  # noqa: E402
from squigulator_amd import api, model, profiles  # noqa: E402

argv = [a for a in sys.argv[1:] if not a.startswith("--")]
TRIM, NO_PREFIX = "--trim" in sys.argv, "--no-prefix" in sys.argv
WORKLOAD = sys.argv[sys.argv.index("--workload") + 1] if "--workload" in sys.argv else "hg38-r10"
if WORKLOAD in argv:
    argv.remove(WORKLOAD)
if WORKLOAD not in ("hg38-r10", "sequin-rna004"):
    sys.exit(f"unknown workload {WORKLOAD}")
SEQUIN = WORKLOAD == "sequin-rna004"
K = int(argv[0]) if len(argv) > 0 else (8192 if SEQUIN else 32768)
REP = int(argv[1]) if len(argv) > 1 else 5
MB = float(argv[2]) if len(argv) > 2 else None
TR = dict(trim=True) if TRIM else {}
dev = torch.device("cuda", 0)
if SEQUIN:
    prof, fl = profiles.get_profile("rna004-prom")
    if not NO_PREFIX:
        fl |= profiles.SQ_PREFIX
    if (fl & profiles.SQ_PREFIX) and not TRIM:
        sys.exit("a --prefix=yes context takes the trimmed chunk calls only: add --trim (or --no-prefix)")
    mean, stdv = model.synthetic_model(9)
    gen = api.SignalGenerator(prof, fl, 9, mean, stdv, 42, num_workers=1, mode=api.MODE_CERTIFIED)
    gen.load_genome(bench.load_contigs(bench.SEQUINS), 10000, api.SAMPLE_RNA)
    what = f"{K} sampled sequin transcripts (rna004-prom{'' if NO_PREFIX else ', --prefix=yes'}, -t 1, certified)"
else:
    prof, fl = profiles.get_profile("dna-r10-prom")
    mean, stdv = model.synthetic_model(9)
    seq, lens = bench.synthetic_genome_device(MB, dev)
    gen = api.SignalGenerator(prof, fl, 9, mean, stdv, 42, num_workers=1, mode=api.MODE_CERTIFIED)
    gen.load_genome_device(seq.data_ptr(), lens, 10000, api.SAMPLE_DNA)
    what = f"{K} sampled 10-kb reads (dna-r10-prom, -t 1, certified)"
workers = np.zeros(K, np.int32)
for _ in range(2):                                          # warm-up batches (allocation, placement calibration starts)
    gen.sample(K, workers).run().wait().free()
b = gen.sample(K, workers).run().wait()
gen_ms = gen.timing()["total_ms"]
N = int(b.n_samples)
store = gen.probe_store_bandwidth(1 << 30, 10)
L, W = 4096, 512
print(f"# sqg_batch_chunks{'_trimmed' if TRIM else ''} on one MI355X: {what}, N = {N:.4g} samples\n")
print(f"generation of this batch (sqg_timing_t.total_ms): {gen_ms:.2f} ms; streaming-store probe: {store / 1e12:.2f} TB/s; "
      f"median of {REP} timed calls after one warm-up call, wall clock around the blocking call\n")
print("| setting | chunks | call ms | generation ms | bytes moved | GB/s | of the store probe |")
print("|---|---|---|---|---|---|---|")
if TRIM:                                                    # the segments call alone: one wavefront per read, under 600 B of dwells each
    ts = []
    for it in range(REP + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        seg, _ = b.segments()
        ts.append((time.perf_counter() - t0) * 1e3)
    N = int((seg[:, 4] - seg[:, 3]).sum())                  # what the trimmed calls read: the inserts
    print(f"| Batch.segments (seg + shift, 56 B per read out) | - | {float(np.median(ts[1:])):.3f} (min {min(ts[1:]):.3f}, max {max(ts[1:]):.3f}) | {gen_ms:.2f} | - | - | - |")
    print(f"| (the inserts hold {N:.4g} of the batch's {int(b.n_samples):.4g} samples) | | | | | | |")
    del seg
for name, S, kw in (("L 4096, S = L, f16 medmad, W 512", L, {}), ("L 4096, S = L/2, f16 medmad, W 512", L // 2, {}),
                    ("statistics pass alone (signal = labels = NULL)", L, dict(signal=False, labels=False)),
                    ("statistics + emit, S = L (labels = NULL)", L, dict(labels=False)),
                    ("statistics + labels, S = L (signal = NULL)", L, dict(signal=False))):
    ts = []
    for it in range(REP + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ch = b.chunks(L, S, W, **kw, **TR)
        ts.append((time.perf_counter() - t0) * 1e3)
        nc = ch.n_chunks
        del ch
    ms = float(np.median(ts[1:]))
    moved = 2 * N + (2 * L * nc if kw.get("signal", True) else 0) + (W * nc if kw.get("labels", True) else 0)
    print(f"| {name} | {nc} | {ms:.2f} (min {min(ts[1:]):.2f}, max {max(ts[1:]):.2f}) | {gen_ms:.2f} | {moved / 1e9:.2f} GB | {moved / ms / 1e6:.0f} | {moved / (ms * 1e-3) / store:.2f} |")

print(f"\n# sqg_batch_chunk_targets{'_trimmed' if TRIM else ''} on the same batch (L {L}, S = L, f16 medmad)\n")
print("| outputs | statistics | chunks | call ms | bytes written | GB/s | of the store probe |")
print("|---|---|---|---|---|---|---|")
stats = b.chunks(L, L, 0, signal=False, labels=False, **TR)
for name, per_sample, kw in (("clean + moves", 3, dict(clean=True, moves=True)), ("moves alone", 1, dict(clean=False, moves=True)),
                             ("clean_raw alone", 2, dict(clean=False, moves=False, clean_raw=True)),
                             ("clean, clean_raw, moves, kmer", 9, dict(clean=True, clean_raw=True, moves=True, kmer=True))):
    for how, extra in (("computed by the call", {}), ("passed in", dict(chunks=stats))):
        if not kw["clean"] and extra:
            continue                                        # no clean: no statistics either way
        ts = []
        for it in range(REP + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tg = b.chunk_targets(L, L, **kw, **extra, **TR)
            ts.append((time.perf_counter() - t0) * 1e3)
            nc = tg.n_chunks
            del tg
        ms = float(np.median(ts[1:]))
        wrote = per_sample * L * nc
        print(f"| {name} | {how if kw['clean'] else '-'} | {nc} | {ms:.2f} (min {min(ts[1:]):.2f}, max {max(ts[1:]):.2f}) | {wrote / 1e9:.2f} GB | "
              f"{wrote / ms / 1e6:.0f} | {wrote / (ms * 1e-3) / store:.2f} |")
del stats
b.free()
gen.close()
