#!/usr/bin/env python3
"""Rate of sqg_batch_events (include/sqg_events.h) on the shape of BASELINE.json configs[2]: K sampled 10-kb reads, -x dna-r10-prom
(k = 9), -t 1, certified.  Wall-clock milliseconds around the blocking C calls on preallocated outputs (median of the timed calls after
a warm-up call), next to the batch's generation time (sqg_timing_t.total_ms):
  scan     ev_read, ev_start, ev_len, kmer, level_raw, seg alone: k_evtab_scan writing every column it has
  places   ev_read, ev_start alone: k_evtab_scan writing what the reduce pass needs
  cheap    ev_read, ev_start, ev_len, seg: the scan without the k-mer ranks and the pore-table look-ups
  stats    med2, mad4 alone: the statistics pass of k_chunks.h (k_chunk_stats), which reads the same samples once
  sums     sum, sumsq, vmin, vmax, mean, sd (PA) with ev_read, ev_start: places + k_evtab_reduce; the reduce pass is sums - places
  all      every output, PA and MEDMAD (MEDMAD adds the statistics pass)
and the bytes the two passes move per event.  Prints markdown (profiles/events.md).  SQG_LIB=... runs a kernel build variant
(tools/README.md).
usage: python tools/events_rate.py [reads_per_batch=32768] [timed_calls=7] [genome_mb=200]"""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (first: the HIP runtime torch brings is the one the library then uses)

torch.zeros(1, device="cuda")
import bench  # noqa: E402
from squigulator_amd import api, model, profiles  # noqa: E402

K = int(sys.argv[1]) if len(sys.argv) > 1 else 32768
REP = int(sys.argv[2]) if len(sys.argv) > 2 else 7
MB = float(sys.argv[3]) if len(sys.argv) > 3 else 200.0
dev = torch.device("cuda", 0)
prof, fl = profiles.get_profile("dna-r10-prom")
k = 9
mean, stdv = model.synthetic_model(k)
seq, lens = bench.synthetic_genome_device(MB, dev)
gen = api.SignalGenerator(prof, fl, k, mean, stdv, 42, num_workers=1, mode=api.MODE_CERTIFIED)
gen.load_genome_device(seq.data_ptr(), lens, 10000, api.SAMPLE_DNA)
workers = np.zeros(K, np.int32)
for _ in range(2):                                          # warm-up batches (allocation, placement calibration starts)
    gen.sample(K, workers).run().wait().free()
b = gen.sample(K, workers).run().wait()
gen_ms = gen.timing()["total_ms"]
N, NE = int(b.n_samples), int(b.n_events)
store = gen.probe_store_bandwidth(1 << 30, 10)
ev = b.events("pa")                                         # the outputs, allocated once
ptr = {n: getattr(ev, n).data_ptr() for n in api.EVENT_OUTPUTS}
long_events = int((ev.ev_len > 64).sum())
longest = int(ev.ev_len.max())


def timed(call):
    ts = []
    for it in range(REP + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts[1:])), min(ts[1:]), max(ts[1:])


def events(names, norm=api.CHUNK_PA):
    cfg = api.CEventCfg(norm, 0)
    out = api.CEventOut(*[ptr[n] if n in names else None for n in api.EVENT_OUTPUTS])
    return lambda: gen._chk(gen.L.sqg_batch_events(gen.ctx, b.handle, C.byref(cfg), C.byref(out)), "sqg_batch_events")


PLACES = ("ev_read", "ev_start")
SUMS = ("sum", "sumsq", "vmin", "vmax", "mean", "sd")
scan = timed(events(PLACES + ("ev_len", "kmer", "level_raw", "seg")))
places = timed(events(PLACES))
cheap = timed(events(PLACES + ("ev_len", "seg")))
stats = timed(events(("med2", "mad4")))
sums = timed(events(PLACES + SUMS))
all_pa = timed(events(api.EVENT_OUTPUTS[:-2]))
all_medmad = timed(events(api.EVENT_OUTPUTS, api.CHUNK_MEDMAD))
reduce_ms = sums[0] - places[0]
scan_b = (2 + 1, 4 + 8 + 4 + 4 + 2 + 1)                     # read: dwell, base; written: ev_read, ev_start, ev_len, kmer, level_raw, seg
red_b = (2 * N / NE + 8 + 4 + 2, 8 + 8 + 2 + 2 + 4 + 4)     # read: the samples, ev_start, ev_read, dwell; written: sum, sumsq, vmin, vmax, mean, sd
print(f"# sqg_batch_events on one MI355X: {K} sampled 10-kb reads (dna-r10-prom, -t 1, certified), N = {N:.4g} samples, "
      f"{NE:.4g} events ({N / NE:.2f} samples per event; {long_events} longer than 64 samples, the longest {longest}), library {os.path.basename(api.LOADED_PATH)}\n")
print(f"generation of this batch (sqg_timing_t.total_ms): {gen_ms:.2f} ms; streaming-store probe: {store / 1e12:.2f} TB/s; "
      f"median of {REP} timed calls after one warm-up call, wall clock around the blocking C call, outputs preallocated\n")
print("| call | ms (min, max) | generation ms |")
print("|---|---|---|")
for name, t in (("scan: ev_read, ev_start, ev_len, kmer, level_raw, seg alone", scan), ("places: ev_read, ev_start alone", places), ("cheap: ev_read, ev_start, ev_len, seg alone", cheap),
                ("stats: med2, mad4 alone (k_chunk_stats)", stats), ("sums: sum, sumsq, vmin, vmax, mean, sd with ev_read, ev_start, PA (places + reduce)", sums),
                ("all twelve per-event outputs, PA", all_pa), ("all fourteen outputs, MEDMAD", all_medmad)):
    print(f"| {name} | {t[0]:.3f} ({t[1]:.3f}, {t[2]:.3f}) | {gen_ms:.2f} |")
print(f"\nscan pass: {scan[0]:.3f} ms; {scan_b[0]} B read + {scan_b[1]} B written per event = {NE * sum(scan_b) / 1e9:.2f} GB, {NE * sum(scan_b) / scan[0] / 1e6:.0f} GB/s")
print(f"reduce pass = sums - places = {reduce_ms:.3f} ms; {red_b[0]:.1f} B read + {red_b[1]} B written per event = {NE * sum(red_b) / 1e9:.2f} GB, "
      f"{NE * sum(red_b) / reduce_ms / 1e6:.0f} GB/s, {NE * sum(red_b) / (reduce_ms * 1e-3) / store:.2f} of the store probe; "
      f"k_chunk_stats over the same samples: {stats[0]:.3f} ms ({reduce_ms / stats[0]:.2f} x)")
b.free()
gen.close()
