#!/usr/bin/env python3
"""Rate of sqg_detect_plan and sqg_batch_detect (include/sqg_detect.h) on the shape of BASELINE.json configs[2]: K sampled 10-kb reads,
-x dna-r10-prom (k = 9), -t 1, certified, the DNA preset.  Wall-clock milliseconds around the blocking C calls on preallocated outputs
(median of the timed calls after a warm-up call), next to the batch's generation time (sqg_timing_t.total_ms) and to sqg_batch_events
with all its per-event outputs on the same batch:
  plan        sqg_detect_plan: one walk of k_detect_walk (counting) and the copy-back of the per-read counts
  boundaries  sqg_batch_detect with dt_read, dt_start alone: the plan's walk and the walk that writes
  all         every per-row output, PA: the two walks, k_evtab_scan for true_ev, k_detect_rows
  all medmad  every output, MEDMAD (adds the statistics pass)
and the bytes a walk moves per sample, the detected-to-true row ratio and how the reads' lengths fill the lanes.  Prints markdown
(profiles/detect.md).  SQG_LIB=... runs a kernel build variant (tools/README.md).
usage: python tools/detect_rate.py [reads_per_batch=32768] [timed_calls=5] [genome_mb=200]"""
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
REP = int(sys.argv[2]) if len(sys.argv) > 2 else 5
MB = float(sys.argv[3]) if len(sys.argv) > 3 else 200.0
TILE, HALO = 256, 64                                        # k_detect.h: DET_T, DET_H
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
dt = b.detect("dna", "pa")                                  # the outputs, allocated once
NR = int(dt.n_rows)
ptr = {n: getattr(dt, n).data_ptr() for n in api.DETECT_OUTPUTS}
ev = b.events("pa")
eptr = {n: getattr(ev, n).data_ptr() for n in api.EVENT_OUTPUTS}
hit = int(torch.unique(dt.true_ev).numel())                 # true events with at least one detected row starting in them
exact = int(((ev.ev_start[dt.true_ev] == dt.dt_start) & (ev.ev_read[dt.true_ev] == dt.dt_read)).sum())
lengths = np.diff(b.sig_off)
waves = [lengths[i:i + 64] for i in range(0, K, 64)]
walked = sum(int(w.max()) * 64 for w in waves)              # lane-steps the wavefronts spend, idle lanes included


def timed(call):
    ts = []
    for it in range(REP + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts[1:])), min(ts[1:]), max(ts[1:])


def detect(names, norm=api.CHUNK_PA):
    cfg = api.CDetectCfg(*api.DETECT_PRESETS["dna"], norm, 0)
    out = api.CDetectOut(*[ptr[n] if n in names else None for n in api.DETECT_OUTPUTS])
    return lambda: gen._chk(gen.L.sqg_batch_detect(gen.ctx, b.handle, C.byref(cfg), C.byref(out)), "sqg_batch_detect")


def plan():
    cfg = api.CDetectCfg(*api.DETECT_PRESETS["dna"], api.CHUNK_PA, 0)
    nr = C.c_int64()
    gen._chk(gen.L.sqg_detect_plan(gen.ctx, b.handle, C.byref(cfg), None, C.byref(nr)), "sqg_detect_plan")


def events():
    cfg = api.CEventCfg(api.CHUNK_PA, 0)
    out = api.CEventOut(*[eptr[n] if n not in ("med2", "mad4") else None for n in api.EVENT_OUTPUTS])
    gen._chk(gen.L.sqg_batch_events(gen.ctx, b.handle, C.byref(cfg), C.byref(out)), "sqg_batch_events")


t_plan = timed(plan)
t_bound = timed(detect(("dt_read", "dt_start")))
t_all = timed(detect(api.DETECT_OUTPUTS[:-2]))
t_medmad = timed(detect(api.DETECT_OUTPUTS, api.CHUNK_MEDMAD))
t_events = timed(events)
walk_b = 2.0 * (TILE + 2 * HALO) / TILE                     # read per sample: the tile with its halo
print(f"# sqg_batch_detect on one MI355X: {K} sampled 10-kb reads (dna-r10-prom, -t 1, certified), the DNA preset, N = {N:.4g} samples, "
      f"{NE:.4g} true events, {NR:.4g} detected rows, library {os.path.basename(api.LOADED_PATH)}\n")
print(f"generation of this batch (sqg_timing_t.total_ms): {gen_ms:.2f} ms; median of {REP} timed calls after one warm-up call, wall clock "
      f"around the blocking C call, outputs preallocated\n")
print("| call | ms (min, max) | generation ms |")
print("|---|---|---|")
for name, t in (("sqg_detect_plan (one walk)", t_plan), ("sqg_batch_detect: dt_read, dt_start alone (two walks)", t_bound),
                ("sqg_batch_detect: all ten per-row outputs, PA", t_all), ("sqg_batch_detect: all twelve outputs, MEDMAD", t_medmad),
                ("sqg_batch_events: all twelve per-event outputs, PA", t_events)):
    print(f"| {name} | {t[0]:.3f} ({t[1]:.3f}, {t[2]:.3f}) | {gen_ms:.2f} |")
print(f"\none walk: {t_plan[0]:.3f} ms for {N:.4g} samples = {N / t_plan[0] / 1e6:.2f} Gsamples/s; {walk_b:.1f} B read per sample (int16 tiles of {TILE} with a halo of "
      f"{HALO} on either side) = {N * walk_b / t_plan[0] / 1e6:.0f} GB/s")
print(f"rows pass and true_ev = all - boundaries = {t_all[0] - t_bound[0]:.3f} ms for {NR:.4g} rows")
print(f"lanes: {K} reads in {len(waves)} wavefronts of one read per lane; the wavefronts walk {walked:.4g} lane-steps for {N:.4g} samples: "
      f"{N / walked:.3f} of the lanes' steps hold a sample (reads of {lengths.min()} .. {lengths.max()} samples)")
print(f"detected rows / true events: {NR / NE:.3f}; true events in which a detected row starts: {hit / NE:.3f}; detected rows that start exactly where a true event does: {exact / NR:.3f}")
b.free()
gen.close()
