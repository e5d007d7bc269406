#!/usr/bin/env python3
"""Rate and accuracy of sqg_batch_align (include/sqg_align.h) on the shape of BASELINE.json configs[2]: K sampled 10-kb reads,
-x dna-r10-prom (k = 9), -t 1, certified, the rows sqg_batch_detect finds under the DNA preset.  First the candidates of
SQG_ALIGN_DEFAULT -- stay_pen, skip_pen in {0, 256, 1024, 4096}, cost_cap in {4096, 16384, 65536} --, each scored against the
detector's true_ev: the share of rows with al_ev == true_ev, with |al_ev - true_ev| <= 1, and the mean of al_edge.  Then, with the
best triple, wall-clock milliseconds around the blocking C calls on preallocated outputs (median of the timed calls after a warm-up
call), next to sqg_batch_detect making the same rows and to the batch's generation time (sqg_timing_t.total_ms):
  al_cost alone   k_evtab_scan (level_raw) and the forward pass without its trace
  al_edge alone   the forward pass with its trace, the traceback without the al_ev store
  all             all three outputs
Prints markdown (profiles/align.md).  --no-sweep: SQG_ALIGN_DEFAULT as it stands and the times alone (under tools/kstats.sh: the kernels'
own durations).  SQG_LIB=... runs a kernel build variant (tools/README.md).
usage: python tools/align_rate.py [reads_per_batch=32768] [timed_calls=3] [genome_mb=200] [--no-sweep]"""
import ctypes as C
import itertools
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (first: the HIP runtime torch brings is the one the library then uses)

torch.zeros(1, device="cuda")
import bench  # noqa: E402
from squigulator_amd import api, model, profiles  # noqa: E402

SWEEP = "--no-sweep" not in sys.argv
ARGS = [a for a in sys.argv[1:] if a != "--no-sweep"]
K = int(ARGS[0]) if len(ARGS) > 0 else 32768
REP = int(ARGS[1]) if len(ARGS) > 1 else 3
MB = float(ARGS[2]) if len(ARGS) > 2 else 200.0
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
DT_NAMES = ("sum", "dt_len", "true_ev")
dt = b.detect("dna", "pa", outputs=DT_NAMES)                # the rows, made once
NR = int(dt.n_rows)
off = np.ascontiguousarray(dt.det_off, np.int64)
rows = np.diff(off)
al = b.align(off, dt.sum, dt.dt_len, api.ALIGN_DEFAULT)     # the outputs, allocated once
aptr = {n: getattr(al, n).data_ptr() for n in api.ALIGN_OUTPUTS}
cin = api.CAlignIn(dt.sum.data_ptr(), dt.dt_len.data_ptr())
poff = off.ctypes.data_as(C.POINTER(C.c_int64))


def timed(call):
    ts = []
    for it in range(REP + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts[1:])), min(ts[1:]), max(ts[1:])


def align(names, triple):
    cfg = api.CAlignCfg(*triple)
    out = api.CAlignOut(*[aptr[n] if n in names else None for n in api.ALIGN_OUTPUTS])
    return lambda: gen._chk(gen.L.sqg_batch_align(gen.ctx, b.handle, C.byref(cfg), poff, C.byref(cin), C.byref(out)), "sqg_batch_align")


def detect():
    cfg = api.CDetectCfg(*api.DETECT_PRESETS["dna"], api.CHUNK_PA, 0)
    out = api.CDetectOut(*[getattr(dt, n).data_ptr() if n in DT_NAMES else None for n in api.DETECT_OUTPUTS])
    gen._chk(gen.L.sqg_batch_detect(gen.ctx, b.handle, C.byref(cfg), C.byref(out)), "sqg_batch_detect")


print(f"# sqg_batch_align on one MI355X: {K} sampled 10-kb reads (dna-r10-prom, -t 1, certified), rows of the DNA detect preset, N = {N:.4g} samples, "
      f"{NE:.4g} true events, {NR:.4g} detected rows ({NR / NE:.3f} per true event; {rows.min()} .. {rows.max()} rows per read), "
      f"library {os.path.basename(api.LOADED_PATH)}\n")


def score(triple):
    align(api.ALIGN_OUTPUTS, triple)()
    d = al.al_ev - dt.true_ev
    return float((d == 0).double().mean()), float((d.abs() <= 1).double().mean()), float(al.al_edge.double().mean()), float(al.al_cost.double().sum()) / NR


if SWEEP:
    print("## The candidates of SQG_ALIGN_DEFAULT\n")
    print("| stay_pen | skip_pen | cost_cap | al_ev == true_ev | abs(al_ev - true_ev) <= 1 | mean al_edge | mean al_cost per row |")
    print("|---|---|---|---|---|---|---|")
table = []
for triple in itertools.product((0, 256, 1024, 4096), (0, 256, 1024, 4096), (4096, 16384, 65536)) if SWEEP else [api.ALIGN_DEFAULT]:
    same, near, edge, cost = score(triple)
    table.append((same, triple, near, edge))
    if SWEEP:
        print(f"| {triple[0]} | {triple[1]} | {triple[2]} | {same:.6f} | {near:.6f} | {edge:.2f} | {cost:.1f} |")
best = max(table)
print(f"\n{'best' if SWEEP else 'SQG_ALIGN_DEFAULT'}: stay_pen {best[1][0]}, skip_pen {best[1][1]}, cost_cap {best[1][2]}: {best[0]:.6f} of the detected rows on their "
      f"true event, {best[2]:.6f} within one event, mean al_edge {best[3]:.2f}; SQG_ALIGN_DEFAULT of the binding: {api.ALIGN_DEFAULT}\n")
t_cost = timed(align(("al_cost",), best[1]))
t_edge = timed(align(("al_edge",), best[1]))
t_all = timed(align(api.ALIGN_OUTPUTS, best[1]))
t_det = timed(detect)
print("## Times\n")
print(f"generation of this batch (sqg_timing_t.total_ms): {gen_ms:.2f} ms; median of {REP} timed calls after one warm-up call, wall clock "
      f"around the blocking C call, outputs preallocated\n")
print("| call | ms (min, max) |")
print("|---|---|")
for name, t in (("sqg_batch_align: al_cost alone (level scan, forward pass without trace)", t_cost),
                ("sqg_batch_align: al_edge alone (forward pass with trace, traceback)", t_edge),
                ("sqg_batch_align: all three outputs", t_all),
                ("sqg_batch_detect: sum, dt_len, true_ev (the rows aligned here)", t_det)):
    print(f"| {name} | {t[0]:.3f} ({t[1]:.3f}, {t[2]:.3f}) |")
print(f"\nforward pass: {t_cost[0]:.3f} ms for {NR:.4g} rows = {NR / t_cost[0] / 1e6:.2f} Grows/s, {t_cost[0] * 1e3 / rows.max():.3f} us per row of the longest read "
      f"({rows.max()} rows) if that read alone bounded it")
print(f"trace and traceback = all - al_cost alone = {t_all[0] - t_cost[0]:.3f} ms: 20 B per row written and read back ({NR * 40 / 1e9:.1f} GB), 8 B per row of al_ev")
b.free()
gen.close()
