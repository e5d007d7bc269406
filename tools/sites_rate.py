#!/usr/bin/env python3
"""Rate of sqg_site_plan / sqg_batch_sites (include/sqg_sites.h) on the headline workload's shape with a methylation table set: K sampled
10-kb reads, -x dna-r10-prom (5-letter table, k = 9), -t 1, every CpG of a synthetic genome methylated at frequency 1/2.  L = 256,
before = 128, B = 21, f16 / MEDMAD.  Wall-clock milliseconds around the blocking C calls on preallocated outputs (median of the timed
calls after a warm-up call), next to the batch's generation time (sqg_timing_t.total_ms):
  plan    sqg_site_plan, its plan not in the scratch (two `before` values alternate): k_site_scan<0>, the copy-back, two synchronisations
  scan    sqg_batch_sites for label / site_read / site_pos / win_start alone, the plan in the scratch: k_site_scan<1>
  stats   sqg_batch_sites for med2 / mad4 alone: the statistics pass of k_chunks.h
  all     every output: stats + scan + k_site_emit; the emit is all - scan - stats
and the emit's bytes (2 L read + 2 L + B + 4 (B + 1) written per site) per second next to sqg_probe_store_bandwidth.  Prints markdown
(profiles/sites.md).  SQG_LIB=... runs a kernel build variant (tools/README.md).
usage: python tools/sites_rate.py [reads_per_batch=32768] [timed_calls=7] [genome_mb=200]"""
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
fl |= profiles.SQ_METH
k = 9
mean, stdv = model.synthetic_model(k, meth=True)
seq, lens = bench.synthetic_genome_device(MB, dev)
gen = api.SignalGenerator(prof, fl, k, mean, stdv, 42, num_workers=1, mode=api.MODE_CERTIFIED)
gen.load_genome_device(seq.data_ptr(), lens, 10000, api.SAMPLE_DNA)
cpg = torch.zeros_like(seq)
cpg[:-1] = ((seq[:-1] == ord("C")) & (seq[1:] == ord("G"))).to(torch.uint8) * 128     # frequency 128 / 255 on the C of every CpG
freq, has = cpg.cpu().numpy(), np.ones(len(lens), np.uint8)
gen._chk(gen.L.sqg_genome_set_meth(gen.ctx, freq.ctypes.data, has.ctypes.data), "sqg_genome_set_meth")
del cpg
workers = np.zeros(K, np.int32)
for _ in range(2):                                          # warm-up batches (allocation, placement calibration starts)
    gen.sample(K, workers).run().wait().free()
b = gen.sample(K, workers).run().wait()
gen_ms = gen.timing()["total_ms"]
N = int(b.n_samples)
store = gen.probe_store_bandwidth(1 << 30, 10)
L, BEFORE, B, CB, F = 256, 128, 21, 10, k // 2
st = b.sites(L, BEFORE, F, B, CB)                           # the outputs, allocated once
ns = st.n_sites
n1 = int(st.label.sum())
cfgs = [api.CSiteCfg(L, BEFORE - i, F, B, CB, api.CHUNK_F16, api.CHUNK_MEDMAD) for i in (0, 1)]
ptr = {n: getattr(st, n).data_ptr() for n in api.SITE_OUTPUTS}


def timed(call, before=None):
    ts = []
    for it in range(REP + 1):
        if before:
            before(it)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call(it)
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts[1:])), min(ts[1:]), max(ts[1:])


def sites(names):
    out = api.CSiteOut(*[ptr[n] if n in names else None for n in api.SITE_OUTPUTS])
    return lambda it: gen._chk(gen.L.sqg_batch_sites(gen.ctx, b.handle, C.byref(cfgs[0]), C.byref(out)), "sqg_batch_sites")


cnt = C.c_int64()
plan = timed(lambda it: gen._chk(gen.L.sqg_site_plan(gen.ctx, b.handle, C.byref(cfgs[it & 1]), None, C.byref(cnt)), "sqg_site_plan"))
gen._chk(gen.L.sqg_site_plan(gen.ctx, b.handle, C.byref(cfgs[0]), None, C.byref(cnt)), "sqg_site_plan")      # the plan of cfgs[0] into the scratch
assert cnt.value == ns
scan = timed(sites(("label", "site_read", "site_pos", "win_start")))
stats = timed(sites(("med2", "mad4")))
everything = timed(sites(api.SITE_OUTPUTS))
rows = timed(sites(("signal", "context", "ctx_start")))
emit_ms = everything[0] - scan[0] - stats[0]
moved = ns * (2 * L + 2 * L + B + 4 * (B + 1))
print(f"# sqg_site_plan / sqg_batch_sites on one MI355X: {K} sampled 10-kb reads (dna-r10-prom with the 5-letter table, -t 1, certified), "
      f"N = {N:.4g} samples, library {os.path.basename(api.LOADED_PATH)}\n")
print(f"L {L}, before {BEFORE}, focus {F}, B {B}, f16 medmad: {ns} sites ({n1} with label 1), {ns * L / N:.2f} window samples per signal sample\n")
print(f"generation of this batch (sqg_timing_t.total_ms): {gen_ms:.2f} ms; streaming-store probe: {store / 1e12:.2f} TB/s; "
      f"median of {REP} timed calls after one warm-up call, wall clock around the blocking C call, outputs preallocated\n")
print("| call | ms (min, max) | generation ms |")
print("|---|---|---|")
for name, t in (("plan: sqg_site_plan, no plan in the scratch", plan), ("scan: label, site_read, site_pos, win_start alone", scan),
                ("stats: med2, mad4 alone", stats), ("rows: signal, context, ctx_start (stats + scan + emit)", rows), ("all nine outputs", everything)):
    print(f"| {name} | {t[0]:.3f} ({t[1]:.3f}, {t[2]:.3f}) | {gen_ms:.2f} |")
print(f"\nemit = all - scan - stats = {emit_ms:.3f} ms: {moved / 1e9:.3f} GB moved, {moved / emit_ms / 1e6:.0f} GB/s, "
      f"{moved / (emit_ms * 1e-3) / store:.2f} of the store probe")
b.free()
gen.close()
