#!/usr/bin/env python3
"""Rate of sqg_batch_scale and sqg_batch_align_scaled (include/sqg_scale.h) on the headline batch of tools/align_rate.py: K sampled 10-kb
reads, -x dna-r10-prom (k = 9), -t 1, certified, the rows sqg_batch_detect finds under the DNA preset.  Three parts:
  times       wall-clock milliseconds around the blocking C calls on preallocated outputs (median of the timed calls after a warm-up call),
              all in one process on one batch: sqg_batch_scale in both modes, sqg_batch_align_scaled under the identity scaling next to
              sqg_batch_align on the same rows (the same paths: what differs is the scaling alone; the two are called in turn),
              sqg_batch_collapse's row pass, and as a
              yardstick torch sums over the arrays each mode reads
  estimates   gain / 65536 and shift / 256 over the reads, by MOMENTS and by FIT over sqg_batch_align's al_ev, next to the truth (1, 0)
  the loop    rows miscalibrated per read (a gain in 0.8 .. 1.25, an offset in +-60 codes: sum' = round(a sum) + b len), then the share
              of al_ev == true_ev under (a) the plain aligner, (b) scaled by MOMENTS, (c) scaled by FIT over (b)'s al_ev, (d) the plain
              aligner on the untouched rows
Prints markdown (profiles/scale.md).  SQG_LIB=... runs a kernel build variant (tools/README.md).
usage: python tools/scale_rate.py [reads_per_batch=32768] [timed_calls=3] [genome_mb=200]"""
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

ARGS = sys.argv[1:]
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
N, NE = int(b.n_samples), int(b.n_events)
dt = b.detect("dna", "pa", outputs=("sum", "sumsq", "dt_len", "true_ev"))      # the rows, made once
NR = int(dt.n_rows)
off = np.ascontiguousarray(dt.det_off, np.int64)
rows = np.diff(off)
poff = off.ctypes.data_as(C.POINTER(C.c_int64))
cfg_al = api.CAlignCfg(*api.ALIGN_DEFAULT)
al = b.align(off, dt.sum, dt.dt_len, api.ALIGN_DEFAULT)     # (d), and the outputs of the timed calls, allocated once
sc = b.scale(off, dt.sum, dt.dt_len, al.al_ev)
level = b.events(outputs=("level_raw",)).level_raw
one = (torch.full((K,), 65536, dtype=torch.int32, device=dev), torch.zeros(K, dtype=torch.int32, device=dev))


def timed(call):
    ts = []
    for it in range(REP + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts[1:])), min(ts[1:]), max(ts[1:])


def timed_pair(first, second):
    """the two calls in turn, REP + 1 rounds, the first round dropped: neither is measured on a device the other has warmed for it"""
    ts = ([], [])
    for it in range(REP + 1):
        for call, t in zip((first, second), ts):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            t.append((time.perf_counter() - t0) * 1e3)
    return tuple((float(np.median(t[1:])), min(t[1:]), max(t[1:])) for t in ts)


def scale(mode, ev):
    cfg = api.CScaleCfg(mode)
    cin = api.CScaleIn(dt.sum.data_ptr(), dt.dt_len.data_ptr(), None if ev is None else ev.data_ptr())
    out = api.CScaleOut(*[getattr(sc, n).data_ptr() for n in api.SCALE_OUTPUTS])
    return lambda: gen._chk(gen.L.sqg_batch_scale(gen.ctx, b.handle, C.byref(cfg), poff, C.byref(cin), C.byref(out)), "sqg_batch_scale")


def align(scaling):
    cin = api.CAlignIn(dt.sum.data_ptr(), dt.dt_len.data_ptr())
    out = api.CAlignOut(*[getattr(al, n).data_ptr() for n in api.ALIGN_OUTPUTS])
    if scaling is None:
        return lambda: gen._chk(gen.L.sqg_batch_align(gen.ctx, b.handle, C.byref(cfg_al), poff, C.byref(cin), C.byref(out)), "sqg_batch_align")
    s = api.CAlignScale(scaling[0].data_ptr(), scaling[1].data_ptr())
    return lambda: gen._chk(gen.L.sqg_batch_align_scaled(gen.ctx, b.handle, C.byref(cfg_al), poff, C.byref(cin), C.byref(s), C.byref(out)), "sqg_batch_align_scaled")


print(f"# sqg_batch_scale and sqg_batch_align_scaled on one MI355X: {K} sampled 10-kb reads (dna-r10-prom, -t 1, certified), rows of the DNA detect preset, "
      f"N = {N:.4g} samples, {NE:.4g} true events, {NR:.4g} detected rows ({NR / NE:.3f} per true event; {rows.min()} .. {rows.max()} rows per read), "
      f"SQG_ALIGN_DEFAULT {api.ALIGN_DEFAULT}, library {os.path.basename(api.LOADED_PATH)}\n")

# ---- times
al_ev = al.al_ev.clone()                                    # FIT's assignment: (d)'s, kept while the timed align calls overwrite al
ch = b.collapse(off, al_ev, dt.sum, dt.sumsq, dt.dt_len, outputs=("ob_rows", "ob_len", "ob_sum", "ob_sumsq", "rd_dropped"))
ccfg = api.CCollapseCfg(api.CHUNK_PA, 0)
ccin = api.CCollapseIn(al_ev.data_ptr(), dt.sum.data_ptr(), dt.sumsq.data_ptr(), dt.dt_len.data_ptr())
cout = api.CCollapseOut(*[None if getattr(ch, n) is None else getattr(ch, n).data_ptr() for n in api.COLLAPSE_OUTPUTS])
t_mom = timed(scale(api.SCALE_MOMENTS, None))
t_fit = timed(scale(api.SCALE_FIT, al_ev))
t_plain, t_scaled = timed_pair(align(None), align(one))
t_rows = timed(lambda: gen._chk(gen.L.sqg_batch_collapse(gen.ctx, b.handle, C.byref(ccfg), poff, C.byref(ccin), C.byref(cout)), "sqg_batch_collapse"))
t_ymom = timed(lambda: (dt.sum.sum(), dt.dt_len.sum(), level.sum(), torch.cuda.synchronize()))
t_yfit = timed(lambda: (dt.sum.sum(), dt.dt_len.sum(), al_ev.sum(), level.sum(), torch.cuda.synchronize()))
del ch
b_mom, b_fit = 12 * NR + 2 * NE, 22 * NR
print("## Times\n")
print(f"median of {REP} timed calls after one warm-up call, wall clock around the blocking C call, outputs preallocated; all in one process on one batch\n")
print("| call | ms (min, max) |")
print("|---|---|")
for name, t in (("sqg_batch_scale MOMENTS: all ten outputs (memset, level scan, k_scale_sums over rows and over events, k_scale_derive)", t_mom),
                ("sqg_batch_scale FIT over al_ev: all ten outputs (memset, level scan, k_scale_sums, k_scale_derive)", t_fit),
                ("sqg_batch_align: all three outputs (in turn with the next line)", t_plain),
                ("sqg_batch_align_scaled, gain 65536 and shift 0: all three outputs", t_scaled),
                ("sqg_batch_collapse: the four sums and rd_dropped (memsets, k_collapse_rows)", t_rows),
                ("yardstick, torch sums of sum, dt_len and level_raw (what MOMENTS reads)", t_ymom),
                ("yardstick, torch sums of sum, dt_len, al_ev and level_raw (what FIT reads, its gather as one stream)", t_yfit)):
    print(f"| {name} | {t[0]:.3f} ({t[1]:.3f}, {t[2]:.3f}) |")
print(f"\nbytes: MOMENTS reads 12 B per row (sum 8, len 4) and 2 B per event (level_raw): {b_mom / 1e9:.3f} GB, {b_mom / t_mom[0] / 1e6:.1f} GB/s, "
      f"{NR / t_mom[0] / 1e6:.2f} Grows/s; FIT 22 B per row (sum 8, len 4, ev 8, the gathered level_raw 2): {b_fit / 1e9:.3f} GB, {b_fit / t_fit[0] / 1e6:.1f} GB/s, "
      f"{NR / t_fit[0] / 1e6:.2f} Grows/s.  Streamed once at 8 TB/s: {b_mom / 8e12 * 1e3:.3f} and {b_fit / 8e12 * 1e3:.3f} ms.")
print(f"sqg_batch_scale against sqg_batch_collapse's row pass ({t_rows[0]:.3f} ms): MOMENTS {'below' if t_mom[0] < t_rows[0] else 'NOT below'}, "
      f"FIT {'below' if t_fit[0] < t_rows[0] else 'NOT below'}")
print(f"sqg_batch_align_scaled {t_scaled[0]:.3f} ms against sqg_batch_align's spread {t_plain[1]:.3f} .. {t_plain[2]:.3f} ms: "
      f"{'inside' if t_plain[1] <= t_scaled[0] <= t_plain[2] else 'OUTSIDE'} ({(t_scaled[0] / t_plain[0] - 1) * 100:+.2f} % of the median)\n")


# ---- the estimates next to the truth
def spread(x):
    x = x.double()
    q = torch.quantile(x, torch.tensor([0.01, 0.99], dtype=torch.float64, device=dev))
    return f"{float(x.mean()):.5f} | {float(x.std()):.5f} | {float(q[0]):.5f} | {float(q[1]):.5f}"


print("## The estimates next to the truth (gain 1, shift 0), untouched rows\n")
print("| estimate | mean | sd | 1st percentile | 99th percentile |")
print("|---|---|---|---|---|")
for name, est in (("MOMENTS", b.scale(off, dt.sum, dt.dt_len)), ("FIT over al_ev", b.scale(off, dt.sum, dt.dt_len, al_ev))):
    print(f"| {name}: gain / 65536 | {spread(est.gain.double() / 65536.0)} |")
    print(f"| {name}: shift / 256, codes | {spread(est.shift.double() / 256.0)} |")
    if est.rd_dropped.sum() > 0:
        print(f"| {name}: dropped rows | {int(est.rd_dropped.sum())} | | | |")
del est

# ---- the loop
rng = np.random.default_rng(1)
ga = torch.from_numpy(rng.uniform(0.8, 1.25, K)).to(dev)
ob = torch.from_numpy(rng.integers(-60, 61, K)).to(dev)
rd = torch.repeat_interleave(torch.arange(K, device=dev), torch.from_numpy(rows).to(dev))
bent = torch.round(ga[rd] * dt.sum.double()).long() + ob[rd] * dt.dt_len.long()
del rd


def score(a):
    d = a.al_ev - dt.true_ev
    have = a.al_cost >= 0
    return (float((d == 0).double().mean()), float((d.abs() <= 1).double().mean()), float(a.al_cost[have].double().sum()) / NR, float(a.al_edge.double().mean()))


res = [("(d) sqg_batch_align on the untouched rows", score(al))]
del al_ev
a = b.align(off, bent, dt.dt_len, api.ALIGN_DEFAULT)
res.insert(0, ("(a) sqg_batch_align on the miscalibrated rows", score(a)))
m = b.scale(off, bent, dt.dt_len, outputs=("gain", "shift"))
a = b.align(off, bent, dt.dt_len, api.ALIGN_DEFAULT, scale=(m.gain, m.shift))
res.insert(1, ("(b) scaled by MOMENTS", score(a)))
f = b.scale(off, bent, dt.dt_len, a.al_ev, outputs=("gain", "shift"))
a = b.align(off, bent, dt.dt_len, api.ALIGN_DEFAULT, scale=(f.gain, f.shift))
res.insert(2, ("(c) scaled by FIT over (b)'s al_ev", score(a)))
print("\n## The loop: a gain in 0.8 .. 1.25 and an offset in +-60 codes per read, sum' = round(a sum) + b len\n")
print("| rows and scaling | al_ev == true_ev | abs(al_ev - true_ev) <= 1 | mean al_cost per row | mean al_edge |")
print("|---|---|---|---|---|")
for name, (same, near, cost, edge) in res:
    print(f"| {name} | {same:.6f} | {near:.6f} | {cost:.1f} | {edge:.2f} |")
want_g, want_s = 1.0 / ga, -ob.double() / ga
for name, est in (("MOMENTS", m), ("FIT", f)):
    print(f"\n{name} against the inverse of the injection (1 / a, -b / a): gain / 65536 - 1 / a: {spread(est.gain.double() / 65536.0 - want_g).replace(' | ', ', ')}; "
          f"shift / 256 + b / a, codes: {spread(est.shift.double() / 256.0 - want_s).replace(' | ', ', ')}  (mean, sd, 1st and 99th percentile)")
b.free()
gen.close()
