#!/usr/bin/env python3
"""Rate of sqg_batch_collapse and sqg_batch_pileup_rows (include/sqg_collapse.h) on the headline batch of tools/align_rate.py: K sampled
10-kb reads, -x dna-r10-prom (k = 9), -t 1, certified, the rows sqg_batch_detect finds under the DNA preset, assigned by
sqg_batch_align under SQG_ALIGN_DEFAULT (al_ev).  Wall-clock milliseconds around the blocking C calls on preallocated outputs (median of
the timed calls after a warm-up call), in the same process next to sqg_batch_pileup and sqg_batch_events(mean, sd) on that batch.  Beside
the times: the atomics k_collapse_rows issues per row with and without the run combining -- counted from al_ev on the device, not timed --
the bytes the passes move per row and per event, and what the feature exists to produce: per site the share of observed events, and the
mean of |observed - true| of mean_sum / n by position and by pore-table row.
Prints markdown (profiles/collapse.md).  SQG_LIB=... runs a kernel build variant (tools/README.md).
usage: python tools/collapse_rate.py [reads_per_batch=32768] [timed_calls=3] [genome_mb=200]"""
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
dt = b.detect("dna", "pa", outputs=("sum", "sumsq", "dt_len"))      # the rows, made once
NR = int(dt.n_rows)
off = np.ascontiguousarray(dt.det_off, np.int64)
al = b.align(off, dt.sum, dt.dt_len, api.ALIGN_DEFAULT, outputs=("al_ev",))
rows = (al.al_ev, dt.sum, dt.sumsq, dt.dt_len)
cin = api.CCollapseIn(*(t.data_ptr() for t in rows))
poff = off.ctypes.data_as(C.POINTER(C.c_int64))
ch = b.collapse(off, *rows)                                 # the outputs, allocated once
ev = b.events("pa", outputs=("mean", "sd"))


def timed(call):
    ts = []
    for it in range(REP + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts[1:])), min(ts[1:]), max(ts[1:])


def collapse(names):
    cfg = api.CCollapseCfg(api.CHUNK_PA, 0)
    out = api.CCollapseOut(*[getattr(ch, n).data_ptr() if n in names else None for n in api.COLLAPSE_OUTPUTS])
    return lambda: gen._chk(gen.L.sqg_batch_collapse(gen.ctx, b.handle, C.byref(cfg), poff, C.byref(cin), C.byref(out)), "sqg_batch_collapse")


def events():
    cfg = api.CEventCfg(api.CHUNK_PA, 0)
    out = api.CEventOut(*[getattr(ev, n).data_ptr() if n in ("mean", "sd") else None for n in api.EVENT_OUTPUTS])
    gen._chk(gen.L.sqg_batch_events(gen.ctx, b.handle, C.byref(cfg), C.byref(out)), "sqg_batch_events")


def pile_out(p):
    return api.CPileupOut(*[None if getattr(p, n) is None else getattr(p, n).data_ptr() for n in api.PILEUP_OUTPUTS])


def pileup(p):
    out, st = pile_out(p), api.CPileupStat()
    return lambda: gen._chk(gen.L.sqg_batch_pileup(gen.ctx, b.handle, C.byref(p.cfg), None, C.byref(out), C.byref(st)), "sqg_batch_pileup")


def pileup_rows(p):
    out, st = pile_out(p), api.CPileupRowsStat()
    return lambda: gen._chk(gen.L.sqg_batch_pileup_rows(gen.ctx, b.handle, C.byref(p.cfg), None, poff, C.byref(cin), C.byref(out), C.byref(st)), "sqg_batch_pileup_rows")


print(f"# sqg_batch_collapse and sqg_batch_pileup_rows on one MI355X: {K} sampled 10-kb reads (dna-r10-prom, -t 1, certified), rows of the DNA detect preset "
      f"assigned by sqg_batch_align (SQG_ALIGN_DEFAULT), N = {N:.4g} samples, {NE:.4g} true events, {NR:.4g} detected rows ({NR / NE:.3f} per true event), "
      f"library {os.path.basename(api.LOADED_PATH)}\n")

# ---- counted, not timed: the atomics of k_collapse_rows.  A row counts iff its event is one of its read's; a lane is a head if its row is
# dropped, it is lane 0, or its ev differs from the lane before (or that lane's row is dropped); the last lane of every run of a counted row adds
e = al.al_ev
rd = torch.repeat_interleave(torch.arange(K, device=dev), torch.from_numpy(np.diff(off)).to(dev))
ev_off = torch.from_numpy(np.asarray(b.ev_off, np.int64)).to(dev)
counts = (e >= ev_off[rd]) & (e < ev_off[rd + 1])
idx = torch.arange(NR, device=dev)
prev_same = torch.zeros(NR, dtype=torch.bool, device=dev)
prev_same[1:] = (e[1:] == e[:-1]) & counts[:-1]
head = ~counts | (idx % 64 == 0) | ~prev_same
tail = torch.ones(NR, dtype=torch.bool, device=dev)
tail[:-1] = head[1:] | (idx[:-1] % 64 == 63)
n_counts, n_tails = int(counts.sum()), int((tail & counts).sum())
runs = int((counts & (~prev_same)).sum())
print("## Atomics of k_collapse_rows (counted from al_ev, four sums per add site)\n")
print(f"rows that count: {n_counts} of {NR} ({NR - n_counts} dropped); runs of equal ev: {runs} ({n_counts / max(runs, 1):.3f} rows per run); "
      f"run ends inside the wavefronts' cuts: {n_tails}\n")
print("| | add sites | atomics (4 sums) | per row |")
print("|---|---|---|---|")
print(f"| one add per row (no combining) | {n_counts} | {4 * n_counts} | {4 * n_counts / NR:.3f} |")
print(f"| one add per run and wavefront (as built) | {n_tails} | {4 * n_tails} | {4 * n_tails / NR:.3f} |\n")

# ---- times
p_true, p_obs = gen.new_pileup(), gen.new_pileup()
t_rows = timed(collapse(("ob_rows", "ob_len", "ob_sum", "ob_sumsq", "rd_dropped")))
t_all = timed(collapse(api.COLLAPSE_OUTPUTS))
t_ev = timed(events)
t_pile = timed(pileup(p_true))
t_prow = timed(pileup_rows(p_obs))
print("## Times\n")
print(f"median of {REP} timed calls after one warm-up call, wall clock around the blocking C call, outputs preallocated; all in one process on one batch\n")
print("| call | ms (min, max) |")
print("|---|---|")
for name, t in (("sqg_batch_collapse: the four sums and rd_dropped (memsets, k_collapse_rows)", t_rows),
                ("sqg_batch_collapse: all seven outputs (+ k_evtab_scan for ev_read, k_collapse_derive)", t_all),
                ("sqg_batch_events: mean, sd (scan, k_evtab_reduce over the samples)", t_ev),
                ("sqg_batch_pileup: six sums by position (scan, k_pileup over the samples)", t_pile),
                ("sqg_batch_pileup_rows: six sums by position (memsets, k_collapse_rows, scan, k_pileup_rows)", t_prow)):
    print(f"| {name} | {t[0]:.3f} ({t[1]:.3f}, {t[2]:.3f}) |")
row_b, ev_b = 28, 28 + 28 + 4
stream_ms = NR * row_b / 8e12 * 1e3
print(f"\nbytes: a row is read once, {row_b} B (ev 8, sum 8, sumsq 8, len 4): {NR * row_b / 1e9:.3f} GB; per event the row pass zero-fills 28 B (rows 4, len / sum / sumsq 8 each) "
      f"and adds into them, the event pass reads them and ev_read ({ev_b} B) and writes 8 B of mean / sd, or 4 + 5 x 8 B of atomics per counted event: "
      f"{NE * (ev_b + 8) / 1e9:.3f} GB.")
print(f"sqg_batch_collapse's row pass: {NR / t_rows[0] / 1e6:.2f} Grows/s, {NR * row_b / t_rows[0] / 1e6:.1f} GB/s of row bytes (one streaming read of the rows at "
      f"8 TB/s: {stream_ms:.3f} ms).")
print(f"yardstick: sqg_batch_pileup {t_pile[0]:.3f} ms + one streaming read of the rows {stream_ms:.3f} ms = {t_pile[0] + stream_ms:.3f} ms; "
      f"sqg_batch_pileup_rows {t_prow[0]:.3f} ms ({'within' if t_prow[0] <= t_pile[0] + stream_ms else 'above'} it)\n")

# ---- what the feature is for: observed against true, by position and by pore-table row
print("## Observed against true (al_ev rows; PA, units of mean_sum / n are pA)\n")
print("| key | eligible true events | observed (share) | unseen | dropped rows | sites with both | mean abs(observed - true) of mean_sum / n, pA | mean abs difference of dwell / n, samples |")
print("|---|---|---|---|---|---|---|---|")
del p_true, p_obs
for by in ("ref", "kmer"):
    pt, po = gen.new_pileup(by=by, outputs=("n", "dwell", "mean_sum")), gen.new_pileup(by=by, outputs=("n", "dwell", "mean_sum"))
    counted, outside = b.pileup(pt)
    c2, o2, unseen, dropped = b.pileup_rows(po, off, *rows)
    nt, no = pt.n[0].to(torch.float64), po.n[0].to(torch.float64)
    both = (nt > 0) & (no > 0)
    dm = ((po.mean_sum[0][both].to(torch.float64) / no[both] - pt.mean_sum[0][both].to(torch.float64) / nt[both]).abs() / 4096.0).mean()
    dd = (po.dwell[0][both].to(torch.float64) / no[both] - pt.dwell[0][both].to(torch.float64) / nt[both]).abs().mean()
    print(f"| {by} | {counted + outside} | {c2 + o2} ({(c2 + o2) / max(counted + outside, 1):.4f}) | {unseen} | {dropped} | {int(both.sum())} | {float(dm):.4f} | {float(dd):.3f} |")
    del pt, po
b.free()
gen.close()
