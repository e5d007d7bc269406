#!/usr/bin/env python3
"""Rate and recovery of sqg_map_track / sqg_batch_map (include/sqg_map.h): N sampled reads of 1500 bases over the nCoV reference
(dna-r9-prom, k = 6, certified), mapped against the whole genome on both strands with row_count 128 and 256.
  times      wall-clock milliseconds around the binding's blocking calls (each allocates its output tensors, then makes the C call, which
             ends in a stream synchronise), REPS calls after a warm-up call: sqg_map_track, sqg_batch_map on the true rows (sqg_batch_events' sum, ev_len, ev_off) and on the
             detector's, next to sqg_batch_events and sqg_batch_align on the same batch; cells per second = mapped rows * W * 2 / the WHOLE call's time
             (k_map_rows, k_map_finish, the offsets' upload and the output allocations included: the kernel's own rate is no lower).
  recovery   the share of reads with map_step equal to the sampler's strand and |map_key0 - (key0 + step * row_first)| <= k, on the true
             and on the detected rows, under Batch.map_shift() and without a scale; the distribution of map_cost_other - map_cost.
Prints markdown (profiles/map.md).
usage: python tools/map_rate.py [sampled_reads=4096] [reps=3]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (first: the HIP runtime torch brings is the one the library then uses)

torch.zeros(1, device="cuda")
from squigulator_amd import api, model, profiles  # noqa: E402

ARGS = sys.argv[1:]
N = int(ARGS[0]) if len(ARGS) > 0 else 4096
REPS = int(ARGS[1]) if len(ARGS) > 1 else 3
k = 6
prof, fl = profiles.get_profile("dna-r9-prom")
mean, stdv = model.synthetic_model(k)


def wall(call):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = call()
    return (time.perf_counter() - t0) * 1e3, out


def timed(call):
    call()                                                  # warm-up
    ts = [wall(call) for _ in range(REPS)]
    return [t for t, _ in ts], ts[-1][1]


def med(ts):
    return f"{np.median(ts):.3f} ({min(ts):.3f}, {max(ts):.3f})"


seqs = []
for ln in open(os.path.join(ROOT, "tests", "golden", "inputs", "nCoV-2019.reference.fasta"), "rb"):
    if ln.startswith(b">"):
        seqs.append([])
    else:
        seqs[-1].append(ln.strip())
contigs = [b"".join(s) for s in seqs]
off = np.concatenate(([0], np.cumsum([len(c) for c in contigs])))
W = int(off[-1])
gen = api.SignalGenerator(prof, fl, k, mean, stdv, 42, num_workers=8, mode=api.MODE_CERTIFIED)
gen.load_genome(contigs, 1500)
b = gen.sample(N).run().wait()
s = b.sampled
minus = np.frombuffer(bytes(s["strand"]), np.uint8) == ord("-")
key0 = off[np.asarray(s["ref_idx"])] + np.asarray(s["ref_pos"], np.int64) + np.where(minus, np.asarray(s["rlen"], np.int64) - k, 0)
step = np.where(minus, -1, 1)

t_track, tr = timed(lambda: gen.new_map_track())
t_ev, ev = timed(lambda: b.events(outputs=("sum", "ev_len")))
dt = b.detect("dna", "pa", outputs=("sum", "dt_len"))
t_al, _ = timed(lambda: b.align(b.ev_off, ev.sum, ev.ev_len, outputs=("al_cost",)))
shift = b.map_shift()
rows = {"true": (b.ev_off, ev.sum, ev.ev_len), "detected": (dt.det_off, dt.sum, dt.dt_len)}

print(f"# sqg_map_track and sqg_batch_map on one MI355X: {N} sampled reads of 1500 bases over the nCoV reference ({W} positions, both strands; "
      f"dna-r9-prom, k = {k}, certified), {int(b.n_events)} true rows, {int(dt.det_off[-1])} detected rows, penalties and cap of SQG_MAP_DEFAULT "
      f"{api.MAP_DEFAULT[:3]}, library {os.path.basename(api.LOADED_PATH)}\n")
print("## Times\n")
print(f"median (min, max) over {REPS} calls after a warm-up call, wall clock around the blocking call of the binding (output tensors allocated inside it)\n")
print("| call | ms | cells / s of the whole call |")
print("|---|---|---|")
print(f"| sqg_map_track, both strands, the whole genome (k_map_track) | {med(t_track)} | |")
res = {}
for rc in (128, 256):
    cfg = api.MAP_DEFAULT[:4] + (rc, 3)
    for name, (ro, sm, ln) in rows.items():
        m = np.minimum(np.diff(ro), rc).sum()
        ts, out = timed(lambda: b.map(ro, sm, ln, tr, cfg=cfg, scale=shift))
        res[name, rc, True] = out
        res[name, rc, False] = b.map(ro, sm, ln, tr, cfg=cfg)
        print(f"| sqg_batch_map, {name} rows, row_count {rc}, map_shift() (k_map_rows, k_map_dp, k_map_finish) | {med(ts)} | {m * W * 2 / np.median(ts) / 1e9 * 1e3:.1f} G |")
print(f"| sqg_batch_events, sum and ev_len (the comparator) | {med(t_ev)} | |")
print(f"| sqg_batch_align on the true rows, al_cost (the comparator) | {med(t_al)} | |")

print("\n## Recovery\n")
print("a read is recovered when map_step is the sampler's strand and |map_key0 - key0| <= k (row_first = 0)\n")
print("| rows | row_count | scale | recovered | share | map_cost_other - map_cost: 5 % | median | 95 % |")
print("|---|---|---|---|---|---|---|---|")
for (name, rc, scaled), out in res.items():
    st, k0 = out.map_step.cpu().numpy(), out.map_key0.cpu().numpy()
    hit = (st == step) & (np.abs(k0 - key0) <= k)
    gap = (out.map_cost_other.cpu().numpy().astype(np.int64) - out.map_cost.cpu().numpy())
    p = np.percentile(gap, [5, 50, 95])
    print(f"| {name} | {rc} | {'map_shift()' if scaled else 'none'} | {int(hit.sum())} | {hit.mean():.4f} | {p[0]:.0f} | {p[1]:.0f} | {p[2]:.0f} |")
b.free(); gen.close()
