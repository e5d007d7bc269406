#!/usr/bin/env python3
"""Rate of sqg_batch_pileup (include/sqg_pileup.h) next to sqg_batch_events(mean, sd) on the same batch: K sampled 10-kb reads, -t 1,
certified, one shape per process:
  a    BASELINE.json configs[2]'s shape (-x dna-r10-prom, k = 9, the 200-MB synthetic genome), by position; the window is the first contig,
       about 1/12 of the genome: most events fall outside it
  b    the same reads from a 30-kb genome, whole window: every event lands, about K / 3 adds hit each address
  c9   the batch of a, by pore-table row: 4^9 rows
  c6   -x dna-r9-prom (k = 6), by pore-table row: 4^6 rows
Wall-clock milliseconds around the blocking C calls on preallocated outputs (median of the timed calls after a warm-up call).  The adds
are 4 B (n) and 5 x 8 B (the sums) per counted event; the added-bytes rate is set against the 1.3 TB/s measured for 32-bit float adds
on this part.  Prints markdown (profiles/pileup.md).  SQG_LIB=... runs a kernel build variant (tools/README.md).
usage: python tools/pileup_rate.py a|b|c9|c6 [reads_per_batch=32768] [timed_calls=7] [genome_mb=200]"""
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

SHAPE = sys.argv[1] if len(sys.argv) > 1 else "a"
K = int(sys.argv[2]) if len(sys.argv) > 2 else 32768
REP = int(sys.argv[3]) if len(sys.argv) > 3 else 7
MB = float(sys.argv[4]) if len(sys.argv) > 4 else 200.0
FLOAT_ADD_RATE = 1.3e12                                     # B/s of added bytes, 32-bit float global atomics
ADD_BYTES = 4 + 5 * 8
assert SHAPE in ("a", "b", "c9", "c6"), __doc__
dev = torch.device("cuda", 0)
pname, k = ("dna-r9-prom", 6) if SHAPE == "c6" else ("dna-r10-prom", 9)
prof, fl = profiles.get_profile(pname)
mean, stdv = model.synthetic_model(k)
gen = api.SignalGenerator(prof, fl, k, mean, stdv, 42, num_workers=1, mode=api.MODE_CERTIFIED)
if SHAPE == "b":
    small = np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(1).integers(0, 4, 30000)].tobytes()
    gen.load_genome([small], 10000, api.SAMPLE_DNA)
    lens = [30000]
else:
    seq, lens = bench.synthetic_genome_device(MB, dev)
    gen.load_genome_device(seq.data_ptr(), lens, 10000, api.SAMPLE_DNA)
workers = np.zeros(K, np.int32)
for _ in range(2):                                          # warm-up batches (allocation, placement calibration starts)
    gen.sample(K, workers).run().wait().free()
b = gen.sample(K, workers).run().wait()
gen_ms = gen.timing()["total_ms"]
N, NE = int(b.n_samples), int(b.n_events)
if SHAPE in ("a", "b"):
    kw, what = dict(by="ref", lo=0, hi=int(lens[0])), f"by position, window [0, {int(lens[0])}) of {sum(int(x) for x in lens)}"
else:
    kw, what = dict(by="kmer"), f"by pore-table row, {4 ** k} rows"
p = gen.new_pileup(**kw)
ev = b.events("pa", outputs=("mean", "sd"))


def timed(call):
    ts = []
    for it in range(REP + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts[1:])), min(ts[1:]), max(ts[1:])


def events():
    cfg = api.CEventCfg(api.CHUNK_PA, 0)
    out = api.CEventOut(*[getattr(ev, n).data_ptr() if n in ("mean", "sd") else None for n in api.EVENT_OUTPUTS])
    return lambda: gen._chk(gen.L.sqg_batch_events(gen.ctx, b.handle, C.byref(cfg), C.byref(out)), "sqg_batch_events")


stat = api.CPileupStat()


def pileup(names):
    out = api.CPileupOut(*[getattr(p, n).data_ptr() if n in names and getattr(p, n).numel() else None for n in api.PILEUP_OUTPUTS])
    return lambda: gen._chk(gen.L.sqg_batch_pileup(gen.ctx, b.handle, C.byref(p.cfg), None, C.byref(out), C.byref(stat)), "sqg_batch_pileup")


t_ev = timed(events())
t_all = timed(pileup(api.PILEUP_OUTPUTS))
counted, outside = int(stat.counted), int(stat.outside)
t_cnt = timed(pileup(("n", "dwell", "dwell_sq")))
t_none = timed(pileup(()))
keys = int(p.n.numel())
hit = int((p.n != 0).sum())
deepest = int(p.n.view(-1).to(torch.int64).bitwise_and(0xffffffff).max()) // (REP + 1) if keys else 0
print(f"## shape {SHAPE}: {K} sampled 10-kb reads ({pname}, k = {k}, -t 1, certified), {what}\n")
print(f"N = {N:.4g} samples, {NE:.4g} events; counted {counted:.4g}, outside {outside:.4g}; {keys} keys, {hit} of them hit, at most {deepest} adds to one key per call; "
      f"generation of this batch: {gen_ms:.2f} ms; library {os.path.basename(api.LOADED_PATH)}; median of {REP} timed calls after one warm-up call (min, max)\n")
print("| call | ms (min, max) | ns per counted event | added GB/s | of 1.3 TB/s |")
print("|---|---|---|---|---|")
print(f"| sqg_batch_events, mean and sd alone (PA) | {t_ev[0]:.3f} ({t_ev[1]:.3f}, {t_ev[2]:.3f}) | | | |")
for name, t, nb in (("sqg_batch_pileup, all six sums (PA)", t_all, ADD_BYTES), ("sqg_batch_pileup, n, dwell, dwell_sq alone (no sample is read)", t_cnt, 20),
                    ("sqg_batch_pileup, no output (scan, eligibility and the two counters)", t_none, 0)):
    rate = counted * nb / (t[0] * 1e-3)
    print(f"| {name} | {t[0]:.3f} ({t[1]:.3f}, {t[2]:.3f}) | {t[0] * 1e6 / max(counted, 1):.3f} | {rate / 1e9:.1f} | {rate / FLOAT_ADD_RATE:.3f} |")
print(f"\natomic bytes per counted event: {ADD_BYTES} (n 4, five 64-bit sums 40); pileup / events = {t_all[0] / t_ev[0]:.2f}\n")
b.free()
gen.close()
