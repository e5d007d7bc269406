#!/usr/bin/env python3
"""Rate and recovery of sqg_call_plan / sqg_batch_call (include/sqg_call.h).  Two parts:
  times and agreement   tools/meth_probe.py's batch: K staged reads of 10 kb, dna-r9-prom, k = 6, the 5-letter table, 70 % of the CpGs
                        methylated, T = K workers, certified.  Wall-clock milliseconds around the blocking C calls on preallocated outputs,
                        one timed call per batch over BATCHES batches after a warm-up batch (the plans are kept per batch: every timed
                        plan call is a batch's first): sqg_call_plan and sqg_batch_call next to sqg_site_plan and sqg_batch_events, which
                        read the same bytes.  Then agree / called and the called fraction under SQG_CALL_DEFAULT and call_model(), for the
                        true rows and for detected -> aligned -> collapsed rows.
  called frequency      the dense --meth-freq file of tools/make_methfreq.py over the nCoV reference: N sampled reads of 1500 bases of both
                        strands, true rows, freq over the genome; per position with a byte in the file and called coverage >= 10:
                        meth / called against byte / 255.
Prints markdown (profiles/call.md).
usage: python tools/call_rate.py [reads_per_batch=8192] [batches=3] [sampled_reads=4096]"""
import ctypes as C
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
K = int(ARGS[0]) if len(ARGS) > 0 else 8192
BATCHES = int(ARGS[1]) if len(ARGS) > 1 else 3
NS = int(ARGS[2]) if len(ARGS) > 2 else 4096
L, k = 10000, 6
prof, fl = profiles.get_profile("dna-r9-prom")
fl |= profiles.SQ_METH
mean, stdv = model.synthetic_model(k, meth=True)


def wall(call):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = call()
    return (time.perf_counter() - t0) * 1e3, out


def med(ts):
    return f"{np.median(ts):.3f} ({min(ts):.3f}, {max(ts):.3f})"


# ---- part 1: meth_probe's batch
rng = np.random.default_rng(1)
flat = rng.choice(np.frombuffer(b"ACGT", np.uint8), K * L)
cpg = np.flatnonzero((flat[:-1] == ord("C")) & (flat[1:] == ord("G")))
flat[cpg[rng.random(len(cpg)) < 0.7]] = ord("M")
reads = [flat[i * L:(i + 1) * L].tobytes() for i in range(K)]
gen = api.SignalGenerator(prof, fl, k, mean, stdv, 42, num_workers=K, mode=api.MODE_CERTIFIED)
mw, mc = gen.call_model()
cfg = api.CCallCfg(*api.CALL_DEFAULT)
cmod = api.CCallModel(mw.data_ptr(), mc.data_ptr())
scfg = api.CSiteCfg(256, 128, k // 2, 0, 0, api.CHUNK_F16, api.CHUNK_MEDMAD)
ecfg = api.CEventCfg(api.CHUNK_PA, 0)
t = dict(call_plan=[], site_plan=[], events=[], call=[])
ev = ch = None
for bi in range(BATCHES + 1):
    b = gen.stage(reads).run().wait()
    total = C.c_int64()
    t_cp, _ = wall(lambda: gen._chk(gen.L.sqg_call_plan(gen.ctx, b.handle, None, C.byref(total)), "sqg_call_plan"))
    t_sp, _ = wall(lambda: gen._chk(gen.L.sqg_site_plan(gen.ctx, b.handle, C.byref(scfg), None, C.byref(total)), "sqg_site_plan"))
    if ev is None:                                          # the outputs of the timed calls, allocated once
        ev = b.events(outputs=("sum", "ev_len"))
        ch = b.call(ev.sum, ev.ev_len)
    eout = api.CEventOut(); eout.sum, eout.ev_len = ev.sum.data_ptr(), ev.ev_len.data_ptr()
    t_ev, _ = wall(lambda: gen._chk(gen.L.sqg_batch_events(gen.ctx, b.handle, C.byref(ecfg), C.byref(eout)), "sqg_batch_events"))
    cin = api.CCallIn(ev.sum.data_ptr(), None, ev.ev_len.data_ptr())
    cout = api.CCallOut(*[None if getattr(ch, n) is None else getattr(ch, n).data_ptr() for n in api.CALL_OUTPUTS])
    st = api.CCallStat()
    t_ca, _ = wall(lambda: gen._chk(gen.L.sqg_batch_call(gen.ctx, b.handle, C.byref(cfg), C.byref(cin), C.byref(cmod), None, None, C.byref(cout), None, C.byref(st)), "sqg_batch_call"))
    if bi:
        for name, v in zip(("call_plan", "site_plan", "events", "call"), (t_cp, t_sp, t_ev, t_ca)):
            t[name].append(v)
    if bi < BATCHES:
        b.free()
NE, NSITES, NB = int(b.n_events), int(st.sites), K * L
print(f"# sqg_call_plan and sqg_batch_call on one MI355X: {K} staged reads of {L} bases (dna-r9-prom, k = {k}, 5-letter table, 70 % of the CpGs 'M', "
      f"T = {K}, certified), {NB:.4g} bases, {NE:.4g} events, {NSITES:.4g} sites, SQG_CALL_DEFAULT {api.CALL_DEFAULT}, library {os.path.basename(api.LOADED_PATH)}\n")
print("## Times\n")
print(f"median (min, max) over {BATCHES} batches after a warm-up batch, one call per batch, wall clock around the blocking C call, outputs preallocated\n")
print("| call | ms |")
print("|---|---|")
print(f"| sqg_call_plan, a batch's first (k_call_scan<0> over the bases, copy-back of the counts) | {med(t['call_plan'])} |")
print(f"| sqg_site_plan, a batch's first, win_len 256 (k_site_scan<0> over the dwell scan; the comparator) | {med(t['site_plan'])} |")
print(f"| sqg_batch_call on the true rows, all outputs but site_key, plan kept (k_call_scan<1>, k_call_score) | {med(t['call'])} |")
print(f"| sqg_batch_events, sum and ev_len (k_evtab_scan, k_evtab_reduce; the comparator) | {med(t['events'])} |")
print(f"\n{NB / np.median(t['call_plan']) / 1e6:.2f} Gbases/s through the plan, {NSITES / np.median(t['call']) / 1e6:.3f} Gsites/s through the call.\n")


def share(c):
    s = c.stat
    return f"{s[0]} | {s[2]} | {s[2] / max(s[0], 1):.4f} | {s[3]} | {s[3] / max(s[2], 1):.4f}"


print("## Agreement with the labels, SQG_CALL_DEFAULT, call_model()\n")
print("| rows | sites | called | called / sites | agree | agree / called |")
print("|---|---|---|---|---|---|")
print(f"| the true table (sum, ev_len) | {share(b.call(ev.sum, ev.ev_len, outputs=('call',)))} |")
dt = b.detect("dna", "pa", outputs=("sum", "sumsq", "dt_len"))
al = b.align(dt.det_off, dt.sum, dt.dt_len, outputs=("al_ev",))
co = b.collapse(dt.det_off, al.al_ev, dt.sum, dt.sumsq, dt.dt_len, outputs=("ob_sum", "ob_len"))
print(f"| detected (DNA preset) -> aligned (SQG_ALIGN_DEFAULT) -> collapsed (ob_sum, ob_len; {float((co.ob_len == 0).double().mean()):.4f} of the events unobserved) | "
      f"{share(b.call(co.ob_sum, co.ob_len, outputs=('call',)))} |")
del dt, al, co, ev, ch
b.free(); gen.close()

# ---- part 2: the called frequency against the frequency file
inputs = os.path.join(ROOT, "tests", "golden", "inputs")
names, seqs = [], []
for ln in open(os.path.join(inputs, "nCoV-2019.reference.fasta"), "rb"):
    if ln.startswith(b">"):
        names.append(ln[1:].split()[0].decode()); seqs.append([])
    else:
        seqs[-1].append(ln.strip())
contigs = [b"".join(s) for s in seqs]
mfreq = os.path.join(inputs, "mfreq_dense.tsv")
gen = api.SignalGenerator(prof, fl, k, mean, stdv, 42, num_workers=8, mode=api.MODE_CERTIFIED)
gen.load_genome(contigs, 1500)
gen.set_meth(contigs, names, mfreq)
byte, _ = api.load_meth_freq(contigs, names, mfreq)
listed = np.zeros(len(byte), bool)
for ln in open(mfreq):
    if not ln.startswith("#"):
        listed[int(ln.split("\t")[1])] = True               # (one contig)
fq = gen.new_call_freq()
b = gen.sample(NS).run().wait()
ev = b.events(outputs=("sum", "ev_len"))
c = b.call(ev.sum, ev.ev_len, freq=fq, outputs=("call",))
cov, truth, called, meth = (getattr(fq, n).cpu().numpy().view(np.uint32).astype(np.float64) for n in api.CALL_FREQ)
ok = listed & (called >= 10)
want, got, sim = byte[ok] / 255.0, meth[ok] / called[ok], truth[ok] / cov[ok]
print(f"\n## The called frequency per position against the frequency file\n")
print(f"{NS} sampled reads of 1500 bases over the nCoV reference ({len(byte)} bases), tests/golden/inputs/mfreq_dense.tsv, true rows: {c.stat[0]} sites, "
      f"{c.stat[2]} called, {c.stat[3]} agree; {int(listed.sum())} positions in the file, {int(ok.sum())} of them with 10 called sites or more "
      f"(coverage {cov[ok].min():.0f} .. {cov[ok].max():.0f})\n")
print("| per position | mean abs difference | largest | correlation |")
print("|---|---|---|---|")
print(f"| meth / called against the file's byte / 255 | {np.abs(got - want).mean():.4f} | {np.abs(got - want).max():.4f} | {np.corrcoef(got, want)[0, 1]:.4f} |")
print(f"| truth / cov (the simulated frequency) against the file's byte / 255 | {np.abs(sim - want).mean():.4f} | {np.abs(sim - want).max():.4f} | {np.corrcoef(sim, want)[0, 1]:.4f} |")
print(f"| meth / called against truth / cov | {np.abs(got - sim).mean():.4f} | {np.abs(got - sim).max():.4f} | {np.corrcoef(got, sim)[0, 1]:.4f} |")
b.free(); gen.close()
