"""Per-step time of a 1024^2, 30-step, bf16 text-to-image denoise (UNet batch 2) without and with FreeU (SDXL's published values): the
two plans of ONE engine (unet.enable_freeu / disable_freeu under one conditioning and schedule) alternating in one process on the
full-width UNet with seeded weights: two warm-up denoises per case, then REPS timed ones; the median and the spread are printed with the
shader clock sampled while they ran, and written to OUT.  The "plain" arm is the plan of a UNet without FreeU: the baseline.  Also
reported: the launch counts, and the time of each of the six FreeU concat launches inside the plan (imh_plan_time_ops, median of five
sweeps) against its byte floor, (bytes read + written) / 8 TB/s.
python tools/freeu_time.py [reps=7] [out=profiles/freeu_timing.json]"""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, '.')
import bench
from imagharmony_amd import lib as L
from imagharmony_amd.denoise import DenoiseEngine
from imagharmony_amd.schedulers import DDIMScheduler

DEV = torch.device("cuda:0")
STEPS, H = 30, 128
FREEU = (0.6, 0.4, 1.1, 1.2)
HBM_PEAK = 8e12
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join("profiles", "freeu_timing.json")

u = bench.build_unet(DEV, torch.bfloat16, 4)
pe, ne, po, no = [t.to(DEV) for t in bench.synthetic_conditioning(4)]
lat = torch.randn(1, 4, H, H, generator=torch.Generator().manual_seed(0))
sch = DDIMScheduler()

e = DenoiseEngine(u, DEV, torch.bfloat16)
e.set_conditioning(pe, ne, po, no, 8 * H, 8 * H, guidance_scale=5.0)
plans = {}


def one(name):
    if name == "freeu":
        u.enable_freeu(*FREEU)
    else:
        u.disable_freeu()
    e.set_schedule(sch, STEPS)
    torch.cuda.synchronize()
    t = time.perf_counter()
    e.denoise(lat)
    torch.cuda.synchronize()
    plans[name] = e.plan
    return (time.perf_counter() - t) * 1e3 / STEPS


names = ("plain", "freeu")
for name in names:
    one(name); one(name)
assert plans["plain"] is not plans["freeu"]
clk = bench.ClockSampler(period=0.5)
ms = {name: [] for name in names}
for _ in range(reps):
    for name in names:                       # alternating: drift of the box hits both plans alike
        ms[name].append(one(name))
clocks = clk.stop()

# the concat launches by themselves, in the plan they run in
p = plans["freeu"]
sweeps = []
for _ in range(5):
    e.eager.ew(L.EW_STEP_SET, e.st.step, i=(0, 1, 0, 0, 0, 0), descr="step=0")      # the plan ends with step++: every sweep reads row 0 of its tables
    sweeps.append(p.time_ops())
concat = []
for j, t in enumerate(p.tags):
    if t[2] == "freeu.concat":
        a = p._ops[j][1]
        nbytes = 2.0 * 2 * a.n * (a.i0 + a.i1)          # reads n * (i0 + i1) 16-bit elements, writes as many
        us = statistics.median(s[j] for s in sweeps) * 1e3
        concat.append({"pixels": a.n, "hidden": a.i0, "skip": a.i1, "H": a.i2, "W": a.i3, "us": us, "bytes": nbytes,
                       "floor_us": nbytes / HBM_PEAK * 1e6, "tb_per_s": nbytes / (us * 1e-6) / 1e12})
stats = [statistics.median(s[j] for s in sweeps) * 1e3 for j, t in enumerate(p.tags) if t[2] == "gn_stats" and t[0] in (40, 41)]
out = {"steps": STEPS, "reps": reps, "latent": [H, H], "unet_batch": 2, "dtype": "bfloat16", "freeu": list(FREEU),
       "sclk_mhz": clocks and clocks["sclk_mhz"],
       "ms_per_step": {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in ms.items()},
       "launches_per_step": {k: q.lib.imh_plan_size(q.plan) for k, q in plans.items()},
       "freeu_concat_launches": concat, "freeu_concat_us_per_step": sum(c["us"] for c in concat),
       "freeu_concat_floor_us_per_step": sum(c["floor_us"] for c in concat), "up01_gn_stats_us_per_step": sum(stats)}
print(json.dumps(out))
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as f:
    json.dump(out, f, indent=1, sort_keys=True)
