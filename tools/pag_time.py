"""Per-step time of a 1024^2, 30-step, bf16 text-to-image denoise (S = 1) without and with perturbed-attention guidance in the mid block
(layers "mid": ten self-attention layers): the PAG-off plan (UNet batch 2) and the PAG-on plan (UNet batch 3) of ONE engine -- the two
conditionings the engine keeps across the switch (DenoiseEngine.set_conditioning(pag_scale=)) -- alternating in one process on the
full-width UNet with seeded weights: two warm-up denoises per case, then REPS timed ones; the median and the spread are printed with
the shader clock sampled while they ran, and written to OUT.  Also reported: the launch counts of both plans, and the time of each of
the ten identity-rows copy launches inside the PAG plan (imh_plan_time_ops, median of five sweeps) with their sum and byte floor,
(bytes read + written) / 8 TB/s.  Nobody has tuned the batch-3 GEMM and conv shapes: they run the default tiles.
python tools/pag_time.py [reps=7] [out=profiles/pag_timing.json]"""
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
PAG_SCALE, LAYERS = 3.0, "mid"
HBM_PEAK = 8e12
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join("profiles", "pag_timing.json")

u = bench.build_unet(DEV, torch.bfloat16, 4)
u.set_pag_applied_layers(LAYERS)
pe, ne, po, no = [t.to(DEV) for t in bench.synthetic_conditioning(4)]
lat = torch.randn(1, 4, H, H, generator=torch.Generator().manual_seed(0))
sch = DDIMScheduler()

e = DenoiseEngine(u, DEV, torch.bfloat16)
plans, conds = {}, {}


def one(name):
    e.set_conditioning(pe, ne, po, no, 8 * H, 8 * H, guidance_scale=5.0, **({"pag_scale": PAG_SCALE} if name == "pag" else {}))
    e.set_schedule(sch, STEPS)
    torch.cuda.synchronize()
    t = time.perf_counter()
    e.denoise(lat)
    torch.cuda.synchronize()
    plans[name], conds[name] = e.plan, e.st
    return (time.perf_counter() - t) * 1e3 / STEPS


names = ("plain", "pag")
first = {}
for k in range(2):
    for name in names:                       # (alternating here too: the first switch conditions and records, every later one finds both kept)
        one(name)
        first.setdefault(name, (plans[name], conds[name]))
# after the first switch each mode's conditioning and plan are kept: nothing is projected or recorded inside the timed region
assert all(first[n] == (plans[n], conds[n]) for n in names) and plans["plain"] is not plans["pag"]
clk = bench.ClockSampler(period=0.5)
ms = {name: [] for name in names}
for _ in range(reps):
    for name in names:                       # alternating: drift of the box hits both plans alike
        ms[name].append(one(name))
clocks = clk.stop()
assert all(first[n] == (plans[n], conds[n]) for n in names)

# the copy launches by themselves, in the plan they run in
one("pag")
p = plans["pag"]
sweeps = []
for _ in range(5):
    e.eager.ew(L.EW_STEP_SET, e.st.step, i=(0, 1, 0, 0, 0, 0), descr="step=0")      # the plan ends with step++: every sweep reads row 0 of its tables
    sweeps.append(p.time_ops())
copies = []
for j, t in enumerate(p.tags):
    if t[2] == "self.pag_rows":
        a = p._ops[j][1]
        nbytes = 2.0 * 2 * a.n * a.i1                    # reads n * C 16-bit elements, writes as many
        us = statistics.median(s[j] for s in sweeps) * 1e3
        copies.append({"rows": a.n, "channels": a.i1, "col0": a.i4, "ldvt": a.i5, "us": us, "bytes": nbytes,
                       "floor_us": nbytes / HBM_PEAK * 1e6, "tb_per_s": nbytes / (us * 1e-6) / 1e12})
med = {k: statistics.median(v) for k, v in ms.items()}
out = {"steps": STEPS, "reps": reps, "latent": [H, H], "samples": 1, "unet_batch": {"plain": 2, "pag": 3}, "dtype": "bfloat16",
       "pag_scale": PAG_SCALE, "pag_layers": LAYERS, "chosen_layers": len(u.pag_layer_names()),
       "sclk_mhz": clocks and clocks["sclk_mhz"],
       "ms_per_step": {k: {"median": med[k], "min": min(v), "max": max(v)} for k, v in ms.items()},
       "ratio_pag_over_plain": med["pag"] / med["plain"],
       "ranges_overlap": not (min(ms["pag"]) > max(ms["plain"]) or min(ms["plain"]) > max(ms["pag"])),
       "launches_per_step": {k: q.lib.imh_plan_size(q.plan) for k, q in plans.items()},
       "copy_launches": copies, "copy_us_per_step": sum(c["us"] for c in copies), "copy_floor_us_per_step": sum(c["floor_us"] for c in copies)}
print(json.dumps(out))
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as f:
    json.dump(out, f, indent=1, sort_keys=True)
