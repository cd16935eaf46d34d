"""Per-step time of a 1024^2, 30-step, bf16 text-to-image denoise (UNet batch 2) without regional image prompts and with N = 1, 2 and 4
of them: the plans of ONE engine (set_ip_regions, a conditioning per N, one schedule) alternating in one process on the full-width UNet
with seeded weights -- two warm-up denoises per case, then REPS timed ones; the median and the min-max spread are printed with the shader
clock sampled while they ran, and written to OUT.  A difference is claimed only where the ranges of two cases do not overlap.  Also
reported: the launch counts of the recorded step -- equal with and without regions, because one launch kind replaces another in the ten
layers with an image-prompt branch -- and how many of them are csrc/xattn_regions.hip's.
python tools/ip_regions_time.py [reps=7] [out=profiles/ip_regions_timing.json]"""
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
from imagharmony_amd.regions import IPRegions
from imagharmony_amd.schedulers import DDIMScheduler

DEV = torch.device("cuda:0")
STEPS, H, T = 30, 128, 4
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join("profiles", "ip_regions_timing.json")

u = bench.build_unet(DEV, torch.bfloat16, T)
pe, ne, po, no = [t.to(DEV) for t in bench.synthetic_conditioning(T)]
lat = torch.randn(1, 4, H, H, generator=torch.Generator().manual_seed(0))
sch = DDIMScheduler()
g = torch.Generator().manual_seed(5)


def regions(n):
    """n vertical stripes of the picture with a soft edge, weights 1.0, 0.9, ..."""
    x = torch.linspace(0.0, 1.0, 8 * H)
    m = torch.stack([((x - i / n) * 20).clamp(0, 1) * (((i + 1) / n - x) * 20).clamp(0, 1) for i in range(n)])
    return IPRegions(m[:, None, :].expand(n, 8 * H, 8 * H).contiguous(), [1.0 - 0.1 * i for i in range(n)])


def conditioning(n):
    """the synthetic conditioning with n image prompts: the text tokens, then n x T image tokens"""
    more = lambda t: torch.cat([t] + [torch.randn(t.shape[0], T, t.shape[2], generator=g).to(t) for _ in range(n - 1)], 1)
    return more(pe), more(ne), po, no


cases = {"plain": None, "n1": regions(1), "n2": regions(2), "n4": regions(4)}
engines, plans = {}, {}
for name, r in cases.items():                 # one engine per case on the same UNet: each keeps its conditioning and its recorded plan
    e = engines[name] = DenoiseEngine(u, DEV, torch.bfloat16)
    if r is not None:
        e.set_ip_regions(r)
    e.set_conditioning(*conditioning(r.n if r else 1), 8 * H, 8 * H, guidance_scale=5.0)
    e.set_schedule(sch, STEPS)
    e.denoise(lat)
    plans[name] = e.plan
e.set_ip_regions(None)           # the shared UNet's processors as they were; the recorded plans keep what they read


def one(name):
    e = engines[name]
    torch.cuda.synchronize()
    t = time.perf_counter()
    e.denoise(lat)
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / STEPS


for name in cases:
    one(name); one(name)
clk = bench.ClockSampler(period=0.5)
ms = {name: [] for name in cases}
for _ in range(reps):
    for name in cases:                        # alternating: drift of the box hits the plans alike
        ms[name].append(one(name))
clocks = clk.stop()
kinds = lambda p: [p.lib.imh_plan_get_kind(p.plan, i) for i in range(p.lib.imh_plan_size(p.plan))]
out = {"steps": STEPS, "reps": reps, "latent": [H, H], "unet_batch": 2, "dtype": "bfloat16", "sclk_mhz": clocks and clocks["sclk_mhz"],
       "ms_per_step": {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in ms.items()},
       "launches_per_step": {k: len(kinds(p)) for k, p in plans.items()},
       "regions_launches_per_step": {k: kinds(p).count(L.OP_XATTN_REGIONS) for k, p in plans.items()}}
print(json.dumps(out))
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as f:
    json.dump(out, f, indent=1, sort_keys=True)
