"""A 1024^2, 30-step, bf16 Euler-ancestral denoise (CFG, UNet batch 2) with the step noise from the host-filled bank and from the
seeded generator (set_schedule(seeded_noise=True)), in one process on the full-width UNet with seeded weights: the two plans of one
engine, two warm-up denoises per case, then REPS timed ones with the cases alternating.  Per case: the host milliseconds before the
loop (bank: the torch draw and the copy into the bank; seeded: the copy of the seed rows), the milliseconds per step of the rest, and
the device memory the schedule's step state holds.  Medians and spreads, with the shader clock sampled while they ran.
python tools/seeded_noise_time.py [reps=7]"""
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, '.')
import bench
from imagharmony_amd.denoise import GENERAL_STEP, DenoiseEngine
from imagharmony_amd.schedulers import EulerAncestralDiscreteScheduler

DEV = torch.device("cuda:0")
STEPS, H = 30, 128
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7

u = bench.build_unet(DEV, torch.bfloat16, 4)
pe, ne, po, no = [t.to(DEV) for t in bench.synthetic_conditioning(4)]
lat = torch.randn(1, 4, H, H, generator=torch.Generator().manual_seed(0))
sch = EulerAncestralDiscreteScheduler()
e = DenoiseEngine(u, DEV, torch.bfloat16)
e.set_conditioning(pe, ne, po, no, 8 * H, 8 * H, guidance_scale=5.0)
gen = torch.Generator().manual_seed(1)
CASES = {"bank": (dict(), lambda: dict(generator=gen)), "seeded": (dict(seeded_noise=True), lambda: dict(step_seeds=[1234]))}


def sync():
    torch.cuda.synchronize(DEV)


def one(name):
    """-> (host ms before the loop, ms of the whole denoise call)"""
    skw, nkw = CASES[name]
    e.set_schedule(sch, STEPS, **skw)            # a plan-cache hit after the first call: pointers only
    sync()
    t = time.perf_counter()
    e._start_general_step(**nkw())               # what denoise() does before the loop, by itself
    sync()
    host = (time.perf_counter() - t) * 1e3
    t = time.perf_counter()
    e.denoise(lat, **nkw())
    sync()
    return host, (time.perf_counter() - t) * 1e3


mem = {}
for name in CASES:
    one(name); one(name)
    st = e.st
    mem[name] = {k: (0 if getattr(st, k, None) is None else getattr(st, k).numel() * getattr(st, k).element_size()) for k in GENERAL_STEP}
clk = bench.ClockSampler(period=0.5)
host, total = {n: [] for n in CASES}, {n: [] for n in CASES}
for _ in range(reps):
    for name in CASES:                           # alternating: drift of the box hits both cases alike
        h, t = one(name)
        host[name].append(h); total[name].append(t)
clocks = clk.stop()
stat = lambda v: {"median": statistics.median(v), "min": min(v), "max": max(v)}
out = {"steps": STEPS, "reps": reps, "sclk_mhz": clocks and clocks["sclk_mhz"],
       "host_ms_before_loop": {k: stat(v) for k, v in host.items()},
       "ms_per_denoise": {k: stat(v) for k, v in total.items()},
       "ms_per_step": {k: stat([(t - h) / STEPS for t, h in zip(total[k], host[k])]) for k in CASES},
       "schedule_state_bytes": mem,
       "launches_per_step": e.plan.lib.imh_plan_size(e.plan.plan)}
print(json.dumps(out))
