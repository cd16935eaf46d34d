"""Per-step time of a 1024^2, 30-step, bf16 inpaint denoise in both modes (4-channel UNet: masked blend in the step; 9-channel UNet:
conv_in over [latents | mask | masked-image latents]) next to an img2img denoise of the same strength, in one process on the
full-width UNet with seeded weights: two warm-up denoises per case, then REPS timed ones with the cases alternating; the median
and the spread are printed with the shader clock sampled while they ran.
python tools/inpaint_time.py [strength=0.9999] [reps=7]"""
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, '.')
import bench
from imagharmony_amd.denoise import DenoiseEngine
from imagharmony_amd.schedulers import DDIMScheduler, get_timesteps

DEV = torch.device("cuda:0")
STEPS, H = 30, 128
strength = float(sys.argv[1]) if len(sys.argv) > 1 else 0.9999
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7


def unet(cin):
    if cin == 4:
        return bench.build_unet(DEV, torch.bfloat16, 4)
    from imagharmony_amd.ip_adapter import install_ip_processors
    from imagharmony_amd.unet import UNet2DConditionModel, UNetConfig
    with torch.device(DEV):
        u = UNet2DConditionModel(UNetConfig(in_channels=9))
    u.init_random_(1234)
    u = u.to(torch.bfloat16)
    procs = install_ip_processors(u, num_tokens=4, scale=1.0, device=DEV, dtype=torch.bfloat16, init="empty")
    g = torch.Generator(device=DEV).manual_seed(4321)          # as bench.build_unet fills them
    for p in procs.values():
        for q in p.parameters():
            q.data.copy_(torch.randn(q.shape, generator=g, device=DEV) * (q.shape[1] ** -0.5))
    return u


g = torch.Generator().manual_seed(0)
mom = torch.randn(1, H, H, 8, generator=g)
n1, n2, n3 = (torch.randn(1, 4, H, H, generator=g) for _ in range(3))
mask = torch.zeros(1, 1, H, H)
mask[..., H // 2:] = 1.0
pe, ne, po, no = [t.to(DEV) for t in bench.synthetic_conditioning(4)]
sch = DDIMScheduler()
sch.set_timesteps(STEPS)
_, t_start = get_timesteps(sch, STEPS, strength)
ab = sch.add_noise_coefficients(t_start)
ran = STEPS - t_start

u4, u9 = unet(4), unet(9)
cases = {}
for name, u, inpaint in (("img2img", u4, False), ("inpaint_blend", u4, True), ("inpaint_concat9", u9, True)):
    e = DenoiseEngine(u, DEV, torch.bfloat16)
    e.set_conditioning(pe, ne, po, no, 8 * H, 8 * H, guidance_scale=5.0)
    e.set_schedule(sch, STEPS, t_start=t_start, inpaint=inpaint)
    if inpaint:
        prep = lambda e=e: e.prepare_inpaint(mom, n1, n2, 0.13025, ab[0], ab[1], mask, masked_moments=mom, n3=n3)
    else:
        prep = lambda e=e: e.prepare_img2img(mom, n1, n2, 0.13025, ab[0], ab[1])
    cases[name] = (e, prep)


def one(name):
    e, prep = cases[name]
    prep()
    torch.cuda.synchronize()
    t = time.perf_counter()
    e.denoise(None)
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / ran


for name in cases:
    one(name); one(name)
clk = bench.ClockSampler(period=0.5)
ms = {name: [] for name in cases}
for _ in range(reps):
    for name in cases:                       # alternating: drift of the box hits every case alike
        ms[name].append(one(name))
clocks = clk.stop()
out = {"strength": strength, "steps_run": ran, "reps": reps, "sclk_mhz": clocks and clocks["sclk_mhz"],
       "ms_per_step": {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in ms.items()},
       "launches_per_step": {k: c[0].plan.lib.imh_plan_size(c[0].plan.plan) for k, c in cases.items()}}
print(json.dumps(out))
