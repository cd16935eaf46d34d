"""Per-step time of a 1024^2, 30-step, bf16 text-to-image denoise (UNet batch 2) without layout control, with the T2I-Adapter's four gated
adds, and -- for the side-by-side -- with the ControlNet branch: the three plans of ONE engine (set_adapter / set_controlnet on and off
under one conditioning and schedule) alternating in one process on the full-width UNet with seeded weights, an adapter made from it
(from_unet: init_random_ weights at the XL widths) and a ControlNet as tools/controlnet_time.py makes its: two warm-up denoises per case,
then REPS timed ones; the median and the spread are printed with the shader clock sampled while they ran, and written to OUT.  The
"plain" arm is the plan of an engine without an adapter: the baseline.  Also reported: the first-call time of the adapter's per-image
state (its 29 launches, weight packing included), of a repeat with another image (packed weights cached), and the launch counts.
python tools/t2i_adapter_time.py [reps=7] [out=profiles/t2i_adapter_timing.json]"""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, '.')
import bench
from imagharmony_amd.attention_processor import CNAttnProcessor2_0
from imagharmony_amd.controlnet import ControlNetModel
from imagharmony_amd.denoise import DenoiseEngine
from imagharmony_amd.schedulers import DDIMScheduler
from imagharmony_amd.t2i_adapter import T2IAdapter

DEV = torch.device("cuda:0")
STEPS, H = 30, 128
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join("profiles", "t2i_adapter_timing.json")

u = bench.build_unet(DEV, torch.bfloat16, 4)
ad = T2IAdapter.from_unet(u)
cn = ControlNetModel.from_unet(u)
g = torch.Generator(device=DEV).manual_seed(99)
with torch.no_grad():
    for conv in cn.zero_convs():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g, device=DEV) * (conv.weight[0].numel() ** -0.5) * 0.1)
cn.set_attn_processor(CNAttnProcessor2_0(num_tokens=4))
pe, ne, po, no = [t.to(DEV) for t in bench.synthetic_conditioning(4)]
lat = torch.randn(1, 4, H, H, generator=torch.Generator().manual_seed(0))
img = torch.rand(1, 3, 8 * H, 8 * H, generator=torch.Generator().manual_seed(1))
img2 = torch.rand(1, 3, 8 * H, 8 * H, generator=torch.Generator().manual_seed(2))
sch = DDIMScheduler()

e = DenoiseEngine(u, DEV, torch.bfloat16)
e.set_conditioning(pe, ne, po, no, 8 * H, 8 * H, guidance_scale=5.0)
e.set_adapter(ad)
setup = {}
for key, im in (("first_call", img2), ("second_image", img)):
    torch.cuda.synchronize()
    t = time.perf_counter()
    e.set_adapter_image(im, conditioning_scale=1.0)
    torch.cuda.synchronize()
    setup[key] = (time.perf_counter() - t) * 1e3
e.set_adapter(None)
e.set_controlnet(cn)
e.set_control_image(img, conditioning_scale=1.0)
e.set_controlnet(None)
plans = {}


def one(name):
    e.set_controlnet(None)
    e.set_adapter(None)
    if name == "adapter":
        e.set_adapter(ad)
    elif name == "controlnet":
        e.set_controlnet(cn)
    e.set_schedule(sch, STEPS)
    torch.cuda.synchronize()
    t = time.perf_counter()
    e.denoise(lat)
    torch.cuda.synchronize()
    plans[name] = e.plan
    return (time.perf_counter() - t) * 1e3 / STEPS


names = ("plain", "adapter", "controlnet")
for name in names:
    one(name); one(name)
clk = bench.ClockSampler(period=0.5)
ms = {name: [] for name in names}
for _ in range(reps):
    for name in names:                       # alternating: drift of the box hits the three plans alike
        ms[name].append(one(name))
clocks = clk.stop()
out = {"steps": STEPS, "reps": reps, "latent": [H, H], "unet_batch": 2, "dtype": "bfloat16", "sclk_mhz": clocks and clocks["sclk_mhz"],
       "ms_per_step": {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in ms.items()},
       "launches_per_step": {k: p.lib.imh_plan_size(p.plan) for k, p in plans.items()},
       "adapter_launches_per_image": 29, "adapter_image_setup_ms": setup}
print(json.dumps(out))
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as f:
    json.dump(out, f, indent=1, sort_keys=True)
