"""What a preview decode costs: AutoencoderKL (native 16-bit path and the fp32 path, the reference's rule for an fp16 VAE) against
AutoencoderTiny (csrc/tinyvae.hip) at latent 128^2 (a 1024^2 image), bf16, seeded random weights, S = 1 and S = 8 previews -- the three
arms alternating in one process: two warm-ups per arm, then REPS timed decodes each, host clock around a device synchronise; medians and
min-max with the shader clock sampled while they ran.
Also the 64 -> 64 body launch alone (device events around REPS x 10 launches) at 1024^2 and 512^2 output, with and without UP2, in
microseconds and as a share of its floor: the larger of FLOPs / 2.5 PF (2 x pixels x 64 x 576) and bytes / 8 TB/s (input + output + residual +
weight); which of the two bounds is stated.
python tools/tiny_vae_time.py [reps=7] [out=profiles/tiny_vae_timing.json]"""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, '.')
import bench
from imagharmony_amd import AutoencoderTiny
from imagharmony_amd.ctx import Ctx
from imagharmony_amd.vae import AutoencoderKL, decode_latents

DEV = torch.device("cuda:0")
DT = torch.bfloat16
PEAK_FLOPS, PEAK_BYTES = 2.5e15, 8.0e12
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join("profiles", "tiny_vae_timing.json")
stat = lambda v: {"median": statistics.median(v), "min": min(v), "max": max(v)}      # noqa: E731


def host_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


kl = AutoencoderKL().init_random_(1).to(DEV, DT)
tiny = AutoencoderTiny().init_random_(1).to(DEV, DT)
decode = {}
with torch.no_grad():
    for S in (1, 8):
        lat = (torch.randn(S, 4, 128, 128, generator=torch.Generator().manual_seed(S)) * 0.13025).to(DEV)
        arms = {"autoencoder_kl_native": lambda: decode_latents(kl, lat, precision="native"),
                "autoencoder_kl_fp32": lambda: decode_latents(kl, lat, precision="fp32"),
                "autoencoder_tiny": lambda: decode_latents(tiny, lat)}
        for fn in arms.values():
            host_ms(fn); host_ms(fn)
        clk = bench.ClockSampler(period=0.5)
        ms = {k: [] for k in arms}
        for _ in range(reps):
            for k, fn in arms.items():
                ms[k].append(host_ms(fn))
        clocks = clk.stop()
        st = {k: stat(v) for k, v in ms.items()}
        slowest_tiny, fastest_kl = st["autoencoder_tiny"]["max"], min(st["autoencoder_kl_native"]["min"], st["autoencoder_kl_fp32"]["min"])
        decode[f"S{S}"] = {"latent": [S, 4, 128, 128], "ms": st, "sclk_mhz": clocks and clocks["sclk_mhz"],
                           "ranges_overlap": bool(slowest_tiny >= fastest_kl),
                           "kl_native_over_tiny": st["autoencoder_kl_native"]["median"] / st["autoencoder_tiny"]["median"],
                           "kl_fp32_over_tiny": st["autoencoder_kl_fp32"]["median"] / st["autoencoder_tiny"]["median"]}

# ---- the body launch alone
INNER = 10
body = {}
ctx = Ctx(DEV, DT)
g = torch.Generator().manual_seed(0)
w = (torch.randn(64, 576, generator=g) / 24).to(DEV, DT)
b = (torch.randn(64, generator=g) * 0.05).to(DEV, DT)
with torch.no_grad():
    for out_hw in (1024, 512):
        for up2 in (False, True):
            hw = out_hw // 2 if up2 else out_hw
            x = torch.randn(1, hw, hw, 64, generator=g).to(DEV, DT)
            r = torch.randn(1, out_hw, out_hw, 64, generator=g).to(DEV, DT)

            def launch():
                ctx.free(ctx.tinyvae_conv(x, w, bias=b, residual=r, up2=up2, relu=True))
            for _ in range(2 * INNER):
                launch()
            clk = bench.ClockSampler(period=0.5)
            us = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(INNER):
                    launch()
                e1.record()
                torch.cuda.synchronize()
                us.append(e0.elapsed_time(e1) * 1e3 / INNER)
            clocks = clk.stop()
            flops = 2.0 * out_hw * out_hw * 64 * 576
            nbytes = 2.0 * (x.numel() + 2 * r.numel() + w.numel() + b.numel())
            t_flops, t_bytes = flops / PEAK_FLOPS * 1e6, nbytes / PEAK_BYTES * 1e6
            floor = max(t_flops, t_bytes)
            s = stat(us)
            body[f"{out_hw}{'_up2' if up2 else ''}"] = {
                "input": list(x.shape), "output": list(r.shape), "us": s, "gflop": flops * 1e-9, "mbytes": nbytes * 1e-6,
                "floor_us": floor, "floor_flops_us": t_flops, "floor_bytes_us": t_bytes, "bound_by": "flops" if t_flops >= t_bytes else "bytes",
                "share_of_floor": floor / s["median"], "tflops": flops / s["median"] * 1e-6, "sclk_mhz": clocks and clocks["sclk_mhz"],
                "launches_per_sample": INNER}

out = {"reps": reps, "warmups": 2, "dtype": "bfloat16", "weights": "seeded random", "decode": decode, "body_launch": body,
       "peaks": {"flops": PEAK_FLOPS, "bytes_per_s": PEAK_BYTES}, "tiny_launches_per_decode": 35}
print(json.dumps(out))
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as f:
    json.dump(out, f, indent=1, sort_keys=True)
