"""What a LoRA costs on the full-width SDXL UNet (seeded weights, bf16), every arm alternating in one process: two warm-ups per arm, then REPS
timed repetitions; medians and min-max are printed with the shader clock sampled while they ran, and written to OUT.
(a) a weight change: ``set_adapters`` end to end (the strengths' copy, the grouped merge launch, the version bumps; host clock around a device
    synchronise) and the merge launch alone (device events), for a synthetic adapter over every attention, feed-forward and proj_in / proj_out
    Linear at rank 16 and at rank 64 -- against a torch arm on the same GPU: per module ``addmm`` in fp32 from the same snapshot, then a cast.
(b) per-step time and launch count of a 1024^2, 30-step DDIM, batch-2 denoise with the rank-64 adapter merged and with it disabled.
(c) the time from the switch (enable_lora / disable_lora) to the end of the first replayed step: the merge, set_conditioning (K / V caches from
    the new weights), the re-pack of every derived weight copy and the re-record of the plan.  The XCD cell pick is made once per process and
    shape (denoise._XCD_PICK) and falls into the warm-up.
python tools/lora_time.py [reps=7] [out=profiles/lora_timing.json]"""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, '.')
import bench
from imagharmony_amd import lora
from imagharmony_amd.denoise import DenoiseEngine
from imagharmony_amd.schedulers import DDIMScheduler

DEV = torch.device("cuda:0")
STEPS, H = 30, 128
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join("profiles", "lora_timing.json")
stat = lambda v: {"median": statistics.median(v), "min": min(v), "max": max(v)}      # noqa: E731

u = bench.build_unet(DEV, torch.bfloat16, 4)
select = lambda n: lora.ATTN_FF_PROJ.search(n) is not None                           # noqa: E731


def host_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def torch_merge(st):
    """the comparison arm: what the merge computes, module by module, with torch ops from the same snapshots and factors"""
    ws = st._weights()
    for mod, cols in st.layout:
        if not cols:
            ws[mod].copy_(st.snap[mod])
            continue
        U, D = st.U[mod], st.D[mod]
        g = st.g_dev[cols[0][3]:cols[0][3] + U.shape[1]]
        ws[mod].view(U.shape[0], -1).copy_(torch.addmm(st.snap[mod].view(U.shape[0], -1).float(), U * g[None, :], D))


def merge_only(st):
    import ctypes as C
    from imagharmony_amd import lib as L
    a = L.LoraMergeArgs()
    a.items_host, a.items_dev, a.tile_start_dev = C.addressof(st.items), st.items_dev.data_ptr(), st.prefix_dev.data_ptr()
    a.n_items, a.total_tiles, a.dtype = len(st.layout), st.total_tiles, L.IMH_DT_BF16
    L.check(L.load().imh_lora_merge(C.byref(a), torch.cuda.current_stream(DEV).cuda_stream), "imh_lora_merge")


merge = {}
with torch.no_grad():
    for rank in (16, 64):
        t_load = host_ms(lambda: u.load_lora_weights(lora.synthetic_adapter(u, rank=rank, seed=rank, select=select), adapter_name=f"r{rank}"))
        st = u._lora
        wts = iter(0.3 + 0.01 * i for i in range(1000))
        arms = {"set_adapters": lambda: host_ms(lambda: u.set_adapters([f"r{rank}"], [next(wts)])),
                "merge_launch": lambda: event_ms(lambda: merge_only(st)),
                "torch_addmm_cast": lambda: host_ms(lambda: torch_merge(st))}
        for fn in arms.values():
            fn(); fn()
        clk = bench.ClockSampler(period=0.5)
        ms = {k: [] for k in arms}
        for _ in range(reps):
            for k, fn in arms.items():
                ms[k].append(fn())
        clocks = clk.stop()
        params = sum(st.snap[m].numel() for m, _ in st.layout)
        merge[f"rank{rank}"] = {"modules": len(st.layout), "weight_elements": params, "total_tiles": st.total_tiles, "load_ms": t_load,
                                "gflop": 2e-9 * rank * params, "weight_bytes_read_and_written": 4 * params,
                                "ms": {k: stat(v) for k, v in ms.items()}, "sclk_mhz": clocks and clocks["sclk_mhz"]}
        if rank == 16:
            u.delete_adapters("r16")
    u.set_adapters(["r64"], [1.0])

pe, ne, po, no = [t.to(DEV) for t in bench.synthetic_conditioning(4)]
lat = torch.randn(1, 4, H, H, generator=torch.Generator().manual_seed(0))
sch = DDIMScheduler()
e = DenoiseEngine(u, DEV, torch.bfloat16)
plans, first = {}, {}


def one(name):
    """-> (ms from the switch to the end of the first replayed step, ms per step of a second, whole denoise)"""
    seen = []
    torch.cuda.synchronize()
    t = time.perf_counter()
    (u.enable_lora if name == "lora_r64" else u.disable_lora)()
    e.set_conditioning(pe, ne, po, no, 8 * H, 8 * H, guidance_scale=5.0)
    e.set_schedule(sch, STEPS)
    e.denoise(lat, callback=lambda i, ts, x: seen.append(time.perf_counter()), callback_steps=10 * STEPS)      # (the callback follows a synchronise)
    to_first = (seen[0] - t) * 1e3
    per_step = host_ms(lambda: e.denoise(lat)) / STEPS
    plans[name] = [e.plan.lib.imh_plan_get_kind(e.plan.plan, i) for i in range(e.plan.lib.imh_plan_size(e.plan.plan))]
    return to_first, per_step


names = ("plain", "lora_r64")
for name in names:
    one(name); one(name)
clk = bench.ClockSampler(period=0.5)
ms = {name: [] for name in names}
tf = {name: [] for name in names}
for _ in range(reps):
    for name in names:
        a, b = one(name)
        tf[name].append(a); ms[name].append(b)
clocks = clk.stop()
out = {"reps": reps, "warmups": 2, "dtype": "bfloat16", "merge": merge,
       "denoise": {"steps": STEPS, "latent": [H, H], "unet_batch": 2, "sclk_mhz": clocks and clocks["sclk_mhz"],
                   "ms_per_step": {k: stat(v) for k, v in ms.items()}, "launches_per_step": {k: len(v) for k, v in plans.items()},
                   "plans_identical": plans["plain"] == plans["lora_r64"],
                   "switch_to_first_step_ms": {k: stat(v) for k, v in tf.items()}}}
print(json.dumps(out))
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as f:
    json.dump(out, f, indent=1, sort_keys=True)
