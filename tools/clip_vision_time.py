"""Time of one CLIP vision forward, the HIP encoder (imagharmony_amd.clip_vision.CLIPVisionEncoder) against the stock transformers
module on the same GPU, in the same dtype, with seeded random weights and random pixel values: both towers (ViT-H/14, 32 layers;
ViT-bigG/14, 48 layers) at B = 1 and B = 8 (the judge's shape in two-stage PNS).  Every measurement is a FRESH child process (the
arms alternate, so drift of the box hits both alike); a child warms up, then times REPS forwards one by one with a device
synchronisation around each and prints its median.  A last child times imh_attention_enc alone at the two towers' B = 8 shapes and
reports the fraction of the bf16 MFMA peak (2.5 PFLOP/s, as bench.py counts it).
python tools/clip_vision_time.py [rounds=3] [reps=20] [dtype=bf16]   ->  profiles/clip_vision_timing.json"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TOWERS = {"vit_h": dict(hidden_size=1280, intermediate_size=5120, num_hidden_layers=32, num_attention_heads=16, projection_dim=1024),
          "vit_bigg": dict(hidden_size=1664, intermediate_size=8192, num_hidden_layers=48, num_attention_heads=16, projection_dim=1280)}
PEAK_TFLOPS = 2500.0


def child(arm, tower, B, reps, dtype_name):
    import torch
    dev, dtype = torch.device("cuda:0"), {"bf16": torch.bfloat16, "fp16": torch.float16}[dtype_name]
    torch.manual_seed(0)
    if arm == "attn":
        from imagharmony_amd.ctx import Ctx
        ctx, out = Ctx(dev, dtype), {}
        for H, d, L_ in ((16, 80, 257), (16, 104, 257)):
            qkv = torch.randn(B * L_, 3 * H * d, device=dev).to(dtype)
            q, k, v = qkv[:, :H * d], qkv[:, H * d:2 * H * d], qkv[:, 2 * H * d:]
            o = ctx.attention_enc(q, k, v, B, H, L_, d)
            for _ in range(5):
                ctx.attention_enc(q, k, v, B, H, L_, d, out=o)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                ctx.attention_enc(q, k, v, B, H, L_, d, out=o)
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) * 1e3 / reps
            fl = 4.0 * B * H * L_ * L_ * d
            out[f"H{H}_d{d}_L{L_}_B{B}"] = {"us": us, "tflops": fl / us / 1e6, "frac_of_bf16_mfma_peak": fl / us / 1e6 / PEAK_TFLOPS}
        print(json.dumps(out))
        return
    with torch.device(dev):
        if arm == "hip":
            from imagharmony_amd.clip_vision import CLIPVisionEncoder, CLIPVisionEncoderConfig
            m = CLIPVisionEncoder(CLIPVisionEncoderConfig(**TOWERS[tower]))
        else:
            from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
            m = CLIPVisionModelWithProjection(CLIPVisionConfig(hidden_act="gelu", **TOWERS[tower])).eval()
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() > 1:
                p.normal_(0, 0.02)
        m = m.to(dtype)
        px = torch.randn(B, 3, 224, 224, device=dev).to(dtype)
        for _ in range(3):
            m(px).image_embeds
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            t = time.perf_counter()
            m(px).image_embeds
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t) * 1e3)
    print(json.dumps({"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}))


def run_child(args):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + [str(a) for a in args], capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    if r.returncode != 0:
        raise SystemExit(f"child {args} failed ({r.returncode}):\n{r.stderr[-2000:]}")     # stop: start nothing more on the GPU
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    dtype = sys.argv[3] if len(sys.argv) > 3 else "bf16"
    out = {"dtype": dtype, "rounds": rounds, "reps_per_process": reps, "forward_ms": {}}
    for tower in TOWERS:
        for B in (1, 8):
            runs = {"hip": [], "transformers": []}
            for _ in range(rounds):
                for arm in runs:                                  # alternating fresh processes
                    runs[arm].append(run_child([arm, tower, B, reps, dtype])["median_ms"])
            e = {arm: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "runs_ms": v} for arm, v in runs.items()}
            e["spread_ms"] = max(e[a]["max_ms"] - e[a]["min_ms"] for a in runs)
            e["hip_minus_transformers_ms"] = e["hip"]["median_ms"] - e["transformers"]["median_ms"]
            out["forward_ms"][f"{tower}_B{B}"] = e
            print(tower, B, json.dumps(e), flush=True)
    out["attention_enc"] = run_child(["attn", "-", 8, 200, dtype])
    print(json.dumps(out["attention_enc"]), flush=True)
    path = os.path.join(ROOT, "profiles", "clip_vision_timing.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("wrote", path)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5]), sys.argv[6])
    else:
        main()
