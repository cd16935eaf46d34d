"""Time of the PNS judge from decoded images to scores, with its preprocessing as the chain of torch ops
(ClipPreferenceJudge(preprocess_backend="torch"): scale, clamp, antialiased bicubic, clamp, crop, mean / std, cast, im2col copy, then the
HIP tower's forward) against one imh_clip_preprocess launch into the tower's patch buffer (preprocess_backend="hip":
CLIPVisionEncoder.embed_decoded).  Same tower (ViT-H/14, seeded random weights, bf16), same 1024 x 1024 fp32 images, S = 1 and S = 8 (the
judge's shape in two-stage PNS).  Every measurement is a FRESH child process and the arms alternate, so drift of the box hits both alike; a
child runs two warm-up calls, then times seven calls one by one with a device synchronisation around each, and samples the shader clock
while they and two more seconds of the same call run.  A number, not a gate: "torch" stays the default whatever this prints.
python tools/clip_judge_time.py [rounds=3]   ->  profiles/clip_judge_timing.json"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
VIT_H = dict(hidden_size=1280, intermediate_size=5120, num_hidden_layers=32, num_attention_heads=16, projection_dim=1024)
WARM, REPS = 2, 7


def child(arm, S):
    import torch
    import bench
    from imagharmony_amd import pns
    from imagharmony_amd.clip_vision import CLIPVisionEncoder, CLIPVisionEncoderConfig
    dev, dtype = torch.device("cuda:0"), torch.bfloat16
    torch.manual_seed(0)
    with torch.device(dev):
        enc = CLIPVisionEncoder(CLIPVisionEncoderConfig(**VIT_H))
    with torch.no_grad():
        for p in enc.parameters():
            if p.dim() > 1:
                p.normal_(0, 0.02)
    enc = enc.to(dtype)
    images = (torch.rand(S, 3, 1024, 1024, device=dev) * 2.2 - 1.1).contiguous()          # "decoded" images, a little beyond [-1, 1]
    target = torch.randn(1, VIT_H["projection_dim"], device=dev)
    judge = pns.ClipPreferenceJudge(lambda z: z, enc, target, preprocess_backend=arm)
    for _ in range(WARM):
        judge(images)
    torch.cuda.synchronize()
    clk = bench.ClockSampler(period=0.2)
    ms = []
    for _ in range(REPS):
        t = time.perf_counter()
        s = judge(images)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3)
    # seven calls last a fraction of a second and one rocm-smi sample takes about as long: keep the same call running (untimed) until
    # the sampler has had two seconds of it, so that the clock reported is the clock under this very workload
    t_end = time.perf_counter() + 2.0
    while time.perf_counter() < t_end:
        judge(images)
        torch.cuda.synchronize()
    clocks = clk.stop()
    print(json.dumps({"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "runs_ms": ms,
                      "sclk_mhz": clocks and clocks["sclk_mhz"], "sclk_samples": clocks and clocks["samples"], "scores": [float(v) for v in s]}))


def run_child(args):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + [str(a) for a in args], capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    if r.returncode != 0:
        raise SystemExit(f"child {args} failed ({r.returncode}):\n{r.stderr[-2000:]}")     # stop: start nothing more on the GPU
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    out = {"tower": "vit_h", "dtype": "bf16", "image": "1024x1024 fp32", "rounds": rounds, "warmups": WARM, "reps_per_process": REPS, "judge_ms": {}}
    for S in (1, 8):
        runs = {"torch": [], "hip": []}
        for _ in range(rounds):
            for arm in runs:                                      # alternating fresh processes
                runs[arm].append(run_child([arm, S]))
        e = {}
        for arm, v in runs.items():
            every = [m for r in v for m in r["runs_ms"]]
            clk = [r["sclk_mhz"] for r in v if r["sclk_mhz"]]
            e[arm] = {"median_ms": statistics.median(r["median_ms"] for r in v), "min_ms": min(every), "max_ms": max(every),
                      "process_medians_ms": [r["median_ms"] for r in v], "sclk_mhz": statistics.mean(clk) if clk else None}
        e["score_diff_max"] = max(abs(a - b) for a, b in zip(runs["torch"][0]["scores"], runs["hip"][0]["scores"]))
        e["ranges_overlap"] = not (e["hip"]["max_ms"] < e["torch"]["min_ms"] or e["torch"]["max_ms"] < e["hip"]["min_ms"])
        e["hip_minus_torch_ms"] = e["hip"]["median_ms"] - e["torch"]["median_ms"]
        out["judge_ms"][f"S{S}"] = e
        print(S, json.dumps(e), flush=True)
    path = os.path.join(ROOT, "profiles", "clip_judge_timing.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("wrote", path)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], int(sys.argv[3]))
    else:
        main()
