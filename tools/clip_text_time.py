"""Time of one CLIP text forward, the HIP encoder (imagharmony_amd.clip_text.CLIPTextEncoder) against the stock transformers module on
the same GPU, in the same dtype, with seeded random weights and random token ids: both towers of SDXL (CLIP-L, 12 layers, as
CLIPTextModel; OpenCLIP bigG, 32 layers, as CLIPTextModelWithProjection) at B = 1 and B = 2 (one prompt; prompt + negative prompt),
77 tokens, output_hidden_states=True as SDXLPromptEncoder calls them.  Every measurement is a FRESH child process under its own time
limit (the arms alternate, so drift of the box hits both alike); a child warms up, then times REPS forwards one by one with a device
synchronisation around each and prints its median.  The first child that fails stops the run: nothing more is started on the GPU.
python tools/clip_text_time.py [rounds=3] [reps=20] [dtype=bf16] [out=profiles/clip_text_timing.json]"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TOWERS = {"clip_l": dict(hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12, projection_dim=768,
                         hidden_act="quick_gelu"),
          "open_clip_bigg": dict(hidden_size=1280, intermediate_size=5120, num_hidden_layers=32, num_attention_heads=20, projection_dim=1280,
                                 hidden_act="gelu")}
CHILD_TIMEOUT_S = 240


def child(arm, tower, B, reps, dtype_name):
    import torch
    from transformers import CLIPTextConfig, CLIPTextModel, CLIPTextModelWithProjection
    dev, dtype = torch.device("cuda:0"), {"bf16": torch.bfloat16, "fp16": torch.float16}[dtype_name]
    torch.manual_seed(0)
    cfg = CLIPTextConfig(vocab_size=49408, max_position_embeddings=77, bos_token_id=49406, eos_token_id=2, pad_token_id=1, **TOWERS[tower])
    with torch.no_grad():
        m = (CLIPTextModel if tower == "clip_l" else CLIPTextModelWithProjection)(cfg).eval().to(dev, dtype)
        if arm == "hip":
            from imagharmony_amd.clip_text import CLIPTextEncoder
            m = CLIPTextEncoder.from_hf(m)
        ids = torch.randint(3, 40000, (B, 77), generator=torch.Generator().manual_seed(1))
        ids[:, 0], ids[:, 20:] = 49406, 49407
        ids = ids.to(dev)
        for _ in range(3):
            m(ids, output_hidden_states=True)[0]
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            t = time.perf_counter()
            m(ids, output_hidden_states=True)[0]
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t) * 1e3)
    print(json.dumps({"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}))


def run_child(args):
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + [str(a) for a in args], capture_output=True, text=True,
                           timeout=CHILD_TIMEOUT_S, cwd=ROOT)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"child {args} ran past {CHILD_TIMEOUT_S} s")                    # stop: start nothing more on the GPU
    if r.returncode != 0:
        raise SystemExit(f"child {args} failed ({r.returncode}):\n{r.stderr[-2000:]}")     # likewise
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    dtype = sys.argv[3] if len(sys.argv) > 3 else "bf16"
    path = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "clip_text_timing.json")
    out = {"dtype": dtype, "rounds": rounds, "reps_per_process": reps, "tokens": 77, "forward_ms": {}}
    for tower in TOWERS:
        for B in (1, 2):
            runs = {"hip": [], "transformers": []}
            for _ in range(rounds):
                for arm in runs:                                  # alternating fresh processes
                    runs[arm].append(run_child([arm, tower, B, reps, dtype])["median_ms"])
            e = {arm: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "runs_ms": v} for arm, v in runs.items()}
            e["spread_ms"] = max(e[a]["max_ms"] - e[a]["min_ms"] for a in runs)
            e["hip_minus_transformers_ms"] = e["hip"]["median_ms"] - e["transformers"]["median_ms"]
            out["forward_ms"][f"{tower}_B{B}"] = e
            print(tower, B, json.dumps(e), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("wrote", path)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5]), sys.argv[6])
    else:
        main()
