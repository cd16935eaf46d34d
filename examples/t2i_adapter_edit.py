"""Layout control at four launches a step: an SDXL T2I-Adapter steers the IP-Adapter generation with a control image (edges, depth,
sketch, pose -- whatever the adapter checkpoint was trained on).  The adapter is a small conv net that reads the control image alone: it
runs once per image, and its four feature maps are added to the UNet's down path at every step.  Real checkpoints are optional -- without
them every model is seeded random, which exercises the whole path (PIL control image in -> the adapter's features once -> the UNet with
four gated adds per step in one replayed graph -> VAE tiled decode -> PIL out) but of course produces noise, not a picture.

--seeds s1 s2 ... runs preference-guided noise selection over those candidate seeds (a short preview each, the judged-best one in
full); one control image serves every candidate, and the winner is the pipe's own call with that seed's generator.

    python examples/t2i_adapter_edit.py --out out.png [--control control.png] [--unet unet.safetensors] [--adapter adapter.safetensors]
                                        [--vae vae.safetensors] [--ip-ckpt ip_adapter.bin] [--adapter-scale 0.8] [--adapter-factor 1.0]
                                        [--steps 30] [--seed 0] [--size 1024] [--samples 1] [--seeds 1 2 3 [--preview-steps 10]]
"""
import argparse
import os
import sys

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imagharmony_amd.ip_adapter import IPAdapterXL                        # noqa: E402
from imagharmony_amd.modules import HarmonyAttention                      # noqa: E402
from imagharmony_amd.pipeline import StableDiffusionXLAdapterCustomPipeline   # noqa: E402
from imagharmony_amd.schedulers import DDIMScheduler                      # noqa: E402
from imagharmony_amd.t2i_adapter import T2IAdapter                        # noqa: E402
from imagharmony_amd.unet import UNet2DConditionModel, UNetConfig         # noqa: E402
from imagharmony_amd.vae import AutoencoderKL                             # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="out.png")
    ap.add_argument("--control")
    ap.add_argument("--unet"); ap.add_argument("--adapter"); ap.add_argument("--vae"); ap.add_argument("--ip-ckpt")
    ap.add_argument("--adapter-scale", type=float, default=0.8)
    ap.add_argument("--adapter-factor", type=float, default=1.0, help="fraction of the steps, from the first, that get the features")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--samples", type=int, default=1)
    ap.add_argument("--size", type=int, default=1024, help="a multiple of 32")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--guidance", type=float, default=5.0)
    ap.add_argument("--seeds", type=int, nargs="+", help="preference-guided noise selection over these candidate seeds (instead of --seed)")
    ap.add_argument("--preview-steps", type=int, default=10, help="with --seeds: steps of every candidate's preview")
    a = ap.parse_args()
    if a.size % 32:
        ap.error("--size must be a multiple of 32 (2 x the adapter's downscale factor)")
    dev, dtype = torch.device("cuda:0"), torch.bfloat16
    cfg = UNetConfig()
    if a.unet:
        unet = UNet2DConditionModel.from_safetensors(a.unet, cfg).to(dev, dtype)
    else:
        with torch.device(dev):                                            # 2.6 B parameters: create them on the GPU
            unet = UNet2DConditionModel(cfg)
        unet = unet.init_random_(1234).to(dtype)
    adapter = T2IAdapter.from_safetensors(a.adapter, device=dev, dtype=dtype) if a.adapter else T2IAdapter.from_unet(unet, seed=7)
    vae = AutoencoderKL.from_safetensors(a.vae, device=dev, dtype=dtype) if a.vae else AutoencoderKL().init_random_(1).to(dev, dtype)
    pipe = StableDiffusionXLAdapterCustomPipeline(unet, adapter, scheduler=DDIMScheduler(), device=dev, dtype=dtype, vae=vae)
    pipe.enable_vae_tiling()
    ha = HarmonyAttention(image_hidden_size=1280, text_context_dim=2048, inter_dim=2560, cross_heads=8, reshape_blocks=8,
                          cross_value_dim=64, scale=1.0, fusion_method="cross_attention")
    ip = IPAdapterXL(pipe, None, a.ip_ckpt, dev, num_tokens=4, inference=True, number_class_crossattention=ha, dtype=dtype)

    if a.control:
        control = Image.open(a.control).convert("RGB").resize((a.size, a.size))     # the adapter's image is not resized by the pipeline
    else:                                                                  # a stand-in layout: a bright box on black
        m = np.zeros((a.size, a.size, 3), "uint8")
        m[a.size // 4:3 * a.size // 4, a.size // 3:2 * a.size // 3] = 255
        control = Image.fromarray(m)
    # encoders are outside the path (no tokenizer vocabulary / CLIP weights offline): stand-in embeddings of the right shape
    g = torch.Generator().manual_seed(0)
    n = a.samples
    clip_embeds = torch.randn(1, 1280, generator=g)
    prompt = tuple(t.repeat(n, *([1] * (t.dim() - 1))) for t in (torch.randn(1, 77, 2048, generator=g), torch.randn(1, 77, 2048, generator=g),
                                                                 torch.randn(1, 1280, generator=g), torch.randn(1, 1280, generator=g)))
    extra = torch.randn(1, 77, 2048, generator=g)
    ad_kw = dict(adapter_conditioning_scale=a.adapter_scale, adapter_conditioning_factor=a.adapter_factor)
    if a.seeds:
        r = ip.generate_pns(a.seeds, clip_image_embeds=clip_embeds, prompt_embeds=tuple(t[:1] for t in prompt), extra_prompt_embeds=extra,
                            scale=a.scale, preview_steps=a.preview_steps, num_inference_steps=a.steps, guidance_scale=a.guidance,
                            adapter_image=control, height=a.size, width=a.size, **ad_kw)
        images = r["images"]
        what = f"seeds {a.seeds} -> scores {[round(float(x), 4) for x in r['scores']]}, best seed {r['best_seed']}"
    else:
        images = ip.generate(clip_image_embeds=clip_embeds, prompt_embeds=prompt, extra_prompt_embeds=extra, scale=a.scale, num_samples=n,
                             seed=a.seed, num_inference_steps=a.steps, guidance_scale=a.guidance, image=control, height=a.size, width=a.size, **ad_kw)
        what = f"seed {a.seed}"
    images[0].save(a.out)
    print(f"generated; {what}: {len(images)} image(s) {images[0].size} under a T2I-Adapter at scale {a.adapter_scale}, factor {a.adapter_factor} "
          f"({adapter.launches} adapter launches in all); wrote {a.out}")


if __name__ == "__main__":
    main()
