"""Regional image prompts: "this reference image for the left half, that one for the right half".  Every region is an image prompt of its
own (its own CLIP embedding, its own harmony-aware correction, its own softmax in the cross-attention) that applies where its mask says,
with a weight -- diffusers' ip_adapter_masks with several images per adapter, here one fused launch per active layer and step.  Real
checkpoints are optional: without them every model is seeded random, which exercises the whole path (masks in -> per-grid mask rows once ->
the UNet with N masked image prompts per step in one replayed graph -> VAE tiled decode -> PIL out) but of course produces noise, not a
picture.

    python examples/regional_prompts.py --out out.png [--left left.png --right right.png --clip clip_vision_dir]
                                        [--unet unet.safetensors] [--vae vae.safetensors] [--ip-ckpt ip_adapter.bin]
                                        [--weights 1.0 1.0] [--soft] [--steps 30] [--seed 0] [--size 1024]
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
from imagharmony_amd.pipeline import StableDiffusionXLCustomPipeline      # noqa: E402
from imagharmony_amd.schedulers import DDIMScheduler                      # noqa: E402
from imagharmony_amd.unet import UNet2DConditionModel, UNetConfig         # noqa: E402
from imagharmony_amd.vae import AutoencoderKL                             # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="out.png")
    ap.add_argument("--left"); ap.add_argument("--right")
    ap.add_argument("--clip", help="a CLIP vision model directory (with --left / --right); without it stand-in embeddings are used")
    ap.add_argument("--unet"); ap.add_argument("--vae"); ap.add_argument("--ip-ckpt")
    ap.add_argument("--weights", type=float, nargs=2, default=(1.0, 1.0))
    ap.add_argument("--soft", action="store_true", help="keep the masks' soft edge instead of binarising at 0.5")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--size", type=int, default=1024, help="a multiple of 32")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--guidance", type=float, default=5.0)
    a = ap.parse_args()
    if a.size % 32:
        ap.error("--size must be a multiple of 32")
    dev, dtype = torch.device("cuda:0"), torch.bfloat16
    cfg = UNetConfig()
    if a.unet:
        unet = UNet2DConditionModel.from_safetensors(a.unet, cfg).to(dev, dtype)
    else:
        with torch.device(dev):                                            # 2.6 B parameters: create them on the GPU
            unet = UNet2DConditionModel(cfg)
        unet = unet.init_random_(1234).to(dtype)
    vae = AutoencoderKL.from_safetensors(a.vae, device=dev, dtype=dtype) if a.vae else AutoencoderKL().init_random_(1).to(dev, dtype)
    pipe = StableDiffusionXLCustomPipeline(unet, scheduler=DDIMScheduler(), device=dev, dtype=dtype, vae=vae)
    pipe.enable_vae_tiling()
    ha = HarmonyAttention(image_hidden_size=1280, text_context_dim=2048, inter_dim=2560, cross_heads=8, reshape_blocks=8,
                          cross_value_dim=64, scale=1.0, fusion_method="cross_attention")
    ip = IPAdapterXL(pipe, a.clip, a.ip_ckpt, dev, num_tokens=4, inference=True, number_class_crossattention=ha, dtype=dtype)

    # the two masks: the left and the right half, with a soft edge a tenth of the picture wide (binarised unless --soft)
    ramp = np.clip((0.55 - np.linspace(0.0, 1.0, a.size)) / 0.1, 0.0, 1.0)
    left = Image.fromarray((np.tile(ramp, (a.size, 1)) * 255).astype("uint8"))
    right = Image.fromarray((np.tile(1.0 - ramp, (a.size, 1)) * 255).astype("uint8"))
    # encoders are outside the path (no tokenizer vocabulary / CLIP weights offline): stand-in embeddings of the right shape
    g = torch.Generator().manual_seed(0)
    prompt = (torch.randn(1, 77, 2048, generator=g), torch.randn(1, 77, 2048, generator=g), torch.randn(1, 1280, generator=g), torch.randn(1, 1280, generator=g))
    regions = []
    for path, mask, w in ((a.left, left, a.weights[0]), (a.right, right, a.weights[1])):
        r = dict(mask=mask, weight=w, extra_prompt_embeds=torch.randn(1, 77, 2048, generator=g))
        if path and a.clip:
            r["pil_image"] = Image.open(path).convert("RGB")
        else:
            r["clip_image_embeds"] = torch.randn(1, 1280, generator=g)
        regions.append(r)
    images = ip.generate_regions(regions, prompt_embeds=prompt, scale=a.scale, num_samples=1, seed=a.seed, num_inference_steps=a.steps,
                                 guidance_scale=a.guidance, height=a.size, width=a.size, binarize=not a.soft)
    images[0].save(a.out)
    print(f"generated; seed {a.seed}: {len(images)} image(s) {images[0].size} under {len(regions)} regional image prompts, weights {list(a.weights)}; wrote {a.out}")


if __name__ == "__main__":
    main()
