"""Inpainting on the MI355X path: keep the scene, repaint what the mask covers.  Real checkpoints are optional -- without them
every model is seeded random, which exercises the whole path (PIL image and mask in -> VAE encode -> masked denoise ->
VAE tiled decode -> PIL out) but of course produces noise inside the mask, not a picture.  The mode follows the UNet: --in-channels
4 (SDXL base: the region outside the mask is put back after every step) or 9 (the SDXL inpainting UNet: conv_in reads the mask
and the masked image's latents).

    python examples/inpaint_edit.py --out out.png [--image in.png] [--mask mask.png] [--unet unet.safetensors] [--vae vae.safetensors]
                                    [--ip-ckpt ip_adapter.bin] [--in-channels 4] [--strength 0.9999] [--steps 30] [--seed 0] [--size 1024]
                                    [--seeds 0 1 2 3 --preview-steps 10]

With --seeds the edit runs preference-guided noise selection over them (IPAdapterXL.generate_pns(image=, mask_image=)): every seed gets a
short preview edit, the judged-best one the full edit; seed s stands for the draws of torch.Generator("cpu").manual_seed(s).
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
from imagharmony_amd.pipeline import StableDiffusionXLInpaintCustomPipeline   # noqa: E402
from imagharmony_amd.schedulers import DDIMScheduler                      # noqa: E402
from imagharmony_amd.unet import UNet2DConditionModel, UNetConfig         # noqa: E402
from imagharmony_amd.vae import AutoencoderKL                             # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="out.png")
    ap.add_argument("--image"); ap.add_argument("--mask")
    ap.add_argument("--unet"); ap.add_argument("--vae"); ap.add_argument("--ip-ckpt")
    ap.add_argument("--in-channels", type=int, default=4, choices=(4, 9))
    ap.add_argument("--strength", type=float, default=0.9999)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--seeds", type=int, nargs="+", help="several candidate seeds: noise selection (PNS) over them instead of the one --seed")
    ap.add_argument("--preview-steps", type=int, default=10)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--guidance", type=float, default=5.0)
    a = ap.parse_args()
    dev, dtype = torch.device("cuda:0"), torch.bfloat16
    cfg = UNetConfig(in_channels=a.in_channels)
    if a.unet:
        unet = UNet2DConditionModel.from_safetensors(a.unet, cfg).to(dev, dtype)
    else:
        with torch.device(dev):                                            # 2.6 B parameters: create them on the GPU
            unet = UNet2DConditionModel(cfg)
        unet = unet.init_random_(1234).to(dtype)
    vae = AutoencoderKL.from_safetensors(a.vae, device=dev, dtype=dtype, with_encoder=True) if a.vae \
        else AutoencoderKL(with_encoder=True).init_random_(1).to(dev, dtype)
    pipe = StableDiffusionXLInpaintCustomPipeline(unet, scheduler=DDIMScheduler(), device=dev, dtype=dtype, vae=vae)
    pipe.enable_vae_tiling()
    ha = HarmonyAttention(image_hidden_size=1280, text_context_dim=2048, inter_dim=2560, cross_heads=8, reshape_blocks=8,
                          cross_value_dim=64, scale=1.0, fusion_method="cross_attention")
    ip = IPAdapterXL(pipe, None, a.ip_ckpt, dev, num_tokens=4, inference=True, number_class_crossattention=ha, dtype=dtype)

    rs = np.random.RandomState(0)
    image = Image.open(a.image).convert("RGB").resize((a.size, a.size)) if a.image \
        else Image.fromarray((rs.rand(a.size, a.size, 3) * 255).astype("uint8"))
    if a.mask:
        mask = Image.open(a.mask)
    else:                                                                  # repaint the centre, keep the border
        m = np.zeros((a.size, a.size), "uint8")
        m[a.size // 4:3 * a.size // 4, a.size // 4:3 * a.size // 4] = 255
        mask = Image.fromarray(m, mode="L")
    # encoders are outside the path (no tokenizer vocabulary / CLIP weights offline): stand-in embeddings of the right shape
    g = torch.Generator().manual_seed(0)
    clip_embeds = torch.randn(1, 1280, generator=g)
    prompt = (torch.randn(1, 77, 2048, generator=g), torch.randn(1, 77, 2048, generator=g),
              torch.randn(1, 1280, generator=g), torch.randn(1, 1280, generator=g))
    extra = torch.randn(1, 77, 2048, generator=g)
    if a.seeds:
        r = ip.generate_pns(a.seeds, clip_image_embeds=clip_embeds, prompt_embeds=prompt, extra_prompt_embeds=extra, scale=a.scale,
                            preview_steps=a.preview_steps, num_inference_steps=a.steps, guidance_scale=a.guidance, image=image, mask_image=mask,
                            strength=a.strength)
        r["images"][0].save(a.out)
        print(f"inpainted {r['images'][0].size} with in_channels={a.in_channels}, strength {a.strength}; seeds {a.seeds} -> scores "
              f"{[round(float(s), 4) for s in r['scores']]}, best seed {r['best_seed']}; wrote {a.out}")
        return
    out = ip.generate(clip_image_embeds=clip_embeds, prompt_embeds=prompt, extra_prompt_embeds=extra, scale=a.scale, num_samples=1,
                      seed=a.seed, num_inference_steps=a.steps, guidance_scale=a.guidance, image=image, mask_image=mask,
                      strength=a.strength)[0]
    out.save(a.out)
    print(f"inpainted {out.size} with in_channels={a.in_channels}, strength {a.strength}, seed {a.seed}; wrote {a.out}")


if __name__ == "__main__":
    main()
