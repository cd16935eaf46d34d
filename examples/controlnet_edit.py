"""Layout control on the MI355X path: an SDXL ControlNet steers the IP-Adapter generation with a control image (edges, depth, pose --
whatever the ControlNet checkpoint was trained on).  Real checkpoints are optional -- without them every model is seeded random (the
ControlNet is made from the UNet, its zero convs filled so that the branch is not a no-op), which exercises the whole path (PIL control
image in -> hint tower once -> ControlNet branch + UNet per step in one replayed graph -> VAE tiled decode -> PIL out) but of course
produces noise, not a picture.

    python examples/controlnet_edit.py --out out.png [--control control.png] [--unet unet.safetensors] [--controlnet controlnet.safetensors]
                                       [--vae vae.safetensors] [--ip-ckpt ip_adapter.bin] [--cn-scale 0.7] [--cn-start 0.0] [--cn-end 1.0]
                                       [--steps 30] [--seed 0] [--size 1024] [--samples 1]
"""
import argparse
import os
import sys

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imagharmony_amd.controlnet import ControlNetModel                    # noqa: E402
from imagharmony_amd.ip_adapter import IPAdapterXL                        # noqa: E402
from imagharmony_amd.modules import HarmonyAttention                      # noqa: E402
from imagharmony_amd.pipeline import StableDiffusionXLControlNetCustomPipeline   # noqa: E402
from imagharmony_amd.schedulers import DDIMScheduler                      # noqa: E402
from imagharmony_amd.unet import UNet2DConditionModel, UNetConfig         # noqa: E402
from imagharmony_amd.vae import AutoencoderKL                             # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="out.png")
    ap.add_argument("--control")
    ap.add_argument("--unet"); ap.add_argument("--controlnet"); ap.add_argument("--vae"); ap.add_argument("--ip-ckpt")
    ap.add_argument("--cn-scale", type=float, default=0.7)
    ap.add_argument("--cn-start", type=float, default=0.0)
    ap.add_argument("--cn-end", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--samples", type=int, default=1)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--guidance", type=float, default=5.0)
    a = ap.parse_args()
    dev, dtype = torch.device("cuda:0"), torch.bfloat16
    cfg = UNetConfig()
    if a.unet:
        unet = UNet2DConditionModel.from_safetensors(a.unet, cfg).to(dev, dtype)
    else:
        with torch.device(dev):                                            # 2.6 B parameters: create them on the GPU
            unet = UNet2DConditionModel(cfg)
        unet = unet.init_random_(1234).to(dtype)
    if a.controlnet:
        cn = ControlNetModel.from_safetensors(a.controlnet, cfg).to(dev, dtype)
    else:
        cn = ControlNetModel.from_unet(unet)                               # upstream's recipe: the UNet's encoder, zero convs at zero ...
        g = torch.Generator().manual_seed(7)
        with torch.no_grad():                                              # ... which would add nothing: give them small weights
            for conv in cn.zero_convs():
                conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * 0.1 * conv.weight[0].numel() ** -0.5)
    vae = AutoencoderKL.from_safetensors(a.vae, device=dev, dtype=dtype) if a.vae else AutoencoderKL().init_random_(1).to(dev, dtype)
    pipe = StableDiffusionXLControlNetCustomPipeline(unet, cn, scheduler=DDIMScheduler(), device=dev, dtype=dtype, vae=vae)
    pipe.enable_vae_tiling()
    ha = HarmonyAttention(image_hidden_size=1280, text_context_dim=2048, inter_dim=2560, cross_heads=8, reshape_blocks=8,
                          cross_value_dim=64, scale=1.0, fusion_method="cross_attention")
    # the adapter installs its IP processors on the UNet and CNAttnProcessor2_0 on pipe.controlnet (text tokens only there)
    ip = IPAdapterXL(pipe, None, a.ip_ckpt, dev, num_tokens=4, inference=True, number_class_crossattention=ha, dtype=dtype)

    if a.control:
        control = Image.open(a.control).convert("RGB")                     # resized to the output size by the pipeline, not normalised
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
    images = ip.generate(clip_image_embeds=clip_embeds, prompt_embeds=prompt, extra_prompt_embeds=extra, scale=a.scale, num_samples=n,
                         seed=a.seed, num_inference_steps=a.steps, guidance_scale=a.guidance, height=a.size, width=a.size,
                         image=control, controlnet_conditioning_scale=a.cn_scale, controlnet_guidance_start=a.cn_start,
                         controlnet_guidance_end=a.cn_end)
    images[0].save(a.out)
    print(f"generated {len(images)} image(s) {images[0].size} under a ControlNet at scale {a.cn_scale}, window [{a.cn_start}, {a.cn_end}], "
          f"seed {a.seed}; wrote {a.out}")


if __name__ == "__main__":
    main()
