"""Layout control on the MI355X path: an SDXL ControlNet steers the IP-Adapter generation with a control image (edges, depth, pose --
whatever the ControlNet checkpoint was trained on).  Real checkpoints are optional -- without them every model is seeded random (the
ControlNet is made from the UNet, its zero convs filled so that the branch is not a no-op), which exercises the whole path (PIL control
image in -> hint tower once -> ControlNet branch + UNet per step in one replayed graph -> VAE tiled decode -> PIL out) but of course
produces noise, not a picture.

Without --init-image: text-to-image under the ControlNet.  With --init-image the control steers an EDIT of that image (image-to-image:
the VAE encoder, then the steps --strength leaves), with --mask as well an inpainting of its white region (the masked blend rides in the
recorded step).  --seeds s1 s2 ... runs preference-guided noise selection over those candidate seeds (a short preview each, the judged-best
one in full) in whichever of the three modes the other arguments select; the winner is the pipe's own call with that seed's generator.

    python examples/controlnet_edit.py --out out.png [--control control.png] [--unet unet.safetensors] [--controlnet controlnet.safetensors]
                                       [--vae vae.safetensors] [--ip-ckpt ip_adapter.bin] [--cn-scale 0.7] [--cn-start 0.0] [--cn-end 1.0]
                                       [--steps 30] [--seed 0] [--size 1024] [--samples 1]
                                       [--init-image init.png [--mask mask.png] [--strength 0.6]] [--seeds 1 2 3 [--preview-steps 10]]
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
from imagharmony_amd.pipeline import (StableDiffusionXLControlNetCustomPipeline, StableDiffusionXLControlNetImg2ImgCustomPipeline,   # noqa: E402
                                      StableDiffusionXLControlNetInpaintCustomPipeline)
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
    ap.add_argument("--init-image", help="edit this image under the ControlNet (image-to-image) instead of generating from noise")
    ap.add_argument("--mask", help="with --init-image: inpaint the white region of this mask, keep the rest of the image")
    ap.add_argument("--strength", type=float, default=0.6, help="with --init-image: how far the edit departs from the image (0 .. 1)")
    ap.add_argument("--seeds", type=int, nargs="+", help="preference-guided noise selection over these candidate seeds (instead of --seed)")
    ap.add_argument("--preview-steps", type=int, default=10, help="with --seeds: steps of every candidate's preview")
    a = ap.parse_args()
    if a.mask and not a.init_image:
        ap.error("--mask needs --init-image")
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
    enc_kw = {"with_encoder": True} if a.init_image else {}                 # an edit encodes its image on the HIP VAE encoder
    vae = AutoencoderKL.from_safetensors(a.vae, device=dev, dtype=dtype, **enc_kw) if a.vae else AutoencoderKL(**enc_kw).init_random_(1).to(dev, dtype)
    pipe_cls = (StableDiffusionXLControlNetInpaintCustomPipeline if a.mask else StableDiffusionXLControlNetImg2ImgCustomPipeline if a.init_image
                else StableDiffusionXLControlNetCustomPipeline)
    pipe = pipe_cls(unet, cn, scheduler=DDIMScheduler(), device=dev, dtype=dtype, vae=vae)
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
    cn_kw = dict(controlnet_conditioning_scale=a.cn_scale, controlnet_guidance_start=a.cn_start, controlnet_guidance_end=a.cn_end)
    # the text-to-image class calls its control image `image`; for an edit `image` is the init image and the control is `control_image`
    if a.init_image:
        init = Image.open(a.init_image).convert("RGB").resize((a.size, a.size))
        call = dict(image=init, strength=a.strength)
        if a.mask:
            call["mask_image"] = Image.open(a.mask).convert("L").resize((a.size, a.size))
        what = f"{'inpainted' if a.mask else 'edited'} {a.init_image} at strength {a.strength}"
    else:
        call = dict(height=a.size, width=a.size)
        what = "generated"
    if a.seeds:
        r = ip.generate_pns(a.seeds, clip_image_embeds=clip_embeds, prompt_embeds=tuple(t[:1] for t in prompt), extra_prompt_embeds=extra,
                            scale=a.scale, preview_steps=a.preview_steps, num_inference_steps=a.steps, guidance_scale=a.guidance,
                            control_image=control, **call, **cn_kw)
        images = r["images"]
        what += f"; seeds {a.seeds} -> scores {[round(float(x), 4) for x in r['scores']]}, best seed {r['best_seed']}"
    else:
        call["control_image" if a.init_image else "image"] = control
        images = ip.generate(clip_image_embeds=clip_embeds, prompt_embeds=prompt, extra_prompt_embeds=extra, scale=a.scale, num_samples=n,
                             seed=a.seed, num_inference_steps=a.steps, guidance_scale=a.guidance, **call, **cn_kw)
        what += f"; seed {a.seed}"
    images[0].save(a.out)
    print(f"{what}: {len(images)} image(s) {images[0].size} under a ControlNet at scale {a.cn_scale}, window [{a.cn_start}, {a.cn_end}]; "
          f"wrote {a.out}")


if __name__ == "__main__":
    main()
