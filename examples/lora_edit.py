"""LoRA on the SDXL UNet at no cost per step: one or two LoRA files (diffusers / PEFT or kohya naming, SGM module paths included) are merged
into the UNet's weights by one grouped launch, so the replayed step graph is launch for launch what it is without them; changing the
adapter weights is one more merge, not a reload.  Real checkpoints are optional -- without them the UNet, the VAE and the adapters are
seeded random, which exercises the whole path (state dict -> name tables -> snapshot -> merge -> re-packed weights -> the denoise graph ->
VAE tiled decode -> PIL out) but of course produces noise, not a picture.

    python examples/lora_edit.py --out out.png [--lora style.safetensors [character.safetensors]] [--weights 0.8 [0.5]] [--rank 16]
                                 [--unet unet.safetensors] [--vae vae.safetensors] [--ip-ckpt ip_adapter.bin] [--skip-text-encoder]
                                 [--steps 30] [--seed 0] [--size 1024] [--samples 1] [--compare]

--compare also writes the picture of the same seed with the adapters disabled (out_base.png): one more merge, no reload.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imagharmony_amd import lora                                          # noqa: E402
from imagharmony_amd.ip_adapter import IPAdapterXL                        # noqa: E402
from imagharmony_amd.modules import HarmonyAttention                      # noqa: E402
from imagharmony_amd.pipeline import StableDiffusionXLCustomPipeline      # noqa: E402
from imagharmony_amd.schedulers import DDIMScheduler                      # noqa: E402
from imagharmony_amd.unet import UNet2DConditionModel, UNetConfig         # noqa: E402
from imagharmony_amd.vae import AutoencoderKL                             # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="out.png")
    ap.add_argument("--lora", nargs="*", default=[], help="one or two .safetensors LoRA files; none: two seeded random adapters")
    ap.add_argument("--weights", type=float, nargs="*", help="one adapter weight per LoRA (default 1.0 each)")
    ap.add_argument("--rank", type=int, default=16, help="rank of the seeded random adapters")
    ap.add_argument("--skip-text-encoder", action="store_true", help="leave a file's text-encoder keys out instead of refusing the file")
    ap.add_argument("--unet"); ap.add_argument("--vae"); ap.add_argument("--ip-ckpt")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--samples", type=int, default=1)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--guidance", type=float, default=5.0)
    ap.add_argument("--compare", action="store_true")
    a = ap.parse_args()
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
    ip = IPAdapterXL(pipe, None, a.ip_ckpt, dev, num_tokens=4, inference=True, number_class_crossattention=ha, dtype=dtype)

    # the adapters: files, or seeded random ones over the attention / feed-forward / proj_in / proj_out Linears in kohya-SGM naming
    usual = lambda n: lora.ATTN_FF_PROJ.search(n) is not None                   # noqa: E731
    sources = a.lora or [lora.synthetic_adapter(unet, rank=a.rank, seed=s, select=usual, alpha=a.rank / 2, naming="sgm") for s in (1, 2)]
    names = []
    for i, src in enumerate(sources):
        rep = pipe.load_lora_weights(src, adapter_name=f"lora{i}", text_encoder="skip" if a.skip_text_encoder else "error")
        names.append(rep["adapter_name"])
        print(f"{rep['adapter_name']}: {len(rep['modules'])} modules, rank {rep['rank']}, {len(rep['skipped'])} keys skipped")
    weights = a.weights or [1.0] * len(names)
    torch.cuda.synchronize()
    t = time.perf_counter()
    pipe.set_adapters(names, weights)                                      # one merge launch over every touched weight
    torch.cuda.synchronize()
    t_merge = (time.perf_counter() - t) * 1e3

    # encoders are outside the path (no tokenizer vocabulary / CLIP weights offline): stand-in embeddings of the right shape
    g = torch.Generator().manual_seed(0)
    n = a.samples
    clip_embeds = torch.randn(1, 1280, generator=g)
    prompt = tuple(t.repeat(n, *([1] * (t.dim() - 1))) for t in (torch.randn(1, 77, 2048, generator=g), torch.randn(1, 77, 2048, generator=g),
                                                                 torch.randn(1, 1280, generator=g), torch.randn(1, 1280, generator=g)))
    extra = torch.randn(1, 77, 2048, generator=g)
    kw = dict(clip_image_embeds=clip_embeds, prompt_embeds=prompt, extra_prompt_embeds=extra, scale=a.scale, num_samples=n, seed=a.seed,
              num_inference_steps=a.steps, guidance_scale=a.guidance, height=a.size, width=a.size)
    images = ip.generate(**kw)
    images[0].save(a.out)
    print(f"adapters {pipe.get_active_adapters()} at weights {weights} (merge: {t_merge:.1f} ms): {len(images)} image(s) {images[0].size}; wrote {a.out}")
    if a.compare:
        pipe.disable_lora()                                                # the snapshots' bits: the base model, no reload
        base = ip.generate(**kw)
        root, ext = os.path.splitext(a.out)
        base[0].save(root + "_base" + ext)
        pipe.enable_lora()
        print(f"the same seed with the adapters disabled: wrote {root}_base{ext}")


if __name__ == "__main__":
    main()
