"""The reference's test.py flow (test.py:28-104) on the MI355X path, with preference-guided noise selection over
several seeds.  Real checkpoints are optional -- without them every model is seeded random, which exercises the
whole path (PIL in -> CLIP-shaped embeddings -> HarmonyAttention + ImageProjModel -> 30-step denoise per candidate
-> PNS winner -> VAE tiled decode -> PIL out) but of course produces noise, not a picture.

    python examples/pns_edit.py --out out.png [--unet unet.safetensors] [--vae vae.safetensors] [--ip-ckpt ip_adapter.bin]
                                [--seeds 0 1 2 3] [--steps 30] [--preview-steps 10] [--size 1024]
                                [--scheduler euler-a --step-noise seed]
                                [--init-image in.png --strength 0.6] [--clip-backend hip --judge-preprocess hip]
                                [--preview-vae taesdxl.safetensors | --preview-vae random]
                                [--freeu 0.6 0.4 1.1 1.2]
                                [--seeds 0 --pag-scale 3.0 --pag-layers mid]

With --init-image the candidates are image-to-image EDITS of that image (IPAdapterXL.generate_pns(image=, strength=)): every seed fixes its
posterior and add-noise draws, the previews are decoded and scored by the CLIP judge when a tower is attached (--clip-backend), and
--judge-preprocess hip takes the decoded previews to the HIP tower's patch rows in one launch.  --preview-vae lets the judge see the
previews through AutoencoderTiny (diffusers' TAESDXL decoder, 35 small launches per decode) instead of the full VAE; the winner's image
still comes from the full VAE.  --freeu S1 S2 B1 B2 switches FreeU on (pipe.enable_freeu, diffusers' argument order; SDXL's published
values are 0.6 0.4 1.1 1.2): previews and finals alike run the UNet with the re-weighted skip concats of its first two up blocks.
--pag-scale S (with ONE seed) adds perturbed-attention guidance: pipe.set_pag_applied_layers(--pag-layers, default "mid") and the pipe's
own call with pag_scale=S through IPAdapterXL.generate -- one more UNet batch member per step whose self-attention maps in the chosen
layers are the identity.  Noise selection over several seeds is not built with PAG: the script says so and stops.

Launch under torch.distributed.run with N ranks to shard the seeds over N GPUs (one process per GPU, RCCL).
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imagharmony_amd import pns                                           # noqa: E402
from imagharmony_amd.ip_adapter import IPAdapterXL                        # noqa: E402
from imagharmony_amd.modules import HarmonyAttention                      # noqa: E402
from imagharmony_amd.pipeline import StableDiffusionXLCustomPipeline, StableDiffusionXLImg2ImgCustomPipeline      # noqa: E402
from imagharmony_amd import schedulers as hs                              # noqa: E402
from imagharmony_amd.unet import UNet2DConditionModel, UNetConfig         # noqa: E402
from imagharmony_amd.vae import AutoencoderKL, decode_latents, postprocess   # noqa: E402


SCHEDULERS = {
    "ddim": hs.DDIMScheduler,
    "euler": hs.EulerDiscreteScheduler,
    "dpmpp2m": hs.DPMSolverMultistepScheduler,
    "dpmpp2m-karras": lambda: hs.DPMSolverMultistepScheduler(use_karras_sigmas=True),
    "euler-a": hs.EulerAncestralDiscreteScheduler,           # stochastic: reads noise at every step (--step-noise says from where)
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scheduler", choices=sorted(SCHEDULERS), default="ddim",
                    help="sampler of the preview and the final denoise (dpmpp2m-karras at 20-25 steps is the usual SDXL choice)")
    ap.add_argument("--step-noise", choices=("global", "seed"), default="global",
                    help="per-step noise of a stochastic scheduler (euler-a): global = drawn from torch's global generator per denoise (a seed "
                         "fixes the initial noise only); seed = generated on the device from each candidate's seed, so the same command "
                         "prints the same winner and writes the same image twice.  Deterministic schedulers draw none")
    ap.add_argument("--out", default="out.png")
    ap.add_argument("--unet"); ap.add_argument("--vae"); ap.add_argument("--ip-ckpt")
    ap.add_argument("--seeds", type=int, nargs="+", default=[0, 1, 2, 3])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--preview-steps", type=int, default=10)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--guidance", type=float, default=5.0)
    ap.add_argument("--clip-backend", choices=("none", "hip", "transformers"), default="none",
                    help="CLIP vision tower behind the image prompt: none = stand-in embeddings (default); hip = imagharmony_amd's "
                         "CLIPVisionEncoder; transformers = the stock module.  --clip DIR loads a saved tower, else seeded random weights at ViT-bigG/14 size")
    ap.add_argument("--clip")
    ap.add_argument("--init-image", help="edit this image (image-to-image PNS) instead of generating from noise")
    ap.add_argument("--strength", type=float, default=0.6, help="with --init-image: how far the edit departs from the image (0 .. 1)")
    ap.add_argument("--judge-preprocess", choices=("torch", "hip"), default="torch",
                    help="with --init-image and a CLIP tower: how the judge gets from decoded previews to the tower's input (hip needs --clip-backend hip)")
    ap.add_argument("--preview-vae", nargs="?", const="random", default=None, metavar="PATH",
                    help="with --init-image and a CLIP tower: decode the judge's previews with AutoencoderTiny -- PATH = a diffusers taesdxl "
                         "safetensors file; no value or `random` = seeded random weights")
    ap.add_argument("--freeu", type=float, nargs=4, metavar=("S1", "S2", "B1", "B2"), default=None,
                    help="FreeU: skip scales s1, s2 and backbone scales b1, b2 of up blocks 0 and 1 (SDXL: 0.6 0.4 1.1 1.2)")
    ap.add_argument("--pag-scale", type=float, default=0.0, help="perturbed-attention guidance scale (0 = off); single seed only")
    ap.add_argument("--pag-layers", nargs="+", default=["mid"], metavar="REGEX",
                    help='with --pag-scale: the self-attention layers that get the identity map, as diffusers\' pag_applied_layers ("mid", "down_blocks.2", ...)')
    a = ap.parse_args()
    if a.pag_scale > 0 and len(a.seeds) > 1:
        ap.error("--pag-scale runs a single seed: noise selection over several seeds (generate_pns) is not built with PAG")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.distributed.init_process_group("nccl")
    dev, dtype = torch.device(f"cuda:{local}"), torch.bfloat16
    torch.cuda.set_device(dev)
    torch.manual_seed(0)                                                  # the stand-in weights below: the same on every rank and in every run

    if a.unet:
        unet = UNet2DConditionModel.from_safetensors(a.unet, UNetConfig()).to(dev, dtype)
    else:
        with torch.device(dev):                                            # 2.6 B parameters: create them on the GPU
            unet = UNet2DConditionModel(UNetConfig())
        unet = unet.init_random_(1234).to(dtype)
    enc_kw = {"with_encoder": True} if a.init_image else {}
    vae = AutoencoderKL.from_safetensors(a.vae, device=dev, dtype=dtype, **enc_kw) if a.vae else AutoencoderKL(**enc_kw).init_random_(1).to(dev, dtype)
    pns.broadcast_module_(unet)                                           # identical replicas on every rank
    pipe_cls = StableDiffusionXLImg2ImgCustomPipeline if a.init_image else StableDiffusionXLCustomPipeline
    pipe = pipe_cls(unet, scheduler=SCHEDULERS[a.scheduler](), device=dev, dtype=dtype, vae=vae)
    pipe.enable_vae_tiling()                                              # test.py:73
    if a.freeu:
        pipe.enable_freeu(*a.freeu)
    ha = HarmonyAttention(image_hidden_size=1280, text_context_dim=2048, inter_dim=2560, cross_heads=8, reshape_blocks=8,
                          cross_value_dim=64, scale=1.0, fusion_method="cross_attention")     # test.py:82-91
    ip = IPAdapterXL(pipe, None, a.ip_ckpt, dev, num_tokens=4, inference=True, number_class_crossattention=ha, dtype=dtype)

    # encoders are outside the path (no tokenizer vocabulary / CLIP weights offline): stand-in embeddings of the right shape
    g = torch.Generator().manual_seed(0)
    clip_embeds = torch.randn(1, 1280, generator=g)
    enc = None
    if a.clip_backend != "none":                                          # the image prompt through a real tower (random pixels stand in for the image)
        px = torch.randn(1, 3, 224, 224, generator=g).to(dev, dtype)
        if a.clip_backend == "hip":
            from imagharmony_amd import CLIPVisionEncoder, CLIPVisionEncoderConfig
            if a.clip:
                enc = CLIPVisionEncoder.from_pretrained(a.clip, device=dev, dtype=dtype)
            else:
                torch.manual_seed(4321)
                with torch.device(dev):
                    enc = CLIPVisionEncoder(CLIPVisionEncoderConfig.vit_bigg())
                for prm in enc.parameters():                              # LayerNorm-scale activations: weights of a trained tower's order
                    if prm.dim() > 1:
                        prm.normal_(0, 0.02)
                enc = enc.to(dtype)
        else:
            from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
            enc = (CLIPVisionModelWithProjection.from_pretrained(a.clip) if a.clip else CLIPVisionModelWithProjection(CLIPVisionConfig(
                hidden_size=1664, intermediate_size=8192, num_hidden_layers=48, num_attention_heads=16, projection_dim=1280,
                hidden_act="gelu"))).eval().to(dev, dtype)
        clip_embeds = enc(px).image_embeds
    prompt = (torch.randn(1, 77, 2048, generator=g), torch.randn(1, 77, 2048, generator=g),
              torch.randn(1, 1280, generator=g), torch.randn(1, 1280, generator=g))
    extra = torch.randn(1, 77, 2048, generator=g)
    if a.pag_scale > 0:
        # one seed, no selection: the pipe's own call (text-to-image, or the image-to-image edit of --init-image) with PAG
        pipe.set_pag_applied_layers(a.pag_layers)
        kw = {}
        if a.init_image:
            from PIL import Image
            kw = dict(image=Image.open(a.init_image).convert("RGB").resize((a.size, a.size)), strength=a.strength)
        else:
            kw = dict(height=a.size, width=a.size)
        images = ip.generate(clip_image_embeds=clip_embeds, prompt_embeds=prompt, extra_prompt_embeds=extra, scale=a.scale, num_samples=1,
                             seed=a.seeds[0], num_inference_steps=a.steps, guidance_scale=a.guidance, pag_scale=a.pag_scale, **kw)
        if int(os.environ.get("RANK", "0")) == 0:
            images[0].save(a.out)
            print(f"seed {a.seeds[0]} with PAG {a.pag_scale} in {len(unet.pag_layer_names())} layers {a.pag_layers}; wrote {a.out} {images[0].size}")
        if world > 1:
            torch.distributed.destroy_process_group()
        return
    if a.init_image:
        from PIL import Image
        ip.image_encoder = enc                                            # the judge's tower (None: the latent-statistic scorer)
        init = Image.open(a.init_image).convert("RGB").resize((a.size, a.size))
        preview_vae = None
        if a.preview_vae is not None:
            from imagharmony_amd import AutoencoderTiny
            preview_vae = AutoencoderTiny().init_random_(7).to(dev, dtype) if a.preview_vae == "random" else \
                AutoencoderTiny.from_safetensors(a.preview_vae, device=dev, dtype=dtype)
        r = ip.generate_pns(a.seeds, clip_image_embeds=clip_embeds, prompt_embeds=prompt, extra_prompt_embeds=extra, scale=a.scale,
                            preview_steps=a.preview_steps, num_inference_steps=a.steps, guidance_scale=a.guidance, image=init,
                            strength=a.strength, step_noise=a.step_noise, judge_preprocess=a.judge_preprocess, preview_vae=preview_vae)
        if int(os.environ.get("RANK", "0")) == 0:
            r["images"][0].save(a.out)
            print(f"seeds {a.seeds} -> scores {[round(float(s), 4) for s in r['scores']]}; best seed {r['best_seed']}; "
                  f"edited {a.init_image} at strength {a.strength}; wrote {a.out} {r['images'][0].size}")
        if world > 1:
            torch.distributed.destroy_process_group()
        return
    ipe, uipe = ip.get_image_embeds(clip_image_embeds=clip_embeds, extra_prompt_embeds=extra)
    ip.set_scale(a.scale)
    pe = torch.cat([prompt[0].to(dev, dtype), ipe], 1)
    ne = torch.cat([prompt[1].to(dev, dtype), uipe], 1)
    eng = pipe.engine
    eng.set_conditioning(pe, ne, prompt[2].to(dev, dtype), prompt[3].to(dev, dtype), a.size, a.size, guidance_scale=a.guidance)

    by_seed = a.step_noise == "seed" and getattr(pipe.scheduler, "stochastic", False)
    preview, final = pns.two_stage_fns(eng, pipe.scheduler, a.preview_steps, a.steps, step_noise="seed" if by_seed else "global")
    r = pns.run_pns(preview, a.seeds, (1, 4, a.size // 8, a.size // 8), device=dev, final_fn=final, pass_seeds=by_seed)
    if int(os.environ.get("RANK", "0")) == 0:
        img = postprocess(decode_latents(vae, r["latents"]), "pil")[0]
        img.save(a.out)
        print(f"seeds {a.seeds} -> scores {[round(float(s), 4) for s in r['scores']]}; best seed {r['best_seed']} "
              f"(rank {r['owner']}); wrote {a.out} {img.size}")
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
