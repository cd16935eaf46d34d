"""GPU: preference-guided noise selection over EDITS -- IPAdapterXL.generate_pns on the image-to-image pipe and on both inpainting modes
(4-channel UNet: blend in the step; 9-channel UNet: conv_in over [latents | mask | masked-image latents]).

The contract under test is what a candidate seed means: for seed s every draw comes from torch.Generator("cpu").manual_seed(s) in the
pipe's order, so the winner's final latents are, bit for bit, the pipe's own call with generator=[that generator].  The tiny UNet / VAE
pair is the one tests/test_gpu_inpaint.py builds (and caches)."""
import pytest
import torch

from oracle.detfill import det_fill, det_randn
from test_gpu_inpaint import IMG, build_pair, build_vae_pair, centred_mask

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEEDS = [3, 9, 27, 81]
PREVIEW, FINAL, STRENGTH = 4, 6, 0.6            # 4 x 0.6 -> the preview runs rows 2..3; 6 x 0.6 -> the final runs rows 3..5
MODES = ["img2img", "inpaint4", "inpaint9"]


def _scorer(lat):
    """pns.default_scorer, one candidate at a time on the CPU: a function of the candidate's latents alone (torch's reductions over a
    stacked tensor and over a single one may round differently; what is under test is the latents)"""
    from imagharmony_amd import pns
    return torch.cat([pns.default_scorer(lat[k:k + 1].float().cpu()) for k in range(lat.shape[0])])


def _scheduler(kind):
    from imagharmony_amd import schedulers as hs
    return hs.DDIMScheduler() if kind == "ddim" else hs.EulerAncestralDiscreteScheduler()


def _adapter(mode, dtype, sched="ddim", image_encoder=None):
    """(IPAdapterXL over the mode's pipe on the tiny pair, the keyword arguments every call below shares)"""
    from imagharmony_amd.ip_adapter import IPAdapterXL
    from imagharmony_amd.modules import HarmonyAttention
    from imagharmony_amd.pipeline import StableDiffusionXLImg2ImgCustomPipeline, StableDiffusionXLInpaintCustomPipeline
    _, hu, ocfg = build_pair(dtype, 9 if mode == "inpaint9" else 4)
    _, hv = build_vae_pair()
    cls = StableDiffusionXLImg2ImgCustomPipeline if mode == "img2img" else StableDiffusionXLInpaintCustomPipeline
    pipe = cls(hu, scheduler=_scheduler(sched), device=DEV, dtype=dtype, vae=hv)
    cd = ocfg.cross_attention_dim
    dim = 128 if image_encoder is None else image_encoder.config.projection_dim
    ha = det_fill(HarmonyAttention(image_hidden_size=dim, text_context_dim=cd, inter_dim=512, cross_heads=8, reshape_blocks=8,
                                   cross_value_dim=64), 3)
    ip = IPAdapterXL(pipe, None, None, DEV, num_tokens=4, inference=True, number_class_crossattention=ha, dtype=dtype,
                     clip_embeddings_dim=dim, image_encoder=image_encoder)
    det_fill(ip.image_proj_model, 5)
    embeds4 = (det_randn((1, 77, cd), 1), det_randn((1, 77, cd), 2), det_randn((1, ocfg.pooled_dim), 3), det_randn((1, ocfg.pooled_dim), 4))
    kw = dict(clip_image_embeds=det_randn((1, dim), 5), prompt_embeds=embeds4, extra_prompt_embeds=det_randn((1, 77, cd), 6), scale=0.8,
              guidance_scale=5.0, image=IMG(), strength=STRENGTH)
    if mode != "img2img":
        kw["mask_image"] = centred_mask(256, 256)
    return ip, kw


def _direct(ip, kw, seed, steps, **extra):
    """the pipe's own call for one seed: generate_pns's conditioning (text + image-prompt tokens), generator=[manual_seed(seed)]"""
    fused = ip.fused_clip_embeds(None, kw["clip_image_embeds"], kw["extra_prompt_embeds"])
    ipe = ip._g(ip.image_proj_model)(fused)
    uipe = ip._g(ip.image_proj_model)(torch.zeros_like(fused))
    pe, ne, ppe, npe = kw["prompt_embeds"]
    pe = torch.cat([pe.to(ipe.device, ip.dtype), ipe], dim=1)
    ne = torch.cat([ne.to(ipe.device, ip.dtype), uipe], dim=1)
    edit = {k: kw[k] for k in ("image", "mask_image", "strength") if k in kw}
    return ip.pipe(prompt_embeds=pe, negative_prompt_embeds=ne, pooled_prompt_embeds=ppe, negative_pooled_prompt_embeds=npe,
                   num_inference_steps=steps, guidance_scale=kw["guidance_scale"], output_type="latent",
                   generator=[torch.Generator("cpu").manual_seed(int(seed))], **edit, **extra).images


# ------------------------------------------------------------------------------------ 7. equivalence under DDIM
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("mode", MODES)
def test_edit_pns_winner_equals_the_pipes_own_call(mode, dtype):
    ip, kw = _adapter(mode, dtype)
    run = lambda batch: ip.generate_pns(SEEDS, preview_steps=PREVIEW, num_inference_steps=FINAL, batch=batch, output_type="latent",      # noqa: E731
                                        scorer=_scorer, **kw)
    r2 = run(2)
    lat = r2["latents"].to(DEV)
    assert lat.shape == (1, 4, 32, 32) and torch.isfinite(lat).all() and r2["best_seed"] in SEEDS
    assert r2["scores"].unique().numel() == len(SEEDS)                      # four different candidates
    if mode == "inpaint4":
        # outside the mask the result is the image latents, to the bit: the pipeline's property survives stacking
        z = ip.pipe.engine.st.inp_z.clone()
        keep = (ip.pipe.engine.st.inp_mask == 0).expand_as(z)
        assert z.shape == lat.shape and 0.7 < keep.float().mean().item() < 0.8
        assert torch.equal(lat[keep], z[keep]) and not torch.equal(lat[~keep], z[~keep])
    direct = _direct(ip, kw, r2["best_seed"], FINAL)
    assert torch.equal(direct.float(), lat)
    # the previews too are the pipe's own short calls: score of seed s = scorer(pipe(preview_steps, generator=[s]))
    s0 = _scorer(_direct(ip, kw, SEEDS[1], PREVIEW))
    assert float(s0[0]) == float(r2["scores"][1])
    r1 = run(1)
    assert torch.equal(r1["scores"], r2["scores"]) and r1["best_seed"] == r2["best_seed"]      # scores do not depend on `batch`
    assert torch.equal(r1["latents"], r2["latents"])


# ------------------------------------------------------------------------------------ 8. the same under Euler ancestral, seeded step noise
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("mode", MODES)
def test_edit_pns_under_euler_ancestral_with_step_noise_from_the_seed(mode, dtype):
    ip, kw = _adapter(mode, dtype, sched="euler-a")
    r = ip.generate_pns(SEEDS, preview_steps=PREVIEW, num_inference_steps=FINAL, batch=2, output_type="latent", scorer=_scorer,
                        step_noise="seed", **kw)
    assert ip.pipe.engine.seeded and torch.isfinite(r["latents"]).all()
    direct = _direct(ip, kw, r["best_seed"], FINAL, step_noise="seeded")
    assert torch.equal(direct.float(), r["latents"].to(DEV))
    other = _direct(ip, kw, r["best_seed"], FINAL)                          # the generator's own step noise: another trajectory
    assert not torch.equal(other.float(), r["latents"].to(DEV))


# ------------------------------------------------------------------------------------ strength 1.0 (inpainting's strength_max paths)
@pytest.mark.parametrize("mode", ["inpaint4", "inpaint9"])
def test_edit_pns_at_full_strength_follows_the_pipelines_rules(mode):
    """strength == 1.0: the initial latents are pure noise (is_strength_max); a 9-channel UNet skips the image's encoder pass and still
    makes its draw"""
    dtype = torch.float16
    ip, kw = _adapter(mode, dtype)
    kw = dict(kw, strength=1.0)
    r = ip.generate_pns(SEEDS[:2], preview_steps=2, num_inference_steps=3, batch=2, output_type="latent", scorer=_scorer, **kw)
    direct = _direct(ip, kw, r["best_seed"], 3)
    assert torch.equal(direct.float(), r["latents"].to(DEV))


# ------------------------------------------------------------------------------------ the CLIP judge on the HIP path, end to end
def test_edit_pns_with_the_hip_judge_end_to_end():
    from test_gpu_clip_preprocess import _tower
    dtype = torch.bfloat16
    enc, hf = _tower(dtype)
    ip, kw = _adapter("img2img", dtype, image_encoder=enc)
    r = ip.generate_pns(iter(SEEDS), preview_steps=PREVIEW, num_inference_steps=FINAL, batch=2, output_type="latent",
                        judge_preprocess="hip", **kw)                       # (a generator as `seeds`: every candidate is still scored)
    assert r["scores"].shape == (4,) and torch.isfinite(r["scores"]).all() and float(r["scores"].abs().max()) <= 1.0 + 1e-3
    assert r["scores"].unique().numel() == 4
    assert torch.equal(_direct(ip, kw, r["best_seed"], FINAL).float(), r["latents"].to(DEV))
    # refusals, before any GPU work
    ip2, kw2 = _adapter("img2img", dtype)                                   # no image encoder at all
    with pytest.raises(ValueError, match="hip"):
        ip2.generate_pns(SEEDS, judge_preprocess="hip", output_type="latent", **kw2)
    with pytest.raises(ValueError, match="no denoising step"):
        ip2.generate_pns(SEEDS, preview_steps=2, num_inference_steps=6, output_type="latent", **dict(kw2, strength=0.3))
    with pytest.raises(NotImplementedError):
        ip2.generate_pns(SEEDS, output_type="latent", **{k: v for k, v in kw2.items() if k != "image"})
    with pytest.raises(ValueError, match="mask_image"):
        ip2.generate_pns(SEEDS, output_type="latent", mask_image=centred_mask(256, 256), **kw2)
