"""GPU, BASELINE.json full sizes (SDXL UNet, 1024^2, CFG batch 2): the CPU oracle cannot finish these in seconds,
so parity is checked through size-independent properties of the path (seeded random weights of the exact SDXL
architecture):
  * CFG identity: identical cond / uncond conditioning -> the guidance scale has no effect on the trajectory;
  * batch consistency: the two CFG halves of one forward are bitwise equal when their conditioning is equal;
  * IP-scale 0 == the image-prompt branch contributes nothing (same latents as with different IP tokens);
  * dtype consistency: bf16 and fp16 trajectories agree to their rounding level;
  * determinism: a seed reproduces its latent bit-for-bit.
Also checks the FLOP accounting of the recorded forward against SURVEY.md's 13.5 TFLOP figure."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def sdxl():
    import bench
    from imagharmony_amd.pipeline import StableDiffusionXLCustomPipeline
    from imagharmony_amd.schedulers import DDIMScheduler
    unet = bench.build_unet(DEV, torch.bfloat16, 4)
    pipe = StableDiffusionXLCustomPipeline(unet, scheduler=DDIMScheduler(), device=DEV, dtype=torch.bfloat16)
    pe, ne, po, no = [t.to(DEV) for t in bench.synthetic_conditioning(4)]
    return pipe, (pe, ne, po, no)


def run(pipe, pe, ne, po, no, guidance=5.0, steps=2, seed=3):
    z = torch.randn(1, 4, 128, 128, generator=torch.Generator("cpu").manual_seed(seed))
    return pipe(prompt_embeds=pe, negative_prompt_embeds=ne, pooled_prompt_embeds=po, negative_pooled_prompt_embeds=no,
                height=1024, width=1024, num_inference_steps=steps, guidance_scale=guidance, latents=z,
                output_type="latent").images.clone()


def test_fullsize_properties(sdxl):
    pipe, (pe, ne, po, no) = sdxl
    a = run(pipe, pe, ne, po, no)
    assert a.shape == (1, 4, 128, 128) and torch.isfinite(a).all()
    assert torch.equal(a, run(pipe, pe, ne, po, no))                              # determinism
    # CFG identity (custom_pipelines.py:348-350): u == c  =>  u + g (c - u) == u for every g
    g2 = run(pipe, pe, pe, po, po, guidance=2.0)
    g9 = run(pipe, pe, pe, po, po, guidance=9.0)
    assert (g2 - g9).abs().max().item() <= 2e-2 * g2.abs().max().item()           # only bf16 rounding of c - u != 0
    # IP scale 0: the image tokens must not matter
    pipe.set_scale(0.0)
    pe2 = pe.clone(); pe2[:, 77:] = torch.randn_like(pe2[:, 77:])
    s0a, s0b = run(pipe, pe, ne, po, no), run(pipe, pe2, ne, po, no)
    pipe.set_scale(1.0)
    assert torch.equal(s0a, s0b)
    assert not torch.equal(run(pipe, pe2, ne, po, no), a)                         # ... and they do at scale 1


def test_fullsize_cfg_halves_and_flops(sdxl):
    from imagharmony_amd import lib as L
    pipe, (pe, ne, po, no) = sdxl
    eng = pipe.engine
    eng.set_conditioning(pe, pe, po, po, 1024, 1024, guidance_scale=5.0)          # identical halves
    eng.set_schedule(pipe.scheduler, 2)
    eng.denoise(torch.randn(1, 4, 128, 128))
    torch.cuda.synchronize()
    npred = eng.noise_pred.float()                                                # [2, HW, 4] of the last forward
    assert torch.equal(npred[0], npred[1])
    tflop = sum(t[3] for t in eng.plan.tags) / 1e12
    assert 13.3 < tflop < 13.6, tflop                                             # 13.528 with per-step K/V recompute


def test_fullsize_bf16_vs_fp16(sdxl):
    import bench
    from imagharmony_amd.pipeline import StableDiffusionXLCustomPipeline
    from imagharmony_amd.schedulers import DDIMScheduler
    pipe, (pe, ne, po, no) = sdxl
    a = run(pipe, pe, ne, po, no, steps=1)
    u16 = bench.build_unet(DEV, torch.float16, 4)
    p16 = StableDiffusionXLCustomPipeline(u16, scheduler=DDIMScheduler(), device=DEV, dtype=torch.float16)
    b = run(p16, pe, ne, po, no, steps=1)
    rel = ((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt()).item()
    assert rel < 3e-2, rel


def test_fullsize_vae_decode_1024():
    """SDXL-size VAE decoder (random weights): 128x128 latent -> 1024x1024 image, untiled and tiled (9 tiles with
    linear blends, test.py:73): finite, deterministic, and the two agree away from seams up to the per-tile
    GroupNorm statistics"""
    from imagharmony_amd.vae import AutoencoderKL, decode_latents, postprocess
    vae = AutoencoderKL().init_random_(1).to(DEV, torch.bfloat16)
    lat = torch.randn(1, 4, 128, 128, generator=torch.Generator().manual_seed(0)).to(DEV) * 0.13025
    a = decode_latents(vae, lat)
    assert a.shape == (1, 3, 1024, 1024) and torch.isfinite(a).all()
    assert torch.equal(a, decode_latents(vae, lat))
    vae.enable_tiling()
    t = decode_latents(vae, lat)
    assert t.shape == a.shape and torch.isfinite(t).all() and not torch.equal(t, a)
    assert postprocess(t, "pil")[0].size == (1024, 1024)


def test_fullsize_vae_decode_1024_reference_precision():
    """the same decode at the reference's precision (a float16 module is upcast: fp32 activations / weights / arithmetic on csrc/f32.hip,
    incl. the 16384 x 16384 fp32 score matrix of the mid-block attention): finite, deterministic, tiled and untiled, and the bf16 decode of
    the same weights agrees with it to bf16's precision"""
    from imagharmony_amd.vae import AutoencoderKL, decode_latents
    vae = AutoencoderKL().init_random_(1).to(DEV, torch.float16)
    assert vae.precision_for() == "fp32"
    lat = torch.randn(1, 4, 128, 128, generator=torch.Generator().manual_seed(0)).to(DEV) * 0.13025
    a = decode_latents(vae, lat)
    assert a.shape == (1, 3, 1024, 1024) and a.dtype == torch.float32 and torch.isfinite(a).all()
    assert torch.equal(a, decode_latents(vae, lat))
    vae.enable_tiling()
    t = decode_latents(vae, lat)
    assert t.shape == a.shape and torch.isfinite(t).all() and not torch.equal(t, a)
    vae.enable_tiling(False)
    b = decode_latents(vae.to(torch.bfloat16), lat)                 # bfloat16 module -> native 16-bit decode (weights rounded to bf16 as well)
    rel = ((a - b).pow(2).mean().sqrt() / a.pow(2).mean().sqrt()).item()
    assert rel < 4e-2, rel


def test_fullsize_vae_decode_ragged_100x100():
    """the full-size SDXL VAE on a 100x100 latent (800x800: 10000 tokens in the mid-block attention, not a multiple of 64): the native
    bf16 decode and the fp32-precision decode of the same weights are finite and agree within the bf16-vs-fp32 bound of the 1024^2 test
    (measured 1.24e-2)"""
    from imagharmony_amd.vae import AutoencoderKL, decode_latents
    vae = AutoencoderKL().init_random_(1).to(DEV, torch.float16)
    lat = torch.randn(1, 4, 100, 100, generator=torch.Generator().manual_seed(0)).to(DEV) * 0.13025
    a = decode_latents(vae, lat)
    assert a.shape == (1, 3, 800, 800) and a.dtype == torch.float32 and torch.isfinite(a).all()
    b = decode_latents(vae.to(torch.bfloat16), lat)
    assert b.shape == a.shape and torch.isfinite(b).all()
    rel = ((a - b).pow(2).mean().sqrt() / a.pow(2).mean().sqrt()).item()
    print(f"full-size VAE 100x100: native bf16 vs fp32 rel-rms {rel:.3e}")
    assert rel < 4e-2, rel


@pytest.mark.parametrize("dtype,S,T,sched", [(torch.float16, 4, 16, "euler"), (torch.bfloat16, 4, 32, "ddim")])
def test_fullsize_stacked_candidates_configs_3_and_4(dtype, S, T, sched):
    """BASELINE.json configs[3] (batch 4 per GPU, 16 Resampler tokens, fp16) and configs[4] (4 PNS candidates per GPU,
    2 x 16 image tokens; its fp8 attention is not built -- bf16 here) at the full SDXL size: S candidates stacked
    into one UNet batch of 2S.  Properties: finite; every candidate equals its own batch-1 run up to rounding
    (candidates are independent rows of every op); identical candidates give bitwise identical rows."""
    import bench
    from imagharmony_amd import schedulers as hs
    from imagharmony_amd.pipeline import StableDiffusionXLCustomPipeline
    unet = bench.build_unet(DEV, dtype, T)
    mk = (lambda: hs.EulerDiscreteScheduler()) if sched == "euler" else (lambda: hs.DDIMScheduler())
    pipe = StableDiffusionXLCustomPipeline(unet, scheduler=mk(), device=DEV, dtype=dtype)
    pe, ne, po, no = [t.to(DEV) for t in bench.synthetic_conditioning(T)]
    z = torch.randn(S, 4, 128, 128, generator=torch.Generator("cpu").manual_seed(11))
    z[3] = z[0]                                                                     # candidate 3 == candidate 0
    kw = dict(height=1024, width=1024, num_inference_steps=2, guidance_scale=5.0, output_type="latent")
    stacked = pipe(prompt_embeds=pe.repeat(S, 1, 1), negative_prompt_embeds=ne.repeat(S, 1, 1),
                   pooled_prompt_embeds=po.repeat(S, 1), negative_pooled_prompt_embeds=no.repeat(S, 1), latents=z, **kw).images.clone()
    assert stacked.shape == (S, 4, 128, 128) and torch.isfinite(stacked).all()
    assert torch.equal(stacked[3], stacked[0]) and not torch.equal(stacked[1], stacked[0])
    one = pipe(prompt_embeds=pe, negative_prompt_embeds=ne, pooled_prompt_embeds=po, negative_pooled_prompt_embeds=no,
               latents=z[1:2], **kw).images
    rel = ((stacked[1:2] - one).pow(2).mean().sqrt() / one.pow(2).mean().sqrt()).item()
    assert rel < (1e-2 if dtype == torch.float16 else 3e-2), rel


def test_fullsize_replay_race_screen(sdxl):
    """race screen for the LDS-DMA pipelines (counted vmcnt + raw barriers): 40 replays of the full-size forward
    (968 kernel launches each, every tile shape of the table) must be bitwise identical -- an early LDS read or a
    late restage shows up as a tile that differs between runs"""
    pipe, (pe, ne, po, no) = sdxl
    eng = pipe.engine
    eng.set_conditioning(pe, ne, po, no, 1024, 1024, guidance_scale=5.0)
    eng.set_schedule(pipe.scheduler, 1)
    z = torch.randn(1, 4, 128, 128, generator=torch.Generator("cpu").manual_seed(5))
    first = eng.denoise(z).clone()
    npred = eng.noise_pred.clone()
    assert torch.isfinite(first).all()
    for i in range(40):
        out = eng.denoise(z)
        assert torch.equal(out, first), f"replay {i} differs"
    assert torch.equal(eng.noise_pred, npred)
