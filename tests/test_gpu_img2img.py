"""GPU: SDXL image-to-image on the HIP path -- the right / bottom padded stride-2 conv3x3 (imh_gemm_args.pad = 1) in every 16-bit
variant and both fp32 kernels against F.conv2d(F.pad(x, (0, 1, 0, 1)), stride 2), the VAE encoder (plain and tiled) against the
CPU oracle, the fused initial-latents op against its torch formula, the img2img trajectory against the oracle modules composed
like diffusers' StableDiffusionXLImg2ImgPipeline, plan reuse between text-to-image and img2img, and IPAdapterXL.generate's
kwargs reaching the img2img pipeline."""
import pytest
import torch
import torch.nn.functional as F

from conftest import record_parity, rel_rms
from oracle.detfill import det_fill, det_randn
from oracle.pipeline import denoise as oracle_denoise
from oracle.vae import AutoencoderKL as OracleVAE
from oracle.vae import tiny_vae_config

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ref_conv(x, w, b):
    """x NHWC fp32 -> NHWC: diffusers Downsample2D(padding=0)"""
    return F.conv2d(F.pad(x.permute(0, 3, 1, 2), (0, 1, 0, 1)), w, b, stride=2).permute(0, 2, 3, 1)


# (B, H, W, C): the encoder's three downsamplers at a 1024^2 image, a ragged and an odd input (Ho = (H - 2) // 2 + 1)
PAD_CASES = [(1, 1024, 1024, 128), (1, 512, 512, 256), (1, 256, 256, 512), (1, 250, 126, 128), (2, 125, 93, 64)]
# every conv-capable 16-bit variant of the default library a tuning.json entry or the heuristic can hand a stride-2 conv (None = _config's pick)
VARIANTS = [None, (64, 64, 1), (128, 128, 1), (128, 64, 1), (64, 128, 1), (64, 128, 4), (128, 128, 2), (3064, 64, 1), (5258, 320, 1),
            (1464, 160, 1), (2464, 160, 1), (2464, 160, 2), (24128, 160, 1), (23256, 160, 1)]


@pytest.mark.parametrize("case", PAD_CASES)
def test_pad_mode_conv_matches_right_bottom_padded_conv(case):
    from imagharmony_amd import lib as L
    from imagharmony_amd.ctx import Ctx
    B, H, W, C_ = case
    g = torch.Generator().manual_seed(sum(case))
    x = torch.randn(B, H, W, C_, generator=g)
    w = torch.randn(C_, C_, 3, 3, generator=g) * (9 * C_) ** -0.5
    b = torch.randn(C_, generator=g) * 0.1
    wp = w.permute(0, 2, 3, 1).reshape(C_, 9 * C_).contiguous()
    Ho, Wo = (H - 2) // 2 + 1, (W - 2) // 2 + 1
    ran = []
    for dtype, tol in ((torch.bfloat16, 1e-2), (torch.float16, 2e-3)):
        ctx = Ctx(DEV, dtype)
        xd, wd, bd = x.to(DEV, dtype), wp.to(DEV, dtype), b.to(DEV, dtype)
        ref = _ref_conv(xd.float().cpu(), wd.float().cpu().view(C_, 3, 3, C_).permute(0, 3, 1, 2), bd.float().cpu())
        for cfg in (VARIANTS if dtype == torch.bfloat16 else [None]):          # every listed variant must take the launch
            y = ctx.conv3x3(xd, wd, bias=bd, stride=2, pad=1, cfg=cfg)
            torch.cuda.synchronize()
            assert tuple(y.shape) == (B, Ho, Wo, C_)
            r = rel_rms(y.float().cpu(), ref)
            assert r < tol, (case, dtype, cfg, r)
            ran.append((dtype, cfg))
        # the variants that do not implement mode 1 -- the LDS-halo conv3x3 (stride 1), the ping-pong and the sixteen-wave Linear forms --
        # refuse it with IMH_ERR_ARG instead of returning a silently wrong result
        for cfg in ((7128, 320, 1), (7256, 160, 1), (8256, 256, 1), (9128, 320, 1), (9256, 320, 1), (26256, 320, 1)):
            with pytest.raises(L.ImhError, match=r"status -1\)"):
                ctx.conv3x3(xd, wd, bias=bd, stride=2, pad=1, cfg=cfg)
    assert ran == [(torch.bfloat16, c) for c in VARIANTS] + [(torch.float16, None)]
    # fp32: the bf16 hi / lo kernel (default) and the exact fp32 MFMA kernel
    ctx = Ctx(DEV, torch.bfloat16)
    ref = _ref_conv(x, w, b)
    lib = L.load()
    try:
        for exact, tol in ((0, 3e-5), (1, 2e-6)):
            lib.imh_debug_set(10, exact)
            y = ctx.f32_conv3x3(x.to(DEV), wp.to(DEV), bias=b.to(DEV), stride=2, pad=1)
            torch.cuda.synchronize()
            r = rel_rms(y.cpu(), ref)
            print(f"pad-mode conv {case} fp32 exact={exact}: rel-rms {r:.2e}")
            assert tuple(y.shape) == (B, Ho, Wo, C_) and r < tol, (case, exact, r)
    finally:
        lib.imh_debug_set(10, 0)


def build_vae_pair(dtype):
    from imagharmony_amd.vae import AutoencoderKL, VAEConfig
    ocfg = tiny_vae_config()
    ov = det_fill(OracleVAE(ocfg), 3).eval()
    hv = AutoencoderKL(VAEConfig(**{k: getattr(ocfg, k) for k in VAEConfig.__dataclass_fields__}), with_encoder=True)
    hv.load_state_dict(ov.state_dict(), strict=True)
    return ov, hv.to(DEV, dtype)


@pytest.mark.parametrize("shape", [(2, 3, 256, 256), (1, 3, 200, 136)])
def test_vae_encoder_matches_oracle(shape):
    """fp32 mode (a float32 module) <= 1e-4 and bf16 <= 3e-2 rel-RMS on the moments quant_conv(encoder(x))"""
    x = (torch.rand(shape, generator=torch.Generator().manual_seed(1)) * 2 - 1)
    for dtype, tol in ((torch.float32, 1e-4), (torch.bfloat16, 3e-2)):
        ov, hv = build_vae_pair(dtype)
        with torch.no_grad():
            ref = ov.quant_conv(ov.encoder(x))
        dist = hv.encode(x.to(DEV)).latent_dist
        got = dist.parameters.cpu()
        assert got.shape == ref.shape == (shape[0], 8, shape[2] // 8, shape[3] // 8)
        r = rel_rms(got, ref)
        print(f"vae encode {shape} {dtype}: rel-rms {r:.2e}")
        assert r < tol, (dtype, r)
        m, lv = ref.chunk(2, 1)
        assert rel_rms(dist.mean.cpu(), m) < tol and rel_rms(dist.logvar.cpu(), lv.clamp(-30, 20)) < tol
        assert torch.equal(dist.std, torch.exp(0.5 * dist.logvar)) and torch.equal(dist.mode(), dist.mean)
        g1, g2 = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
        want = dist.mean + dist.std * torch.randn(dist.mean.shape, generator=g2).to(DEV)
        assert torch.equal(dist.sample(g1), want)


def test_full_sdxl_vae_encoder_at_1024_matches_oracle_in_fp32_mode():
    """The full SDXL VAE config (128 / 256 / 512 / 512 channels) at a 1024^2 image, as the reference runs it: a float16 module with
    force_upcast encodes in fp32 (the conv_in with Cin padded to 16, the pad-mode downsamplers, the 16384-token mid-block attention).
    The oracle holds the same fp16-rounded weights in fp32; bound as test_gpu_vae's fp32 mode (1e-4)."""
    from imagharmony_amd.vae import AutoencoderKL, VAEConfig
    from oracle.vae import VAEConfig as OracleVAEConfig
    ov = det_fill(OracleVAE(OracleVAEConfig()), 3).eval()
    with torch.no_grad():
        for p in ov.parameters():
            p.copy_(p.half().float())                       # the weights a float16 checkpoint holds, exactly
    hv = AutoencoderKL(VAEConfig(), with_encoder=True)
    hv.load_state_dict(ov.state_dict(), strict=True)
    hv = hv.to(DEV, torch.float16)
    assert hv.precision_for() == "fp32"
    x = torch.rand(1, 3, 1024, 1024, generator=torch.Generator().manual_seed(7)) * 2 - 1
    got = hv.encode(x.to(DEV)).latent_dist.parameters.cpu()
    with torch.no_grad():
        ref = ov.quant_conv(ov.encoder(x))
    assert got.shape == ref.shape == (1, 8, 128, 128) and torch.isfinite(got).all()
    r = rel_rms(got, ref)
    print(f"vae encode full SDXL config 1024^2 fp32 mode: rel-rms {r:.2e}")
    record_parity("vae_encode.full_1024.fp32", r, 1e-4)
    assert r < 1e-4, r


def _oracle_tiled_encode(ov, x):
    """diffusers 0.30 AutoencoderKL.tiled_encode over the oracle encoder (in-place blends)"""
    overlap = int(ov.tile_sample_min_size * (1 - ov.tile_overlap_factor))
    extent = int(ov.tile_latent_min_size * ov.tile_overlap_factor)
    limit = ov.tile_latent_min_size - extent
    rows = []
    for i in range(0, x.shape[2], overlap):
        rows.append([ov.quant_conv(ov.encoder(x[:, :, i:i + ov.tile_sample_min_size, j:j + ov.tile_sample_min_size]))
                     for j in range(0, x.shape[3], overlap)])
    out_rows = []
    for i, row in enumerate(rows):
        out = []
        for j, t in enumerate(row):
            if i > 0:
                t = ov.blend_v(rows[i - 1][j], t, extent)
            if j > 0:
                t = ov.blend_h(row[j - 1], t, extent)
            out.append(t[:, :, :limit, :limit])
        out_rows.append(torch.cat(out, dim=3))
    return torch.cat(out_rows, dim=2)


def test_vae_tiled_encode_with_ragged_edge_tiles_matches_oracle_tiled():
    x = torch.rand(1, 3, 448, 328, generator=torch.Generator().manual_seed(2)) * 2 - 1      # 256-px tiles at stride 192: ragged edges
    for dtype, tol in ((torch.float32, 1e-4), (torch.bfloat16, 3e-2)):
        ov, hv = build_vae_pair(dtype)
        hv.enable_tiling()
        with torch.no_grad():
            ref = _oracle_tiled_encode(ov, x)
        got = hv.encode(x.to(DEV)).latent_dist.parameters.cpu()
        assert got.shape == ref.shape == (1, 8, 56, 41)
        r = rel_rms(got, ref)
        print(f"vae tiled encode {dtype}: rel-rms {r:.2e}")
        assert r < tol, (dtype, r)


@pytest.mark.parametrize("M,N,S", [(1, 1, 1), (1, 1, 3), (2, 4, 4), (2, 2, 6)])
def test_img2img_init_op_matches_torch_formula(M, N, S):
    from imagharmony_amd.ctx import Ctx
    from imagharmony_amd.schedulers import DDIMScheduler, EulerDiscreteScheduler
    g = torch.Generator().manual_seed(M * 100 + N * 10 + S)
    h, w = 13, 22
    mo = torch.randn(M, h, w, 8, generator=g) * 3
    mo[..., 4:] = torch.randn(M, h, w, 4, generator=g) * 20            # logvar beyond the clamp at both ends
    n1, n2 = torch.randn(N, 4, h, w, generator=g), torch.randn(S, 4, h, w, generator=g)
    ctx = Ctx(DEV, torch.bfloat16)
    for sch in (DDIMScheduler(), EulerDiscreteScheduler()):
        sch.set_timesteps(30)
        a, b = sch.add_noise_coefficients(21)
        out = torch.empty(S, 4, h, w, device=DEV)
        ctx.img2img_init(out, mo.to(DEV), n1.to(DEV), n2.to(DEV), 0.13025, a, b)
        m = mo.permute(0, 3, 1, 2)
        mean, logvar = m[:, :4], m[:, 4:].clamp(-30.0, 20.0)
        idx_m, idx_n = torch.arange(S) % M, torch.arange(S) % N
        z = 0.13025 * (mean[idx_m] + torch.exp(0.5 * logvar[idx_m]) * n1[idx_n])
        assert torch.allclose(out.cpu(), a * z + b * n2, rtol=1e-5, atol=1e-5), type(sch).__name__


class _FromStep:
    """the oracle scheduler run from step t_start (diffusers get_timesteps + set_begin_index): no init_noise_sigma scaling"""
    order = 1
    init_noise_sigma = 1.0

    def __init__(self, inner, t_start):
        self.inner, self.t_start = inner, t_start

    def set_timesteps(self, n, device=None):
        self.inner.set_timesteps(n)
        self.timesteps = self.inner.timesteps[self.t_start:]
        if hasattr(self.inner, "_i"):
            self.inner._i = self.t_start

    def scale_model_input(self, x, t):
        return self.inner.scale_model_input(x, t)

    def step(self, eps, t, x, **kw):
        return self.inner.step(eps, t, x)


def _img2img_pair(dtype, sched, strength, steps, cg_end=1.0, S=1, seed=11, cg_start=0.0):
    """HIP img2img pipeline vs oracle: oracle encoder -> restated prepare_latents (same draws) -> loop over timesteps[t_start:]"""
    from imagharmony_amd import schedulers as hs
    from imagharmony_amd.pipeline import StableDiffusionXLImg2ImgCustomPipeline
    from oracle.schedulers import DDIMScheduler as OracleDDIM
    from oracle.schedulers import EulerDiscreteScheduler as OracleEuler
    from smoke_impl import build_pair
    ou, hu, ocfg = build_pair(DEV, dtype)
    ov, hv = build_vae_pair(torch.float32)
    hw = 32
    img = torch.rand(1, 3, hw * 8, hw * 8, generator=torch.Generator().manual_seed(3)) * 2 - 1
    cd = ocfg.cross_attention_dim
    pe, ne = det_randn((S, 81, cd), 4), det_randn((S, 81, cd), 5)
    po, no = det_randn((S, ocfg.pooled_dim), 6), det_randn((S, ocfg.pooled_dim), 7)
    hsch = hs.DDIMScheduler() if sched == "ddim" else hs.EulerDiscreteScheduler()
    pipe = StableDiffusionXLImg2ImgCustomPipeline(hu, scheduler=hsch, device=DEV, dtype=dtype, vae=hv)
    out = pipe(image=img, strength=strength, prompt_embeds=pe, negative_prompt_embeds=ne, pooled_prompt_embeds=po,
               negative_pooled_prompt_embeds=no, num_inference_steps=steps, guidance_scale=5.0, control_guidance_start=cg_start,
               control_guidance_end=cg_end, generator=torch.Generator().manual_seed(seed), output_type="latent").images.float().cpu()
    # the oracle side
    hsch.set_timesteps(steps)
    init = min(int(steps * strength), steps)
    t_start = max(steps - init, 0)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        mom = ov.quant_conv(ov.encoder(img))
    mean, logvar = mom.chunk(2, 1)
    z = (mean + torch.exp(0.5 * logvar.clamp(-30, 20)) * torch.randn(mean.shape, generator=g)) * ov.config.scaling_factor
    z = torch.cat([z] * S, 0)
    a, b = hsch.add_noise_coefficients(t_start)
    x0 = z * a + torch.randn(z.shape, generator=g) * b
    osch = _FromStep(OracleDDIM() if sched == "ddim" else OracleEuler(), t_start)
    with torch.no_grad():
        ref = oracle_denoise(ou, osch, x0, pe, ne, po, no, hw * 8, hw * 8, num_inference_steps=steps, guidance_scale=5.0,
                             control_guidance_start=cg_start, control_guidance_end=cg_end)       # the window counts timesteps[t_start:]
    return out, ref, pipe, (pe, ne, po, no)


# strength < 1 with a gating window (the last two cases): the IP-scale window counts the truncated list -- euler 0.6 x 10 runs steps 4..9 and
# gates the last three of those six (over the full list of ten it would gate four); ddim 0.5 x 8 runs steps 4..7 and gates the first two
# (over the full list, none)
@pytest.mark.parametrize("dtype,sched,strength,steps,cg_start,cg_end,tol", [
    (torch.float16, "ddim", 0.3, 10, 0.0, 1.0, 1e-2), (torch.float16, "euler", 0.3, 10, 0.0, 1.0, 1e-2),
    (torch.float16, "ddim", 1.0, 3, 0.0, 0.5, 1e-2), (torch.float16, "euler", 1.0, 3, 0.0, 1.0, 1e-2),
    (torch.bfloat16, "ddim", 0.6, 5, 0.0, 1.0, 4e-2),
    (torch.float16, "euler", 0.6, 10, 0.0, 0.6, 1e-2), (torch.float16, "ddim", 0.5, 8, 0.3, 1.0, 1e-2)])
def test_img2img_trajectory_matches_oracle(dtype, sched, strength, steps, cg_start, cg_end, tol):
    out, ref, pipe, (pe, ne, po, no) = _img2img_pair(dtype, sched, strength, steps, cg_end, cg_start=cg_start)
    r = rel_rms(out, ref)
    print(f"img2img {dtype} {sched} strength {strength} steps {steps} cg {cg_start}-{cg_end}: rel-rms {r:.2e}")
    assert torch.isfinite(out).all() and r < tol, r
    if strength < 1.0:
        from imagharmony_amd.pipeline import StableDiffusionXLCustomPipeline, randn_latents
        t2i = StableDiffusionXLCustomPipeline.__call__(
            pipe, prompt_embeds=pe, negative_prompt_embeds=ne, pooled_prompt_embeds=po, negative_pooled_prompt_embeds=no,
            height=256, width=256, num_inference_steps=steps, guidance_scale=5.0, control_guidance_start=cg_start, control_guidance_end=cg_end,
            latents=randn_latents((1, 4, 32, 32), torch.Generator().manual_seed(11)), output_type="latent").images.float().cpu()
        assert rel_rms(out, t2i) > 0.1


def test_text2img_img2img_alternation_on_one_pipeline_equals_fresh_pipelines():
    from imagharmony_amd import schedulers as hs
    from imagharmony_amd.pipeline import StableDiffusionXLCustomPipeline, StableDiffusionXLImg2ImgCustomPipeline
    from smoke_impl import build_pair
    dtype = torch.bfloat16
    ou, hu, ocfg = build_pair(DEV, dtype)
    _, hv = build_vae_pair(torch.float32)
    cd = ocfg.cross_attention_dim
    emb = dict(prompt_embeds=det_randn((2, 81, cd), 4), negative_prompt_embeds=det_randn((2, 81, cd), 5),
               pooled_prompt_embeds=det_randn((2, ocfg.pooled_dim), 6), negative_pooled_prompt_embeds=det_randn((2, ocfg.pooled_dim), 7),
               guidance_scale=5.0, output_type="latent")
    img = torch.rand(1, 3, 256, 256, generator=torch.Generator().manual_seed(3))
    t2i = lambda p: StableDiffusionXLCustomPipeline.__call__(p, height=256, width=256, num_inference_steps=4,
                                                             generator=torch.Generator().manual_seed(1), **emb).images.clone()
    i2i = lambda p: p(image=img, strength=0.5, num_inference_steps=4, generator=[torch.Generator().manual_seed(s) for s in (1, 2)],
                      **emb).images.clone()
    for sch in (hs.DDIMScheduler, hs.EulerDiscreteScheduler):
        new = lambda: StableDiffusionXLImg2ImgCustomPipeline(hu, scheduler=sch(), device=DEV, dtype=dtype, vae=hv)
        one = new()
        seq = [t2i(one), i2i(one), t2i(one)]
        fresh = [t2i(new()), i2i(new()), t2i(new())]
        for a, b in zip(seq, fresh):
            assert torch.equal(a, b), sch.__name__
        assert torch.equal(seq[0], seq[2]) and not torch.equal(seq[0], seq[1])
        assert not torch.equal(seq[1][0], seq[1][1])                      # a generator list: one posterior draw per sample


def test_ipadapterxl_generate_reaches_the_img2img_pipeline():
    from PIL import Image
    import numpy as np
    from imagharmony_amd.ip_adapter import IPAdapterXL
    from imagharmony_amd.modules import HarmonyAttention
    from imagharmony_amd.pipeline import StableDiffusionXLImg2ImgCustomPipeline
    from imagharmony_amd.utils import get_generator
    from smoke_impl import build_pair
    dtype = torch.bfloat16
    ou, hu, ocfg = build_pair(DEV, dtype)
    _, hv = build_vae_pair(torch.float32)
    pipe = StableDiffusionXLImg2ImgCustomPipeline(hu, device=DEV, dtype=dtype, vae=hv)
    cd = ocfg.cross_attention_dim
    ha = det_fill(HarmonyAttention(image_hidden_size=128, text_context_dim=cd, inter_dim=512, cross_heads=8,
                                   reshape_blocks=8, cross_value_dim=64), 3)
    ip = IPAdapterXL(pipe, None, None, DEV, num_tokens=4, inference=True, number_class_crossattention=ha, dtype=dtype,
                     clip_embeddings_dim=128)
    det_fill(ip.image_proj_model, 5)
    init = Image.fromarray((np.random.RandomState(0).rand(258, 290, 3) * 255).astype("uint8"))     # 290 x 258 -> 288 x 256 (multiples of 8)
    embeds = (det_randn((1, 77, cd), 1), det_randn((1, 77, cd), 2), det_randn((1, ocfg.pooled_dim), 3),
              det_randn((1, ocfg.pooled_dim), 4))
    kw = dict(clip_image_embeds=det_randn((1, 128), 5), prompt_embeds=embeds, extra_prompt_embeds=det_randn((1, 77, cd), 6),
              num_samples=1, seed=42, num_inference_steps=4, guidance_scale=5.0, image=init, strength=0.5)
    pil = ip.generate(output_type="pil", **kw)
    assert len(pil) == 1 and all(isinstance(p, Image.Image) and p.size == (288, 256) for p in pil)
    seen = {}

    class Spy:
        def __getattr__(self, k):
            return getattr(pipe, k)

        def __call__(self, **a):
            seen.update(a)
            return pipe(**a)
    ip.pipe = Spy()
    lat = ip.generate(output_type="latent", **kw)
    ip.pipe = pipe
    assert seen["strength"] == 0.5 and seen["image"] is init and lat.shape == (1, 4, 32, 36)
    direct = pipe(**{**seen, "generator": get_generator(42, "cpu")}).images
    assert torch.equal(lat, direct)
    with pytest.raises(NotImplementedError):
        ip.generate_pns([1, 2], clip_image_embeds=det_randn((1, 128), 5), prompt_embeds=embeds, output_type="latent")
