"""CPU (no GPU): the host side of SDXL inpainting -- the per-schedule blend table against a restatement of diffusers 0.30
StableDiffusionXLInpaintPipeline's add_noise(image_latents, noise, timesteps[i + 1]), mask_processor.preprocess and the latent
mask against torch restatements, the inpaint pipeline's argument refusals, dry recordings of a 9-channel conv_in, and the ABI 11
fields in header and binding."""
import dataclasses
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _restated_alphas_cumprod():
    # diffusers scaled_linear betas, fp32 cumprod (DDIMScheduler / EulerDiscreteScheduler __init__)
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float32) ** 2
    return torch.cumprod(1.0 - betas, dim=0)


def _restated_add_noise_pair(kind, n, row):
    """(a, b) of scheduler.add_noise(x, noise, timesteps[row]) = a x + b noise under leading spacing, steps_offset 1: DDIM reads
    alphas_cumprod[t]; Euler (begin index set, or after a step) reads sigmas[row], interpolated at the float timesteps"""
    ac = _restated_alphas_cumprod()
    ts = (np.arange(0, n) * (1000 // n)).round()[::-1].copy().astype(np.int64) + 1
    if kind == "ddim":
        a = ac[int(ts[row])]
        return float(a ** 0.5), float((1 - a) ** 0.5)
    sig = np.interp(ts.astype(np.float32), np.arange(1000), (((1 - ac.double()) / ac.double()) ** 0.5).numpy())
    return 1.0, float(np.float32(sig[row]))


@pytest.mark.parametrize("kind", ["ddim", "euler"])
@pytest.mark.parametrize("strength", [1.0, 0.5, 0.3])
@pytest.mark.parametrize("denoising_end", [None, 0.8])
def test_blend_table_matches_restatement(kind, strength, denoising_end):
    """row r = add_noise_coefficients(r + 1) for every row but the last that runs, which is (1, 0); the last running row is n - 1 as
    set_schedule counts n under denoising_end; the rows that run are t_start .. n - 1 whatever the strength"""
    from imagharmony_amd.denoise import DenoiseEngine
    from imagharmony_amd.schedulers import DDIMScheduler, EulerDiscreteScheduler, get_timesteps
    N = 30
    sch = DDIMScheduler() if kind == "ddim" else EulerDiscreteScheduler()
    sch.set_timesteps(N)
    _, t_start = get_timesteps(sch, N, strength)
    assert t_start == N - min(int(N * strength), N)
    n = N
    if denoising_end is not None:                       # set_schedule's count: timesteps at or above the cut-off, at least t_start
        cutoff = int(round(1000 - denoising_end * 1000))
        n = max(int((sch.tables()["timesteps"] >= cutoff).sum().item()), t_start)
        assert t_start < n < N
    tab = DenoiseEngine.blend_table(sch, N, n)
    assert tab.shape == (N, 2) and tab.dtype == torch.float32
    for r in range(t_start, n - 1):
        want = _restated_add_noise_pair(kind, N, r + 1)
        got = (float(tab[r, 0]), float(tab[r, 1]))
        assert got == tuple(float(np.float32(v)) for v in sch.add_noise_coefficients(r + 1)), r
        assert abs(got[0] - want[0]) <= 1e-6 and abs(got[1] - want[1]) <= 1e-6 * max(1.0, want[1]), (r, got, want)
    assert tuple(tab[n - 1].tolist()) == (1.0, 0.0)
    assert torch.isfinite(tab).all()


def test_mask_preprocessing_follows_mask_processor_rules():
    from PIL import Image
    from imagharmony_amd.vae import latent_mask, preprocess_mask
    rs = np.random.RandomState(0)
    H, W = 48, 64
    arr = (rs.rand(H, W) * 255).astype("uint8")
    arr[0, :4] = (126, 127, 128, 129)                                       # 127 / 255 < 0.5 <= 128 / 255
    want = torch.from_numpy((arr.astype(np.float32) / 255.0 >= 0.5).astype(np.float32))[None, None]
    m_l = preprocess_mask(Image.fromarray(arr, mode="L"), H, W)
    m_rgb = preprocess_mask(Image.fromarray(np.stack([arr] * 3, -1), mode="RGB"), H, W)       # grey RGB -> "L" keeps the value
    m_t = preprocess_mask(torch.from_numpy(arr.astype(np.float32) / 255.0), H, W)
    for m in (m_l, m_rgb, m_t):
        assert m.shape == (1, 1, H, W) and m.dtype == torch.float32
        assert torch.equal(m, want)
    assert m_l[0, 0, 0, :4].tolist() == [0.0, 0.0, 1.0, 1.0]
    # the threshold is at exactly 0.5: < 0.5 -> 0, else 1
    edge = torch.tensor([[0.0, 0.49999997, 0.5, 0.50000006, 1.0, 0.25, 0.75, 0.5]]).repeat(8, 1)
    assert preprocess_mask(edge, 8, 8)[0, 0, 0].tolist() == [0.0, 0.0, 1.0, 1.0, 1.0, 0.0, 1.0, 1.0]
    # tensor shapes: [B, H, W] gets its channel axis at 1, [B, 1, H, W] is taken as is; a list of PIL masks is a batch
    t3 = torch.rand(2, H, W, generator=torch.Generator().manual_seed(1))
    assert torch.equal(preprocess_mask(t3, H, W), (t3 >= 0.5).float().unsqueeze(1))
    assert torch.equal(preprocess_mask(t3.unsqueeze(1), H, W), (t3 >= 0.5).float().unsqueeze(1))
    two = preprocess_mask([Image.fromarray(arr), Image.fromarray(255 - arr)], H, W)
    assert two.shape == (2, 1, H, W) and torch.equal(two[0], want[0])
    # resized to the image's size by preprocess's rules: PIL Lanczos before the grey conversion, tensors nearest
    big = Image.fromarray((rs.rand(50, 67) * 255).astype("uint8"))
    ref = np.asarray(big.resize((W, H), resample=Image.LANCZOS).convert("L")).astype(np.float32) / 255.0
    assert torch.equal(preprocess_mask(big, H, W), torch.from_numpy((ref >= 0.5).astype(np.float32))[None, None])
    tb = torch.rand(1, 1, 96, 128, generator=torch.Generator().manual_seed(2))
    assert torch.equal(preprocess_mask(tb, H, W), (torch.nn.functional.interpolate(tb, size=(H, W)) >= 0.5).float())
    # the latent mask: nearest, source index floor(i * H / h) -- for multiples of 8 every eighth pixel
    m = preprocess_mask(t3, H, W)
    lm = latent_mask(m, H // 8, W // 8)
    assert lm.shape == (2, 1, H // 8, W // 8) and torch.equal(lm, m[..., ::8, ::8])
    for bad in ("mask.png", torch.rand(1, 3, H, W), torch.rand(1, 1, 1, H, W)):
        with pytest.raises(ValueError):
            preprocess_mask(bad, H, W)


def _bare_pipe():
    from imagharmony_amd.pipeline import StableDiffusionXLInpaintCustomPipeline
    from imagharmony_amd.schedulers import DDIMScheduler
    from imagharmony_amd.unet import UNetConfig

    class _U:
        config = UNetConfig()
    pipe = StableDiffusionXLInpaintCustomPipeline.__new__(StableDiffusionXLInpaintCustomPipeline)
    pipe.vae = pipe.vae_decode = None
    pipe.scheduler = DDIMScheduler()
    pipe.unet = _U()
    return pipe


def test_inpaint_pipeline_argument_checks_need_no_gpu():
    import inspect
    import imagharmony_amd
    from imagharmony_amd.pipeline import StableDiffusionXLCustomPipeline, StableDiffusionXLInpaintCustomPipeline
    from imagharmony_amd.vae import AutoencoderKL, VAEConfig
    assert imagharmony_amd.StableDiffusionXLInpaintCustomPipeline is StableDiffusionXLInpaintCustomPipeline
    assert issubclass(StableDiffusionXLInpaintCustomPipeline, StableDiffusionXLCustomPipeline)
    pipe = _bare_pipe()
    img, mask = torch.rand(1, 3, 64, 64), torch.ones(1, 1, 64, 64)
    kw = dict(prompt_embeds=torch.zeros(1, 81, 8), pooled_prompt_embeds=torch.zeros(1, 8), output_type="latent")
    with pytest.raises(NotImplementedError, match="padding_mask_crop"):
        pipe(image=img, mask_image=mask, padding_mask_crop=32, **kw)
    with pytest.raises(NotImplementedError, match="masked_image_latents"):
        pipe(image=img, mask_image=mask, masked_image_latents=torch.zeros(1, 4, 8, 8), **kw)
    with pytest.raises(NotImplementedError, match="latent"):
        pipe(image=torch.rand(1, 4, 8, 8), mask_image=mask, **kw)
    with pytest.raises(NotImplementedError, match="latents="):
        pipe(image=img, mask_image=mask, latents=torch.zeros(1, 4, 8, 8), **kw)
    with pytest.raises(NotImplementedError, match="denoising_start"):
        pipe(image=img, mask_image=mask, denoising_start=0.5, **kw)
    with pytest.raises(NotImplementedError, match="eta"):
        pipe(image=img, mask_image=mask, eta=0.5, **kw)
    with pytest.raises(NotImplementedError, match="needs a VAE"):
        pipe(image=img, mask_image=mask, prompt_embeds=torch.zeros(1, 81, 8))
    with pytest.raises(ValueError, match="mask_image"):
        pipe(image=img, **kw)
    with pytest.raises(ValueError, match="image"):
        pipe(mask_image=mask, **kw)
    with pytest.raises(ValueError, match="mask"):                                       # three channels: not a mask
        pipe(image=img, mask_image=torch.rand(1, 3, 64, 64), **kw)
    with pytest.raises(ValueError, match="strength"):
        pipe(image=img, mask_image=mask, strength=1.5, **kw)
    with pytest.raises(NotImplementedError, match="resize the image"):
        pipe(image=img, mask_image=mask, height=128, width=128, **kw)
    with pytest.raises(NotImplementedError, match="with_encoder"):
        pipe(image=img, mask_image=mask, **kw)
    pipe.vae = AutoencoderKL(VAEConfig(block_out_channels=(64, 64), layers_per_block=1, sample_size=64), with_encoder=True)
    with pytest.raises(ValueError, match="mask batch"):                                 # two masks cannot be repeated to three samples
        pipe(image=img, mask_image=torch.ones(2, 1, 64, 64), prompt_embeds=torch.zeros(3, 81, 8), pooled_prompt_embeds=torch.zeros(3, 8),
             output_type="latent")
    with pytest.raises(ValueError, match="image batch"):
        pipe(image=torch.rand(2, 3, 64, 64), mask_image=mask, prompt_embeds=torch.zeros(3, 81, 8), pooled_prompt_embeds=torch.zeros(3, 8),
             output_type="latent")
    with pytest.raises(ValueError, match="no denoising step"):
        pipe(image=img, mask_image=mask, strength=0.05, num_inference_steps=10, **kw)
    ps = inspect.signature(StableDiffusionXLInpaintCustomPipeline.__call__).parameters
    assert ps["strength"].default == 0.9999 and ps["num_inference_steps"].default == 50 and ps["output_type"].default == "pil"
    assert ps["height"].default is None and ps["width"].default is None
    for k in ("image", "mask_image", "denoising_end", "control_guidance_start", "control_guidance_end", "generator", "callback"):
        assert k in ps, k


def _tiny_unet(in_channels):
    from imagharmony_amd.attention_processor import AttnProcessor2_0, IPAttnProcessor2_0
    from imagharmony_amd.unet import UNet2DConditionModel, UNetConfig
    cfg = UNetConfig(block_out_channels=(64, 128, 256), transformer_layers_per_block=(1, 1, 2),
                     attention_head_dim=(1, 2, 4), cross_attention_dim=256, addition_time_embed_dim=64,
                     projection_class_embeddings_input_dim=128 + 6 * 64, sample_size=32)
    u = UNet2DConditionModel(dataclasses.replace(cfg, in_channels=in_channels)).to(torch.bfloat16)
    procs = {}
    for name in u.attn_processors:
        if name.endswith("attn1.processor"):
            procs[name] = AttnProcessor2_0()
        else:
            hidden = 256 if name.startswith("mid_block") else (
                list(reversed(cfg.block_out_channels))[int(name[len("up_blocks.")])] if name.startswith("up_blocks")
                else cfg.block_out_channels[int(name[len("down_blocks.")])])
            procs[name] = IPAttnProcessor2_0(hidden, 256, num_tokens=4, skip="down_blocks.2.attentions.1" not in name).to(torch.bfloat16)
    u.set_attn_processor(procs)
    return u


def _dry_forward(u, extra):
    from imagharmony_amd.ctx import Ctx
    ctx = Ctx("cpu", torch.bfloat16, record=True, dry=True)
    st = u.prepare_conditioning(ctx, torch.zeros(4, 81, 256), torch.zeros(4, 128), torch.zeros(4, 6))
    n_prep = ctx.lib.imh_plan_size(ctx.plan)
    st.t_value = torch.zeros(4)
    st.latents = torch.zeros(2, 4, 32, 24)
    st.conv_in_extra = extra
    out = u.emit_forward(ctx, st, 2, 32, 24, cfg_dup=True)
    assert out.shape == (4, 32 * 24, 4)
    idx = [i for i, t in enumerate(ctx.tags) if t[2] == "conv_in"]
    assert len(idx) == 1
    return ctx.lib.imh_plan_size(ctx.plan) - n_prep, ctx._ops[idx[0]][1], ctx


def test_nine_channel_conv_in_dry_recording():
    from imagharmony_amd import lib as L
    from imagharmony_amd.unet import UNet2DConditionModel, UNetConfig
    n4, a4, _ = _dry_forward(_tiny_unet(4), None)
    u9 = _tiny_unet(9)
    assert tuple(u9.conv_in.weight.shape) == (64, 9, 3, 3)
    extra = torch.zeros(2, 5, 32, 24)
    n9, a9, ctx9 = _dry_forward(u9, extra)
    assert n9 == n4                                           # the five extra channels cost no launch
    # the 4-channel launch carries what it carried before ABI 11: no second source, channel count left at 0
    assert not a4.x2 and a4.i5 == 0 and (a4.i0, a4.i1, a4.i2, a4.i3, a4.i4) == (2, 32, 24, 64, 4)
    assert not (a4.noise or a4.mask or a4.blend_tab)
    assert a9.x2 == extra.data_ptr() and a9.i5 == 9 and (a9.i0, a9.i1, a9.i2, a9.i3, a9.i4) == (2, 32, 24, 64, 4)
    assert any(t is extra for t in ctx9.keep)                 # the plan keeps the buffer it points at alive
    with pytest.raises(L.ImhError, match="conv_in_extra"):
        _dry_forward(u9, None)
    with pytest.raises(L.ImhError, match="conv_in_extra"):
        _dry_forward(u9, torch.zeros(2, 4, 32, 24))           # wrong channel count
    with pytest.raises(ValueError, match="in_channels"):
        UNet2DConditionModel(UNetConfig(block_out_channels=(64, 128, 256), transformer_layers_per_block=(1, 1, 2), attention_head_dim=(1, 2, 4),
                                        cross_attention_dim=256, addition_time_embed_dim=64,
                                        projection_class_embeddings_input_dim=128 + 6 * 64, sample_size=32, in_channels=5))


def test_abi_11_fields_in_header_and_binding():
    from imagharmony_amd import lib
    hdr = open(os.path.join(ROOT, "include", "imh.h")).read()
    assert int(re.search(r"#define IMH_ABI_VERSION (\d+)", hdr).group(1)) == lib.ABI_VERSION == lib.load().imh_abi_version()
    assert lib.ABI_VERSION >= 11
    names = [f[0] for f in lib.EwArgs._fields_]
    assert names[-4:] == ["x2", "noise", "mask", "blend_tab"] and names[-5] == "dtype"      # appended: the ABI 10 prefix is untouched
    body = re.search(r"typedef struct imh_ew_args \{(.*?)\} imh_ew_args;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert [d.split()[-1].lstrip("*") for d in body.split(";") if d.strip()][-4:] == ["x2", "noise", "mask", "blend_tab"]
    # no thirteenth elementwise op: the blend and the 9-channel conv_in ride on IMH_EW_CFG_STEP / IMH_EW_CONV_IN
    assert len(set(re.findall(r"\bIMH_EW_[A-Z0-9_]+(?= =)", hdr))) == 12
    # the library refuses a blend without its operands, and a conv_in channel count it does not run, as status codes
    l = lib.load()
    e = lib.EwArgs()
    e.y = e.a = e.mask = 64
    e.i0, e.i1, e.i4 = 1, 64, 1
    assert l.imh_elementwise(lib.EW_CFG_STEP, lib.C.byref(e), None) == -1 and b"blend" in l.imh_last_error()
    e = lib.EwArgs()
    e.y = e.a = e.w = 64
    e.i0, e.i1, e.i2, e.i3, e.i4, e.i5 = 1, 8, 8, 64, 1, 5
    assert l.imh_elementwise(lib.EW_CONV_IN, lib.C.byref(e), None) == -1 and b"input channels" in l.imh_last_error()
    e.i5 = 9
    assert l.imh_elementwise(lib.EW_CONV_IN, lib.C.byref(e), None) == -1 and b"x2" in l.imh_last_error()
