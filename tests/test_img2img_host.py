"""CPU (no GPU): the host side of SDXL image-to-image -- diffusers 0.30 get_timesteps truncation and add-noise coefficients of
both product schedulers against a restatement, VaeImageProcessor.preprocess rules, the opt-in VAE encoder's parameters and
loading, the pad-mode variant filter and the img2img pipeline's argument refusals."""
import numpy as np
import pytest
import torch


def _restated_alphas_cumprod():
    # diffusers scaled_linear betas, fp32 cumprod (DDIMScheduler / EulerDiscreteScheduler __init__)
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float32) ** 2
    return torch.cumprod(1.0 - betas, dim=0)


@pytest.mark.parametrize("n", [10, 30, 50])
@pytest.mark.parametrize("strength", [0.05, 0.3, 0.6, 1.0])
def test_get_timesteps_and_add_noise_coefficients_match_restatement(n, strength):
    from imagharmony_amd.schedulers import DDIMScheduler, EulerDiscreteScheduler, get_timesteps
    init = min(int(n * strength), n)
    t_start = max(n - init, 0)
    ac = _restated_alphas_cumprod()
    for sch in (DDIMScheduler(), EulerDiscreteScheduler()):
        sch.set_timesteps(n)
        if n - t_start < 1:
            with pytest.raises(ValueError):
                get_timesteps(sch, n, strength)
            continue
        ts, ts0 = get_timesteps(sch, n, strength)
        assert ts0 == t_start and torch.equal(ts, sch.timesteps[t_start:]) and len(ts) == init
        a, b = sch.add_noise_coefficients(t_start)
        t = int(sch.timesteps[t_start])
        if isinstance(sch, DDIMScheduler):
            assert (a, b) == (float(ac[t] ** 0.5), float((1 - ac[t]) ** 0.5))
        else:
            # leading spacing, steps_offset 1, sigmas interpolated at the (float) timesteps; add_noise at begin_index t_start
            sig = np.interp(sch.timesteps.numpy(), np.arange(1000), (((1 - ac.double()) / ac.double()) ** 0.5).numpy())
            assert a == 1.0 and abs(b - float(np.float32(sig[t_start]))) <= 1e-6 * max(1.0, b)
        x, nz = torch.randn(2, 4, 8, 8), torch.randn(2, 4, 8, 8)
        assert torch.equal(sch.add_noise(x, nz, t_start), x * a + nz * b)


def test_get_timesteps_refuses_strength_outside_unit_interval():
    from imagharmony_amd.schedulers import DDIMScheduler, get_timesteps
    s = DDIMScheduler()
    s.set_timesteps(30)
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            get_timesteps(s, 30, bad)


def test_preprocess_follows_vae_image_processor_rules():
    from PIL import Image
    from imagharmony_amd.vae import preprocess
    rs = np.random.RandomState(0)
    arr = (rs.rand(48, 64, 3) * 255).astype("uint8")
    x = preprocess(Image.fromarray(arr))                                     # sides multiples of 8: no resize
    assert x.shape == (1, 3, 48, 64) and x.dtype == torch.float32
    assert torch.equal(x, 2.0 * torch.from_numpy(arr.astype(np.float32) / 255.0).permute(2, 0, 1)[None] - 1.0)
    odd = Image.fromarray((rs.rand(50, 67, 3) * 255).astype("uint8"))      # 67 x 50 -> 64 x 48, Lanczos
    y = preprocess([odd, odd])
    want = np.asarray(odd.resize((64, 48), resample=Image.LANCZOS)).astype(np.float32) / 255.0
    assert y.shape == (2, 3, 48, 64)
    assert torch.equal(y[1], 2.0 * torch.from_numpy(want).permute(2, 0, 1) - 1.0)
    t01 = torch.rand(2, 3, 16, 24)
    assert torch.equal(preprocess(t01), 2.0 * t01 - 1.0)                    # [0, 1] tensor: normalised
    tpm = torch.rand(1, 3, 16, 24) * 2 - 1
    assert torch.equal(preprocess(tpm), tpm)                                # min() < 0: already in [-1, 1]
    with pytest.raises(ValueError):
        preprocess("image.png")


def test_vae_encoder_is_opt_in_and_loads_strictly():
    from imagharmony_amd.vae import AutoencoderKL, VAEConfig
    from oracle.detfill import det_fill
    from oracle.vae import AutoencoderKL as OracleVAE
    from oracle.vae import tiny_vae_config
    ocfg = tiny_vae_config()
    cfg = VAEConfig(**{k: getattr(ocfg, k) for k in VAEConfig.__dataclass_fields__})
    ov = det_fill(OracleVAE(ocfg), 3)
    full = AutoencoderKL(cfg, with_encoder=True)
    missing, unexpected = full.load_state_dict(ov.state_dict(), strict=True)
    assert not missing and not unexpected
    assert set(full.state_dict()) == set(ov.state_dict())                   # diffusers' key names, encoder.* and quant_conv.* included
    assert torch.equal(full.encoder.down_blocks[0].downsamplers[0].conv.weight, ov.encoder.down_blocks[0].downsamplers[0].conv.weight)
    assert torch.equal(full.quant_conv.bias, ov.quant_conv.bias)
    dec = AutoencoderKL(cfg)                                                # default: decode-only, encoder keys dropped
    missing, unexpected = dec.load_state_dict(ov.state_dict(), strict=True)
    assert not missing and not unexpected and not hasattr(dec, "encoder")
    assert all(not k.startswith(("encoder.", "quant_conv.")) for k in dec.state_dict())
    with pytest.raises(RuntimeError):                                       # the encoder's keys are required once it exists
        AutoencoderKL(cfg, with_encoder=True).load_state_dict(dec.state_dict(), strict=True)
    with pytest.raises(NotImplementedError):
        dec.encode(torch.zeros(1, 3, 64, 64))
    a, b = AutoencoderKL(cfg).init_random_(7), AutoencoderKL(cfg, with_encoder=True).init_random_(7)
    sa = a.state_dict()
    for k, v in sa.items():
        assert torch.equal(v, b.state_dict()[k]), k                        # decoder + post_quant_conv bit-equal either way


def test_pad_mode_variant_filter_falls_back_from_the_halo_entry():
    """a tuning.json stride-2 entry that names an LDS-halo variant (stride-1 only) must not be handed a pad-mode launch"""
    from imagharmony_amd import lib
    from imagharmony_amd.ctx import Ctx
    assert not Ctx._variant_ok(7128, 1, 0, 1, 2, False, pad=1)
    assert not Ctx._variant_ok(8256, 1, 0, 1, 2, False, pad=1)
    for bm in (64, 128, 3064, 5064, 1464, 2464, 24128, 23256):
        assert Ctx._variant_ok(bm, 1, 0, 1, 2, False, pad=1), bm
    c = Ctx.__new__(Ctx)
    c.lib = lib.load()
    M, N, K = 1 * 512 * 512, 128, 9 * 128
    c.tuning = {(M, N, K, 1, 2): [7128, 320, 1], (M, N, K, 1): [7128, 320, 1]}
    bm, bn, sp = c._config(M, N, K, 1, 0, stride=2, pad=1)
    assert bm not in Ctx._HALO and Ctx._variant_ok(bm, sp, 0, 1, 2, False, pad=1)
    c.tuning = {(M, N, K, 1, 2): [128, 64, 1]}
    assert c._config(M, N, K, 1, 0, stride=2, pad=1) == (128, 64, 1)


def test_img2img_pipeline_argument_checks_need_no_gpu():
    from imagharmony_amd.pipeline import StableDiffusionXLImg2ImgCustomPipeline
    from imagharmony_amd.schedulers import DDIMScheduler
    from imagharmony_amd.vae import AutoencoderKL, VAEConfig
    pipe = StableDiffusionXLImg2ImgCustomPipeline.__new__(StableDiffusionXLImg2ImgCustomPipeline)
    pipe.vae = pipe.vae_decode = None
    pipe.scheduler = DDIMScheduler()
    img = torch.rand(1, 3, 64, 64)
    kw = dict(prompt_embeds=torch.zeros(1, 81, 8), pooled_prompt_embeds=torch.zeros(1, 8), output_type="latent")
    with pytest.raises(NotImplementedError, match="denoising_start"):
        pipe(image=img, denoising_start=0.5, **kw)
    with pytest.raises(NotImplementedError, match="eta"):
        pipe(image=img, eta=0.5, **kw)
    with pytest.raises(NotImplementedError, match="prompt_2"):
        pipe(image=img, prompt_2="x", **kw)
    with pytest.raises(NotImplementedError, match="latent"):
        pipe(image=torch.rand(1, 4, 8, 8), **kw)
    with pytest.raises(NotImplementedError, match="needs a VAE"):
        pipe(image=img, prompt_embeds=torch.zeros(1, 81, 8))
    with pytest.raises(ValueError, match="strength"):
        pipe(image=img, strength=1.5, **kw)
    with pytest.raises(NotImplementedError, match="with_encoder"):
        pipe(image=img, **kw)
    pipe.vae = AutoencoderKL(VAEConfig(block_out_channels=(64, 64), layers_per_block=1, sample_size=64), with_encoder=True)
    with pytest.raises(ValueError, match="no denoising step"):
        pipe(image=img, strength=0.05, num_inference_steps=10, **kw)
    with pytest.raises(ValueError, match="duplicate"):
        pipe(image=torch.rand(2, 3, 64, 64), prompt_embeds=torch.zeros(3, 81, 8), pooled_prompt_embeds=torch.zeros(3, 8), output_type="latent")
    import inspect
    ps = inspect.signature(StableDiffusionXLImg2ImgCustomPipeline.__call__).parameters
    assert ps["strength"].default == 0.3 and ps["num_inference_steps"].default == 50 and ps["output_type"].default == "pil"
