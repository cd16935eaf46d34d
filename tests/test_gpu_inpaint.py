"""GPU: SDXL inpainting on the HIP path -- the masked blend behind the CFG + scheduler step against its torch formula, the
9-channel conv_in against F.conv2d, inpaint trajectories in both modes (4-channel UNet: blend in the step; 9-channel UNet:
conv_in over [latents | mask | masked-image latents]) against the oracle modules composed like diffusers 0.30
StableDiffusionXLInpaintPipeline, the exact invariants of the blend, plan hygiene between text-to-image, img2img and inpainting,
IPAdapterXL.generate's kwargs reaching the inpaint pipeline, and one full-width 1024^2 run per mode.

oracle.pipeline.denoise has no hook for the blend, so this file carries its own loop over the oracle UNet and the oracle
schedulers (_oracle_inpaint); the draws are made on the CPU in upstream's order: posterior noise of the image, add-noise noise,
then (9 channels) posterior noise of the masked image."""
import dataclasses
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import record_parity, rel_rms
from oracle import modules as om
from oracle.detfill import det_fill, det_randn
from oracle.pipeline import install_ip_processors as oracle_install
from oracle.pipeline import set_scale as oracle_set_scale
from oracle.schedulers import DDIMScheduler as OracleDDIM
from oracle.schedulers import EulerDiscreteScheduler as OracleEuler
from oracle.sdxl_unet import UNet2DConditionModel as OracleUNet
from oracle.sdxl_unet import tiny_config
from oracle.vae import AutoencoderKL as OracleVAE
from oracle.vae import tiny_vae_config

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


def assert_close(y, ref, dtype, what, k=4.0):
    """the criterion of tests/test_gpu_ops.py: a few output-dtype ulps of the result scale, and 2 ulps rel-RMS"""
    ref, y = ref.float(), y.float()
    scale = ref.abs().max().item() + 1e-6
    err = (y - ref).abs().max().item()
    rms = ((y - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt().clamp_min(1e-12)).item()
    print(f"{what}: max err {err:.3e} (scale {scale:.3e}), rel-rms {rms:.3e}")
    assert math.isfinite(err), f"{what}: non-finite output"
    assert err <= k * EPS[dtype] * scale and rms <= 2 * EPS[dtype], f"{what}: max err {err:.3e} (scale {scale:.3e}), rel-rms {rms:.3e}"


# ------------------------------------------------------------------------------------ the two kernels
@pytest.mark.parametrize("S,Mb", [(1, 1), (3, 1), (3, 3)])
@pytest.mark.parametrize("with_step", [True, False])
def test_blend_op_matches_torch_formula(S, Mb, with_step):
    """IMH_EW_CFG_STEP with a mask: y = (1 - m) (a z + b n) + m y' with (a, b) = blend_tab[*step], y' the CFG + scheduler update
    (with_step) or y itself (a == NULL: the blend alone); fp32, bound of the fp32 step update in tests/test_gpu_ops.py"""
    from imagharmony_amd import lib as L
    from imagharmony_amd.ctx import Ctx
    ctx = Ctx(DEV, torch.bfloat16)
    g = torch.Generator().manual_seed(10 * S + Mb)
    H, W = 13, 22
    HW = H * W
    z, n, lat = (torch.randn(S, 4, H, W, generator=g).to(DEV) for _ in range(3))
    mask = (torch.rand(Mb, 1, H, W, generator=g) < 0.5).float().to(DEV)
    tab = torch.tensor([[0.9, 0.1], [0.7, 0.6], [1.0, 14.5], [1.0, 0.0]], device=DEV)
    coef = torch.tensor([[0.5, 0.25], [0.9, -0.3], [1.0, -0.7], [1.1, 0.2]], device=DEV)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    npred = (torch.randn(2 * S, HW, 4, generator=g)).to(torch.bfloat16).to(DEV)
    for row in (2, 1, 3):
        ctx.ew(L.EW_STEP_SET, step, i=(row, 1, 0, 0, 0, 0))
        y = lat.clone()
        if with_step:
            ctx.ew(L.EW_CFG_STEP, y, a=npred, tab=coef, step=step, i=(S, HW, 0, 1, Mb, 0), f=(0.0, 0.0, 5.0, 0.0),
                   x2=z, noise=n, mask=mask, blend_tab=tab)
            p = npred.float().view(2, S, HW, 4).permute(0, 1, 3, 2).reshape(2, S, 4, H, W)
            upd = coef[row, 0] * lat + coef[row, 1] * (p[0] + 5.0 * (p[1] - p[0]))
        else:
            ctx.ew(L.EW_CFG_STEP, y, step=step, i=(S, HW, 0, 0, Mb, 0), x2=z, noise=n, mask=mask, blend_tab=tab)
            upd = lat
        m = mask.repeat(S // Mb, 1, 1, 1)
        ref = (1 - m) * (tab[row, 0] * z + tab[row, 1] * n) + m * upd
        err = (y - ref).abs().max().item()
        print(f"blend S={S} Mb={Mb} with_step={with_step} row {row}: max abs {err:.2e}")
        assert err < 1e-5, (row, err)
        if row == 3:                                          # (1, 0): the image latents, exactly, outside the mask
            assert torch.equal(torch.where(m.expand_as(y) == 0, y, z), z)
    # a blend without its operands is a status code
    with pytest.raises(L.ImhError, match=r"status -1\)"):
        ctx.ew(L.EW_CFG_STEP, lat.clone(), a=npred, tab=coef, step=step, i=(S, HW, 0, 1, Mb, 0), f=(0.0, 0.0, 5.0, 0.0), mask=mask)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("C0", [64, 320])
def test_conv_in_nine_channels_matches_conv2d(dtype, C0):
    """channels 0-3: the latents times the step's input scale; 4-8: the second buffer, unscaled; both rounded to the compute dtype;
    S = 2 with CFG duplication (b % S), non-square, the scale from a table row picked by the device step counter"""
    from imagharmony_amd import lib as L
    from imagharmony_amd.ctx import Ctx
    ctx = Ctx(DEV, dtype)
    g = torch.Generator().manual_seed(C0)
    S, H, W = 2, 24, 40
    lat = torch.randn(S, 4, H, W, generator=g).to(DEV) * 3
    extra = torch.randn(S, 5, H, W, generator=g).to(DEV)
    extra[:, 0] = (extra[:, 0] > 0).float()                                   # the mask channel
    w = (torch.randn(C0, 9, 3, 3, generator=g) / 9).to(dtype).to(DEV)
    bias = torch.randn(C0, generator=g).to(dtype).to(DEV)
    tab = torch.tensor([1.0, 0.068, 0.37], device=DEV)
    step = torch.full((1,), 2, dtype=torch.int32, device=DEV)
    out = ctx.new(2 * S, H, W, C0)
    ctx.ew(L.EW_CONV_IN, out, a=lat, w=w, bias=bias, tab=tab, step=step, i=(S, H, W, C0, 2 * S, 9), f=(1.0, 0, 0, 0), x2=extra)
    torch.cuda.synchronize()
    xin = torch.cat([(lat * tab[2]).to(dtype).float(), extra.to(dtype).float()], 1)
    ref = F.conv2d(torch.cat([xin, xin]), w.float(), bias.float(), padding=1).permute(0, 2, 3, 1)
    assert_close(out, ref, dtype, f"conv_in 9ch C0={C0} {dtype}")
    # ... and the 4-channel launch next to it, immediate scale (the existing check's form at this shape)
    w4 = w[:, :4].contiguous()
    out4 = ctx.new(2 * S, H, W, C0)
    ctx.ew(L.EW_CONV_IN, out4, a=lat, w=w4, bias=bias, i=(S, H, W, C0, 2 * S, 0), f=(0.5, 0, 0, 0))
    x4 = (lat * 0.5).to(dtype).float()
    assert_close(out4, F.conv2d(torch.cat([x4, x4]), w4.float(), bias.float(), padding=1).permute(0, 2, 3, 1), dtype, f"conv_in 4ch C0={C0}")
    with pytest.raises(L.ImhError, match=r"status -1\)"):                     # nine channels without the second source
        ctx.ew(L.EW_CONV_IN, out, a=lat, w=w, bias=bias, i=(S, H, W, C0, 2 * S, 9), f=(1.0, 0, 0, 0))


# ------------------------------------------------------------------------------------ model pairs
_PAIRS = {}


def build_pair(dtype, in_channels=4, num_tokens=4, scale=0.8):
    """smoke_impl.build_pair's construction over dataclasses.replace(tiny_config(), in_channels=...)"""
    from imagharmony_amd.attention_processor import AttnProcessor2_0, IPAttnProcessor2_0
    from imagharmony_amd.unet import UNet2DConditionModel, UNetConfig
    key = (dtype, in_channels)
    if key in _PAIRS:
        return _PAIRS[key]
    ocfg = dataclasses.replace(tiny_config(), in_channels=in_channels)
    with torch.no_grad():
        ou = det_fill(OracleUNet(ocfg), 5).eval()
        procs = oracle_install(ou, num_tokens=num_tokens, scale=scale)
        for n, p in procs.items():
            if isinstance(p, om.IPAttnProcessor2_0):
                det_fill(p, 7, prefix=n)
    hu = UNet2DConditionModel(UNetConfig(**{k: getattr(ocfg, k) for k in UNetConfig.__dataclass_fields__}))
    hp = {}
    for name, p in procs.items():
        hp[name] = AttnProcessor2_0() if isinstance(p, om.AttnProcessor2_0) else \
            IPAttnProcessor2_0(p.hidden_size, p.cross_attention_dim, scale=p.scale, num_tokens=p.num_tokens, skip=p.skip)
    hu.set_attn_processor(hp)
    hu.load_state_dict(ou.state_dict(), strict=True)
    _PAIRS[key] = (ou, hu.to(DEV, dtype), ocfg)
    return _PAIRS[key]


def build_vae_pair(dtype=torch.float32):
    from imagharmony_amd.vae import AutoencoderKL, VAEConfig
    if "vae" not in _PAIRS:
        ocfg = tiny_vae_config()
        ov = det_fill(OracleVAE(ocfg), 3).eval()
        hv = AutoencoderKL(VAEConfig(**{k: getattr(ocfg, k) for k in VAEConfig.__dataclass_fields__}), with_encoder=True)
        hv.load_state_dict(ov.state_dict(), strict=True)
        _PAIRS["vae"] = (ov, hv.to(DEV, dtype))
    return _PAIRS["vae"]


def embeds(ocfg, S):
    cd = ocfg.cross_attention_dim
    return dict(prompt_embeds=det_randn((S, 81, cd), 4), negative_prompt_embeds=det_randn((S, 81, cd), 5),
                pooled_prompt_embeds=det_randn((S, ocfg.pooled_dim), 6), negative_pooled_prompt_embeds=det_randn((S, ocfg.pooled_dim), 7))


def centred_mask(H, W):
    """a centred rectangle of half the height and half the width: a quarter of the area, so both regions are exercised"""
    m = torch.zeros(1, 1, H, W)
    m[..., H // 4:H // 4 + H // 2, W // 4:W // 4 + W // 2] = 1.0
    return m


def _draw(shape, gens):
    if isinstance(gens, (list, tuple)):
        return torch.cat([torch.randn((1,) + tuple(shape[1:]), generator=g) for g in gens], 0)
    return torch.randn(tuple(shape), generator=gens)


@torch.no_grad()
def _oracle_inpaint(ou, ov, sched, img, mask, strength, steps, S, gens, emb, guidance=5.0, cg_start=0.0, cg_end=1.0):
    """diffusers 0.30 StableDiffusionXLInpaintPipeline.__call__ over the oracle modules, fp32: get_timesteps, prepare_latents
    (posterior sample x scaling factor, add_noise or the is_strength_max start), prepare_mask_latents, then the loop with the blend
    (num_channels_unet == 4) or the 9-channel model input.  img [1, 3, H, W] in [-1, 1], mask [1, 1, H, W] binary."""
    nine = ou.config.in_channels == 9
    per_sample = isinstance(gens, (list, tuple))
    osch = OracleDDIM() if sched == "ddim" else OracleEuler()
    osch.set_timesteps(steps)
    init = min(int(steps * strength), steps)
    t_start = max(steps - init, 0)
    ts = osch.timesteps[t_start:]

    def pair(row):                                             # scheduler.add_noise(x, noise, timesteps[row]) = a x + b noise
        if sched == "ddim":
            ac = osch.alphas_cumprod[int(osch.timesteps[row])]
            return float(ac ** 0.5), float((1 - ac) ** 0.5)
        return 1.0, float(osch.sigmas[row])                    # begin index / step index row
    h, w = img.shape[2] // 8, img.shape[3] // 8
    sf = ov.config.scaling_factor

    def posterior(x, noise):
        mean, logvar = ov.quant_conv(ov.encoder(x)).chunk(2, 1)
        return (mean.repeat(noise.shape[0], 1, 1, 1) + torch.exp(0.5 * logvar.clamp(-30, 20)).repeat(noise.shape[0], 1, 1, 1) * noise) * sf
    n1 = _draw((S if per_sample else 1, 4, h, w), gens)
    z = posterior(img, n1).repeat(S // n1.shape[0], 1, 1, 1)
    n2 = _draw((S, 4, h, w), gens)
    if strength == 1.0:
        x = n2 * osch.init_noise_sigma
    else:
        a, b = pair(t_start)
        x = a * z + b * n2
    m = F.interpolate(mask, size=(h, w)).repeat(S, 1, 1, 1)
    if nine:
        n3 = _draw((S if per_sample else 1, 4, h, w), gens)
        mz = posterior(img * (mask < 0.5), n3).repeat(S // n3.shape[0], 1, 1, 1)
    if hasattr(osch, "_i"):
        osch._i = t_start
    pe, ne, po, no = (emb[k] for k in ("prompt_embeds", "negative_prompt_embeds", "pooled_prompt_embeds", "negative_pooled_prompt_embeds"))
    H, W = img.shape[2], img.shape[3]
    ids = torch.tensor([[H, W, 0, 0, H, W]], dtype=pe.dtype).repeat(2 * S, 1)
    ehs, text = torch.cat([ne, pe], 0), torch.cat([no, po], 0)
    cond_scale = next(p.scale for p in ou.attn_processors.values() if isinstance(p, om.IPAttnProcessor2_0))
    for i, t in enumerate(ts):
        gated = (i / len(ts) < cg_start) or ((i + 1) / len(ts) > cg_end)
        oracle_set_scale(ou, 0.0 if gated else cond_scale)
        xin = osch.scale_model_input(torch.cat([x] * 2), t)
        if nine:
            xin = torch.cat([xin, torch.cat([m] * 2), torch.cat([mz] * 2)], 1)
        eps = ou(xin, t, encoder_hidden_states=ehs, added_cond_kwargs={"text_embeds": text, "time_ids": ids})[0]
        u, c = eps.chunk(2)
        x = osch.step(u + guidance * (c - u), t, x)[0]
        if not nine:
            p = z
            if i < len(ts) - 1:
                a, b = pair(t_start + i + 1)
                p = a * z + b * n2
            x = (1 - m) * p + m * x
    oracle_set_scale(ou, cond_scale)
    return x, z, m


def _gens(seed, S, as_list):
    return [torch.Generator().manual_seed(seed + s) for s in range(S)] if as_list else torch.Generator().manual_seed(seed)


def _pipe(hu, hv, sched, dtype):
    from imagharmony_amd import schedulers as hs
    from imagharmony_amd.pipeline import StableDiffusionXLInpaintCustomPipeline
    return StableDiffusionXLInpaintCustomPipeline(hu, scheduler=hs.DDIMScheduler() if sched == "ddim" else hs.EulerDiscreteScheduler(),
                                                  device=DEV, dtype=dtype, vae=hv)


IMG = lambda hw=32: torch.rand(1, 3, hw * 8, hw * 8, generator=torch.Generator().manual_seed(3)) * 2 - 1


# (dtype, in_channels, scheduler, strength, steps, S, generator list, cg_start, cg_end, bound): the bounds of test_img2img_trajectory_matches_oracle
# on the same tiny pair, rel-RMS 1e-2 in fp16 and 4e-2 in bf16.  strength 0.9999 x 4 steps runs steps 1..3; 0.5 x 6 runs steps 3..5
TRAJ = [
    (torch.float16, 4, "ddim", 1.0, 3, 1, False, 0.0, 1.0, 1e-2),
    (torch.float16, 4, "euler", 1.0, 3, 1, False, 0.0, 1.0, 1e-2),
    (torch.float16, 4, "ddim", 0.9999, 4, 1, False, 0.0, 1.0, 1e-2),
    (torch.float16, 4, "euler", 0.5, 6, 1, False, 0.0, 0.6, 1e-2),
    (torch.float16, 4, "ddim", 0.5, 6, 2, True, 0.3, 1.0, 1e-2),
    (torch.bfloat16, 4, "euler", 0.9999, 4, 1, False, 0.0, 1.0, 4e-2),
    (torch.float16, 9, "ddim", 1.0, 3, 1, False, 0.0, 1.0, 1e-2),
    (torch.float16, 9, "euler", 0.9999, 4, 1, False, 0.0, 1.0, 1e-2),
    (torch.float16, 9, "euler", 0.5, 6, 2, True, 0.0, 0.6, 1e-2),
    (torch.float16, 9, "ddim", 0.5, 6, 1, False, 0.3, 1.0, 1e-2),
    (torch.bfloat16, 9, "ddim", 0.9999, 4, 1, False, 0.0, 1.0, 4e-2),
]


@pytest.mark.parametrize("dtype,cin,sched,strength,steps,S,glist,cg_start,cg_end,tol", TRAJ)
def test_inpaint_trajectory_matches_oracle(dtype, cin, sched, strength, steps, S, glist, cg_start, cg_end, tol):
    ou, hu, ocfg = build_pair(dtype, cin)
    ov, hv = build_vae_pair()
    img, mask = IMG(), centred_mask(256, 256)
    emb = embeds(ocfg, S)
    pipe = _pipe(hu, hv, sched, dtype)
    out = pipe(image=img, mask_image=mask, strength=strength, num_inference_steps=steps, guidance_scale=5.0,
               control_guidance_start=cg_start, control_guidance_end=cg_end, generator=_gens(11, S, glist), output_type="latent",
               **emb).images.float().cpu()
    ref, z, m = _oracle_inpaint(ou, ov, sched, img, mask, strength, steps, S, _gens(11, S, glist), emb, cg_start=cg_start, cg_end=cg_end)
    assert 0.2 < m.mean().item() < 0.3                                    # about a quarter of the latent is repainted
    r = rel_rms(out, ref)
    name = f"inpaint.{'blend' if cin == 4 else 'concat9'}.{str(dtype).split('.')[-1]}.{sched}.s{strength}.n{steps}.S{S}.cg{cg_start}-{cg_end}"
    print(f"{name}: rel-rms {r:.3e} (bound {tol:g})")
    record_parity(name, r, tol)
    assert out.shape == ref.shape == (S, 4, 32, 32) and torch.isfinite(out).all()
    assert r < tol, (name, r)
    if cin == 4:
        # outside the mask the result is the image latents: the engine's to the bit, the oracle encoder's to the fp32 VAE's error
        keep = (m == 0).expand_as(out)
        assert torch.equal(out[keep], pipe.engine.st.inp_z.cpu()[keep])
        assert rel_rms(out[keep], z[keep]) < 1e-3
    if S == 2:
        assert not torch.equal(out[0], out[1])                            # a generator list: its own draws per sample


# ------------------------------------------------------------------------------------ exact invariants, mode A
@pytest.mark.parametrize("sched", ["ddim", "euler"])
def test_blend_invariants_are_exact(sched):
    from imagharmony_amd.pipeline import StableDiffusionXLImg2ImgCustomPipeline
    dtype = torch.bfloat16
    ou, hu, ocfg = build_pair(dtype, 4)
    _, hv = build_vae_pair()
    img = IMG()
    emb = dict(embeds(ocfg, 2), guidance_scale=5.0, output_type="latent", num_inference_steps=6)
    gen = lambda: torch.Generator().manual_seed(5)
    pipe = _pipe(hu, hv, sched, dtype)
    # any binary mask (a batch of two, one per sample): outside it the final latents are the image latents, to the bit
    mask = (torch.rand(2, 1, 256, 256, generator=torch.Generator().manual_seed(9)) < 0.5).float()
    for strength, de in ((1.0, None), (0.5, None), (1.0, 0.8)):
        out = pipe(image=img, mask_image=mask, strength=strength, denoising_end=de, generator=gen(), **emb).images.cpu()
        z = pipe.engine.st.inp_z.cpu()
        lm = mask[..., ::8, ::8].expand(2, 4, 32, 32)
        assert torch.isfinite(out).all() and 0.3 < lm.mean() < 0.7
        assert torch.equal(out[lm == 0], z[lm == 0]), (strength, de)
        assert not torch.equal(out[lm == 1], z[lm == 1])
    # all-zeros mask: the image latents everywhere
    out = pipe(image=img, mask_image=torch.zeros(1, 1, 256, 256), strength=0.5, generator=gen(), **emb).images.cpu()
    assert torch.equal(out, pipe.engine.st.inp_z.cpu())
    # all-ones mask, strength 0.5: the blend is the identity and the draw order is img2img's -> the img2img pipeline's output, to the bit
    out = pipe(image=img, mask_image=torch.ones(1, 1, 256, 256), strength=0.5, generator=gen(), **emb).images.cpu()
    i2i = StableDiffusionXLImg2ImgCustomPipeline(hu, scheduler=type(pipe.scheduler)(), device=DEV, dtype=dtype, vae=hv)
    ref = i2i(image=img, strength=0.5, generator=gen(), **emb).images.cpu()
    assert torch.equal(out, ref)


# ------------------------------------------------------------------------------------ plans
def _plan_size(eng):
    return eng.plan.lib.imh_plan_size(eng.plan.plan)


def test_inpaint_step_plans_add_no_launch():
    """mode A fuses the blend into the CFG + scheduler launch (at most one launch more than text-to-image is allowed: it is none),
    mode B differs from text-to-image in conv_in's arguments alone; a 9-channel UNet refuses a schedule that is not inpainting"""
    from imagharmony_amd import lib as L
    from imagharmony_amd import schedulers as hs
    from imagharmony_amd.denoise import DenoiseEngine
    dtype = torch.bfloat16
    sizes = {}
    for cin in (4, 9):
        ou, hu, ocfg = build_pair(dtype, cin)
        e = embeds(ocfg, 1)
        eng = DenoiseEngine(hu, DEV, dtype)
        eng.set_conditioning(e["prompt_embeds"], e["negative_prompt_embeds"], e["pooled_prompt_embeds"], e["negative_pooled_prompt_embeds"],
                             256, 256, guidance_scale=5.0)
        for inpaint in (False, True):
            eng.set_schedule(hs.DDIMScheduler(), 4, inpaint=inpaint)
            if cin == 9 and not inpaint:
                with pytest.raises(L.ImhError, match="inpainting"):
                    eng._record()
                continue
            eng._record()
            sizes[(cin, inpaint)] = _plan_size(eng)
            descr = [t[2] for t in eng.plan.tags]
            assert descr[-1] == "step++" and descr[-2] == ("cfg+step+blend" if (cin == 4 and inpaint) else "cfg+step")
    print("step plan sizes", sizes)
    assert sizes[(4, False)] <= sizes[(4, True)] <= sizes[(4, False)] + 1
    assert sizes[(4, True)] == sizes[(4, False)]
    assert sizes[(9, True)] == sizes[(4, False)]


@pytest.mark.parametrize("cin", [4, 9])
def test_alternation_with_text2img_and_img2img_equals_fresh_pipelines(cin):
    """text-to-image -> inpaint -> img2img -> inpaint (another mask, same size) -> text-to-image on ONE pipeline equals fresh
    pipelines, for both schedulers (a 9-channel UNet runs inpainting only: inpaint -> inpaint (another mask) there).  Every pipeline
    call sets the conditioning anew, which drops the recorded plans of the previous one (as for every pipeline here), so "a new
    call copies into the engine's buffers and re-records nothing" is asserted where plans are reused: on the engine, under one
    conditioning -- another mask through prepare_inpaint leaves the plan object in place, and alternating with the text-to-image
    schedule brings the same two plan objects back."""
    from imagharmony_amd import schedulers as hs
    from imagharmony_amd.pipeline import StableDiffusionXLCustomPipeline, StableDiffusionXLImg2ImgCustomPipeline
    from imagharmony_amd.vae import latent_mask
    dtype = torch.bfloat16
    ou, hu, ocfg = build_pair(dtype, cin)
    _, hv = build_vae_pair()
    emb = dict(embeds(ocfg, 2), guidance_scale=5.0, output_type="latent")
    img = IMG()
    mask_a, mask_b = centred_mask(256, 256), 1.0 - centred_mask(256, 256)
    gl = lambda: [torch.Generator().manual_seed(s) for s in (1, 2)]
    t2i = lambda p: StableDiffusionXLCustomPipeline.__call__(p, height=256, width=256, num_inference_steps=4,
                                                             generator=torch.Generator().manual_seed(1), **emb).images.clone()
    i2i = lambda p: StableDiffusionXLImg2ImgCustomPipeline.__call__(p, image=img, strength=0.5, num_inference_steps=4, generator=gl(),
                                                                    **emb).images.clone()
    inp = lambda p, m: p(image=img, mask_image=m, strength=0.75, num_inference_steps=4, generator=gl(), **emb).images.clone()
    for sched in ("ddim", "euler"):
        new = lambda: _pipe(hu, hv, sched, dtype)
        one = new()
        if cin == 4:
            seq = [t2i(one), inp(one, mask_a), i2i(one), inp(one, mask_b), t2i(one)]
            fresh = [t2i(new()), inp(new(), mask_a), i2i(new()), inp(new(), mask_b), t2i(new())]
            assert torch.equal(seq[0], seq[4])                            # text-to-image before and after the inpaint calls
            assert not torch.equal(seq[1], seq[3]) and not torch.equal(seq[0], seq[1]) and not torch.equal(seq[2], seq[1])
        else:
            seq = [inp(one, mask_a), inp(one, mask_b), inp(one, mask_a)]
            fresh = [inp(new(), mask_a), inp(new(), mask_b), inp(new(), mask_a)]
            assert torch.equal(seq[0], seq[2]) and not torch.equal(seq[0], seq[1])
        for k, (a, b) in enumerate(zip(seq, fresh)):
            assert torch.equal(a, b), (sched, k)
        # the engine under the last call's conditioning (that of an inpaint or a text-to-image call: the same embeddings)
        eng, sch = one.engine, one.scheduler
        h = w = 32
        g = torch.Generator().manual_seed(7)
        mom = torch.randn(1, h, w, 8, generator=g)
        n1, n2, n3 = (torch.randn(2, 4, h, w, generator=g) for _ in range(3))
        sch.set_timesteps(4)
        ab = sch.add_noise_coefficients(1)

        def run_inpaint(m):
            eng.set_schedule(sch, 4, t_start=1, inpaint=True)
            eng.prepare_inpaint(mom, n1, n2, 0.13025, ab[0], ab[1], latent_mask(m, h, w), masked_moments=mom, n3=n3)
            return eng.denoise(None).clone(), eng.plan
        o1, p1 = run_inpaint(mask_a)
        o2, p2 = run_inpaint(mask_b)
        assert p2 is p1 and not torch.equal(o1, o2)                       # another mask: copied in, nothing recorded
        if cin == 4:
            eng.set_schedule(sch, 4)
            t1 = eng.denoise(n2).clone()
            pt = eng.plan
            assert pt is not p1                                           # same schedule, different plan: "inpaint" is part of the key
            o3, p3 = run_inpaint(mask_a)
            assert p3 is p1 and torch.equal(o3, o1)
            eng.set_schedule(sch, 4)
            assert eng.plan is pt and torch.equal(eng.denoise(n2), t1)
            f = eng.fork()                                                # a fork carries the mode and the blend table, with buffers of its own
            assert f.inpaint is None and f.st.blend_tab is None
            eng.set_schedule(sch, 4, t_start=1, inpaint=True)
            f = eng.fork()
            assert f.inpaint == "blend" and f.st.blend_tab is eng.st.blend_tab and f.t_start == 1
            f.prepare_inpaint(mom, n1, n2, 0.13025, ab[0], ab[1], latent_mask(mask_a, h, w))
            assert f.st.inp_mask is not eng.st.inp_mask and torch.equal(f.denoise(None), o1)


# ------------------------------------------------------------------------------------ IPAdapterXL
def test_ipadapterxl_generate_reaches_the_inpaint_pipeline():
    from PIL import Image
    import numpy as np
    from imagharmony_amd.ip_adapter import IPAdapterXL
    from imagharmony_amd.modules import HarmonyAttention
    from imagharmony_amd.utils import get_generator
    dtype = torch.bfloat16
    ou, hu, ocfg = build_pair(dtype, 4)
    _, hv = build_vae_pair()
    pipe = _pipe(hu, hv, "ddim", dtype)
    cd = ocfg.cross_attention_dim
    ha = det_fill(HarmonyAttention(image_hidden_size=128, text_context_dim=cd, inter_dim=512, cross_heads=8,
                                   reshape_blocks=8, cross_value_dim=64), 3)
    ip = IPAdapterXL(pipe, None, None, DEV, num_tokens=4, inference=True, number_class_crossattention=ha, dtype=dtype,
                     clip_embeddings_dim=128)
    det_fill(ip.image_proj_model, 5)
    rs = np.random.RandomState(0)
    init = Image.fromarray((rs.rand(258, 290, 3) * 255).astype("uint8"))           # 290 x 258 -> 288 x 256 (multiples of 8)
    marr = np.zeros((258, 290), "uint8")
    marr[60:200, 80:220] = 255
    mask = Image.fromarray(marr, mode="L")                                          # resized with the image to 288 x 256
    embeds4 = (det_randn((1, 77, cd), 1), det_randn((1, 77, cd), 2), det_randn((1, ocfg.pooled_dim), 3),
               det_randn((1, ocfg.pooled_dim), 4))
    kw = dict(clip_image_embeds=det_randn((1, 128), 5), prompt_embeds=embeds4, extra_prompt_embeds=det_randn((1, 77, cd), 6),
              num_samples=1, seed=42, num_inference_steps=4, guidance_scale=5.0, image=init, mask_image=mask, strength=0.75)
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
    assert seen["strength"] == 0.75 and seen["image"] is init and seen["mask_image"] is mask and lat.shape == (1, 4, 32, 36)
    direct = pipe(**{**seen, "generator": get_generator(42, "cpu")}).images
    assert torch.equal(lat, direct)
    with pytest.raises(NotImplementedError):
        ip.generate_pns([1, 2], clip_image_embeds=det_randn((1, 128), 5), prompt_embeds=embeds4, output_type="latent")


# ------------------------------------------------------------------------------------ full width
def test_fullsize_inpaint_smoke_both_modes():
    """the full-width UNet at 1024^2 (C0 = 320, 128 x 128 latents: the launch geometry the tiny pair does not reach -- the 9-channel
    conv_in with its 105 KB weight tile), deterministic weights, 3 steps, bf16, a half-image mask; no oracle: finite outputs, and in
    mode A the exact invariant outside the mask"""
    import bench
    from imagharmony_amd.ip_adapter import install_ip_processors
    from imagharmony_amd.unet import UNet2DConditionModel, UNetConfig
    dtype = torch.bfloat16
    _, hv = build_vae_pair()
    pe, ne, po, no = [t.to(DEV) for t in bench.synthetic_conditioning(4)]
    img = torch.rand(1, 3, 1024, 1024, generator=torch.Generator().manual_seed(3)) * 2 - 1
    mask = torch.zeros(1, 1, 1024, 1024)
    mask[..., :, 512:] = 1.0

    def unet9():                                              # bench.build_unet over UNetConfig(in_channels=9)
        with torch.device(DEV):
            u = UNet2DConditionModel(UNetConfig(in_channels=9))
        u.init_random_(1234)
        u = u.to(dtype)
        procs = install_ip_processors(u, num_tokens=4, scale=1.0, device=DEV, dtype=dtype, init="empty")
        g = torch.Generator(device=DEV).manual_seed(4321)
        for p in procs.values():
            for q in p.parameters():
                q.data.copy_(torch.randn(q.shape, generator=g, device=DEV) * (q.shape[1] ** -0.5))
        return u
    for cin in (4, 9):
        unet = bench.build_unet(DEV, dtype, 4) if cin == 4 else unet9()
        assert tuple(unet.conv_in.weight.shape) == (320, cin, 3, 3)
        pipe = _pipe(unet, hv, "ddim", dtype)
        out = pipe(image=img, mask_image=mask, strength=1.0, num_inference_steps=3, guidance_scale=5.0, prompt_embeds=pe,
                   negative_prompt_embeds=ne, pooled_prompt_embeds=po, negative_pooled_prompt_embeds=no,
                   generator=torch.Generator().manual_seed(3), output_type="latent").images.cpu()
        assert out.shape == (1, 4, 128, 128) and torch.isfinite(out).all()
        assert pipe.engine.steps == 3 and pipe.engine.t_start == 0
        if cin == 4:
            z = pipe.engine.st.inp_z.cpu()
            assert torch.equal(out[..., :64], z[..., :64]) and not torch.equal(out[..., 64:], z[..., 64:])
        else:
            ex = pipe.engine.st.conv_in_extra.cpu()
            assert torch.equal(ex[:, 0, :, :64], torch.zeros(1, 128, 64)) and torch.equal(ex[:, 0, :, 64:], torch.ones(1, 128, 64))
        print(f"full-size inpaint in_channels={cin}: |out| max {out.abs().max().item():.3f}")
        del pipe, unet
        torch.cuda.empty_cache()
