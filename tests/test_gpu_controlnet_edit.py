"""GPU: one ControlNet next to the edits -- image-to-image, both inpainting modes (4-channel UNet: blend in the step; 9-channel UNet:
conv_in over [latents | mask | masked-image latents], the ControlNet on the 4-channel latents alone) -- and PNS over all of them.

Trajectories against the CPU fp32 restatement of diffusers' ControlNet img2img / inpainting loops (tests/controlnet_edit_reference.py;
cases and cached references: tests/controlnet_edit_cases.py) below LOOP_TOL, the bound the project's tiny trajectories are held to
(tests/test_gpu_controlnet.py, from tests/test_gpu_pipeline.py); everything else is exact: plan shapes and launch counts, plan
alternation on one engine, the public classes against the hand-driven engine sequence, PNS winners against the pipe's own call.

Measured rel-RMS of every trajectory case goes to controlnet_edit_parity.json beside the suite's parity record; the committed copy is
profiles/controlnet_edit_parity.json."""
import json
import os

import pytest
import torch

import controlnet_edit_cases as cc
import controlnet_reference as cr
from conftest import PARITY_JSON, rel_rms
from oracle.detfill import det_fill, det_randn
from test_gpu_controlnet import LOOP_TOL, _product_cfg
from test_gpu_inpaint import build_pair, build_vae_pair

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float16, torch.bfloat16]
T_TOKENS = cc.T_TOKENS
PARITY = {}
_CN = {}


def _name(dtype):
    return str(dtype).replace("torch.", "")


def _private_unet(dtype, cin):
    """build_pair's product UNet, built anew: IPAdapterXL(pipe, ...) installs fresh IP processors on pipe.unet, which must not happen to
    the pair tests/test_gpu_inpaint.py caches for the trajectory tests of several modules"""
    from imagharmony_amd.attention_processor import AttnProcessor2_0, IPAttnProcessor2_0
    from imagharmony_amd.unet import UNet2DConditionModel
    from oracle import modules as om
    ou = cc.oracle_unet(cin)
    hu = UNet2DConditionModel(_product_cfg(ou.config))
    hu.set_attn_processor({n: AttnProcessor2_0() if isinstance(p, om.AttnProcessor2_0) else
                           IPAttnProcessor2_0(p.hidden_size, p.cross_attention_dim, scale=p.scale, num_tokens=p.num_tokens, skip=p.skip)
                           for n, p in ou.attn_processors.items()})
    hu.load_state_dict(ou.state_dict(), strict=True)
    return hu.to(DEV, dtype)


def _stack(dtype, cin, private=False):
    """(product UNet with ``cin`` input channels, product ControlNet -- always the 4-channel model --, product VAE, oracle config): the
    weights of the oracle models controlnet_edit_cases fills.  private: a UNet of the test's own, for tests that put an adapter on it"""
    from imagharmony_amd.attention_processor import CNAttnProcessor2_0
    from imagharmony_amd.controlnet import ControlNetModel
    _, hu, ocfg = build_pair(dtype, cin, num_tokens=T_TOKENS)
    if private:
        hu = _private_unet(dtype, cin)
    _, hv = build_vae_pair()
    if dtype not in _CN:
        from oracle.sdxl_unet import tiny_config
        cn = ControlNetModel(_product_cfg(tiny_config()))
        cn.load_state_dict(cc.ref_controlnet().state_dict(), strict=True)
        _CN[dtype] = cn.to(DEV, dtype)
    cn = _CN[dtype]
    cn.set_attn_processor(CNAttnProcessor2_0(num_tokens=T_TOKENS))       # (an IPAdapterXL in another test may have installed its own)
    assert cn.config.in_channels == 4
    return hu, cn, hv, ocfg


def _scheduler(kind):
    from imagharmony_amd import schedulers as hs
    return {"ddim": hs.DDIMScheduler, "euler": hs.EulerDiscreteScheduler, "dpmpp2m": hs.DPMSolverMultistepScheduler,
            "euler-a": hs.EulerAncestralDiscreteScheduler}[kind]()


def _pipe(mode, hu, cn, hv, kind, dtype):
    """mode: 't2i' | 'i2i' | 'inp'; cn None: the plain class of that mode"""
    from imagharmony_amd import pipeline as P
    if cn is None:
        cls = {"t2i": P.StableDiffusionXLCustomPipeline, "i2i": P.StableDiffusionXLImg2ImgCustomPipeline, "inp": P.StableDiffusionXLInpaintCustomPipeline}[mode]
        return cls(hu, scheduler=_scheduler(kind), device=DEV, dtype=dtype, vae=hv)
    cls = {"t2i": P.StableDiffusionXLControlNetCustomPipeline, "i2i": P.StableDiffusionXLControlNetImg2ImgCustomPipeline,
           "inp": P.StableDiffusionXLControlNetInpaintCustomPipeline}[mode]
    return cls(hu, cn, scheduler=_scheduler(kind), device=DEV, dtype=dtype, vae=hv)


def _run_case(name, dtype):
    """the case through the public pipeline class -> (latents on the CPU, the pipe)"""
    c = cc.CASES[name]
    hu, cn, hv, ocfg = _stack(dtype, c["cin"])
    pipe = _pipe(c["mode"], hu, cn, hv, c["kind"], dtype)
    kw = dict(image=cc.image(c["H"], c["W"]), control_image=cc.control_image(c["H"], c["W"]), strength=c["strength"],
              num_inference_steps=c["steps"], guidance_scale=cc.GUIDANCE, generator=cc.gens(c["S"], c["glist"]), output_type="latent",
              controlnet_conditioning_scale=c["scale"], controlnet_guidance_start=c["window"][0], controlnet_guidance_end=c["window"][1],
              **cc.embeds(c["S"]))
    if c["mode"] == "inp":
        kw["mask_image"] = cc.half_mask(c["H"], c["W"])
    return pipe(**kw).images.float().cpu(), pipe


def _check_against_reference(name, dtype, out):
    c = cc.CASES[name]
    ref, ref_plain, m, t_start = cc.reference(name)
    bound = LOOP_TOL[dtype]
    vis = rel_rms(ref, ref_plain)
    # a dead branch cannot pass: on the CPU reference the ControlNet moves the result by more than three times the bound
    assert vis > 3 * bound, f"{name}: the ControlNet moves the reference's latents by {vis:.3e} only"
    r = rel_rms(out, ref)
    print(f"{name} {_name(dtype)}: rel-rms {r:.3e} (bound {bound:.0e}); the control moves the reference by {vis:.3e}")
    PARITY[f"{name}.{_name(dtype)}"] = dict(case=name, dtype=_name(dtype), rel_rms=r, bound=bound, control_visibility=vis)
    try:
        out_dir = os.path.dirname(PARITY_JSON)
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "controlnet_edit_parity.json"), "w") as f:
            json.dump(PARITY, f, indent=1, sort_keys=True)
    except OSError:
        pass
    assert out.shape == ref.shape == (c["S"], 4, c["H"] // 8, c["W"] // 8) and torch.isfinite(out).all()
    assert r < bound, (name, r)
    return m, t_start


# ---------------------------------------------------------------------------------------------------- 1. image-to-image trajectory
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("kind", ["ddim", "dpmpp2m"])
def test_img2img_trajectory_with_controlnet_matches_reference(kind, dtype):
    name = f"i2i.{kind}"
    c = cc.CASES[name]
    out, pipe = _run_case(name, dtype)
    eng = pipe.engine
    t_start = cc.reference(name)[3]
    m = c["steps"] - t_start
    keeps = [cr.keep(i, m, *c["window"]) for i in range(m)]
    assert t_start >= 1 and eng.t_start == t_start and 0.0 in keeps and 1.0 in keeps
    want = [c["scale"]] * t_start + [c["scale"] * k for k in keeps]       # the window counts the steps that run; rows before t_start: the scale
    assert eng.cn_scale_tab.cpu().tolist() == torch.tensor(want, dtype=torch.float32).tolist()
    _check_against_reference(name, dtype, out)


# ---------------------------------------------------------------------------------------------------- 2. inpainting trajectory
INPAINT_CASES = ["inp4.S1", "inp4.S2", "inp4.full", "inp9.S1", "inp9.S2"]


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("name", INPAINT_CASES)
def test_inpaint_trajectory_with_controlnet_matches_reference(name, dtype):
    from imagharmony_amd import lib as L
    c = cc.CASES[name]
    out, pipe = _run_case(name, dtype)
    eng = pipe.engine
    assert eng.inpaint == ("blend" if c["cin"] == 4 else "concat") and eng.controlnet is pipe.controlnet
    kinds = [eng.plan.lib.imh_plan_get_kind(eng.plan.plan, i) for i in range(eng.plan.lib.imh_plan_size(eng.plan.plan))]
    assert kinds.count(L.OP_CONTROL_ADD) == 11 and eng.plan.captured
    m, t_start = _check_against_reference(name, dtype, out)
    assert eng.t_start == t_start and (t_start == 0) == (c["strength"] == 1.0)
    assert 0.45 < m.mean().item() < 0.55                                  # about half of the latent is repainted
    if c["cin"] == 4:
        # test_blend_invariants_are_exact's invariant under the branch: outside the mask the final latents are the image latents, to the bit
        z = eng.st.inp_z.cpu()
        keep = (m == 0).expand_as(out)
        assert torch.equal(out[keep], z[keep]) and not torch.equal(out[~keep], z[~keep])
    if c["S"] == 2:
        assert not torch.equal(out[0], out[1])                            # a generator list: its own draws per sample


# ---------------------------------------------------------------------------------------------------- hand-driven engines
def _conditioned_engine(hu, dtype, S, H, W):
    from imagharmony_amd.denoise import DenoiseEngine
    e = cc.embeds(S)
    eng = DenoiseEngine(hu, DEV, dtype)
    eng.set_conditioning(e["prompt_embeds"], e["negative_prompt_embeds"], e["pooled_prompt_embeds"], e["negative_pooled_prompt_embeds"],
                         H, W, guidance_scale=cc.GUIDANCE)
    return eng


def _edit_hand_over(eng, hv, sched, t_start, cin, img, mask, S, generator, strength):
    """what _EditCall.start does, by hand: the encoder moments, the draws in upstream's order, the fused hand-over"""
    from imagharmony_amd.pipeline import edit_draws, edit_moments, edit_prepare
    from imagharmony_amd.vae import latent_mask
    h, w = img.shape[2] // 8, img.shape[3] // 8
    inpaint = mask is not None
    cin = cin if inpaint else 4
    smax = inpaint and float(strength) == 1.0
    moments, masked = edit_moments(hv, img, isinstance(generator, (list, tuple)), cin, smax, mask)
    draws = edit_draws(generator, S, 1, h, w, Bm=1 if cin == 9 else None)
    edit_prepare(eng, sched, t_start, hv.config.scaling_factor, moments, draws, latent_mask(mask, h, w) if inpaint else None, smax, masked)


def _plan_size(eng):
    return eng.plan.lib.imh_plan_size(eng.plan.plan)


# ---------------------------------------------------------------------------------------------------- 3. plan shape
@pytest.mark.parametrize("S,H,W", [(1, 256, 256), (2, 256, 288)])
def test_inpaint_step_plan_with_the_branch_adds_no_launch(S, H, W):
    from imagharmony_amd import lib as L
    dtype = torch.bfloat16
    sizes = {}
    for cin in (4, 9):
        hu, cn, hv, ocfg = _stack(dtype, cin)
        eng = _conditioned_engine(hu, dtype, S, H, W)
        for with_cn in (False, True):
            eng.set_controlnet(cn if with_cn else None)
            if with_cn and eng.cn is None:
                eng.set_control_image(cc.control_image(H, W), conditioning_scale=0.8)
            for inpaint in ((False, True) if cin == 4 else (True,)):      # (a 9-channel UNet runs inpainting schedules only)
                eng.set_schedule(_scheduler("ddim"), 4, inpaint=inpaint, **(dict(controlnet_guidance_end=0.5) if with_cn else {}))
                eng._record()
                sizes[(cin, with_cn, inpaint)] = _plan_size(eng)
                kinds = [eng.plan.lib.imh_plan_get_kind(eng.plan.plan, i) for i in range(_plan_size(eng))]
                assert kinds.count(L.OP_CONTROL_ADD) == (11 if with_cn else 0) and eng.plan.captured
                descr = [t[2] for t in eng.plan.tags]
                assert descr[-1] == "step++" and descr[-2] == ("cfg+step+blend" if (cin == 4 and inpaint) else "cfg+step")
                conv_in = [t for t in eng.plan.tags if t[2] in ("conv_in", "cn.conv_in")]
                assert [t[2] for t in conv_in] == (["cn.conv_in", "conv_in"] if with_cn else ["conv_in"])
    print("step plan sizes", sizes)
    t2i_cn, t2i_plain = sizes[(4, True, False)], sizes[(4, False, False)]
    assert t2i_cn > t2i_plain
    for cin in (4, 9):
        assert sizes[(cin, True, True)] == t2i_cn
        assert sizes[(cin, True, True)] == sizes[(cin, False, True)] + (t2i_cn - t2i_plain)


# ---------------------------------------------------------------------------------------------------- 4. alternation on one engine
def test_plain_and_controlnet_plans_of_every_mode_alternate_without_rerecording():
    """plain inpainting <-> ControlNet inpainting <-> ControlNet text-to-image on ONE engine under one conditioning: each mode's plan is
    recorded once and comes back as the same object; the results are the first run's and a fresh pipeline's, to the bit.  The keys of
    {plain, ControlNet} x {text-to-image, t_start > 0, blend} coexist in the engine's plan cache (the 9-channel mode: the test below)."""
    from imagharmony_amd.pipeline import randn_latents
    dtype = torch.bfloat16
    hu, cn, hv, ocfg = _stack(dtype, 4)
    H = W = 256
    S, steps, strength, t_start = 2, 4, 0.75, 1
    img, mask, ctrl = cc.image(H, W), cc.half_mask(H, W), cc.control_image(H, W)
    window = dict(controlnet_guidance_start=0.0, controlnet_guidance_end=0.75)
    sched = _scheduler("ddim")
    eng = _conditioned_engine(hu, dtype, S, H, W)
    eng.max_cached_plans = 6
    eng.set_controlnet(cn)
    eng.set_control_image(ctrl, conditioning_scale=0.8)
    gl = lambda: [torch.Generator().manual_seed(s) for s in (1, 2)]

    def run(mode):
        eng.set_controlnet(None if mode.startswith("plain") else cn)
        kw = {} if mode.startswith("plain") else window
        if mode.endswith("t2i"):
            eng.set_schedule(sched, steps, **kw)
            return eng.denoise(randn_latents((S, 4, H // 8, W // 8), gl())).clone(), eng.plan
        inpaint = mode.endswith("inp")
        eng.set_schedule(sched, steps, t_start=t_start, inpaint=inpaint, **kw)
        _edit_hand_over(eng, hv, sched, t_start, 4, img, mask if inpaint else None, S, gl(), strength)
        return eng.denoise(None).clone(), eng.plan
    modes = ["plain.inp", "cn.inp", "cn.t2i"]
    first = {m: run(m) for m in modes}
    assert len({id(p) for _, p in first.values()}) == 3 and len(eng._plans) == 3
    assert not torch.equal(first["plain.inp"][0], first["cn.inp"][0])
    for _ in range(2):
        for m in modes:
            out, plan = run(m)
            assert plan is first[m][1], m
            assert torch.equal(out, first[m][0]), m
    # the remaining combinations record next to them and evict nothing (text-to-image and image-to-image share a plan where their
    # tables agree: t_start is the counter's start, not part of what is recorded)
    for m in ("plain.t2i", "plain.i2i", "cn.i2i"):
        first[m] = run(m)
    assert first["plain.i2i"][1] is first["plain.t2i"][1] and first["plain.t2i"][1] is not first["cn.t2i"][1]
    assert len(eng._plans) == len({id(p) for _, p in first.values()}) >= 4
    for m in modes:
        out, plan = run(m)
        assert plan is first[m][1] and torch.equal(out, first[m][0]), m
    # fresh pipelines, the same inputs through the public classes
    emb = dict(cc.embeds(S), guidance_scale=cc.GUIDANCE, output_type="latent", num_inference_steps=steps)
    cnkw = dict(controlnet_conditioning_scale=0.8, **window)
    fresh = {
        "plain.inp": _pipe("inp", hu, None, hv, "ddim", dtype)(image=img, mask_image=mask, strength=strength, generator=gl(), **emb).images,
        "cn.inp": _pipe("inp", hu, cn, hv, "ddim", dtype)(image=img, mask_image=mask, control_image=ctrl, strength=strength, generator=gl(),
                                                         **cnkw, **emb).images,
        "cn.t2i": _pipe("t2i", hu, cn, hv, "ddim", dtype)(image=ctrl, height=H, width=W, generator=gl(), **cnkw, **emb).images,
        "cn.i2i": _pipe("i2i", hu, cn, hv, "ddim", dtype)(image=img, control_image=ctrl, strength=strength, generator=gl(), **cnkw, **emb).images,
    }
    for m, out in fresh.items():
        assert torch.equal(out, first[m][0]), m
    # a fork under the ControlNet inpainting schedule shares the hint, the caches and the gate table; the blend state is its own
    run("cn.inp")
    fk = eng.fork()
    assert fk.cn is eng.cn and fk.cn_scale_tab is eng.cn_scale_tab and fk.controlnet is cn and fk.inpaint == "blend" and fk.t_start == t_start
    _edit_hand_over(fk, hv, sched, t_start, 4, img, mask, S, gl(), strength)
    assert fk.st.inp_mask is not eng.st.inp_mask and torch.equal(fk.denoise(None), first["cn.inp"][0])


def test_concat_plans_with_and_without_controlnet_alternate_without_rerecording():
    dtype = torch.bfloat16
    hu, cn, hv, ocfg = _stack(dtype, 9)
    H = W = 256
    S, steps, strength, t_start = 1, 4, 0.75, 1
    img, mask, ctrl = cc.image(H, W), cc.half_mask(H, W), cc.control_image(H, W)
    sched = _scheduler("euler")
    eng = _conditioned_engine(hu, dtype, S, H, W)
    eng.set_controlnet(cn)
    eng.set_control_image(ctrl, conditioning_scale=1.0)

    def run(with_cn):
        eng.set_controlnet(cn if with_cn else None)
        eng.set_schedule(sched, steps, t_start=t_start, inpaint=True)
        _edit_hand_over(eng, hv, sched, t_start, 9, img, mask, S, torch.Generator().manual_seed(4), strength)
        return eng.denoise(None).clone(), eng.plan
    a, pa = run(True)
    b, pb = run(False)
    assert pa is not pb and not torch.equal(a, b) and eng.inpaint == "concat"
    for _ in range(2):
        out, p = run(True)
        assert p is pa and torch.equal(out, a)
        out, p = run(False)
        assert p is pb and torch.equal(out, b)
    emb = dict(cc.embeds(S), guidance_scale=cc.GUIDANCE, output_type="latent", num_inference_steps=steps, image=img, mask_image=mask,
               strength=strength)
    assert torch.equal(_pipe("inp", hu, None, hv, "euler", dtype)(generator=torch.Generator().manual_seed(4), **emb).images, b)
    assert torch.equal(_pipe("inp", hu, cn, hv, "euler", dtype)(generator=torch.Generator().manual_seed(4), control_image=ctrl, **emb).images, a)


# ---------------------------------------------------------------------------------------------------- 5. the public surface
def _adapter(pipe, ocfg, dtype):
    from imagharmony_amd.ip_adapter import IPAdapterXL
    from imagharmony_amd.modules import HarmonyAttention
    cd = ocfg.cross_attention_dim
    ha = det_fill(HarmonyAttention(image_hidden_size=128, text_context_dim=cd, inter_dim=512, cross_heads=8, reshape_blocks=8,
                                   cross_value_dim=64), 3)
    ip = IPAdapterXL(pipe, None, None, DEV, num_tokens=T_TOKENS, inference=True, number_class_crossattention=ha, dtype=dtype,
                     clip_embeddings_dim=128)
    det_fill(ip.image_proj_model, 5)
    for n, p in pipe.unet.attn_processors.items():                       # the adapter installed fresh IP processors: fill them
        det_fill(p, 9, prefix=n)
    embeds4 = (det_randn((1, 77, cd), 1), det_randn((1, 77, cd), 2), det_randn((1, ocfg.pooled_dim), 3), det_randn((1, ocfg.pooled_dim), 4))
    kw = dict(clip_image_embeds=det_randn((1, 128), 5), prompt_embeds=embeds4, extra_prompt_embeds=det_randn((1, 77, cd), 6), guidance_scale=cc.GUIDANCE)
    return ip, kw


@pytest.mark.parametrize("mode,cin", [("i2i", 4), ("inp", 4), ("inp", 9)])
def test_pipelines_equal_the_hand_driven_engine_sequence(mode, cin):
    from imagharmony_amd.denoise import DenoiseEngine
    from imagharmony_amd.schedulers import get_timesteps
    dtype = torch.float16
    hu, cn, hv, ocfg = _stack(dtype, cin)
    H, W, S, steps, strength = 256, 288, 2, 5, 0.6
    img, mask, ctrl = cc.image(H, W), (cc.half_mask(H, W) if mode == "inp" else None), cc.control_image(H, W)
    gl = lambda: [torch.Generator().manual_seed(s) for s in (5, 6)]
    e = cc.embeds(S)
    pipe = _pipe(mode, hu, cn, hv, "ddim", dtype)
    assert pipe.controlnet is cn and pipe.engine.controlnet is cn
    out = pipe(image=img, control_image=ctrl, strength=strength, num_inference_steps=steps, guidance_scale=cc.GUIDANCE, generator=gl(),
               output_type="latent", controlnet_conditioning_scale=0.7, controlnet_guidance_start=0.0, controlnet_guidance_end=0.67,
               **({"mask_image": mask} if mask is not None else {}), **e).images
    sched = _scheduler("ddim")
    sched.set_timesteps(steps)
    _, t_start = get_timesteps(sched, steps, strength)
    assert t_start == 2
    eng = DenoiseEngine(hu, DEV, dtype)
    eng.set_controlnet(cn)
    eng.set_conditioning(e["prompt_embeds"], e["negative_prompt_embeds"], e["pooled_prompt_embeds"], e["negative_pooled_prompt_embeds"],
                         H, W, guidance_scale=cc.GUIDANCE)
    eng.set_control_image(ctrl, conditioning_scale=0.7)
    eng.set_schedule(sched, steps, t_start=t_start, inpaint=mode == "inp", controlnet_guidance_start=0.0, controlnet_guidance_end=0.67)
    # three steps run; the window keeps the first two of them
    assert eng.cn_scale_tab.cpu().tolist() == torch.tensor([0.7, 0.7, 0.7, 0.7, 0.0], dtype=torch.float32).tolist()
    _edit_hand_over(eng, hv, sched, t_start, cin, img, mask, S, gl(), strength)
    assert out.shape == (S, 4, H // 8, W // 8) and torch.isfinite(out).all() and torch.equal(out, eng.denoise(None))
    # the same pipe again, at another size and batch (the previous call's control image is not prepared again at the new size)
    out2 = pipe(image=cc.image(256, 256), control_image=cc.control_image(128, 128), strength=strength, num_inference_steps=steps,
                guidance_scale=cc.GUIDANCE, generator=torch.Generator().manual_seed(5), output_type="latent",
                **({"mask_image": cc.half_mask(256, 256)} if mask is not None else {}), **cc.embeds(1)).images
    assert out2.shape == (1, 4, 32, 32) and torch.isfinite(out2).all()


@pytest.mark.parametrize("mode", ["i2i", "inp"])
def test_ipadapterxl_generate_reaches_the_controlnet_edit_pipelines_and_refusals(mode):
    from imagharmony_amd.attention_processor import CNAttnProcessor2_0
    from imagharmony_amd.pipeline import (StableDiffusionXLControlNetImg2ImgCustomPipeline, StableDiffusionXLControlNetInpaintCustomPipeline,
                                          StableDiffusionXLImg2ImgCustomPipeline, StableDiffusionXLInpaintCustomPipeline)
    from imagharmony_amd.utils import get_generator
    dtype = torch.bfloat16
    hu, cn, hv, ocfg = _stack(dtype, 4, private=True)
    pipe = _pipe(mode, hu, cn, hv, "ddim", dtype)
    assert isinstance(pipe, StableDiffusionXLControlNetImg2ImgCustomPipeline if mode == "i2i" else StableDiffusionXLControlNetInpaintCustomPipeline)
    assert isinstance(pipe, StableDiffusionXLImg2ImgCustomPipeline if mode == "i2i" else StableDiffusionXLInpaintCustomPipeline)
    before = next(iter(cn.attn_processors.values()))
    ip, kw = _adapter(pipe, ocfg, dtype)
    procs = list(pipe.controlnet.attn_processors.values())
    assert isinstance(procs[0], CNAttnProcessor2_0) and all(p is procs[0] for p in procs) and procs[0] is not before
    H = W = 256
    img, mask, ctrl = cc.image(H, W), cc.half_mask(H, W), cc.control_image(H, W)
    kw = dict(kw, num_samples=1, seed=42, num_inference_steps=4, image=img, strength=0.75, control_image=ctrl, output_type="latent",
              **({"mask_image": mask} if mode == "inp" else {}))
    seen = {}

    class Spy:
        def __getattr__(self, k):
            return getattr(pipe, k)

        def __call__(self, **a):
            seen.update(a)
            return pipe(**a)
    ip.pipe = Spy()
    a = ip.generate(controlnet_conditioning_scale=0.7, **kw)
    ip.pipe = pipe
    assert seen["control_image"] is ctrl and seen["image"] is img and seen["strength"] == 0.75 and seen["controlnet_conditioning_scale"] == 0.7
    assert (seen.get("mask_image") is mask) == (mode == "inp")
    assert a.shape == (1, 4, 32, 32) and torch.isfinite(a).all()
    assert torch.equal(a, pipe(**{**seen, "generator": get_generator(42, "cpu")}).images)
    b = ip.generate(controlnet_conditioning_scale=0.0, **kw)
    assert not torch.equal(a, b)
    # refusals
    e = dict(cc.embeds(1), image=img, strength=0.75, num_inference_steps=4, output_type="latent", **({"mask_image": mask} if mode == "inp" else {}))
    with pytest.raises(ValueError, match="control_image"):
        pipe(**e)
    for window in ((0.5, 0.25), (-0.1, 1.0), (0.0, 1.5)):
        with pytest.raises(ValueError, match="window"):
            pipe(control_image=ctrl, controlnet_guidance_start=window[0], controlnet_guidance_end=window[1], **e)
    with pytest.raises(NotImplementedError, match="guess_mode"):
        pipe(control_image=ctrl, guess_mode=True, **e)
    with pytest.raises(NotImplementedError, match="list of conditioning scales"):
        pipe(control_image=ctrl, controlnet_conditioning_scale=[0.5, 0.5], **e)
    with pytest.raises(NotImplementedError, match="latents="):           # ... and the parent edit call's own
        pipe(control_image=ctrl, latents=torch.zeros(1, 4, 32, 32), **e)
    with pytest.raises(ValueError, match="strength"):
        pipe(control_image=ctrl, **dict(e, strength=1.5))
    with pytest.raises(ValueError, match="control images"):
        pipe(control_image=torch.cat([ctrl] * 3), **e)

    class Multi:
        nets = [cn, cn]
    with pytest.raises(NotImplementedError, match="MultiControlNetModel"):
        type(pipe)(hu, Multi(), device=DEV, dtype=dtype)


# ---------------------------------------------------------------------------------------------------- 6. PNS
SEEDS = [3, 9, 27]
PREVIEW, FINAL, STRENGTH = 4, 6, 0.6            # as tests/test_gpu_pns_edit.py: the preview runs rows 2..3, the final rows 3..5
WINDOW = dict(controlnet_guidance_start=0.0, controlnet_guidance_end=0.7)


def _scorer(lat):
    from imagharmony_amd import pns
    return torch.cat([pns.default_scorer(lat[k:k + 1].float().cpu()) for k in range(lat.shape[0])])


def _pns_adapter(mode, cin, dtype, kind="ddim"):
    """(IPAdapterXL over the mode's ControlNet pipe, generate_pns's keyword arguments, the pipe call's own keyword arguments)"""
    hu, cn, hv, ocfg = _stack(dtype, cin, private=True)
    pipe = _pipe(mode, hu, cn, hv, kind, dtype)
    ip, kw = _adapter(pipe, ocfg, dtype)
    H = W = 256
    ctrl = cc.control_image(H, W)
    kw = dict(kw, scale=0.8, control_image=ctrl, controlnet_conditioning_scale=0.9, **WINDOW)
    call = dict(controlnet_conditioning_scale=0.9, **WINDOW)
    if mode == "t2i":
        kw.update(height=H, width=W)
        call.update(image=ctrl, height=H, width=W)                        # the text-to-image class calls its control image `image`
    else:
        edit = dict(image=cc.image(H, W), strength=STRENGTH, **({"mask_image": cc.half_mask(H, W)} if mode == "inp" else {}))
        kw.update(edit)
        call.update(edit, control_image=ctrl)
    return ip, kw, call


def _direct(ip, kw, call, seed, steps, **extra):
    """the pipe's own call for one seed under generate_pns's conditioning, generator=[manual_seed(seed)]"""
    fused = ip.fused_clip_embeds(None, kw["clip_image_embeds"], kw["extra_prompt_embeds"])
    ipe = ip._g(ip.image_proj_model)(fused)
    uipe = ip._g(ip.image_proj_model)(torch.zeros_like(fused))
    pe, ne, ppe, npe = kw["prompt_embeds"]
    pe = torch.cat([pe.to(ipe.device, ip.dtype), ipe], dim=1)
    ne = torch.cat([ne.to(ipe.device, ip.dtype), uipe], dim=1)
    return ip.pipe(prompt_embeds=pe, negative_prompt_embeds=ne, pooled_prompt_embeds=ppe, negative_pooled_prompt_embeds=npe,
                   num_inference_steps=steps, guidance_scale=kw["guidance_scale"], output_type="latent",
                   generator=[torch.Generator("cpu").manual_seed(int(seed))], **call, **extra).images


@pytest.mark.parametrize("mode,cin", [("t2i", 4), ("i2i", 4), ("inp", 4), ("inp", 9)])
def test_pns_winner_under_a_controlnet_equals_the_pipes_own_call(mode, cin):
    dtype = torch.float16
    ip, kw, call = _pns_adapter(mode, cin, dtype)
    r = ip.generate_pns(SEEDS, preview_steps=PREVIEW, num_inference_steps=FINAL, batch=2, output_type="latent", scorer=_scorer, **kw)
    lat = r["latents"].to(DEV)
    eng = ip.pipe.engine
    assert r["scores"].shape == (len(SEEDS),) and torch.isfinite(r["scores"]).all() and r["scores"].unique().numel() == len(SEEDS)
    assert lat.shape == (1, 4, 32, 32) and torch.isfinite(lat).all() and r["best_seed"] in SEEDS
    assert eng.controlnet is ip.pipe.controlnet and eng.cn["scale"] == 0.9 and eng.cn["hint"].shape[0] == 1      # one hint for every candidate
    direct = _direct(ip, kw, call, r["best_seed"], FINAL)
    assert torch.equal(direct.float(), lat)
    # the branch acts in PNS: without the control's weight the winner's trajectory is another one
    assert not torch.equal(_direct(ip, kw, dict(call, controlnet_conditioning_scale=0.0), r["best_seed"], FINAL).float(), lat)
    # the previews too are the pipe's own short calls, whether the candidate was stacked (seed 1 of the first pair) or ran alone (the ragged tail)
    for k in (1, 2):
        assert float(_scorer(_direct(ip, kw, call, SEEDS[k], PREVIEW))[0]) == float(r["scores"][k]), k


def test_pns_under_a_controlnet_and_euler_ancestral_with_step_noise_from_the_seed():
    dtype = torch.float16
    ip, kw, call = _pns_adapter("inp", 4, dtype, kind="euler-a")
    r = ip.generate_pns(SEEDS, preview_steps=PREVIEW, num_inference_steps=FINAL, batch=2, output_type="latent", scorer=_scorer,
                        step_noise="seed", **kw)
    lat = r["latents"].to(DEV)
    assert ip.pipe.engine.seeded and torch.isfinite(lat).all()
    assert torch.equal(_direct(ip, kw, call, r["best_seed"], FINAL, step_noise="seeded").float(), lat)
    assert not torch.equal(_direct(ip, kw, call, r["best_seed"], FINAL).float(), lat)         # the generator's own step noise: another trajectory


def test_pns_control_image_refusals_come_before_any_gpu_work(monkeypatch):
    from imagharmony_amd import denoise
    dtype = torch.float16
    ip, kw, call = _pns_adapter("i2i", 4, dtype)
    t2i, tkw, _ = _pns_adapter("t2i", 4, dtype)
    hu, cn, hv, ocfg = _stack(dtype, 4, private=True)
    plain, pkw = _adapter(_pipe("i2i", hu, None, hv, "ddim", dtype), ocfg, dtype)

    def no_ctx(*a, **k):
        raise AssertionError("a Ctx was built before the refusal")
    monkeypatch.setattr(denoise, "Ctx", no_ctx)
    with pytest.raises(ValueError, match="control_image"):
        ip.generate_pns(SEEDS, output_type="latent", **{k: v for k, v in kw.items() if k != "control_image"})
    with pytest.raises(ValueError, match="control_image"):
        plain.generate_pns(SEEDS, output_type="latent", image=kw["image"], strength=STRENGTH, control_image=kw["control_image"], **pkw)
    with pytest.raises(NotImplementedError, match="list of conditioning scales"):
        ip.generate_pns(SEEDS, output_type="latent", **dict(kw, controlnet_conditioning_scale=[1.0, 1.0]))
    with pytest.raises(ValueError, match="image="):                       # the text-to-image ControlNet pipe: image= stays refused
        t2i.generate_pns(SEEDS, output_type="latent", image=kw["image"], **tkw)
