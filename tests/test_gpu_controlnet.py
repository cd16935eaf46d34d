"""GPU tests of the SDXL ControlNet: the gated add with GroupNorm partials (imh_control_add) bit for bit against torch and against the
statistics pass, the hint tower, the forward with residual injection and the denoise loop against the CPU fp32 reference
(tests/controlnet_reference.py), plan / graph equality, and the public pipeline."""
import functools
import json
import math
import os
import types

import pytest
import torch

from conftest import PARITY_JSON, rel_rms
from oracle import modules as om
from oracle.detfill import det_fill, det_randn
from oracle.pipeline import install_ip_processors
from oracle.sdxl_unet import UNet2DConditionModel as OracleUNet
from oracle.sdxl_unet import UNetConfig as OracleConfig
from oracle.sdxl_unet import tiny_config

import controlnet_reference as cr
from test_gpu_unet import TOL, build_pair

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float16, torch.bfloat16]
VAE_CONV_TOL = {torch.bfloat16: 3e-2, torch.float16: 8e-3}      # what tests/test_gpu_vae.py holds its 16-bit conv stacks to
LOOP_TOL = {torch.bfloat16: 3e-2, torch.float16: 1e-2}          # tests/test_gpu_pipeline.py's bounds for its tiny trajectories
T_TOKENS = 4
PARITY = {}


def wide_config():
    """SDXL's widths (320 / 640 / 1280: GroupNorm sub-runs of 10, K up to 1280) on a shallow stack with a narrow text dim: the CPU
    reference's forwards take about a second each; filling its 0.8 + 0.4 G parameters deterministically is the larger cost, paid once
    per session (the reference models and outputs are cached and shared by every case)"""
    return OracleConfig(block_out_channels=(320, 640, 1280), transformer_layers_per_block=(1, 1, 2), attention_head_dim=(5, 10, 20),
                        cross_attention_dim=256, addition_time_embed_dim=64, projection_class_embeddings_input_dim=128 + 6 * 64, sample_size=32)


def _control_image(n=1, hw=256, seed=9):
    """a smooth-ish image in [0, 1] with structure at every scale of the hint tower"""
    return det_randn((n, 3, hw, hw), seed).mul(0.25).add(0.5).clamp(0, 1)


# ---------------------------------------------------------------------------------------------------- the op
OP_SHAPES = [(2, 15, 64, 2),         # fewer pixels than pixel lanes
             (2, 24, 64, 1),         # broadcast of r over the batch
             (2, 1024, 320, 2),      # sub-runs of 10
             (1, 256, 1280, 1)]      # widest channel count
GATES = (0.0, 0.5, 1.0)


def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", OP_SHAPES)
def test_control_add_bits_partials_plan_and_graph(dtype, shape):
    from imagharmony_amd import lib as L
    from imagharmony_amd.ctx import Ctx
    B, HW, C_, Br = shape
    sub = math.gcd(C_ // 32, 10)
    x = det_randn((B, HW, C_), 21).to(dtype).to(DEV)
    r = det_randn((Br, HW, C_), 22).to(dtype).to(DEV)
    tab = torch.tensor(GATES, dtype=torch.float32, device=DEV)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    eager = Ctx(DEV, dtype)
    want = []
    for i, g in enumerate(GATES):
        step.fill_(i)
        y, gs = eager.control_add(x, r, scale=1.0, tab=tab, step=step, gn_sub=sub)
        torch.cuda.synchronize()
        ref = (x.float() + g * r.float().repeat(B // Br, 1, 1)).to(dtype)
        assert torch.equal(_bits(y), _bits(ref)), (shape, g)
        if g == 0.0:
            assert torch.equal(_bits(y), _bits(x))
        st = eager.gn_stats(y, sub)
        torch.cuda.synchronize()
        assert (gs.nblk, gs.sub, gs.npart, gs.C) == (st.nblk, st.sub, 0, C_) and gs.t.shape == st.t.shape
        assert torch.equal(_bits(gs.t), _bits(st.t)), (shape, g)
        assert torch.isfinite(gs.t).all()
        want.append((y.clone(), gs.t.clone()))
        # without partials: the same y
        assert torch.equal(_bits(eager.control_add(x, r, scale=1.0, tab=tab, step=step)), _bits(y))
    # a fixed scale without a table: g = scale
    y5 = eager.control_add(x, r, scale=0.5)
    assert torch.equal(_bits(y5), _bits(want[1][0]))
    # recorded plan and graph replay, the device counter advancing in the plan itself
    rec = Ctx(DEV, dtype, record=True)
    yp, gp = rec.control_add(x, r, scale=1.0, tab=tab, step=step, gn_sub=sub)
    rec.ew(L.EW_STEP_SET, step, i=(0, 0, 0, 0, 0, 0), descr="step++")
    for replay in (False, True):
        if replay:
            rec.capture()
        step.zero_()
        for i in range(len(GATES)):
            yp.zero_(); gp.t.zero_()
            rec.replay() if replay else rec.run()
            torch.cuda.synchronize()
            assert int(step.item()) == i + 1
            assert torch.equal(_bits(yp), _bits(want[i][0])) and torch.equal(_bits(gp.t), _bits(want[i][1])), (shape, replay, i)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", OP_SHAPES)
def test_control_add_guarded_placement(dtype, shape):
    from guarded import run_dense_and_guarded
    B, HW, C_, Br = shape
    sub = math.gcd(C_ // 32, 10)
    x, r = det_randn((B, HW, C_), 21).to(dtype).to(DEV), det_randn((Br, HW, C_), 22).to(dtype).to(DEV)
    tab = torch.tensor(GATES, dtype=torch.float32, device=DEV)
    step = torch.ones(1, dtype=torch.int32, device=DEV)

    def body(ctx, put, out):
        y, gs = ctx.control_add(put(x), put(r), scale=1.0, tab=put(tab), step=put(step), gn_sub=sub)
        return y, gs.t
    dense, guarded, arena = run_dense_and_guarded(DEV, dtype, body)
    arena.check()                                   # no byte outside y and the partials changed; both are finite
    for a, b in zip(dense, guarded):
        assert torch.equal(_bits(a), _bits(b))


def test_control_add_refusals():
    from imagharmony_amd import lib as L
    from imagharmony_amd.ctx import Ctx
    ctx = Ctx(DEV, torch.bfloat16)
    x = torch.zeros(2, 16, 64, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(L.ImhError):
        ctx.control_add(x, torch.zeros(2, 16, 32, dtype=torch.bfloat16, device=DEV))
    with pytest.raises(L.ImhError):
        ctx.control_add(x, x, tab=torch.zeros(3, device=DEV))                       # a table without the counter
    with pytest.raises(L.ImhError):
        ctx.control_add(x, x, gn_sub=7)
    a = L.ControlAddArgs()                                                          # the library's own: the in-place form
    a.x, a.r, a.y, a.B, a.Br, a.HW, a.C, a.dtype = x.data_ptr(), x.data_ptr(), x.data_ptr(), 2, 2, 16, 64, 0
    import ctypes as C
    assert ctx.lib.imh_control_add(C.byref(a), ctx.stream()) == -1


# ---------------------------------------------------------------------------------------------------- stacks
def _product_cfg(ocfg):
    from imagharmony_amd.unet import UNetConfig
    return UNetConfig(**{k: getattr(ocfg, k) for k in UNetConfig.__dataclass_fields__})


def _build_wide(dtype):
    """build_pair's recipe (tests/test_gpu_unet.py) on wide_config()"""
    from imagharmony_amd.attention_processor import AttnProcessor2_0, IPAttnProcessor2_0
    from imagharmony_amd.unet import UNet2DConditionModel
    ocfg = wide_config()
    ou, procs = _wide_oracle()
    hu = UNet2DConditionModel(_product_cfg(ocfg))
    hu.set_attn_processor({n: AttnProcessor2_0() if isinstance(p, om.AttnProcessor2_0) else
                           IPAttnProcessor2_0(p.hidden_size, p.cross_attention_dim, scale=p.scale, num_tokens=p.num_tokens, skip=p.skip)
                           for n, p in procs.items()})
    hu.load_state_dict(ou.state_dict(), strict=True)
    return ou, hu.to(DEV, dtype), ocfg


@functools.lru_cache(maxsize=None)
def _wide_oracle():
    with torch.no_grad():
        ou = det_fill(OracleUNet(wide_config()), 5).eval()
        procs = install_ip_processors(ou, num_tokens=T_TOKENS, scale=0.8)
        for n, p in procs.items():
            if isinstance(p, om.IPAttnProcessor2_0):
                det_fill(p, 7, prefix=n)
    return ou, procs


@functools.lru_cache(maxsize=None)
def _ref_controlnet(width):
    """the reference ControlNet, det_filled -- zero convs included: they are zero by construction and would otherwise test nothing"""
    ocfg = tiny_config() if width == "tiny" else wide_config()
    with torch.no_grad():
        rc = det_fill(cr.RefControlNet(ocfg), 11).eval()
    rc.set_attn_processor(cr.RefCNAttnProcessor(T_TOKENS))
    return rc


def _stack(width, dtype):
    """(oracle UNet, reference ControlNet, product UNet, product ControlNet, config): identical weights on both sides; the product's
    processors installed by IPAdapter.set_ip_adapter's own code (IP processors on the UNet, ONE CNAttnProcessor2_0 on the ControlNet)"""
    from imagharmony_amd.attention_processor import CNAttnProcessor2_0, IPAttnProcessor2_0
    from imagharmony_amd.controlnet import ControlNetModel
    from imagharmony_amd.ip_adapter import IPAdapter
    ou, hu, ocfg = build_pair(dtype, num_tokens=T_TOKENS) if width == "tiny" else _build_wide(dtype)
    rc = _ref_controlnet(width)
    cn = ControlNetModel(_product_cfg(ocfg))
    cn.load_state_dict(rc.state_dict(), strict=True)
    cn = cn.to(DEV, dtype)
    shim = types.SimpleNamespace(pipe=types.SimpleNamespace(unet=hu, controlnet=cn), num_tokens=T_TOKENS, device=DEV, dtype=dtype)
    IPAdapter.set_ip_adapter(shim)
    for name, p in hu.attn_processors.items():                     # set_ip_adapter installed fresh IP processors: the oracle's weights and scale
        if isinstance(p, IPAttnProcessor2_0):
            p.load_state_dict(ou.attn_processors[name].state_dict())
            p.scale = ou.attn_processors[name].scale
            p.to(DEV, dtype)
    procs = list(cn.attn_processors.values())
    assert isinstance(procs[0], CNAttnProcessor2_0) and all(p is procs[0] for p in procs)
    return ou, rc, hu, cn, ocfg


def _inputs(ocfg, hw=32):
    cd = ocfg.cross_attention_dim
    x = det_randn((1, 4, hw, hw), 3)
    ehs = det_randn((2, 77 + T_TOKENS, cd), 4)
    te = det_randn((2, ocfg.pooled_dim), 6)
    ids = torch.tensor([[hw * 8, hw * 8, 0, 0, hw * 8, hw * 8]], dtype=torch.float32).repeat(2, 1)
    return x, ehs, te, ids


def _product_forward(hu, cn, dtype, x, t, ehs, te, ids, img, scale, how="eager"):
    """CFG batch 2 on one latent.  cn None: the plain forward.  how: eager | plan | graph -> NCHW fp32 on the CPU"""
    from imagharmony_amd.controlnet import control_state
    from imagharmony_amd.ctx import Ctx
    Hl, Wl = x.shape[2:]
    pre = Ctx(DEV, dtype)
    st = hu.prepare_conditioning(pre, ehs.to(DEV, dtype), te.to(DEV, dtype), ids.to(DEV))
    st.t_value = torch.full((2,), float(t), device=DEV)
    st.latents = x.to(DEV).float().contiguous()
    ctx = Ctx(DEV, dtype, record=how != "eager")
    control = None
    if cn is not None:
        cst = control_state(st, cn.prepare_conditioning(pre, ehs.to(DEV, dtype), te.to(DEV, dtype), ids.to(DEV)))
        hint = cn.prepare_hint(pre, img, Hl, Wl)
        control = cn.emit_forward(ctx, cst, 1, Hl, Wl, cfg_dup=True, hint=hint, scale=scale)
    out = hu.emit_forward(ctx, st, 1, Hl, Wl, cfg_dup=True, control=control)
    if how == "plan":
        ctx.run()
    elif how == "graph":
        ctx.capture()
        ctx.replay()
    torch.cuda.synchronize()
    return out.view(2, Hl, Wl, 4).permute(0, 3, 1, 2).float().cpu()


# ---------------------------------------------------------------------------------------------------- the hint tower
@functools.lru_cache(maxsize=None)
def _ref_hint(width, S):
    rc = _ref_controlnet(width)
    img = _control_image(S, 128)
    with torch.no_grad():
        return img, rc.controlnet_cond_embedding(img)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("width", ["tiny", "wide"])
def test_hint_tower_matches_reference(width, S, dtype):
    from imagharmony_amd.controlnet import ControlNetModel
    from imagharmony_amd.ctx import Ctx
    ocfg = tiny_config() if width == "tiny" else wide_config()
    rc = _ref_controlnet(width)
    cn = ControlNetModel(_product_cfg(ocfg))
    emb_sd = {k: v for k, v in rc.state_dict().items() if k.startswith("controlnet_cond_embedding")}
    cn.load_state_dict(emb_sd, strict=False)
    cn.controlnet_cond_embedding.to(DEV, dtype)
    img, ref = _ref_hint(width, S)
    hint = cn.prepare_hint(Ctx(DEV, dtype), img, 16, 16)
    torch.cuda.synchronize()
    assert hint.shape == (S, 16, 16, ocfg.block_out_channels[0]) and hint.dtype == dtype and hint.is_contiguous()
    r = rel_rms(hint.permute(0, 3, 1, 2).float().cpu(), ref)
    print(f"hint tower {width} S={S} {dtype}: rel-rms {r:.3e} (bound {VAE_CONV_TOL[dtype]:.0e})")
    assert torch.isfinite(hint).all() and r < VAE_CONV_TOL[dtype], r


# ---------------------------------------------------------------------------------------------------- forward parity
@functools.lru_cache(maxsize=None)
def _ref_forward(width, scale):
    """(reference prediction with the ControlNet, without it), CPU fp32, once per width"""
    ocfg = tiny_config() if width == "tiny" else wide_config()
    ou = det_fill(OracleUNet(tiny_config()), 5).eval() if width == "tiny" else _wide_oracle()[0]
    if width == "tiny":
        with torch.no_grad():
            procs = install_ip_processors(ou, num_tokens=T_TOKENS, scale=0.8)
            for n, p in procs.items():
                if isinstance(p, om.IPAttnProcessor2_0):
                    det_fill(p, 7, prefix=n)
    rc = _ref_controlnet(width)
    x, ehs, te, ids = _inputs(ocfg)
    added = {"text_embeds": te, "time_ids": ids}
    x2 = torch.cat([x, x], 0)
    with torch.no_grad():
        down, mid = rc(x2, torch.tensor(500.0), ehs, _control_image(), conditioning_scale=scale, added_cond_kwargs=added)
        return cr.unet_forward(ou, x2, torch.tensor(500.0), ehs, added, down, mid), cr.unet_forward(ou, x2, torch.tensor(500.0), ehs, added)


FORWARD_SCALE = 1.0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("width", ["tiny", "wide"])
def test_forward_with_controlnet_matches_reference(width, dtype):
    ou, rc, hu, cn, ocfg = _stack(width, dtype)
    ref_cn, ref_plain = _ref_forward(width, FORWARD_SCALE)
    # the condition on the inputs: the control must be visible far above the bound.  On the CPU reference the det_filled ControlNet at
    # scale 1 moves the prediction by 0.82 (tiny) / 0.70 (wide) rel-RMS (profiles/controlnet_parity.json: control_visibility)
    vis = rel_rms(ref_cn, ref_plain)
    assert vis >= 5 * TOL[dtype], f"the ControlNet moves the reference's prediction by {vis:.3e} only"
    x, ehs, te, ids = _inputs(ocfg)
    y_cn = _product_forward(hu, cn, dtype, x, 500.0, ehs, te, ids, _control_image(), FORWARD_SCALE)
    y_plain = _product_forward(hu, None, dtype, x, 500.0, ehs, te, ids, None, 1.0)
    r_cn, r_plain = rel_rms(y_cn, ref_cn), rel_rms(y_plain, ref_plain)
    print(f"forward {width} {dtype}: with ControlNet rel-rms {r_cn:.3e}, plain {r_plain:.3e} (bound {TOL[dtype]:.0e}); "
          f"the control moves the reference by {vis:.3e}")
    PARITY[f"{width}_{str(dtype).replace('torch.', '')}"] = dict(with_controlnet=r_cn, plain=r_plain, bound=TOL[dtype], control_visibility=vis)
    try:
        out_dir = os.path.dirname(PARITY_JSON)          # beside the suite's measured-parity record; the round's copy is profiles/controlnet_parity.json
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "controlnet_parity.json"), "w") as f:
            json.dump(PARITY, f, indent=1, sort_keys=True)
    except OSError:
        pass
    assert torch.isfinite(y_cn).all() and r_cn < TOL[dtype], r_cn
    assert r_plain < TOL[dtype], r_plain


def test_plan_and_graph_equal_eager_with_controlnet():
    dtype = torch.bfloat16
    ou, rc, hu, cn, ocfg = _stack("tiny", dtype)
    x, ehs, te, ids = _inputs(ocfg)
    img = _control_image()
    ys = [_product_forward(hu, cn, dtype, x, 321.0, ehs, te, ids, img, 0.7, how) for how in ("eager", "plan", "graph")]
    assert torch.isfinite(ys[0]).all() and torch.equal(ys[0], ys[1]) and torch.equal(ys[0], ys[2])
    assert not torch.equal(ys[0], _product_forward(hu, None, dtype, x, 321.0, ehs, te, ids, None, 1.0))


# ---------------------------------------------------------------------------------------------------- the loop
STEPS = 4
WINDOW = (0.25, 0.75)          # of 4 steps: the first and the last are gated off
LOOP_SCALE = 0.8


def _loop_inputs(ocfg, S=1):
    cd = ocfg.cross_attention_dim
    return (det_randn((S, 4, 32, 32), 3), det_randn((S, 77 + T_TOKENS, cd), 4), det_randn((S, 77 + T_TOKENS, cd), 5),
            det_randn((S, ocfg.pooled_dim), 6), det_randn((S, ocfg.pooled_dim), 7))


def _schedulers(kind, t_start):
    from imagharmony_amd import schedulers as hs
    from multistep_reference import RefDPMSolverMultistep
    from oracle.schedulers import DDIMScheduler as OracleDDIM
    if kind == "ddim":
        return hs.DDIMScheduler(), OracleDDIM()
    return hs.DPMSolverMultistepScheduler(), RefDPMSolverMultistep(t_start=t_start)


@functools.lru_cache(maxsize=None)
def _ref_loop(kind, t_start):
    ocfg = tiny_config()
    ou = det_fill(OracleUNet(ocfg), 5).eval()
    with torch.no_grad():
        procs = install_ip_processors(ou, num_tokens=T_TOKENS, scale=0.8)
        for n, p in procs.items():
            if isinstance(p, om.IPAttnProcessor2_0):
                det_fill(p, 7, prefix=n)
    lat, pe, ne, po, no = _loop_inputs(ocfg)
    run = lambda net: cr.denoise(ou, net, _schedulers(kind, t_start)[1], lat, pe, ne, po, no, 256, 256, _control_image(), STEPS, guidance_scale=5.0,
                                 conditioning_scale=LOOP_SCALE, controlnet_guidance_start=WINDOW[0], controlnet_guidance_end=WINDOW[1],
                                 t_start=t_start)
    return run(_ref_controlnet("tiny")), run(None)


def _engine(hu, cn, dtype, ocfg):
    from imagharmony_amd.denoise import DenoiseEngine
    lat, pe, ne, po, no = _loop_inputs(ocfg)
    eng = DenoiseEngine(hu, DEV, dtype)
    eng.set_controlnet(cn)
    eng.set_conditioning(pe, ne, po, no, 256, 256, guidance_scale=5.0)
    if cn is not None:
        eng.set_control_image(_control_image(), conditioning_scale=LOOP_SCALE)
    return eng, lat


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("t_start", [0, 1])
@pytest.mark.parametrize("kind", ["ddim", "dpmpp2m"])
def test_denoise_loop_with_controlnet_matches_reference(kind, t_start, dtype):
    ou, rc, hu, cn, ocfg = _stack("tiny", dtype)
    ref, ref_plain = _ref_loop(kind, t_start)
    assert rel_rms(ref, ref_plain) > 3 * LOOP_TOL[dtype]            # the branch is visible in the trajectory (0.15 - 0.21 on the CPU)
    eng, lat = _engine(hu, cn, dtype, ocfg)
    eng.set_schedule(_schedulers(kind, t_start)[0], STEPS, t_start=t_start, controlnet_guidance_start=WINDOW[0], controlnet_guidance_end=WINDOW[1])
    m = STEPS - t_start
    want = [LOOP_SCALE] * t_start + [LOOP_SCALE * cr.keep(i, m, *WINDOW) for i in range(m)]
    assert eng.cn_scale_tab.cpu().tolist() == torch.tensor(want, dtype=torch.float32).tolist()
    out = eng.denoise(lat).float().cpu()
    r = rel_rms(out, ref)
    print(f"{kind} t_start={t_start} {dtype}: {m}-step loop with ControlNet, window {WINDOW}: rel-rms {r:.3e} (bound {LOOP_TOL[dtype]:.0e})")
    assert torch.isfinite(out).all() and r < LOOP_TOL[dtype], r
    from imagharmony_amd import lib as L
    kinds = [eng.plan.lib.imh_plan_get_kind(eng.plan.plan, i) for i in range(eng.plan.lib.imh_plan_size(eng.plan.plan))]
    assert kinds.count(L.OP_CONTROL_ADD) == 11 and eng.plan.captured


def test_plans_with_and_without_controlnet_alternate_without_rerecording():
    from imagharmony_amd import schedulers as hs
    dtype = torch.bfloat16
    ou, rc, hu, cn, ocfg = _stack("tiny", dtype)
    eng, lat = _engine(hu, cn, dtype, ocfg)
    sch = hs.DDIMScheduler()
    eng.set_schedule(sch, 2)
    with_cn = eng.denoise(lat).clone()
    plan_cn = eng.plan
    eng.set_controlnet(None)
    eng.set_schedule(sch, 2)
    plain = eng.denoise(lat).clone()
    plan_plain = eng.plan
    assert plan_plain is not plan_cn and not torch.equal(with_cn, plain) and len(eng._plans) == 2
    for _ in range(2):
        eng.set_controlnet(cn)
        eng.set_schedule(sch, 2)
        assert eng.plan is plan_cn and torch.equal(eng.denoise(lat), with_cn)
        eng.set_controlnet(None)
        eng.set_schedule(sch, 2)
        assert eng.plan is plan_plain and torch.equal(eng.denoise(lat), plain)
    # the plain plan is what an engine that never saw a ControlNet runs
    fresh, _ = _engine(hu, None, dtype, ocfg)
    fresh.set_schedule(hs.DDIMScheduler(), 2)
    assert torch.equal(fresh.denoise(lat), plain)
    # a fork shares the hint, the caches and the table, and computes the same
    eng.set_controlnet(cn)
    eng.set_schedule(sch, 2)
    fk = eng.fork()
    assert fk.cn is eng.cn and fk.cn_scale_tab is eng.cn_scale_tab and fk.controlnet is cn
    assert torch.equal(fk.denoise(lat), with_cn)


# ---------------------------------------------------------------------------------------------------- the public surface
def test_pipeline_equals_engine_and_ipadapter_generate_and_refusals():
    from imagharmony_amd import ControlNetModel, StableDiffusionXLControlNetCustomPipeline
    from imagharmony_amd import schedulers as hs
    from imagharmony_amd.attention_processor import CNAttnProcessor2_0
    from imagharmony_amd.denoise import DenoiseEngine
    from imagharmony_amd.ip_adapter import IPAdapterXL
    from imagharmony_amd.modules import HarmonyAttention
    dtype = torch.float16
    ou, rc, hu, cn, ocfg = _stack("tiny", dtype)
    assert isinstance(cn, ControlNetModel)
    lat, pe, ne, po, no = _loop_inputs(ocfg)
    img = _control_image()
    pipe = StableDiffusionXLControlNetCustomPipeline(hu, cn, scheduler=hs.DDIMScheduler(), device=DEV, dtype=dtype)
    assert pipe.controlnet is cn
    out = pipe(prompt_embeds=pe, negative_prompt_embeds=ne, pooled_prompt_embeds=po, negative_pooled_prompt_embeds=no, image=img,
               height=256, width=256, num_inference_steps=3, guidance_scale=5.0, latents=lat, output_type="latent",
               controlnet_conditioning_scale=0.7, controlnet_guidance_start=0.0, controlnet_guidance_end=0.67).images
    eng = DenoiseEngine(hu, DEV, dtype)
    eng.set_controlnet(cn)
    eng.set_conditioning(pe, ne, po, no, 256, 256, guidance_scale=5.0)
    eng.set_control_image(img, conditioning_scale=0.7)
    eng.set_schedule(hs.DDIMScheduler(), 3, controlnet_guidance_start=0.0, controlnet_guidance_end=0.67)
    assert eng.cn_scale_tab.cpu().tolist() == torch.tensor([0.7, 0.7, 0.0], dtype=torch.float32).tolist()
    assert out.shape == (1, 4, 32, 32) and torch.equal(out, eng.denoise(lat))
    # a PIL control image of another size is resized, not normalised
    from PIL import Image
    pil = Image.fromarray((img[0].permute(1, 2, 0) * 255).round().byte().numpy()).resize((128, 128))
    out_pil = pipe(prompt_embeds=pe, negative_prompt_embeds=ne, pooled_prompt_embeds=po, negative_pooled_prompt_embeds=no, image=pil,
                   height=256, width=256, num_inference_steps=2, guidance_scale=5.0, latents=lat, output_type="latent").images
    assert torch.isfinite(out_pil).all()
    # IPAdapterXL on the pipe: CNAttnProcessor2_0 goes onto the ControlNet through the adapter's own code; one control image, two samples
    ha = det_fill(HarmonyAttention(image_hidden_size=128, text_context_dim=ocfg.cross_attention_dim, inter_dim=512,
                                   cross_heads=8, reshape_blocks=8, cross_value_dim=64), 3)
    before = next(iter(cn.attn_processors.values()))                   # (what _stack installed: the adapter must install its own)
    ip = IPAdapterXL(pipe, None, None, DEV, num_tokens=4, inference=True, number_class_crossattention=ha, dtype=dtype, clip_embeddings_dim=128)
    procs = list(pipe.controlnet.attn_processors.values())
    assert isinstance(procs[0], CNAttnProcessor2_0) and all(p is procs[0] for p in procs) and procs[0] is not before
    det_fill(ip.image_proj_model, 5)
    for n, p in hu.attn_processors.items():
        det_fill(p, 9, prefix=n)
    cd = ocfg.cross_attention_dim
    rep = lambda t: t.repeat(2, *([1] * (t.dim() - 1)))              # (prompt embeddings handed over already tiled to num_samples)
    embeds = tuple(rep(t) for t in (det_randn((1, 77, cd), 1), det_randn((1, 77, cd), 2), det_randn((1, ocfg.pooled_dim), 3), det_randn((1, ocfg.pooled_dim), 4)))
    kw = dict(clip_image_embeds=det_randn((1, 128), 5), prompt_embeds=embeds, extra_prompt_embeds=det_randn((1, 77, cd), 6),
              num_samples=2, num_inference_steps=2, guidance_scale=5.0, height=256, width=256, number_class_crossattention=ha,
              output_type="latent", seed=42)
    a = ip.generate(image=img, controlnet_conditioning_scale=0.7, **kw)
    b = ip.generate(image=img, controlnet_conditioning_scale=0.0, **kw)
    assert a.shape == (2, 4, 32, 32) and torch.isfinite(a).all() and not torch.equal(a, b)
    # refusals
    with pytest.raises(NotImplementedError, match="guess_mode"):
        pipe(prompt_embeds=pe, negative_prompt_embeds=ne, pooled_prompt_embeds=po, negative_pooled_prompt_embeds=no, image=img,
             height=256, width=256, num_inference_steps=2, latents=lat, output_type="latent", guess_mode=True)

    class Multi:
        nets = [cn, cn]
    with pytest.raises(NotImplementedError, match="MultiControlNetModel"):
        StableDiffusionXLControlNetCustomPipeline(hu, Multi(), device=DEV, dtype=dtype)
    with pytest.raises(NotImplementedError, match="MultiControlNetModel"):
        DenoiseEngine(hu, DEV, dtype).set_controlnet(Multi())
    split = DenoiseEngine(hu, DEV, dtype)
    split.set_conditioning(pe, ne, po, no, 256, 256, guidance_scale=5.0, cfg_role=1)
    with pytest.raises(NotImplementedError, match="cfg_role"):
        split.set_controlnet(cn)
    split2 = DenoiseEngine(hu, DEV, dtype)
    split2.set_controlnet(cn)
    with pytest.raises(NotImplementedError, match="cfg_role"):
        split2.set_conditioning(pe, ne, po, no, 256, 256, guidance_scale=5.0, cfg_role=0)
