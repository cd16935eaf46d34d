"""GPU: regional image prompts above the kernel, on the tiny stacks the ControlNet / adapter tests use -- the UNet forward against the
oracle UNet carrying the restated processor (tests/ip_regions_reference.py), eager = plan = replayed graph, the launch lists with and
without regions, the 4-step DDIM loop (text-to-image and 4-channel inpainting) against the restated loop, the plan cache, and
IPAdapterXL.generate_regions on the tiny pipe."""
import contextlib
import functools

import pytest
import torch

import ip_regions_reference as rr
from conftest import rel_rms
from oracle.detfill import det_fill, det_randn
from oracle.pipeline import denoise as oracle_denoise
from oracle.schedulers import DDIMScheduler as OracleDDIM
from test_gpu_controlnet import LOOP_TOL
from test_gpu_inpaint import IMG, _gens, _oracle_inpaint, _pipe, build_vae_pair, centred_mask
from test_gpu_unet import TOL
from test_gpu_unet import build_pair as fresh_pair

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float16, torch.bfloat16]
T_TOKENS, N = 4, 2
WEIGHTS = (1.0, 0.8)
STEPS = 4


@functools.lru_cache(maxsize=None)
def build_pair(dtype, in_channels=4):
    """this module's own (oracle UNet, product UNet, config) per dtype: the pairs other test modules cache get other processors
    installed by their IPAdapterXL tests; every test here leaves the pair as it found it (oracle_regions / product_regions)"""
    assert in_channels == 4
    return fresh_pair(dtype, num_tokens=T_TOKENS)


def _masks(Hl, Wl, flip=False):
    """two soft masks at the call's height x width: image 0 fades out from the left edge, image 1 from the right edge, and the middle
    belongs to neither (the regions touch one transformer of the tiny UNet: with these masks and weights they move the oracle's
    prediction by 0.16 - 0.17 against the unmasked sum, above 5 x the bf16 bound)"""
    ramp = torch.linspace(1.0, 0.0, 8 * Wl)[None, :].expand(8 * Hl, 8 * Wl)
    m = torch.stack([ramp.pow(4), (1.0 - ramp).pow(4)]).contiguous()
    return m.flip(0).contiguous() if flip else m


def _regions(Hl, Wl, flip=False):
    from imagharmony_amd.regions import IPRegions
    return IPRegions(_masks(Hl, Wl, flip), WEIGHTS)


@contextlib.contextmanager
def oracle_regions(ou, masks, weights, grid=None):
    """the oracle UNet with the restated processor in place of its IPAttnProcessor2_0, and back (the pair is shared between tests)"""
    orig = dict(ou.attn_processors)
    try:
        rr.install(ou, masks, weights, grid)
        yield ou
    finally:
        ou.set_attn_processor(orig)


@contextlib.contextmanager
def product_regions(hu, regions):
    from imagharmony_amd.ip_adapter import set_ip_regions
    try:
        set_ip_regions(hu, regions)
        yield hu
    finally:
        set_ip_regions(hu, None)


def _inputs(ocfg, Hl, Wl, B=2):
    cd = ocfg.cross_attention_dim
    return (det_randn((B, 4, Hl, Wl), 3), det_randn((B, 77 + N * T_TOKENS, cd), 4), det_randn((B, ocfg.pooled_dim), 6),
            torch.tensor([[Hl * 8, Wl * 8, 0, 0, Hl * 8, Wl * 8]], dtype=torch.float32).repeat(B, 1))


def _record(hu, dtype, x, ehs, te, ids, t=500.0):
    """one recorded forward over B latents -> (the output view, the recording context)"""
    from imagharmony_amd.ctx import Ctx
    B, _, Hl, Wl = x.shape
    pre = Ctx(DEV, dtype)
    st = hu.prepare_conditioning(pre, ehs.to(DEV, dtype), te.to(DEV, dtype), ids.to(DEV))
    st.t_value = torch.full((B,), float(t), device=DEV)
    st.latents = x.to(DEV).float().contiguous()
    rec = Ctx(DEV, dtype, record=True)
    rec._pre = pre
    return hu.emit_forward(rec, st, B, Hl, Wl, cfg_dup=False).view(B, Hl, Wl, 4).permute(0, 3, 1, 2), rec


# ---------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Hl,Wl", [(32, 32), (40, 24)])
def test_forward_matches_the_oracle_with_the_restated_processor(Hl, Wl, dtype):
    """N = 2.  32 x 32 latents: the active layers have 64 tokens and take the folded-LayerNorm path; 40 x 24: 60 tokens on a 10 x 6 grid,
    the unfused path.  Bound: the one tests/test_gpu_t2i_adapter.py applies to these stacks.  Eager, plan and replayed graph: the same bits."""
    ou, hu, ocfg = build_pair(dtype, 4)
    x, ehs, te, ids = _inputs(ocfg, Hl, Wl)
    reg = _regions(Hl, Wl)
    grid = {(Hl // 4) * (Wl // 4): (Hl // 4, Wl // 4)}
    added = {"text_embeds": te, "time_ids": ids}
    with torch.no_grad():
        with oracle_regions(ou, reg.masks, WEIGHTS, grid):
            ref = ou(x, torch.tensor(500.0), ehs, added_cond_kwargs=added)[0]
        with oracle_regions(ou, torch.ones_like(reg.masks), WEIGHTS, grid):
            unmasked = ou(x, torch.tensor(500.0), ehs, added_cond_kwargs=added)[0]
    vis = rel_rms(ref, unmasked)
    assert vis >= 5 * TOL[dtype], f"the regions move the reference by {vis:.3e} only"
    with product_regions(hu, reg):
        y = hu(x.to(DEV), torch.tensor(500.0), ehs.to(DEV, dtype), added_cond_kwargs={"text_embeds": te.to(DEV, dtype), "time_ids": ids.to(DEV)})[0]
        out, rec = _record(hu, dtype, x, ehs, te, ids)
        rec.run()
        torch.cuda.synchronize()
        y_plan = out.clone()
        out.zero_()
        rec.capture()
        rec.replay()
        torch.cuda.synchronize()
        y_graph = out.clone()
    r = rel_rms(y.float().cpu(), ref)
    print(f"forward {Hl}x{Wl} {dtype}: rel-rms {r:.3e} (bound {TOL[dtype]:.0e}); the regions move the reference by {vis:.3e}")
    assert torch.isfinite(y).all() and r < TOL[dtype], r
    assert torch.equal(y_plan.float(), y.float()) and torch.equal(y_graph.float(), y.float())


def test_launch_lists_with_and_without_regions():
    """without regions a forward records no kind 17 and nothing else than it always did; with them one launch kind replaces another in
    the layers with an image-prompt branch -- the same count, the same order"""
    from imagharmony_amd import lib as L
    dtype = torch.bfloat16
    ou, hu, ocfg = build_pair(dtype, 4)
    x, ehs, te, ids = _inputs(ocfg, 32, 32)
    active = sum(1 for p in hu.attn_processors.values() if hasattr(p, "to_k_ip") and not p.skip)
    _, plain = _record(hu, dtype, x, ehs[:, :77 + T_TOKENS], te, ids)
    with product_regions(hu, _regions(32, 32)):
        _, reg = _record(hu, dtype, x, ehs, te, ids)
    _, again = _record(hu, dtype, x, ehs[:, :77 + T_TOKENS], te, ids)
    kinds = lambda c: [t[1] for t in c.tags]
    assert L.OP_XATTN_REGIONS not in kinds(plain) and active >= 1
    assert [(t[1], t[2]) for t in again.tags] == [(t[1], t[2]) for t in plain.tags]
    assert kinds(reg).count(L.OP_XATTN_REGIONS) == active
    assert [L.OP_XATTN if k == L.OP_XATTN_REGIONS else k for k in kinds(reg)] == kinds(plain)
    assert [t[2] for t in reg.tags if t[1] == L.OP_XATTN_REGIONS] == ["cross.fused+regions"] * active


# ---------------------------------------------------------------------------------------------------- the loop
def _loop_inputs(ocfg):
    cd = ocfg.cross_attention_dim
    return (det_randn((1, 4, 32, 32), 3), det_randn((1, 77 + N * T_TOKENS, cd), 4), det_randn((1, 77 + N * T_TOKENS, cd), 5),
            det_randn((1, ocfg.pooled_dim), 6), det_randn((1, ocfg.pooled_dim), 7))


@pytest.mark.parametrize("dtype", DTYPES)
def test_text_to_image_loop_matches_the_restated_loop_and_the_plan_cache(dtype):
    from imagharmony_amd import lib as L
    from imagharmony_amd import schedulers as hs
    from imagharmony_amd.denoise import DenoiseEngine
    ou, hu, ocfg = build_pair(dtype, 4)
    lat, pe, ne, po, no = _loop_inputs(ocfg)
    reg = _regions(32, 32)
    with torch.no_grad(), oracle_regions(ou, reg.masks, WEIGHTS):
        ref = oracle_denoise(ou, OracleDDIM(), lat, pe, ne, po, no, 256, 256, num_inference_steps=STEPS, guidance_scale=5.0)
    eng = DenoiseEngine(hu, DEV, dtype)
    sch = hs.DDIMScheduler()
    try:
        eng.set_ip_regions(reg)
        eng.set_conditioning(pe, ne, po, no, 256, 256, guidance_scale=5.0)
        eng.set_schedule(sch, STEPS)
        out = eng.denoise(lat).float().cpu()
        r = rel_rms(out, ref)
        print(f"{dtype}: {STEPS}-step DDIM loop with {N} regions: rel-rms {r:.3e} (bound {LOOP_TOL[dtype]:.0e})")
        assert torch.isfinite(out).all() and r < LOOP_TOL[dtype], r
        plan, key = eng.plan, eng._sched_key
        kinds = [plan.lib.imh_plan_get_kind(plan.plan, i) for i in range(plan.lib.imh_plan_size(plan.plan))]
        assert key.regions == reg.digest() and plan.captured and L.OP_XATTN_REGIONS in kinds and L.OP_XATTN in kinds
        # a second set_schedule with the same regions re-records nothing
        eng.set_schedule(sch, STEPS)
        assert eng.plan is plan and eng._sched_key == key
        assert torch.equal(eng.denoise(lat).float().cpu(), out)
        # other masks: another key, another plan, another picture; the first plan is still in the cache
        eng.set_ip_regions(_regions(32, 32, flip=True))
        eng.set_schedule(sch, STEPS)
        assert eng._sched_key != key and eng._sched_key.regions != key.regions and eng.plan is not plan
        other = eng.denoise(lat).float().cpu()
        assert eng.plan is not plan and rel_rms(other, out) > LOOP_TOL[dtype]
        n_reg = plan.lib.imh_plan_size(plan.plan)
        eng.set_ip_regions(reg)
        eng.set_schedule(sch, STEPS)
        assert eng.plan is plan
    finally:
        eng.set_ip_regions(None)
    # without regions: the step of an engine that never heard of them, launch for launch, and as many launches as with them
    eng.set_conditioning(pe[:, :77 + T_TOKENS], ne[:, :77 + T_TOKENS], po, no, 256, 256, guidance_scale=5.0)
    eng.set_schedule(sch, STEPS)
    plain = eng.denoise(lat).clone()
    fresh = DenoiseEngine(hu, DEV, dtype)
    fresh.set_conditioning(pe[:, :77 + T_TOKENS], ne[:, :77 + T_TOKENS], po, no, 256, 256, guidance_scale=5.0)
    fresh.set_schedule(hs.DDIMScheduler(), STEPS)
    assert torch.equal(fresh.denoise(lat), plain)
    launches = lambda p: [(t[1], t[2]) for t in p.tags]
    assert launches(fresh.plan) == launches(eng.plan) and L.OP_XATTN_REGIONS not in [k for k, _ in launches(eng.plan)]
    assert eng._sched_key.regions is None and eng.plan.lib.imh_plan_size(eng.plan.plan) == n_reg
    assert all((p.num_images, p.regions) == (1, None) for p in hu.attn_processors.values() if hasattr(p, "num_images"))


@pytest.mark.parametrize("dtype", DTYPES)
def test_inpainting_loop_through_the_pipeline_matches_the_restated_loop(dtype):
    """the 4-channel inpainting pipe with ip_region_masks=: the blend rides in the step as without regions; afterwards the pipe is as it
    was (a plain call equals the same call made before)"""
    ou, hu, ocfg = build_pair(dtype, 4)
    ov, hv = build_vae_pair()
    cd = ocfg.cross_attention_dim
    img, mask = IMG(), centred_mask(256, 256)
    emb = dict(prompt_embeds=det_randn((1, 77 + N * T_TOKENS, cd), 4), negative_prompt_embeds=det_randn((1, 77 + N * T_TOKENS, cd), 5),
               pooled_prompt_embeds=det_randn((1, ocfg.pooled_dim), 6), negative_pooled_prompt_embeds=det_randn((1, ocfg.pooled_dim), 7))
    plain_emb = dict(emb, prompt_embeds=emb["prompt_embeds"][:, :77 + T_TOKENS], negative_prompt_embeds=emb["negative_prompt_embeds"][:, :77 + T_TOKENS])
    pipe = _pipe(hu, hv, "ddim", dtype)
    call = dict(image=img, mask_image=mask, strength=1.0, num_inference_steps=STEPS, guidance_scale=5.0, output_type="latent")      # all four steps run
    before = pipe(generator=_gens(11, 1, False), **call, **plain_emb).images.clone()
    ref_plain, _, _ = _oracle_inpaint(ou, ov, "ddim", img, mask, 1.0, STEPS, 1, _gens(11, 1, False), plain_emb)
    print(f"{dtype}: the same loop without regions: rel-rms {rel_rms(before.float().cpu(), ref_plain):.3e}")
    masks = _masks(32, 32)
    out = pipe(generator=_gens(11, 1, False), ip_region_masks=masks, ip_region_weights=WEIGHTS, binarize=False, **call, **emb).images.float().cpu()
    with oracle_regions(ou, masks, WEIGHTS):
        ref, _, _ = _oracle_inpaint(ou, ov, "ddim", img, mask, 1.0, STEPS, 1, _gens(11, 1, False), emb)
    r = rel_rms(out, ref)
    print(f"{dtype}: {STEPS}-step DDIM inpainting (blend) with {N} regions: rel-rms {r:.3e} (bound {LOOP_TOL[dtype]:.0e})")
    assert torch.isfinite(out).all() and r < LOOP_TOL[dtype], r
    assert pipe.engine.regions is None and all((p.num_images, p.regions) == (1, None) for p in hu.attn_processors.values() if hasattr(p, "num_images"))
    assert torch.equal(pipe(generator=_gens(11, 1, False), **call, **plain_emb).images, before)


# ---------------------------------------------------------------------------------------------------- the public surface
def test_generate_regions_equals_the_pipe_called_directly_and_restores_the_state():
    import numpy as np
    from PIL import Image
    from imagharmony_amd import schedulers as hs
    from imagharmony_amd.ip_adapter import IPAdapterXL
    from imagharmony_amd.modules import HarmonyAttention
    from imagharmony_amd.pipeline import StableDiffusionXLCustomPipeline
    # (IPAdapterXL installs its own processors: a fresh pair, not this module's shared one)
    dtype = torch.float16
    ou, hu, ocfg = fresh_pair(dtype, num_tokens=T_TOKENS)
    cd = ocfg.cross_attention_dim
    pipe = StableDiffusionXLCustomPipeline(hu, scheduler=hs.DDIMScheduler(), device=DEV, dtype=dtype)
    ha = det_fill(HarmonyAttention(image_hidden_size=128, text_context_dim=cd, inter_dim=512, cross_heads=8, reshape_blocks=8, cross_value_dim=64), 3)
    ip = IPAdapterXL(pipe, None, None, DEV, num_tokens=T_TOKENS, inference=True, number_class_crossattention=ha, dtype=dtype, clip_embeddings_dim=128)
    det_fill(ip.image_proj_model, 5)
    for n, p in hu.attn_processors.items():
        det_fill(p, 9, prefix=n)
    embeds = (det_randn((1, 77, cd), 1), det_randn((1, 77, cd), 2), det_randn((1, ocfg.pooled_dim), 3), det_randn((1, ocfg.pooled_dim), 4))
    a = np.zeros((64, 64), dtype=np.uint8)
    a[:, :28] = 255
    left, right = Image.fromarray(a), Image.fromarray(255 - a)              # PIL masks at another size: resized (Lanczos) to the call's, binarised
    clips, extras = [det_randn((1, 128), 5), det_randn((1, 128), 6)], [det_randn((1, 77, cd), 7), None]
    regions = [dict(clip_image_embeds=clips[0], mask=left, weight=1.0, extra_prompt_embeds=extras[0]), dict(clip_image_embeds=clips[1], mask=right, weight=0.6)]
    common = dict(num_inference_steps=3, guidance_scale=5.0, output_type="latent")
    plain_kw = dict(clip_image_embeds=clips[0], extra_prompt_embeds=extras[0], prompt_embeds=embeds, num_samples=1, seed=42, **common)
    before = ip.generate(**plain_kw).clone()
    out = ip.generate_regions(regions, prompt_embeds=embeds, scale=0.9, num_samples=1, seed=42, **common)
    assert out.shape == (1, 4, 32, 32) and torch.isfinite(out).all()
    # ... is the pipe called directly with the concatenated embeds and ip_region_masks=
    toks = [ip.get_image_embeds(clip_image_embeds=c, extra_prompt_embeds=e) for c, e in zip(clips, extras)]
    pe = torch.cat([embeds[0].to(DEV, dtype)] + [t[0] for t in toks], 1)
    ne = torch.cat([embeds[1].to(DEV, dtype)] + [t[1] for t in toks], 1)
    assert pe.shape[1] == 77 + 2 * T_TOKENS
    direct = lambda **kw: pipe(prompt_embeds=pe, negative_prompt_embeds=ne, pooled_prompt_embeds=embeds[2], negative_pooled_prompt_embeds=embeds[3],
                               generator=torch.Generator("cpu").manual_seed(42), **common, **kw).images
    assert torch.equal(direct(ip_region_masks=[left, right], ip_region_weights=[1.0, 0.6]), out)
    assert not torch.equal(direct(ip_region_masks=[right, left], ip_region_weights=[1.0, 0.6]), out)
    assert not torch.equal(direct(ip_region_masks=[left, right], ip_region_weights=[1.0, 0.1]), out)
    # a following plain generate is the same call made before it, bit for bit
    assert torch.equal(ip.generate(**plain_kw), before)
    assert all((p.num_images, p.regions) == (1, None) for p in hu.attn_processors.values() if hasattr(p, "num_images"))
    with pytest.raises(ValueError, match="list of dicts"):
        ip.generate_regions([dict(clip_image_embeds=clips[0])], prompt_embeds=embeds, **common)
