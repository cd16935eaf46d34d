"""CPU: regional image prompts (imagharmony_amd.regions, include/imh_regions.h) -- the fp32 restatement against the reference's goldens
and against itself in 16 bits on the inputs the GPU cases use, the grid rule and the mask preparation, the surface (ABI 13, plan kind 17,
state-dict keys, PlanKey) and every refusal, raised before any GPU work."""
import ctypes as C
import os
import re

import pytest
import torch

import ip_regions_cases as rc
import ip_regions_reference as rr
from conftest import GOLDEN, cmp_cfg_golden, rel_rms
from oracle.detfill import det_fill
from oracle.gen_golden import ATTN_CASES, ATTN_CFG_CASES, attn_inputs, make_attn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_TOL = 2e-6          # tests/test_oracle_modules.py: fp32 vs fp32, same math, different op order
GRIDS = [(24, 40, 60), (768, 1280, 60), (896, 1152, 1008), (1216, 832, 988), (1024, 1024, 1024)]      # (Hm, Wm, L)


# ---------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("case", list(ATTN_CASES) + list(ATTN_CFG_CASES))
def test_restatement_with_one_all_ones_mask_is_the_reference_processor(case):
    """N = 1, mask of ones: ip_skip0 of every tests/golden/attn_c*.pt, at the bound tests/test_oracle_modules.py holds the oracle to
    (2e-6 on the small cases; the sampled rows and sums of the benchmark shapes at 6e-4, fp16 storage)"""
    g = torch.load(os.path.join(GOLDEN, f"attn_{case}.pt"))
    b, l, c, h, cd, nt, t, scale = {**ATTN_CASES, **ATTN_CFG_CASES}[case]
    hs, ehs = attn_inputs(case)
    attn = make_attn(case, cross=True)
    with torch.no_grad():
        p = det_fill(rr.RegionsProcessor(c, cd, scale=scale, num_tokens=t, masks=torch.ones(1, 1, l), grid={l: (1, l)}), 17, prefix="proc.")
        y = p(attn, hs, encoder_hidden_states=ehs)
    if case in ATTN_CASES:
        assert rel_rms(y, g["ip_skip0"]) < ORACLE_TOL
    else:
        cmp_cfg_golden(y, g, case, "ip_skip0", 6e-4)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("name", list(rc.PARITY))
def test_restatement_in_16_bits_stays_within_half_the_bound_of_its_fp32_self(name, dtype):
    """the GPU parity bound leaves room for the kernel only if the restatement itself, run in the kernel's number format on the GPU
    cases' inputs, uses at most half of it"""
    inp, rows, weights = rc.parity_case(name)
    with torch.no_grad():
        ref = rc.reference(inp, rows, weights)
        low = rc.reference(inp, rows, weights, dtype=dtype)
    r = rel_rms(low.float(), ref)
    print(f"{name} {dtype}: the restatement in 16 bits is {r:.3e} from its fp32 self (half the bound: {rc.TOL[dtype] / 2:.1e})")
    assert r < rc.TOL[dtype] / 2


@pytest.mark.parametrize("name", list(rc.PARITY))
def test_parity_cases_masks_are_visible(name):
    """every parity case's masks move the reference by at least 5 x the widest bound against the unmasked sum"""
    inp, rows, weights = rc.parity_case(name)
    with torch.no_grad():
        vis = rel_rms(rc.reference(inp, rows, weights), rc.reference(inp, torch.ones_like(rows), weights))
    assert vis >= 5 * max(rc.TOL.values()), vis


# ---------------------------------------------------------------------------------------------------- grid rule, mask preparation
def test_token_grid_is_diffusers_float_rule_on_the_listed_sizes():
    from imagharmony_amd.regions import token_grid
    want = [(6, 10), (6, 10), (28, 36), (38, 26), (32, 32)]
    for (Hm, Wm, L), hw in zip(GRIDS, want):
        assert token_grid(L, Hm, Wm) == hw == rr.diffusers_grid(L, Hm, Wm)
        assert hw[0] * hw[1] == L and hw[0] * Wm == hw[1] * Hm
    with pytest.raises(ValueError, match="no grid"):
        token_grid(15, 8, 8)
    for bad in ((0, 8, 8), (16, 0, 8), (2, 64, 1)):
        with pytest.raises(ValueError):
            token_grid(*bad)


def test_mask_preparation_restates_the_mask_processor_defaults():
    import numpy as np
    from PIL import Image
    from imagharmony_amd.regions import IPRegions, prepare_masks
    a = np.zeros((32, 48, 3), dtype=np.uint8)
    a[:, :24] = (255, 255, 255)
    a[:, 24:30] = (100, 100, 100)              # below 0.5 after the grayscale conversion: off
    pil = Image.fromarray(a)
    m = prepare_masks([pil, pil.transpose(Image.FLIP_LEFT_RIGHT)], 64, 96)
    assert m.shape == (2, 64, 96) and m.dtype == torch.float32 and set(m.unique().tolist()) == {0.0, 1.0}
    assert m[0, :, :44].all() and not m[0, :, 52:].any() and torch.equal(m[1], m[0].flip(-1))
    # the same through PIL by hand: grayscale, Lanczos to height x width, / 255, >= 0.5
    by_hand = torch.from_numpy(np.asarray(pil.convert("L").resize((96, 64), resample=Image.LANCZOS), dtype=np.float32) / 255.0)
    assert torch.equal(m[0], (by_hand >= 0.5).float())
    soft = prepare_masks(pil, 64, 96, binarize=False)
    assert torch.equal(soft[0], by_hand) and 0.0 < float(soft[0, 0, 54]) < 0.5
    # tensors: already at the call's size, [H, W] or [N, H, W]
    t = torch.rand(2, 64, 96)
    assert torch.equal(prepare_masks(t, 64, 96, binarize=False), t) and prepare_masks(t[0], 64, 96).shape == (1, 64, 96)
    with pytest.raises(ValueError, match="already be"):
        prepare_masks(t, 32, 96)
    with pytest.raises(ValueError, match="1 .. 8"):
        prepare_masks(torch.rand(9, 8, 8), 8, 8)
    with pytest.raises(ValueError, match="PIL image or a tensor"):
        prepare_masks(["mask.png"], 8, 8)
    r = IPRegions.from_masks(t, 64, 96, weights=(1.0, 0.5), binarize=False)
    assert r.n == 2 and r.size == (64, 96) and r.weights == (1.0, 0.5)
    with pytest.raises(ValueError, match="weights"):
        IPRegions(t, weights=(1.0,))
    # the rows of a grid: diffusers' bicubic resize, not clamped; cached per grid and device
    rows, w = r.rows("cpu", grid=(8, 12))
    assert torch.equal(rows, rr.downsample(t, 8, 12)) and w.tolist() == [1.0, 0.5] and rows.dtype == torch.float32
    assert r.rows("cpu", tokens=96)[0] is rows
    hard = IPRegions(rc.block_masks(2))
    assert float(hard.downsample(6, 10).min()) < 0.0 or float(hard.downsample(6, 10).max()) > 1.0      # bicubic overshoot is kept
    with pytest.raises(ValueError, match="no grid"):
        r.rows("cpu", tokens=100)
    # the digest: N, weights and mask bytes
    assert r.digest() == IPRegions(t.clone(), (1.0, 0.5)).digest() != IPRegions(t, (1.0, 0.25)).digest()
    assert r.digest() != IPRegions(t.flip(0), (1.0, 0.5)).digest()


# ---------------------------------------------------------------------------------------------------- surface
def test_abi_plan_kind_and_struct_mirror():
    from imagharmony_amd import lib as L
    hdr = open(os.path.join(ROOT, "include", "imh.h")).read()
    rhdr = open(os.path.join(ROOT, "include", "imh_regions.h")).read()
    l = L.load()
    assert int(re.search(r"#define IMH_ABI_VERSION (\d+)", hdr).group(1)) == 13 == L.ABI_VERSION == l.imh_abi_version()
    assert "regions" not in hdr.lower() and '#include "imh.h"' in rhdr
    assert int(re.search(r"#define IMH_OP_XATTN_REGIONS (\d+)\b", rhdr).group(1)) == 17 == L.OP_XATTN_REGIONS
    assert int(re.search(r"#define IMH_REGIONS_MAX_IMAGES (\d+)\b", rhdr).group(1)) == 8 == L.REGIONS_MAX_IMAGES
    code = re.sub(r"/\*.*?\*/", "", rhdr, flags=re.S)
    assert set(re.findall(r"\b(imh_[a-z0-9_]+)\s*\(", code)) == {"imh_cross_attention_regions"} == {n for n, _, _ in L.REGIONS_SYMBOLS}
    # the ctypes mirror: the header's fields in the header's order, imh_xattn_args' first
    body = rhdr[rhdr.index("typedef struct imh_xattn_regions_args {"):rhdr.index("} imh_xattn_regions_args;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split("{", 1)[1].split(";") for n in re.findall(r"\*?\s*(\w+)\s*(?:,|$)", decl.strip().split(" ", 1)[-1] if decl.strip() else "")]
    assert names == [f[0] for f in L.XAttnRegionsArgs._fields_]
    assert [f[0] for f in L.XAttnRegionsArgs._fields_][:len(L.XAttnArgs._fields_)] == [f[0] for f in L.XAttnArgs._fields_]
    # kind 17 is a plan kind; 12, 14 and 16 stay refused
    a = L.XAttnRegionsArgs()
    p = l.imh_plan_create()
    for kind in (12, 14, 16):
        assert l.imh_plan_add(p, kind, C.byref(a), 0, 0) < 0
    assert l.imh_plan_add(p, L.OP_XATTN_REGIONS, C.byref(a), 0, 9) == 0 and l.imh_plan_get_kind(p, 0) == 17 and l.imh_plan_get_tag(p, 0) == 9
    a.n_img = 3
    assert l.imh_plan_update(p, 0, C.byref(a)) == 0
    l.imh_plan_destroy(p)


def test_processor_surface_state_dict_and_plan_key():
    from imagharmony_amd.attention_processor import CNAttnProcessor2_0, IPAttnProcessor2_0
    from imagharmony_amd.denoise import PlanKey
    p = IPAttnProcessor2_0(128, 64, num_tokens=4)
    assert list(p.state_dict().keys()) == ["to_k_ip.weight", "to_v_ip.weight"] and not list(p.buffers())
    assert (p.num_images, p.regions) == (1, None) == (CNAttnProcessor2_0().num_images, CNAttnProcessor2_0().regions)
    with pytest.raises(TypeError):
        p(None, None, regions=1)
    base = ("DDIMScheduler", 1000, 4, 0.0, 1.0, None, 1.0, 4, "t", None, None, None, False)
    assert PlanKey(*base) == PlanKey(*base, regions=None) == PlanKey(*base, None) == base and PlanKey(*base).regions is None
    assert hash(PlanKey(*base)) == hash(PlanKey(*base, None)) and len(PlanKey(*base)) == 13          # ... and it is the tuple it always was
    assert PlanKey(*base[:9], controlnet=None, inpaint=None, adapter=None, seeded=False, regions="d") == PlanKey(*base, "d")      # as set_schedule builds it
    assert PlanKey(*base[:9], controlnet=None, inpaint=None, adapter=None, seeded=False, regions=None) == base
    k = PlanKey(*base, regions="d")
    assert k != PlanKey(*base) and k.regions == "d" == k[-1] and k[:-1] == base and k.seeded is False and k == PlanKey(*base, "d")


def test_set_ip_regions_on_a_unet_and_back():
    from imagharmony_amd.attention_processor import AttnProcessor2_0, CNAttnProcessor2_0, IPAttnProcessor2_0
    from imagharmony_amd.ip_adapter import set_ip_regions
    from imagharmony_amd.regions import IPRegions

    class _U:
        attn_processors = {"a": AttnProcessor2_0(), "b": IPAttnProcessor2_0(128, 64), "c": IPAttnProcessor2_0(128, 64, skip=True), "d": CNAttnProcessor2_0()}
    r = IPRegions(torch.ones(3, 8, 8))
    set_ip_regions(_U, r)
    assert all((p.num_images, p.regions) == (3, r) for k, p in _U.attn_processors.items() if k != "a") and not hasattr(_U.attn_processors["a"], "regions")
    set_ip_regions(_U, None)
    assert all((p.num_images, p.regions) == (1, None) for k, p in _U.attn_processors.items() if k != "a")
    with pytest.raises(TypeError):
        set_ip_regions(_U, torch.ones(1, 8, 8))


# ---------------------------------------------------------------------------------------------------- refusals, before any GPU work
def test_engine_and_pipeline_refusals_come_before_a_ctx_exists(monkeypatch):
    from imagharmony_amd import denoise, pipeline as P
    from imagharmony_amd.denoise import DenoiseEngine
    from imagharmony_amd.regions import IPRegions
    from imagharmony_amd.schedulers import DDIMScheduler
    from imagharmony_amd.unet import UNetConfig

    def no_ctx(*a, **k):
        raise AssertionError("a Ctx was built before the refusal")
    monkeypatch.setattr(denoise, "Ctx", no_ctx)

    class _U:
        config = UNetConfig()
        attn_processors = {}
    r = IPRegions(torch.ones(2, 8, 8))
    emb = (torch.zeros(1, 85, 8), torch.zeros(1, 85, 8), torch.zeros(1, 8), torch.zeros(1, 8))
    # regions first, then the other side
    e = DenoiseEngine(_U(), "cpu")
    e.set_ip_regions(r)
    with pytest.raises(NotImplementedError, match="cfg_role"):
        e.set_conditioning(*emb, 64, 64, cfg_role=1)
    e.controlnet = object()
    with pytest.raises(NotImplementedError, match="ControlNet"):
        e.set_conditioning(*emb, 64, 64)
    with pytest.raises(NotImplementedError, match="ControlNet"):
        e.set_schedule(DDIMScheduler(), 4)
    e.controlnet, e.adapter = None, object()
    with pytest.raises(NotImplementedError, match="T2I-Adapter"):
        e.set_conditioning(*emb, 64, 64)
    with pytest.raises(NotImplementedError, match="T2I-Adapter"):
        e.set_schedule(DDIMScheduler(), 4)
    # the other side first, then regions
    for attr, what in (("controlnet", "ControlNet"), ("adapter", "T2I-Adapter"), ("cfg_role", "cfg_role")):
        e = DenoiseEngine(_U(), "cpu")
        setattr(e, attr, 1 if attr == "cfg_role" else object())
        with pytest.raises(NotImplementedError, match=what):
            e.set_ip_regions(r)
        assert e.regions is None
    e = DenoiseEngine(_U(), "cpu")
    with pytest.raises(TypeError):
        e.set_ip_regions(torch.ones(2, 8, 8))
    # regions set after the conditioning: the K / V caches hold another number of image prompts
    class _KV:
        k2 = torch.zeros(2, 64, 128)           # one image prompt per sample of a CFG pair

    class _St:
        kv = {"down_blocks.2.attentions.1.transformer_blocks.0.attn2.processor": _KV}
    e.st, e._cond_in = _St(), (torch.zeros(2, 81, 8), None, None)
    e.set_ip_regions(r)
    with pytest.raises(Exception, match="before set_conditioning"):
        e.set_schedule(DDIMScheduler(), 4)

    # the ControlNet and adapter pipes refuse the keyword; the plain pipes refuse weights without masks
    kw = dict(prompt_embeds=torch.zeros(1, 85, 8), pooled_prompt_embeds=torch.zeros(1, 8), output_type="latent")
    for cls, extra in ((P.StableDiffusionXLControlNetCustomPipeline, dict(image=torch.rand(1, 3, 64, 64))),
                       (P.StableDiffusionXLAdapterCustomPipeline, dict(image=torch.rand(1, 3, 64, 64)))):
        pipe = cls.__new__(cls)
        pipe.vae = pipe.vae_decode = None
        pipe.scheduler, pipe.unet = DDIMScheduler(), _U()
        pipe.controlnet = pipe.adapter = object()
        with pytest.raises(NotImplementedError, match="regional image prompts"):
            pipe(ip_region_masks=torch.ones(2, 64, 64), **kw, **extra)
    pipe = P.StableDiffusionXLCustomPipeline.__new__(P.StableDiffusionXLCustomPipeline)
    pipe.vae = pipe.vae_decode = None
    pipe.scheduler, pipe.unet, pipe.default_sample_size = DDIMScheduler(), _U(), 8
    with pytest.raises(ValueError, match="ip_region_masks"):
        pipe(ip_region_weights=[1.0], **kw)
    with pytest.raises(ValueError, match="already be"):
        pipe(ip_region_masks=torch.ones(2, 32, 32), **kw)               # 64 x 64 is the call's size
    with pytest.raises(ValueError, match="weights"):
        pipe(ip_region_masks=torch.ones(2, 64, 64), ip_region_weights=[1.0], **kw)


def _good_args():
    """a filled argument struct that passes every rule (pointers are never followed: nothing is launched on the CPU)"""
    from imagharmony_amd import lib as L
    a = L.XAttnRegionsArgs()
    for f in ("X", "Wq", "K", "Vt", "K2", "Vt2", "O", "mask"):
        setattr(a, f, 0x1000)
    a.B, a.H, a.Lq, a.C, a.Lk, a.Lk_pad, a.Lk2, a.Lk2_pad = 2, 2, 60, 128, 77, 128, 4, 64
    a.ldx = a.ldw = a.ldk = a.ldk2 = a.ldo = 128
    a.ldvt, a.ldvt2, a.n_img, a.ldm, a.dtype, a.scale = 256, 256, 2, 60, L.IMH_DT_BF16, 0.125
    return a


BAD = [("null mask", dict(mask=None), -1), ("null K2", dict(K2=None), -1), ("mask alignment", dict(mask=0x1002), -1),
       ("weights alignment", dict(weights=0x1001), -1), ("tab without step", dict(scale2_tab=0x1000), -1),
       ("step without tab", dict(step=0x1000), -1), ("ln_s without ln_c", dict(ln_s=0x1000), -1),
       ("n_img 0", dict(n_img=0), -2), ("n_img 9", dict(n_img=9), -2), ("ldm < Lq", dict(ldm=59), -2), ("Lk2 0", dict(Lk2=0), -2),
       ("Lk2_pad % 64", dict(Lk2_pad=96), -2), ("Lk2_pad < Lk2", dict(Lk2=65), -2), ("C != 64 H", dict(C=192), -2),
       ("Lk_pad % 64", dict(Lk_pad=100), -2), ("ld % 8", dict(ldk2=132), -2), ("empty", dict(Lq=0, ldm=0), -2), ("dtype", dict(dtype=5), -3)]


@pytest.mark.parametrize("what,change,status", BAD, ids=[b[0] for b in BAD])
def test_library_and_recorder_refuse_the_same_arguments_without_a_launch(what, change, status):
    """every refusal of include/imh_regions.h returns its status from the library (validation precedes the launch, so this runs without
    a GPU) and has a reason in Ctx.regions_refusal; the good arguments pass the recorder's rules"""
    from imagharmony_amd import lib as L
    from imagharmony_amd.ctx import Ctx
    assert Ctx.regions_refusal(_good_args()) is None
    a = _good_args()
    for k, v in change.items():
        setattr(a, k, v)
    assert Ctx.regions_refusal(a) is not None
    assert L.load().imh_cross_attention_regions(C.byref(a), None) == status
    assert L.load().imh_cross_attention_regions(None, None) == -1
