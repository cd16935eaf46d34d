"""GPU tests of the SDXL T2I-Adapter: the three passes of imh_adapter_op bit for bit against torch, the adapter's features against the
CPU fp32 reference (tests/t2i_adapter_reference.py), the UNet forward with the four injections and the denoise loop against the
reference's, the conditions that need no measured number (scale 0, the factor's gate rows, eager = plan = graph, the launch lists), and
the public pipeline / PNS surface."""
import ctypes as C
import functools
import json
import os

import pytest
import torch
import torch.nn.functional as F

from conftest import PARITY_JSON, rel_rms
from oracle.detfill import det_fill, det_randn
from oracle.sdxl_unet import tiny_config

import t2i_adapter_reference as tr
from test_gpu_controlnet import LOOP_TOL, _build_wide, _wide_oracle, wide_config
from test_gpu_unet import TOL, build_pair

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float16, torch.bfloat16]
T_TOKENS = 4
TINY = (64, 128, 256, 256)
XL = (320, 640, 1280, 1280)
PARITY = {}


def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def _control_image(n=1, hw=256, seed=9):
    """a smooth-ish image in [0, 1]; sample k of a batch is another image"""
    return det_randn((n, 3, hw, hw), seed).mul(0.25).add(0.5).clamp(0, 1)


# ---------------------------------------------------------------------------------------------------- the ops
UNSHUFFLE = [(1, 3, 32, 48, 16, None), (2, 3, 64, 32, 16, None), (1, 3, 16, 24, 8, None),
             (1, 3, 32, 48, 16, 832),          # Cp > Cin f^2: 64 padding zeros per pixel
             (1, 1, 16, 16, 2, 8)]             # Cin f^2 = 4 of Cp = 8; f % 8 != 0: the element-wise path


def _unshuffle_ref(img, f, Cp, dtype):
    ref = F.pixel_unshuffle(img, f).permute(0, 2, 3, 1).to(dtype)
    return F.pad(ref, (0, Cp - ref.shape[-1])) if Cp > ref.shape[-1] else ref.contiguous()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", UNSHUFFLE)
def test_unshuffle_bits_and_guarded_placement(dtype, case):
    from guarded import run_dense_and_guarded
    from imagharmony_amd.ctx import Ctx
    N, Cin, H, W, f, Cp = case
    img = det_randn((N, Cin, H, W), 31).to(DEV)
    y = Ctx(DEV, dtype).pixel_unshuffle(img, f, Cp=Cp)
    torch.cuda.synchronize()
    Cq = Cp or (Cin * f * f + 7) // 8 * 8
    assert y.shape == (N, H // f, W // f, Cq) and y.dtype == dtype and y.is_contiguous()
    ref = _unshuffle_ref(img, f, Cq, dtype)
    assert torch.equal(_bits(y), _bits(ref))
    assert not y[..., Cin * f * f:].any()
    # a sliced (4-byte, not 16-byte aligned) image takes the element-wise path: the same bits
    if f % 8 == 0:
        off = torch.empty(img.numel() + 1, dtype=torch.float32, device=DEV)[1:].view_as(img).copy_(img)
        assert off.data_ptr() % 16 and torch.equal(_bits(Ctx(DEV, dtype).pixel_unshuffle(off, f, Cp=Cp)), _bits(ref))
    dense, guarded, arena = run_dense_and_guarded(DEV, dtype, lambda ctx, put, out: ctx.pixel_unshuffle(put(img), f, Cp=Cp))
    arena.check()                                   # no byte outside y changed; y is finite
    assert torch.equal(_bits(dense[0]), _bits(ref)) and torch.equal(_bits(guarded[0]), _bits(ref))


AVGPOOL = [(1, 5, 7, 64), (1, 1, 1, 8), (2, 16, 16, 128), (1, 8, 9, 1280)]


def _avgpool_ref(x, dtype):
    """the expression of include/imh_adapter.h written with torch ops on the GPU: fp32 raster-order sum of the in-bounds pixels of every window,
    times the exact reciprocal of the count, one rounding"""
    N, H, W, Cc = x.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    xf = x.float()
    out = torch.empty(N, Ho, Wo, Cc, dtype=dtype, device=x.device)
    He, We = H // 2, W // 2                       # full windows
    a, b, c, d = xf[:, 0:2 * He:2, 0:2 * We:2], xf[:, 0:2 * He:2, 1:2 * We:2], xf[:, 1:2 * He:2, 0:2 * We:2], xf[:, 1:2 * He:2, 1:2 * We:2]
    out[:, :He, :We] = (((a + b) + c) + d).mul(0.25).to(dtype)
    if W % 2:                                     # the last column: the two pixels of a column pair
        out[:, :He, We] = (xf[:, 0:2 * He:2, W - 1] + xf[:, 1:2 * He:2, W - 1]).mul(0.5).to(dtype)
    if H % 2:                                     # the last row: the two pixels of a row pair
        out[:, He, :We] = (xf[:, H - 1, 0:2 * We:2] + xf[:, H - 1, 1:2 * We:2]).mul(0.5).to(dtype)
    if H % 2 and W % 2:
        out[:, He, We] = xf[:, H - 1, W - 1].mul(1.0).to(dtype)
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", AVGPOOL)
def test_avgpool2_bits_and_guarded_placement(dtype, shape):
    from guarded import run_dense_and_guarded
    from imagharmony_amd.ctx import Ctx
    x = det_randn(shape, 32).to(dtype).to(DEV)
    y = Ctx(DEV, dtype).avgpool2(x)
    torch.cuda.synchronize()
    N, H, W, Cc = shape
    assert y.shape == (N, (H + 1) // 2, (W + 1) // 2, Cc)
    ref = _avgpool_ref(x, dtype)
    assert torch.equal(_bits(y), _bits(ref))
    # ... which is AvgPool2d(2, 2, ceil_mode=True) itself up to the summation order
    mod = torch.nn.AvgPool2d(2, 2, ceil_mode=True)(x.float().permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    assert torch.allclose(y.float(), mod, rtol=2 ** -7, atol=1e-6)
    dense, guarded, arena = run_dense_and_guarded(DEV, dtype, lambda ctx, put, out: ctx.avgpool2(put(x)))
    arena.check()
    assert torch.equal(_bits(dense[0]), _bits(ref)) and torch.equal(_bits(guarded[0]), _bits(ref))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [8, 8 * 37, 2 * 16 * 16 * 320, 8 * 37 + 5])
def test_relu_values_in_and_out_of_place_and_guarded(dtype, n):
    from guarded import run_dense_and_guarded
    from imagharmony_amd.ctx import Ctx
    x = det_randn((n,), 33).to(dtype).to(DEV)
    x[::7] = 0.0
    ref = torch.clamp_min(x.float(), 0.0).to(dtype)
    ctx = Ctx(DEV, dtype)
    y = ctx.relu(x)
    torch.cuda.synchronize()
    assert y.data_ptr() != x.data_ptr() and torch.equal(y, ref) and not (y < 0).any()
    z = x.clone()
    assert ctx.relu(z, out=z) is z
    torch.cuda.synchronize()
    assert torch.equal(z, ref)

    def body(ctx, put, out):
        a, b = put(x), put(x)
        return ctx.relu(a), ctx.relu(b, out=b)
    dense, guarded, arena = run_dense_and_guarded(DEV, dtype, body)
    arena.check()
    for t in dense + guarded:
        assert torch.equal(t, ref)


def test_adapter_op_refusals_launch_nothing():
    from imagharmony_amd import lib as L
    from imagharmony_amd.ctx import Ctx
    ctx = Ctx(DEV, torch.bfloat16)
    img = torch.zeros(1, 3, 32, 48, device=DEV)
    x = torch.zeros(1, 4, 4, 64, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(L.ImhError):
        ctx.pixel_unshuffle(img, 5)                                   # H % f
    with pytest.raises(L.ImhError):
        ctx.pixel_unshuffle(img, 16, Cp=760)                          # Cp < Cin f^2
    with pytest.raises(L.ImhError):
        ctx.pixel_unshuffle(img.to(torch.bfloat16), 16)               # the image is fp32
    with pytest.raises(L.ImhError):
        ctx.avgpool2(x[..., :12].contiguous())                        # C % 8
    with pytest.raises(L.ImhError):
        ctx.relu(x, out=x.view(-1)[:64])
    with pytest.raises(L.ImhError, match="no plan kind"):
        Ctx(DEV, torch.bfloat16, record=True).relu(x)
    # the library's own: the status code, and the output keeps its bits
    y = torch.full((1, 2, 3, 768), 7.0, dtype=torch.bfloat16, device=DEV)
    a = L.AdapterArgs()
    a.x, a.y, a.mode, a.N, a.C, a.H, a.W, a.f, a.Cp, a.dtype = img.data_ptr(), y.data_ptr(), L.ADAPTER_UNSHUFFLE, 1, 3, 32, 48, 16, 768, 0
    for field, bad, rc in (("H", 33, -2), ("W", 40, -2), ("Cp", 764, -2), ("Cp", 760, -2), ("dtype", 5, -3), ("mode", 9, -1), ("y", y.data_ptr() + 2, -1)):
        b = L.AdapterArgs.from_buffer_copy(a)
        setattr(b, field, bad)
        assert ctx.lib.imh_adapter_op(C.byref(b), ctx.stream()) == rc, field
    a.mode, a.x, a.y, a.C, a.H, a.W = L.ADAPTER_AVGPOOL2, x.data_ptr(), x.data_ptr(), 64, 4, 4
    assert ctx.lib.imh_adapter_op(C.byref(a), ctx.stream()) == -1                      # in place
    a.mode, a.n, a.y = L.ADAPTER_RELU, 64, x.data_ptr() + 32
    assert ctx.lib.imh_adapter_op(C.byref(a), ctx.stream()) == -1                      # a partial overlap
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()) and not x.any()


# ---------------------------------------------------------------------------------------------------- the adapter's features
@functools.lru_cache(maxsize=None)
def _ref_adapter(channels):
    with torch.no_grad():
        return det_fill(tr.RefT2IAdapter(channels=channels), 13).eval()


@functools.lru_cache(maxsize=None)
def _ref_features(channels, N, hw):
    img = _control_image(N, hw)
    with torch.no_grad():
        return img, _ref_adapter(channels)(img)


@functools.lru_cache(maxsize=None)
def _ref_own_error(channels, N, hw, dtype):
    """the reference's own rounding error: RefT2IAdapter run on the CPU in the run dtype (same weights, same image) against its fp32.
    The net has no normalisation, so this depends on the weights' scale; it is the yardstick, not the code under test."""
    import copy
    img, ref = _ref_features(channels, N, hw)
    with torch.no_grad():
        low = copy.deepcopy(_ref_adapter(channels)).to(dtype)(img.to(dtype))
    return [rel_rms(l.float(), r) for l, r in zip(low, ref)]


@functools.lru_cache(maxsize=None)
def _product_adapter(channels, dtype):
    from imagharmony_amd import T2IAdapter
    m = T2IAdapter(channels=channels)
    m.load_state_dict(_ref_adapter(channels).state_dict(), strict=True)
    return m.to(DEV, dtype)


def _write_parity():
    try:
        out_dir = os.path.dirname(PARITY_JSON)          # beside the suite's measured-parity record; the kept copy is profiles/t2i_adapter_parity.json
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "t2i_adapter_parity.json"), "w") as f:
            json.dump(PARITY, f, indent=1, sort_keys=True)
    except OSError:
        pass


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,channels,hw,N", [("tiny", TINY, 256, 1), ("tiny", TINY, 256, 2), ("xl", XL, 128, 1)])
def test_features_match_reference(name, channels, hw, N, dtype):
    """each feature within 3x the rel-RMS the CPU reference itself shows in the run dtype against its own fp32 (a different summation
    order; the margin of profiles/clip_text_parity.json)"""
    from imagharmony_amd.ctx import Ctx
    img, ref = _ref_features(channels, N, hw)
    own = _ref_own_error(channels, N, hw, dtype)
    ad = _product_adapter(channels, dtype)
    n0 = ad.launches
    feats = ad.prepare_features(Ctx(DEV, dtype), img, hw // 8, hw // 8)
    torch.cuda.synchronize()
    assert ad.launches - n0 == 2 + 1 + 2 + 4 * 2 * 3                 # unshuffle, conv_in; avgpool; two in_convs; eight resnets of conv, relu, conv
    shapes = [(N, hw // 16, hw // 16, channels[0]), (N, hw // 16, hw // 16, channels[1]), (N, hw // 32, hw // 32, channels[2]), (N, hw // 32, hw // 32, channels[3])]
    got = []
    for k, (t, r) in enumerate(zip(feats, ref)):
        assert tuple(t.shape) == shapes[k] and t.dtype == dtype and t.is_contiguous() and torch.isfinite(t).all()
        got.append(rel_rms(t.permute(0, 3, 1, 2).float().cpu(), r))
    print(f"adapter features {name} N={N} {dtype}: HIP rel-rms {['%.3e' % v for v in got]}, reference's own in the run dtype {['%.3e' % v for v in own]}")
    PARITY[f"{name}_N{N}_{str(dtype).replace('torch.', '')}"] = dict(hip=got, reference_own=own, bound=[3 * v for v in own])
    _write_parity()
    for k in range(4):
        assert got[k] <= 3 * own[k], (k, got[k], own[k])
    # the diffusers signature: four NCHW tensors, the same values
    out = ad(img.to(DEV))
    assert [tuple(o.shape) for o in out] == [(s[0], s[3], s[1], s[2]) for s in shapes]
    assert all(torch.equal(o, t.permute(0, 3, 1, 2)) for o, t in zip(out, feats))


# ---------------------------------------------------------------------------------------------------- forward with injection
FORWARD_SCALE = 1.0


def _stack(width, dtype):
    """(oracle UNet, product UNet, config, reference adapter's channels) with the IP processors of build_pair / _build_wide"""
    ou, hu, ocfg = build_pair(dtype, num_tokens=T_TOKENS) if width == "tiny" else _build_wide(dtype)
    boc = tuple(ocfg.block_out_channels)
    return ou, hu, ocfg, boc + boc[-1:]


def _inputs(ocfg, S=1, hw=32):
    cd = ocfg.cross_attention_dim
    x = det_randn((S, 4, hw, hw), 3)
    ehs = det_randn((2 * S, 77 + T_TOKENS, cd), 4)
    te = det_randn((2 * S, ocfg.pooled_dim), 6)
    ids = torch.tensor([[hw * 8, hw * 8, 0, 0, hw * 8, hw * 8]], dtype=torch.float32).repeat(2 * S, 1)
    return x, ehs, te, ids


def _product_forward(hu, ad, dtype, x, t, ehs, te, ids, img, scale, how="eager"):
    """CFG batch 2 S on S latents.  ad None: the plain forward.  how: eager | plan | graph -> (NCHW fp32 on the CPU, the context)"""
    from imagharmony_amd.ctx import Ctx
    from imagharmony_amd.t2i_adapter import AdapterResiduals
    S, _, Hl, Wl = x.shape
    pre = Ctx(DEV, dtype)
    st = hu.prepare_conditioning(pre, ehs.to(DEV, dtype), te.to(DEV, dtype), ids.to(DEV))
    st.t_value = torch.full((2 * S,), float(t), device=DEV)
    st.latents = x.to(DEV).float().contiguous()
    ctx = Ctx(DEV, dtype, record=how != "eager")
    kw = {}
    if ad is not None:
        kw["adapter"] = AdapterResiduals(ad.prepare_features(pre, img, Hl, Wl), scale=scale)
    out = hu.emit_forward(ctx, st, S, Hl, Wl, cfg_dup=True, **kw)
    if how == "plan":
        ctx.run()
    elif how == "graph":
        ctx.capture()
        ctx.replay()
    torch.cuda.synchronize()
    return out.view(2 * S, Hl, Wl, 4).permute(0, 3, 1, 2).float().cpu(), ctx


@functools.lru_cache(maxsize=None)
def _ref_forward(width, S, scale, swap=False):
    """(reference prediction with the adapter's features, without them), CPU fp32"""
    ocfg = tiny_config() if width == "tiny" else wide_config()
    ou = build_pair(torch.bfloat16, num_tokens=T_TOKENS)[0] if width == "tiny" else _wide_oracle()[0]
    boc = tuple(ocfg.block_out_channels)
    x, ehs, te, ids = _inputs(ocfg, S)
    added = {"text_embeds": te, "time_ids": ids}
    x2 = torch.cat([x, x], 0)
    img = _control_image(S)
    if swap:
        img = img.flip(0)
    with torch.no_grad():
        feats = [f * scale for f in _ref_adapter(boc + boc[-1:])(img)]
        return (tr.unet_forward(ou, x2, torch.tensor(500.0), ehs, added, feats), tr.unet_forward(ou, x2, torch.tensor(500.0), ehs, added))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("width", ["tiny", "wide"])
def test_forward_with_adapter_matches_reference(width, dtype):
    ou, hu, ocfg, channels = _stack(width, dtype)
    ref_ad, ref_plain = _ref_forward(width, 1, FORWARD_SCALE)
    vis = rel_rms(ref_ad, ref_plain)
    assert vis >= 5 * TOL[dtype], f"the adapter moves the reference's prediction by {vis:.3e} only"
    ad = _product_adapter(channels, dtype)
    x, ehs, te, ids = _inputs(ocfg)
    img = _control_image()
    y_ad, _ = _product_forward(hu, ad, dtype, x, 500.0, ehs, te, ids, img, FORWARD_SCALE)
    y_plain, _ = _product_forward(hu, None, dtype, x, 500.0, ehs, te, ids, None, 1.0)
    r_ad, r_plain = rel_rms(y_ad, ref_ad), rel_rms(y_plain, ref_plain)
    print(f"forward {width} {dtype}: with adapter rel-rms {r_ad:.3e}, plain {r_plain:.3e} (bound {TOL[dtype]:.0e}); the adapter moves the reference by {vis:.3e}")
    PARITY[f"forward_{width}_{str(dtype).replace('torch.', '')}"] = dict(with_adapter=r_ad, plain=r_plain, bound=TOL[dtype], adapter_visibility=vis)
    _write_parity()
    assert torch.isfinite(y_ad).all() and r_ad < TOL[dtype], r_ad
    assert r_plain < TOL[dtype], r_plain


@pytest.mark.parametrize("dtype", DTYPES)
def test_forward_two_samples_two_images_cfg(dtype):
    """S = 2 with one control image per sample (Br = S) under CFG: UNet batch [u0, u1, c0, c1] reads features [0, 1, 0, 1]"""
    ou, hu, ocfg, channels = _stack("tiny", dtype)
    ref, _ = _ref_forward("tiny", 2, FORWARD_SCALE)
    ref_swapped, _ = _ref_forward("tiny", 2, FORWARD_SCALE, True)
    ad = _product_adapter(channels, dtype)
    x, ehs, te, ids = _inputs(ocfg, 2)
    img = _control_image(2)
    assert not torch.equal(img[0], img[1])
    y, _ = _product_forward(hu, ad, dtype, x, 500.0, ehs, te, ids, img, FORWARD_SCALE)
    r = rel_rms(y, ref)
    y_sw, _ = _product_forward(hu, ad, dtype, x, 500.0, ehs, te, ids, img.flip(0).contiguous(), FORWARD_SCALE)
    print(f"forward tiny S=2 {dtype}: rel-rms {r:.3e} (bound {TOL[dtype]:.0e}); swapped images are {rel_rms(y_sw, ref):.3e} away, "
          f"{rel_rms(y_sw, ref_swapped):.3e} from their own reference")
    assert r < TOL[dtype], r
    assert rel_rms(y_sw, ref) > TOL[dtype] and rel_rms(y_sw, y) > TOL[dtype]          # the b % Br mapping: swapping the images is visible
    assert rel_rms(y_sw, ref_swapped) < TOL[dtype]


def test_eager_plan_graph_and_drop_in_forward_agree():
    dtype = torch.bfloat16
    ou, hu, ocfg, channels = _stack("tiny", dtype)
    ad = _product_adapter(channels, dtype)
    x, ehs, te, ids = _inputs(ocfg)
    img = _control_image()
    ys = [_product_forward(hu, ad, dtype, x, 321.0, ehs, te, ids, img, 0.7, how)[0] for how in ("eager", "plan", "graph")]
    assert torch.isfinite(ys[0]).all() and torch.equal(ys[0], ys[1]) and torch.equal(ys[0], ys[2])
    plain = _product_forward(hu, None, dtype, x, 321.0, ehs, te, ids, None, 1.0)[0]
    assert not torch.equal(ys[0], plain)
    # the drop-in forward with down_intrablock_additional_residuals (NCHW, already scaled): at scale 1 the same launches on the same values
    rec = _product_forward(hu, ad, dtype, x, 321.0, ehs, te, ids, img, 1.0, "graph")[0]
    feats = ad(img.to(DEV))
    added = {"text_embeds": te.to(DEV, dtype), "time_ids": ids.to(DEV)}
    y = hu(torch.cat([x, x], 0).to(DEV), torch.tensor(321.0), ehs.to(DEV, dtype), added_cond_kwargs=added, down_intrablock_additional_residuals=feats)[0]
    assert torch.equal(y.float().cpu(), rec)
    assert torch.equal(hu(torch.cat([x, x], 0).to(DEV), torch.tensor(321.0), ehs.to(DEV, dtype), added_cond_kwargs=added)[0].float().cpu(), plain)


# ---------------------------------------------------------------------------------------------------- conditions that need no measured number
STEPS = 4
LOOP_SCALE = 0.8
LOOP_FACTOR = 0.75             # of 4 steps: the last one runs without the features


def _loop_inputs(ocfg, S=1):
    cd = ocfg.cross_attention_dim
    return (det_randn((S, 4, 32, 32), 3), det_randn((S, 77 + T_TOKENS, cd), 4), det_randn((S, 77 + T_TOKENS, cd), 5),
            det_randn((S, ocfg.pooled_dim), 6), det_randn((S, ocfg.pooled_dim), 7))


def _engine(hu, ad, dtype, ocfg, scale=LOOP_SCALE):
    from imagharmony_amd.denoise import DenoiseEngine
    lat, pe, ne, po, no = _loop_inputs(ocfg)
    eng = DenoiseEngine(hu, DEV, dtype)
    eng.set_adapter(ad)
    eng.set_conditioning(pe, ne, po, no, 256, 256, guidance_scale=5.0)
    if ad is not None:
        eng.set_adapter_image(_control_image(), conditioning_scale=scale)
    return eng, lat


def _launches(plan):
    return [(t[1], t[2]) for t in plan.tags]


def test_scale_zero_factor_rows_and_launch_lists():
    from imagharmony_amd import lib as L
    from imagharmony_amd import schedulers as hs
    dtype = torch.bfloat16
    ou, hu, ocfg, channels = _stack("tiny", dtype)
    ad = _product_adapter(channels, dtype)
    sch = hs.DDIMScheduler()
    eng, lat = _engine(hu, ad, dtype, ocfg)
    n_feat = ad.launches
    eng.set_schedule(sch, STEPS)
    full = eng.denoise(lat).clone()
    plan_ad = eng.plan
    assert eng.ad_gate_tab.tolist() == [1.0] * STEPS and plan_ad.captured
    # factor 0.5: rows 2 and 3 are zero -- the bits of the factor-1 plan run over a table zeroed by hand
    eng.set_schedule(sch, STEPS, adapter_conditioning_factor=0.5)
    assert eng.ad_gate_tab.tolist() == [1.0, 1.0, 0.0, 0.0] and eng.plan is not plan_ad
    half = eng.denoise(lat).clone()
    eng.set_schedule(sch, STEPS)
    assert eng.plan is plan_ad
    eng.ad_gate_tab[2:].zero_()
    by_hand = eng.denoise(lat).clone()
    eng.ad_gate_tab.fill_(1.0)
    assert torch.equal(half, by_hand) and not torch.equal(half, full) and torch.isfinite(half).all()
    assert torch.equal(eng.denoise(lat), full)
    # scale 0: the same image computes nothing anew, and the latents are those of the same engine without the adapter
    eng.set_adapter_image(_control_image(), conditioning_scale=0.0)
    assert ad.launches == n_feat
    eng.set_schedule(sch, STEPS)
    assert eng.plan is not plan_ad
    zero = eng.denoise(lat).clone()
    kinds = [eng.plan.lib.imh_plan_get_kind(eng.plan.plan, i) for i in range(eng.plan.lib.imh_plan_size(eng.plan.plan))]
    assert kinds.count(L.OP_CONTROL_ADD) == 4
    n_ad, list_ad = len(kinds), _launches(eng.plan)
    eng.set_adapter(None)
    eng.set_schedule(sch, STEPS)
    plain = eng.denoise(lat).clone()
    assert torch.equal(zero, plain) and not torch.equal(full, plain)
    # the recorded step: exactly four launches more with the adapter, and without it the list of an engine that never heard of adapters
    n_plain, list_plain = eng.plan.lib.imh_plan_size(eng.plan.plan), _launches(eng.plan)
    assert n_ad == n_plain + 4 and [t for t in list_ad if t[0] != L.OP_CONTROL_ADD] == list_plain
    assert [t[1] for t in list_ad if t[0] == L.OP_CONTROL_ADD] == ["adapter.0", "adapter.1", "adapter.2", "adapter.3"]
    fresh, _ = _engine(hu, None, dtype, ocfg)
    fresh.set_schedule(hs.DDIMScheduler(), STEPS)
    assert torch.equal(fresh.denoise(lat), plain) and _launches(fresh.plan) == list_plain
    # a fork shares the features and the table, and computes the same
    eng.set_adapter(ad)
    eng.set_adapter_image(_control_image(), conditioning_scale=LOOP_SCALE)
    eng.set_schedule(sch, STEPS)
    fk = eng.fork()
    assert fk.ad is eng.ad and fk.ad_gate_tab is eng.ad_gate_tab and fk.adapter is ad and ad.launches == n_feat
    assert torch.equal(fk.denoise(lat), full)


# ---------------------------------------------------------------------------------------------------- the loop
@functools.lru_cache(maxsize=None)
def _ref_loop(kind):
    from test_gpu_controlnet import _schedulers
    ocfg = tiny_config()
    ou = build_pair(torch.bfloat16, num_tokens=T_TOKENS)[0]
    lat, pe, ne, po, no = _loop_inputs(ocfg)
    run = lambda net: tr.denoise(ou, net, _schedulers(kind, 0)[1], lat, pe, ne, po, no, 256, 256, _control_image(), STEPS, guidance_scale=5.0,
                                 adapter_conditioning_scale=LOOP_SCALE, adapter_conditioning_factor=LOOP_FACTOR)
    return run(_ref_adapter(TINY)), run(None)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["ddim", "dpmpp2m"])
def test_denoise_loop_with_adapter_matches_reference(kind, dtype):
    from test_gpu_controlnet import _schedulers
    ou, hu, ocfg, channels = _stack("tiny", dtype)
    ref, ref_plain = _ref_loop(kind)
    assert rel_rms(ref, ref_plain) > 3 * LOOP_TOL[dtype]            # the adapter is visible in the trajectory
    eng, lat = _engine(hu, _product_adapter(channels, dtype), dtype, ocfg)
    eng.set_schedule(_schedulers(kind, 0)[0], STEPS, adapter_conditioning_factor=LOOP_FACTOR)
    assert eng.ad_gate_tab.cpu().tolist() == [1.0, 1.0, 1.0, 0.0]
    out = eng.denoise(lat).float().cpu()
    r = rel_rms(out, ref)
    print(f"{kind} {dtype}: {STEPS}-step loop with the adapter at scale {LOOP_SCALE}, factor {LOOP_FACTOR}: rel-rms {r:.3e} (bound {LOOP_TOL[dtype]:.0e}); "
          f"the adapter moves the reference by {rel_rms(ref, ref_plain):.3e}")
    assert torch.isfinite(out).all() and r < LOOP_TOL[dtype], r


# ---------------------------------------------------------------------------------------------------- the public surface
SEEDS = [3, 9, 27]


def _scorer(lat):
    from imagharmony_amd import pns
    return torch.cat([pns.default_scorer(lat[k:k + 1].float().cpu()) for k in range(lat.shape[0])])


def test_pipeline_pil_in_latents_out_generate_and_pns():
    from PIL import Image
    from imagharmony_amd import StableDiffusionXLAdapterCustomPipeline, T2IAdapter
    from imagharmony_amd import schedulers as hs
    from imagharmony_amd.denoise import DenoiseEngine
    from imagharmony_amd.ip_adapter import IPAdapterXL
    from imagharmony_amd.modules import HarmonyAttention
    dtype = torch.float16
    ou, hu, ocfg, channels = _stack("tiny", dtype)
    ad = _product_adapter(channels, dtype)
    assert isinstance(ad, T2IAdapter)
    lat, pe, ne, po, no = _loop_inputs(ocfg)
    pil = Image.fromarray((_control_image()[0].permute(1, 2, 0) * 255).round().byte().numpy())
    img = torch.from_numpy(__import__("numpy").asarray(pil, dtype="float32") / 255.0).permute(2, 0, 1)[None]
    pipe = StableDiffusionXLAdapterCustomPipeline(hu, ad, scheduler=hs.DDIMScheduler(), device=DEV, dtype=dtype)
    assert pipe.adapter is ad and not hasattr(pipe, "controlnet")
    call = dict(prompt_embeds=pe, negative_prompt_embeds=ne, pooled_prompt_embeds=po, negative_pooled_prompt_embeds=no,
                num_inference_steps=3, guidance_scale=5.0, output_type="latent")
    n0 = ad.launches
    out = pipe(image=pil, latents=lat, adapter_conditioning_scale=0.7, adapter_conditioning_factor=0.67, **call).images      # height / width: the image's
    n1 = ad.launches
    assert n1 - n0 == 29
    eng = DenoiseEngine(hu, DEV, dtype)
    eng.set_adapter(ad)
    eng.set_conditioning(pe, ne, po, no, 256, 256, guidance_scale=5.0)
    eng.set_adapter_image(img, conditioning_scale=0.7)
    eng.set_schedule(hs.DDIMScheduler(), 3, adapter_conditioning_factor=0.67)
    assert eng.ad_gate_tab.cpu().tolist() == [1.0, 1.0, 0.0]
    assert out.shape == (1, 4, 32, 32) and torch.isfinite(out).all() and torch.equal(out, eng.denoise(lat))
    # a second call with the same image does not run the adapter again, whatever the scale
    n1 = ad.launches
    again = pipe(image=img, latents=lat, adapter_conditioning_scale=0.7, adapter_conditioning_factor=0.67, height=256, width=256, **call).images
    other = pipe(image=pil, latents=lat, adapter_conditioning_scale=0.2, **call).images
    assert ad.launches == n1 and torch.equal(again, out) and not torch.equal(other, out)
    pipe(image=_control_image(seed=10), latents=lat, **call)
    assert ad.launches == n1 + 29                                       # another image does
    # every sampler of the base pipeline: a stochastic one with the step noise from the seed reproduces itself
    pipe.scheduler = hs.EulerAncestralDiscreteScheduler()
    g = lambda: torch.Generator("cpu").manual_seed(5)
    a = pipe(image=pil, generator=g(), step_noise="seeded", **call).images
    assert torch.isfinite(a).all() and torch.equal(a, pipe(image=pil, generator=g(), step_noise="seeded", **call).images)
    pipe.scheduler = hs.DDIMScheduler()
    # refusals of the call, before any GPU work
    with pytest.raises(ValueError, match="does not match"):
        pipe(image=pil, height=128, width=128, latents=lat, **call)
    with pytest.raises(ValueError, match="needs `image`"):
        pipe(latents=lat, **call)
    with pytest.raises(ValueError, match="one image, or one per sample"):
        pipe(image=torch.cat([img] * 3), latents=lat, **call)
    # IPAdapterXL on the pipe: generate reaches __call__ through its kwargs; generate_pns runs previews and the final with the adapter
    cd = ocfg.cross_attention_dim
    ha = det_fill(HarmonyAttention(image_hidden_size=128, text_context_dim=cd, inter_dim=512, cross_heads=8, reshape_blocks=8, cross_value_dim=64), 3)
    ip = IPAdapterXL(pipe, None, None, DEV, num_tokens=T_TOKENS, inference=True, number_class_crossattention=ha, dtype=dtype, clip_embeddings_dim=128)
    det_fill(ip.image_proj_model, 5)
    for n, p in hu.attn_processors.items():
        det_fill(p, 9, prefix=n)
    embeds = (det_randn((1, 77, cd), 1), det_randn((1, 77, cd), 2), det_randn((1, ocfg.pooled_dim), 3), det_randn((1, ocfg.pooled_dim), 4))
    rep = lambda t: t.repeat(2, *([1] * (t.dim() - 1)))
    kw = dict(clip_image_embeds=det_randn((1, 128), 5), extra_prompt_embeds=det_randn((1, 77, cd), 6), guidance_scale=5.0)
    gk = dict(kw, prompt_embeds=tuple(rep(t) for t in embeds), num_samples=2, num_inference_steps=2, number_class_crossattention=ha, output_type="latent", seed=42)
    a = ip.generate(image=pil, adapter_conditioning_scale=0.7, **gk)
    b = ip.generate(image=pil, adapter_conditioning_scale=0.0, **gk)
    assert a.shape == (2, 4, 32, 32) and torch.isfinite(a).all() and not torch.equal(a, b)
    n2 = ad.launches
    pk = dict(kw, prompt_embeds=embeds, scale=0.8, adapter_image=pil, adapter_conditioning_scale=0.9, adapter_conditioning_factor=0.75)
    r = ip.generate_pns(SEEDS, preview_steps=2, num_inference_steps=4, batch=2, output_type="latent", scorer=_scorer, **pk)
    win = r["latents"].to(DEV)
    assert ad.launches == n2                                            # the image of the generate calls: one control image, computed once, serves all candidates
    assert r["scores"].shape == (3,) and r["scores"].unique().numel() == 3 and r["best_seed"] in SEEDS and win.shape == (1, 4, 32, 32)
    # the winner is the pipe's own call with that seed's generator, bit for bit
    fused = ip.fused_clip_embeds(None, kw["clip_image_embeds"], kw["extra_prompt_embeds"])
    ipe, uipe = ip._g(ip.image_proj_model)(fused), ip._g(ip.image_proj_model)(torch.zeros_like(fused))
    direct = lambda **extra: pipe(prompt_embeds=torch.cat([embeds[0].to(DEV, dtype), ipe], 1), negative_prompt_embeds=torch.cat([embeds[1].to(DEV, dtype), uipe], 1),
                                  pooled_prompt_embeds=embeds[2], negative_pooled_prompt_embeds=embeds[3], num_inference_steps=4, guidance_scale=5.0,
                                  output_type="latent", generator=[torch.Generator("cpu").manual_seed(int(r["best_seed"]))], image=pil,
                                  **dict(dict(adapter_conditioning_scale=0.9, adapter_conditioning_factor=0.75), **extra)).images
    assert torch.equal(direct().float(), win)
    assert not torch.equal(direct(adapter_conditioning_scale=0.0).float(), win) and not torch.equal(direct(adapter_conditioning_factor=0.25).float(), win)
    with pytest.raises(ValueError, match="adapter_image"):
        ip.generate_pns(SEEDS, output_type="latent", **{k: v for k, v in pk.items() if k != "adapter_image"})
    with pytest.raises(ValueError, match="image="):
        ip.generate_pns(SEEDS, output_type="latent", image=pil, **pk)
