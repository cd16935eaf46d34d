"""GPU tests of FreeU: the FreeU form of IMH_EW_CONCAT (csrc/elementwise.hip freeu_concat_kernel) against the float64 specification
(imagharmony_amd/freeu.py) -- hidden channels bit for bit, filtered channels within one ulp and no more differing elements than fp32
FFT arithmetic itself shows --, its needles, determinism and memory discipline; the UNet forward with FreeU against the fp32 oracle
wrapped by tests/freeu_reference.py, alone and behind a ControlNet; the pipeline switch."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from conftest import PARITY_JSON, rel_rms
from oracle.detfill import det_randn

import freeu_reference as FRf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float16, torch.bfloat16]
# (B, H, W, C_hidden, C_skip, scaled): a boundary inside a vector, non-square and no powers of two, the Nyquist case (H = W = 2), odd
# sides with no scaled channel, and a plane larger than one sweep of the workgroup (1024 pixels against 128)
SHAPES = [(2, 8, 8, 16, 16, 8), (1, 6, 10, 8, 24, 4), (2, 2, 2, 24, 8, 12), (1, 5, 3, 8, 8, 0), (2, 32, 32, 64, 32, 32)]
BS = (1.2, 0.4)                 # (b, s) of the op tests: SDXL's up block 1
PARITY = {}


def _name(dtype):
    return str(dtype).replace("torch.", "")


def _bits(t):
    return t.contiguous().view(torch.int16)


def _ordinal(t):
    """16-bit floats as integers that count representable values (both zeros at 0): |difference| = distance in ulps"""
    b = _bits(t).to(torch.int32) & 0xFFFF
    mag = b & 0x7FFF
    return torch.where(b >= 0x8000, -mag, mag)


def _round_to(x64, dtype):
    """float64 numpy -> torch tensor of dtype, rounded ONCE to nearest even (torch's own float64 -> 16-bit cast goes through fp32)"""
    p, emin = (8, -125) if dtype == torch.bfloat16 else (11, -13)            # significand bits; exponent of the smallest normal as frexp counts it
    _, e = np.frexp(x64)
    q = np.ldexp(1.0, np.maximum(e, emin) - p)
    r = np.rint(x64 / q) * q                                                 # exact in float64; representable in dtype, so the cast below is exact
    return torch.from_numpy(r).to(torch.float32).to(dtype)


@functools.lru_cache(maxsize=None)
def _case(shape, dtype):
    """inputs, the torch expression of the hidden half, the specification and the fp32 FFT restatement of the filtered half: once per
    (shape, dtype), shared by every test"""
    from imagharmony_amd import freeu
    B, H, W, C1, C2, scaled = shape
    a = det_randn((B, H, W, C1), 31).to(dtype)
    b = det_randn((B, H, W, C2), 32).to(dtype)
    bb, s = float(np.float32(BS[0])), float(np.float32(BS[1]))               # the launch carries them as fp32
    hid = a.clone()
    hid[..., :scaled] = a[..., :scaled] * bb
    spec = _round_to(freeu.fourier_filter(b.double().numpy(), s), dtype)
    fft = FRf.fourier_filter(b.permute(0, 3, 1, 2), 1, s).permute(0, 2, 3, 1).contiguous().to(dtype)
    return a, b, hid, spec, fft


def _launch(ctx, a, b, scaled, bs=BS):
    return ctx.concat(a, b, descr="freeu.concat", freeu=(scaled, bs[0], bs[1]))


def _write_parity():
    try:
        out_dir = os.path.dirname(PARITY_JSON)          # beside the suite's measured-parity record; the committed copy is profiles/freeu_parity.json
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "freeu_parity.json"), "w") as f:
            json.dump(PARITY, f, indent=1, sort_keys=True)
    except OSError:
        pass


# ---------------------------------------------------------------------------------------------------- the op
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_against_the_specification(dtype, shape):
    """hidden channels: torch's expression, bit for bit.  Filtered channels: every element within 1 ulp of the float64 specification
    rounded to T -- fp32 evaluation errs by about 1e-6 relative, far below half an ulp of either dtype, so only near-ties may flip --
    and the share of elements that differ at all at most 3x the share the fp32 torch.fft restatement shows against the same
    specification on the same inputs (floor: one element)."""
    from imagharmony_amd.ctx import Ctx
    B, H, W, C1, C2, scaled = shape
    a, b, hid, spec, fft = _case(shape, dtype)
    y = _launch(Ctx(DEV, dtype), a.to(DEV), b.to(DEV), scaled)
    torch.cuda.synchronize()
    y = y.cpu()
    assert y.shape == (B, H, W, C1 + C2) and y.dtype == dtype
    assert torch.equal(_bits(y[..., :C1]), _bits(hid)), "hidden channels: a[..., :i4] * b in T, the rest copied"
    got = y[..., C1:].contiguous()
    assert torch.isfinite(got).all()
    ulps = (_ordinal(got) - _ordinal(spec)).abs()
    n, n_kernel, n_fft = got.numel(), int((ulps != 0).sum()), int((_ordinal(fft) - _ordinal(spec) != 0).sum())
    print(f"freeu concat {shape} {_name(dtype)}: max {int(ulps.max())} ulp; {n_kernel} of {n} elements differ from the specification, "
          f"the fp32 FFT restatement's {n_fft}")
    PARITY[f"kernel_{'x'.join(map(str, shape))}_{_name(dtype)}"] = dict(elements=n, max_ulp=int(ulps.max()), share_kernel=n_kernel / n,
                                                                         share_fft_fp32=n_fft / n, differing_kernel=n_kernel, differing_fft_fp32=n_fft)
    _write_parity()
    assert int(ulps.max()) <= 1
    assert n_kernel <= max(3 * n_fft, 1), f"{n_kernel} elements differ, the fp32 FFT's own arithmetic shows {n_fft}"


@pytest.mark.parametrize("dtype", DTYPES)
def test_needles(dtype):
    """a constant plane c comes out as s * c; s = 1, b = 1 returns the bits of the plain concat"""
    from imagharmony_amd.ctx import Ctx
    ctx = Ctx(DEV, dtype)
    B, H, W, C1, C2 = 2, 6, 10, 16, 24
    a = det_randn((B, H, W, C1), 33).to(dtype).to(DEV)
    c = det_randn((B, 1, 1, C2), 34).to(dtype)
    const = c.expand(B, H, W, C2).contiguous()
    y = _launch(ctx, a, const.to(DEV), 8)[..., C1:].cpu()
    want = _round_to(float(np.float32(BS[1])) * const.double().numpy(), dtype)
    assert int((_ordinal(y.contiguous()) - _ordinal(want)).abs().max()) <= 1
    b = det_randn((B, H, W, C2), 35).to(dtype).to(DEV)
    ident, plain = _launch(ctx, a, b, 8, (1.0, 1.0)), ctx.concat(a, b)
    torch.cuda.synchronize()
    assert torch.equal(_bits(ident), _bits(plain)) and torch.equal(_bits(plain), _bits(torch.cat([a, b], -1)))
    assert not torch.equal(_bits(_launch(ctx, a, b, 8)), _bits(plain))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[4]])
def test_eager_recorded_and_repeated_launches_agree_bit_for_bit(dtype, shape):
    from imagharmony_amd.ctx import Ctx
    a, b = (t.to(DEV) for t in _case(shape, dtype)[:2])
    eager = Ctx(DEV, dtype)
    y1 = _launch(eager, a, b, shape[5]).clone()
    y2 = _launch(eager, a, b, shape[5]).clone()
    rec = Ctx(DEV, dtype, record=True)
    out = _launch(rec, a, b, shape[5])
    rec.run()
    torch.cuda.synchronize()
    y3 = out.clone()
    out.zero_()
    rec.capture()
    rec.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(y1), _bits(y2)) and torch.equal(_bits(y1), _bits(y3)) and torch.equal(_bits(y1), _bits(out))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_guarded_placement(dtype, shape):
    """the launch reads the n * i0 and n * i1 elements of its sources and writes the n * (i0 + i1) of y, nothing else"""
    from guarded import run_dense_and_guarded
    a, b = _case(shape, dtype)[:2]

    def body(ctx, put, out):
        return _launch(ctx, put(a.to(DEV)), put(b.to(DEV)), shape[5])
    dense, guarded, arena = run_dense_and_guarded(DEV, dtype, body)
    arena.check()
    assert torch.equal(_bits(dense[0]), _bits(guarded[0]))


def test_ctx_refuses_what_the_library_refuses():
    from imagharmony_amd import lib as L
    from imagharmony_amd.ctx import Ctx
    ctx = Ctx(DEV, torch.bfloat16)
    z = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device=DEV)
    for a, b, scaled in ((z(1, 8, 8, 16), z(1, 8, 8, 16), 24), (z(1, 1, 8, 16), z(1, 1, 8, 16), 8), (z(1, 8, 8, 16), z(1, 8, 4, 16), 8),
                         (z(64, 16), z(64, 16), 8)):
        with pytest.raises(L.ImhError, match="concat"):
            ctx.concat(a, b, descr="freeu.concat", freeu=(scaled, 1.1, 0.6))


# ---------------------------------------------------------------------------------------------------- the UNet
FREEU = (0.6, 0.4, 1.1, 1.2)        # SDXL's published values: on the CPU they move the tiny oracle's prediction by 0.27 rel-RMS
T_STEP = 500.0


@functools.lru_cache(maxsize=None)
def _oracle_refs():
    """(oracle with FreeU, oracle without) on test_gpu_unet's tiny pair and inputs, CPU fp32, once"""
    from test_gpu_unet import build_pair, inputs
    ou, _, ocfg = build_pair(torch.bfloat16)                       # (the oracle half does not depend on the dtype)
    x, ehs, te, ids = inputs(ocfg)
    added = {"text_embeds": te, "time_ids": ids}
    with torch.no_grad():
        plain = ou(x, torch.tensor(T_STEP), ehs, added_cond_kwargs=added)[0]
        with FRf.oracle_freeu(ou, *FREEU):
            fu = ou(x, torch.tensor(T_STEP), ehs, added_cond_kwargs=added)[0]
        assert torch.equal(plain, ou(x, torch.tensor(T_STEP), ehs, added_cond_kwargs=added)[0])      # the wrapper left the oracle as it was
    return fu, plain


@pytest.mark.parametrize("dtype", DTYPES)
def test_unet_forward_with_freeu_matches_the_wrapped_oracle(dtype):
    """tiny config, latent 32 x 32, B = 2: the FreeU regions are 8 x 8 x 256 and 16 x 16 x 128.  test_gpu_unet.py's bounds (rel-RMS 6e-3
    in fp16, 3e-2 in bf16).  The test can fail: the oracle with FreeU lies at least 3x the bound from the oracle without (0.27 with
    SDXL's values and the seeded tiny weights, so no stronger values are needed)."""
    from test_gpu_unet import TOL, build_pair, inputs
    ref_fu, ref_plain = _oracle_refs()
    vis = rel_rms(ref_fu, ref_plain)
    assert vis >= 3 * TOL[dtype], f"FreeU moves the oracle's prediction by {vis:.3e} only"
    _, hu, ocfg = build_pair(dtype)
    x, ehs, te, ids = inputs(ocfg)
    run = lambda: hu(x.to(DEV), torch.tensor(T_STEP), ehs.to(DEV, dtype),
                     added_cond_kwargs={"text_embeds": te.to(DEV, dtype), "time_ids": ids.to(DEV)})[0].float().cpu()
    y_plain = run()
    hu.enable_freeu(*FREEU)
    y_fu = run()
    hu.disable_freeu()
    y_back = run()
    r_fu, r_plain = rel_rms(y_fu, ref_fu), rel_rms(y_plain, ref_plain)
    print(f"unet tiny {_name(dtype)}: with FreeU rel-rms {r_fu:.3e}, plain {r_plain:.3e} (bound {TOL[dtype]:.0e}); FreeU moves the oracle by {vis:.3e}")
    PARITY[f"unet_tiny_{_name(dtype)}"] = dict(with_freeu=r_fu, plain=r_plain, bound=TOL[dtype], freeu_visibility=vis)
    _write_parity()
    assert torch.isfinite(y_fu).all() and r_fu < TOL[dtype], r_fu
    assert r_plain < TOL[dtype] and torch.equal(y_back, y_plain)


@functools.lru_cache(maxsize=None)
def _oracle_refs_controlnet():
    """(oracle with the ControlNet's residuals and FreeU, with the residuals alone), CPU fp32, once: residuals first, filter second"""
    import controlnet_reference as cr
    from oracle import modules as om
    from oracle.detfill import det_fill
    from oracle.pipeline import install_ip_processors
    from oracle.sdxl_unet import UNet2DConditionModel as OracleUNet
    from oracle.sdxl_unet import tiny_config
    from test_gpu_controlnet import FORWARD_SCALE, T_TOKENS, _control_image, _inputs, _ref_controlnet
    ocfg = tiny_config()
    with torch.no_grad():
        ou = det_fill(OracleUNet(ocfg), 5).eval()
        procs = install_ip_processors(ou, num_tokens=T_TOKENS, scale=0.8)
        for n, p in procs.items():
            if isinstance(p, om.IPAttnProcessor2_0):
                det_fill(p, 7, prefix=n)
    rc = _ref_controlnet("tiny")
    x, ehs, te, ids = _inputs(ocfg)
    added = {"text_embeds": te, "time_ids": ids}
    x2 = torch.cat([x, x], 0)
    with torch.no_grad():
        down, mid = rc(x2, torch.tensor(T_STEP), ehs, _control_image(), conditioning_scale=FORWARD_SCALE, added_cond_kwargs=added)
        cn_only = cr.unet_forward(ou, x2, torch.tensor(T_STEP), ehs, added, down, mid)
        with FRf.oracle_freeu(ou, *FREEU):
            both = cr.unet_forward(ou, x2, torch.tensor(T_STEP), ehs, added, down, mid)
    return both, cn_only


@pytest.mark.parametrize("dtype", DTYPES)
def test_unet_forward_with_controlnet_and_freeu_matches_the_wrapped_oracle(dtype):
    """the ControlNet's residuals are added to the skips before the up path, so FreeU filters the sums (diffusers' order); bounds as in
    test_gpu_controlnet.py's forward test (test_gpu_unet.py's)"""
    from test_gpu_controlnet import FORWARD_SCALE, _control_image, _inputs, _product_forward, _stack
    from test_gpu_unet import TOL
    ref_both, ref_cn = _oracle_refs_controlnet()
    vis = rel_rms(ref_both, ref_cn)
    assert vis >= 3 * TOL[dtype], f"FreeU moves the reference's prediction behind the ControlNet by {vis:.3e} only"
    _, _, hu, cn, ocfg = _stack("tiny", dtype)
    x, ehs, te, ids = _inputs(ocfg)
    hu.enable_freeu(*FREEU)
    y = _product_forward(hu, cn, dtype, x, T_STEP, ehs, te, ids, _control_image(), FORWARD_SCALE)
    r = rel_rms(y, ref_both)
    print(f"unet tiny {_name(dtype)} ControlNet + FreeU: rel-rms {r:.3e} (bound {TOL[dtype]:.0e}); FreeU moves the reference by {vis:.3e}")
    PARITY[f"unet_tiny_controlnet_{_name(dtype)}"] = dict(with_freeu=r, bound=TOL[dtype], freeu_visibility=vis)
    _write_parity()
    assert torch.isfinite(y).all() and r < TOL[dtype], r


# ---------------------------------------------------------------------------------------------------- the pipeline
def test_pipeline_switch_changes_the_latents_and_switching_back_restores_them():
    from imagharmony_amd.pipeline import StableDiffusionXLCustomPipeline
    from test_gpu_unet import build_pair
    dtype = torch.bfloat16
    _, hu, ocfg = build_pair(dtype)
    pipe = StableDiffusionXLCustomPipeline(hu, device=DEV, dtype=dtype)
    cd, pd = ocfg.cross_attention_dim, ocfg.pooled_dim
    kw = dict(prompt_embeds=det_randn((1, 81, cd), 41).to(DEV, dtype), negative_prompt_embeds=det_randn((1, 81, cd), 42).to(DEV, dtype),
              pooled_prompt_embeds=det_randn((1, pd), 43).to(DEV, dtype), negative_pooled_prompt_embeds=det_randn((1, pd), 44).to(DEV, dtype),
              height=256, width=256, num_inference_steps=4, output_type="latent", return_dict=False)
    lat = det_randn((1, 4, 32, 32), 45).to(DEV)
    plain = pipe(latents=lat.clone(), **kw)[0].clone()
    pipe.enable_freeu(*FREEU)
    assert pipe.engine.unet.freeu == FREEU
    fu = pipe(latents=lat.clone(), **kw)[0].clone()
    assert sum(t[2] == "freeu.concat" for t in pipe.engine.plan.tags) == 6 and pipe.engine._sched_key.freeu == FREEU
    pipe.disable_freeu()
    back = pipe(latents=lat.clone(), **kw)[0].clone()
    assert not any(t[2] == "freeu.concat" for t in pipe.engine.plan.tags)
    assert torch.isfinite(fu).all() and not torch.equal(fu, plain)
    assert torch.equal(back, plain)
