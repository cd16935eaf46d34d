"""CPU (no GPU): the phase form of Upsample2D's conv (Ctx.conv3x3 up=2, include/imh.h) -- nearest x2 upsampling followed by a 3x3 conv is,
per output phase (py, px), a 2 x 2-tap conv on the LOW-res input whose weights are sums of the 3x3 taps.  Checked here: the algebra in fp32
at awkward geometries, the packed layout on a hand-computed case, and the numerics of the new error source (one rounding of each
pre-summed weight) against the bound the GPU tests use, beside the same figures for the present (nine-tap) path."""
import math

import pytest
import torch
import torch.nn.functional as F

from imagharmony_amd.ctx import phase_pack

EPS = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


def assert_close(y, ref, dtype, what, k=4.0):
    """tests/test_gpu_ops.py assert_close: max error <= k * EPS * scale, rel-RMS <= 2 * EPS"""
    ref, y = ref.float(), y.float()
    scale = ref.abs().max().item() + 1e-6
    err = (y - ref).abs().max().item()
    rms = ((y - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt().clamp_min(1e-12)).item()
    assert math.isfinite(err), f"{what}: non-finite output"
    assert err <= k * EPS[dtype] * scale and rms <= 2 * EPS[dtype], f"{what}: max err {err:.3e} (scale {scale:.3e}), rel-rms {rms:.3e}"
    return err / (EPS[dtype] * scale), rms / EPS[dtype]


def rnd(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def reference(x, w, b=None):
    """x [B, Cin, H, W], w [Cout, Cin, 3, 3] -> F.interpolate(nearest x2) -> F.conv2d(padding 1)"""
    return F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), w, b, padding=1)


def phase_apply(x, wp, b=None):
    """the phase-packed weight wp [4 Cout, 4 Cin] (rows (p, cout), K order (a, b, cin)) applied as the kernels apply it: for phase
    p = 2 py + px, out[:, :, 2y + py, 2x + px] = sum over taps (a, b) of wp[p, :, a, b, :] . x[:, :, y + py - 1 + a, x + px - 1 + b],
    zero outside the low-res image"""
    B, Cin, H, W = x.shape
    Cout = wp.shape[0] // 4
    w5 = wp.view(4, Cout, 2, 2, Cin)
    xp = F.pad(x, (1, 1, 1, 1))                       # xp[.., i + 1, j + 1] = x[.., i, j]
    out = x.new_zeros(B, Cout, 2 * H, 2 * W)
    for py in range(2):
        for px in range(2):
            acc = x.new_zeros(B, Cout, H, W)
            for a in range(2):
                for b_ in range(2):
                    win = xp[:, :, py + a:py + a + H, px + b_:px + b_ + W]           # low-res pixel (y + py - 1 + a, x + px - 1 + b)
                    acc = acc + torch.einsum("oc,bchw->bohw", w5[2 * py + px, :, a, b_, :], win)
            out[:, :, py::2, px::2] = acc
    return out if b is None else out + b.view(1, -1, 1, 1)


@pytest.mark.parametrize("B,H,W,Cin,Cout", [(1, 4, 4, 8, 8), (2, 5, 7, 8, 12), (3, 6, 3, 16, 8), (2, 1, 9, 8, 24), (1, 7, 1, 24, 8), (2, 1, 1, 8, 8)])
def test_phase_form_equals_upsample_then_conv_in_fp32(B, H, W, Cin, Cout):
    """odd and even H / W, B > 1, H or W = 1, Cin != Cout: equal to fp32 round-off (the two sides only differ in summation order)"""
    x, w, b = rnd(B, Cin, H, W, seed=1).double(), rnd(Cout, Cin, 3, 3, seed=2, scale=(9 * Cin) ** -0.5), rnd(Cout, seed=3).double()
    got = phase_apply(x, phase_pack(w).double(), b)
    ref = reference(x, w.double(), b)
    assert got.shape == ref.shape == (B, Cout, 2 * H, 2 * W)
    # phase_pack sums in fp32: up to 4 fp32 terms per entry -> a few 2^-24 relative per weight, K = 4 Cin terms
    assert (got - ref).abs().max().item() <= 8 * 2.0 ** -24 * ref.abs().max().item() * math.sqrt(4 * Cin)
    # ... and exactly the fp32 algebra when everything is fp32
    got32 = phase_apply(x.float(), phase_pack(w), b.float())
    assert (got32 - ref.float()).abs().max().item() <= 64 * 2.0 ** -24 * ref.abs().max().item()


def test_packed_layout_is_pinned_by_a_hand_computed_case():
    """Cout = Cin = 1, w[ky][kx] = 10 ky + kx + 1: row block = phase 2 py + px, K order (a, b)"""
    w = torch.tensor([[1., 2., 3.], [11., 12., 13.], [21., 22., 23.]]).view(1, 1, 3, 3)
    wp = phase_pack(w)
    assert wp.shape == (4, 4) and wp.dtype == torch.float32
    want = torch.tensor([
        # (a, b) = (0, 0)            (0, 1)                         (1, 0)                      (1, 1)
        [1.,                         2. + 3.,                       11. + 21.,                  12. + 13. + 22. + 23.],      # py 0, px 0
        [1. + 2.,                    3.,                            11. + 12. + 21. + 22.,      13. + 23.],                  # py 0, px 1
        [1. + 11.,                   2. + 3. + 12. + 13.,           21.,                        22. + 23.],                  # py 1, px 0
        [1. + 2. + 11. + 12.,        3. + 13.,                      21. + 22.,                  23.]])                       # py 1, px 1
    assert torch.equal(wp, want)
    # two channels each way: rows (p, cout), columns (a, b, cin)
    w2 = torch.stack([torch.stack([w[0, 0], 2 * w[0, 0]]), torch.stack([3 * w[0, 0], 4 * w[0, 0]])])       # [cout, cin] scale (1 2; 3 4)
    wp2 = phase_pack(w2)
    assert wp2.shape == (8, 8)
    sc = torch.tensor([[1., 2.], [3., 4.]])
    for p in range(4):
        for co in range(2):
            for t in range(4):
                for ci in range(2):
                    assert wp2[2 * p + co, 2 * t + ci].item() == want[p, t].item() * sc[co, ci].item()


def _emulate(x, w, b, dtype, phase):
    """the GPU paths' arithmetic on the CPU: operands in `dtype`, exact products, fp32 accumulation (fp64 here: the accumulation-order
    term is below the bound by orders of magnitude), bias, ONE rounding of the output; phase: weights pre-summed in fp32 and rounded once"""
    xd = x.to(dtype).double()
    bd = b.to(dtype).double()
    if phase:
        y = phase_apply(xd, phase_pack(w.to(dtype)).to(dtype).double(), bd)
    else:
        y = reference(xd, w.to(dtype).double(), bd)
    return y.to(dtype)


# the two benchmarked upsamplers' channel counts at a reduced image size, and the up = 1 geometries of tests/test_gpu_ops.py test_conv3x3
EMU_CASES = [(1, 8, 8, 1280, 1280), (1, 12, 12, 640, 640), (2, 8, 8, 64, 64), (2, 16, 24, 64, 320), (2, 8, 8, 64, 320), (1, 12, 20, 64, 200),
             (1, 20, 12, 64, 200), (2, 8, 8, 64, 160)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("B,H,W,Cin,Cout", EMU_CASES)
def test_emulated_phase_path_stays_inside_the_gpu_bound(dtype, B, H, W, Cin, Cout):
    """Figures measured with this test (max error in units of EPS * scale | rel-RMS in units of EPS; the bound is 4 | 2), over all
    cases and both dtypes: present nine-tap path 0.50-0.69 | 0.42-0.43, phase path 0.62-0.84 | 0.51-0.52 (1280 channels bf16: 0.60 | 0.42
    -> 0.74 | 0.52; 640 channels bf16: 0.61 | 0.42 -> 0.76 | 0.52).  The one rounding of each pre-summed weight adds an error of about
    the output rounding's own size; the margin to the bound (3.3 | 1.58 -> 3.2 | 1.48) stays what it was to well within 2x."""
    x, w, b = rnd(B, Cin, H, W, seed=1), rnd(Cout, Cin, 3, 3, seed=2, scale=(9 * Cin) ** -0.5), rnd(Cout, seed=3)
    # the fp32 reference sees the operands as stored (rounded to dtype), like the GPU tests'
    ref = reference(x.to(dtype).double(), w.to(dtype).double(), b.to(dtype).double())
    e9, r9 = assert_close(_emulate(x, w, b, dtype, False), ref, dtype, "emulated nine-tap path")
    e4, r4 = assert_close(_emulate(x, w, b, dtype, True), ref, dtype, "emulated phase path")
    print(f"{dtype} {(B, H, W, Cin, Cout)}: nine-tap max {e9:.2f} EPS*scale rms {r9:.2f} EPS | phase max {e4:.2f} rms {r4:.2f}")
    # the margin to the bound stays what the present path has, to within 2x
    assert 4.0 - e4 >= (4.0 - e9) / 2 and 2.0 - r4 >= (2.0 - r9) / 2


def test_unet_conv_packs_and_caches_the_phase_weight():
    from imagharmony_amd.ctx import Ctx
    from imagharmony_amd.unet import Conv2d
    conv = Conv2d(64, 128, 3)
    with torch.no_grad():
        conv.weight.copy_(rnd(128, 64, 3, 3, seed=5))
    ctx = Ctx("cpu", torch.bfloat16, record=True, dry=True)
    wp = conv.packed_phase(ctx)
    assert wp.shape == (512, 256) and wp.dtype == torch.bfloat16 and wp.is_contiguous()
    assert torch.equal(wp, phase_pack(conv.weight).to(torch.bfloat16)) and conv.packed_phase(ctx) is wp
    assert conv.packed(ctx).shape == (128, 576)            # the nine-tap packing is untouched


def test_host_picks_the_phase_form_only_where_a_column_tile_stays_inside_one_phase():
    """Ctx.conv_up_phase_cfg: the benchmarked upsamplers qualify on their table entries; Cout = 200 (no tile width divides it), Cin = 96
    and a tile family without the phase gather do not -- the caller runs up=1 there; conv3x3(up=2) itself refuses them"""
    from imagharmony_amd import lib as L
    from imagharmony_amd.ctx import Ctx
    ctx = Ctx("cpu", torch.bfloat16, record=True, dry=True)
    for (B, H, W, C) in [(2, 32, 32, 1280), (2, 64, 64, 640)]:
        cfg = ctx.conv_up_phase_cfg(B, H, W, C, C)
        assert cfg is not None and (cfg[0], cfg[1]) in Ctx._PHASE and C % cfg[1] == 0 and cfg[2] == 1
        assert tuple(ctx.tuning[(B * H * W, 4 * C, 4 * C, 1, 4)]) == cfg
    assert ctx.conv_up_phase_cfg(1, 12, 20, 64, 200) is None
    assert ctx.conv_up_phase_cfg(1, 12, 20, 96, 320) is None
    assert ctx.conv_up_phase_cfg(1, 12, 20, 64, 320, cfg=(7128, 160, 1)) is None
    assert ctx.conv_up_phase_cfg(1, 12, 20, 64, 320, cfg=(23256, 160, 1)) == (23256, 160, 1)
    x, w = torch.zeros(1, 12, 20, 64, dtype=torch.bfloat16), torch.zeros(200, 576, dtype=torch.bfloat16)
    with pytest.raises(L.ImhError, match="phase form"):
        ctx.conv3x3(x, w, up=2)
    with pytest.raises(L.ImhError, match="phase form"):
        ctx.conv3x3(x, torch.zeros(320, 576, dtype=torch.bfloat16), up=2, residual=torch.zeros(1, 24, 40, 320, dtype=torch.bfloat16))
    # a qualifying launch records as the conv it computes (output pixels x Cout x 9 Cin, its algorithmic FLOPs, geometry up = 2)
    y, gs = ctx.conv3x3(x, torch.zeros(320, 576, dtype=torch.bfloat16), up=2, gn_groups=1)
    tag = ctx.tags[-1]
    assert y.shape == (1, 24, 40, 320) and tag[5] == (960, 320, 576, 1, (1, 12, 20, 64, 1, 2)) and tag[3] == 2.0 * 960 * 320 * 576
    assert gs is None                                       # 240 low-res pixels are no whole number of 64-row blocks
