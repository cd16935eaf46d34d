"""GPU: the phase form of Upsample2D's conv (Ctx.conv3x3 up=2; include/imh.h, csrc/gemm_ring.hip) -- four 2 x 2-tap convs on the low-res
input in one implicit GEMM (M = B H W, N = 4 Cout, K = 4 Cin) -- against fp32 torch F.interpolate(nearest x2) -> F.conv2d(padding 1) on
the operands as stored, under the bound every conv test uses (tests/test_gpu_ops.py assert_close)."""
import pytest
import torch
import torch.nn.functional as F

from test_gpu_gnstats import _check_groupnorm, _check_partials
from test_gpu_ops import DTYPES, L, assert_close, ctx_for, rnd  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

PHASE_VARIANTS = [(1464, 160, 1), (2464, 160, 1), (24128, 160, 1), (23256, 160, 1), (23256, 128, 1), (5258, 320, 1)]


def pack_conv(w4):
    return w4.permute(0, 2, 3, 1).reshape(w4.shape[0], -1).contiguous()


def _case(B, H, W, Cin, Cout, dtype):
    x = rnd(B, H, W, Cin, dtype=dtype, seed=1)
    w4 = rnd(Cout, Cin, 3, 3, dtype=dtype, seed=2, scale=(9 * Cin) ** -0.5)
    bias = rnd(Cout, dtype=dtype, seed=3)
    return x, w4, bias


def _ref(x, w4, bias):
    """fp32 (TF32 off: the yardstick must not be the loosest link)"""
    old = torch.backends.cudnn.allow_tf32
    torch.backends.cudnn.allow_tf32 = False
    try:
        up = F.interpolate(x.float().permute(0, 3, 1, 2), scale_factor=2.0, mode="nearest")
        return F.conv2d(up, w4.float(), bias.float(), padding=1).permute(0, 2, 3, 1).contiguous()
    finally:
        torch.backends.cudnn.allow_tf32 = old


def _tuned():
    """the phase-form entries of tuning.json (fifth key field 4) -> [(M, N, K, cfg)]"""
    from imagharmony_amd.ctx import _load_tuning
    return [(k[0], k[1], k[2], tuple(v)) for k, v in _load_tuning().items() if len(k) == 5 and k[4] == 4]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,H,W,C", [(2, 32, 32, 1280), (2, 64, 64, 640)])
def test_benchmarked_upsamplers_in_the_phase_form(L, dtype, B, H, W, C):
    """the two upsampler launches of the 1024^2 CFG forward on the variant tuning.json names for them, and on every other variant that
    carries the form; the up=1 form of the same launch agrees to the same bound"""
    from imagharmony_amd.ctx import phase_pack
    ctx = ctx_for(dtype)
    x, w4, bias = _case(B, H, W, C, C, dtype)
    ref = _ref(x, w4, bias)
    tuned = ctx.conv_up_phase_cfg(B, H, W, C, C)
    assert tuned is not None and tuple(ctx.tuning[(B * H * W, 4 * C, 4 * C, 1, 4)]) == tuned
    wp = phase_pack(w4).to(dtype).contiguous()
    assert wp.shape == (4 * C, 4 * C)
    for cfg in [None] + [v for v in PHASE_VARIANTS if C % v[1] == 0]:
        y = ctx.conv3x3(x, None, bias=bias, up=2, w_phase=wp, cfg=cfg)
        assert y.shape == (B, 2 * H, 2 * W, C)
        assert_close(y, ref, dtype, f"phase form {(B, H, W, C)} cfg {cfg or tuned}")
        assert torch.equal(y, ctx.conv3x3(x, pack_conv(w4), bias=bias, up=2, cfg=cfg)), "packing inside conv3x3 == phase_pack"
        ctx.free(y)
    assert_close(ctx.conv3x3(x, pack_conv(w4), bias=bias, up=1), ref, dtype, f"up=1 form {(B, H, W, C)}")


def test_every_phase_entry_of_the_tuning_table_runs():
    ents = _tuned()
    assert {(e[0], e[1], e[2]) for e in ents} >= {(2048, 5120, 5120), (8192, 2560, 2560)}
    ctx = ctx_for(torch.bfloat16)
    for (M, N, K, cfg) in ents:
        Cout, Cin = N // 4, K // 4
        H = W = int(round((M // 2) ** 0.5))
        assert 2 * H * W == M and (cfg[0], cfg[1]) in ctx._PHASE and Cout % cfg[1] == 0
        x, w4, bias = _case(2, H, W, Cin, Cout, torch.bfloat16)
        assert ctx.conv_up_phase_cfg(2, H, W, Cin, Cout) == cfg
        y = ctx.conv3x3(x, pack_conv(w4), bias=bias, up=2)
        assert_close(y, _ref(x, w4, bias), torch.bfloat16, f"tuning entry {(M, N, K)} -> {cfg}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg", PHASE_VARIANTS)
def test_ragged_and_small_geometries(L, dtype, cfg):
    """M no multiple of the tile rows, odd H / W, H or W = 1, B > 1, Cin != Cout, without a bias; every edge of the low-res image is a
    padding edge of some phase"""
    ctx = ctx_for(dtype)
    bn = cfg[1]
    for (B, H, W, Cin, Cout) in [(1, 12, 20, 64, bn), (2, 5, 7, 128, 2 * bn), (3, 1, 9, 64, bn), (1, 7, 1, 192, bn), (2, 1, 1, 64, 2 * bn), (1, 33, 17, 64, bn)]:
        x, w4, bias = _case(B, H, W, Cin, Cout, dtype)
        y = ctx.conv3x3(x, pack_conv(w4), bias=bias, up=2, cfg=cfg)
        assert_close(y, _ref(x, w4, bias), dtype, f"phase form {cfg} {(B, H, W, Cin, Cout)}")
        y0 = ctx.conv3x3(x, pack_conv(w4), up=2, cfg=cfg)
        assert_close(y0, _ref(x, w4, torch.zeros_like(bias)), dtype, f"phase form {cfg} {(B, H, W, Cin, Cout)} no bias")
        ctx.free(y); ctx.free(y0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_launches_that_do_not_qualify_are_refused_and_the_model_falls_back(L, dtype):
    """a column tile must lie inside one phase: B = 1, 12 x 20, Cout = 200 is REFUSED by conv3x3(up=2) and by the library itself
    (IMH_ERR_ARG), and Ctx.conv_up_phase_cfg -- what the UNet asks -- answers None, so the model runs the up=1 form there"""
    import ctypes as C
    ctx = ctx_for(dtype)
    x, w4, bias = _case(1, 12, 20, 64, 200, dtype)
    assert ctx.conv_up_phase_cfg(1, 12, 20, 64, 200) is None
    for cfg in (None, (23256, 160, 1), (2464, 160, 1), (5258, 320, 1)):
        with pytest.raises(L.ImhError, match="phase form"):
            ctx.conv3x3(x, pack_conv(w4), bias=bias, up=2, cfg=cfg)
    assert_close(ctx.conv3x3(x, pack_conv(w4), bias=bias, up=1), _ref(x, w4, bias), dtype, "up=1 fallback")
    # the C ABI: the same launch handed to the library directly, and variants without the phase gather
    from imagharmony_amd.ctx import phase_pack
    wp = phase_pack(w4).to(dtype).contiguous()
    out = torch.zeros(1, 24, 40, 200, dtype=dtype, device=DEV)

    def args(bm, bn, cout=200):
        a = L.GemmArgs()
        a.X, a.W, a.Y, a.bias = x.data_ptr(), wp.data_ptr(), out.data_ptr(), bias.data_ptr()
        a.M, a.N, a.K, a.ldx, a.ldw, a.ldy = 240, 4 * cout, 256, 64, 256, cout
        a.splits, a.dtype, a.conv, a.bm, a.bn = 1, ctx.dt, 1, bm, bn
        a.H, a.Wd, a.Cin, a.Ho, a.Wo, a.stride, a.up = 12, 20, 64, 24, 40, 1, 2
        return a
    for (bm, bn) in [(23256, 160), (5258, 320), (128, 128), (7128, 160), (3064, 64)]:
        assert ctx.lib.imh_gemm(C.byref(args(bm, bn)), ctx.stream()) == -1 and b"phase form" in ctx.lib.imh_last_error(), (bm, bn)
    a = args(23256, 160); a.Ho = 12
    assert ctx.lib.imh_gemm(C.byref(a), ctx.stream()) == -2
    # the A/B knob: key 11 = 0 switches the form off -- the library refuses, the host answers "does not qualify"
    xq, wq4, bq = _case(1, 8, 8, 64, 160, dtype)
    try:
        assert ctx.lib.imh_debug_set(11, 0) == 0 and ctx.lib.imh_debug_set(11, -1) == 0
        assert ctx.conv_up_phase_cfg(1, 8, 8, 64, 160) is None
        with pytest.raises(L.ImhError, match="phase form"):
            ctx.conv3x3(xq, pack_conv(wq4), bias=bq, up=2)
    finally:
        assert ctx.lib.imh_debug_set(11, 1) == 1
    assert_close(ctx.conv3x3(xq, pack_conv(wq4), bias=bq, up=2), _ref(xq, wq4, bq), dtype, "key 11 back on")
    torch.cuda.synchronize()
    assert out.abs().max().item() == 0, "a refused launch wrote nothing"


def _ref_phase_partials(y, B, H, W, rows):
    """y [B, 2H, 2W, C] as stored -> [B, 4 * H W / rows, C / 10, 2] fp64 -> fp32: block ph * (H W / rows) + j holds the phase-ph output
    pixels (2y + py, 2x + px) of low-res pixels [j * rows, (j + 1) * rows) in row-major (y, x) order"""
    C_ = y.shape[-1]
    f = y.double().view(B, H, 2, W, 2, C_).permute(0, 2, 4, 1, 3, 5).reshape(B, 4 * (H * W // rows), rows, C_ // 10, 10)
    s = f.sum(dim=(2, 4))
    mean = f.mean(dim=(2, 4), keepdim=True)
    return torch.stack([s, (f - mean).pow(2).sum(dim=(2, 4))], dim=-1).float()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg,rows", [((1464, 160, 1), 32), ((2464, 160, 1), 32), ((24128, 160, 1), 64), ((23256, 160, 1), 64)])
def test_groupnorm_partials_of_the_phase_form(L, dtype, cfg, rows):
    """gn_groups on: one (sum, M2) pair per (sample, block of `rows` low-res pixels, phase, 10 channels) in the fixed order the header
    states, under the bounds of tests/test_gpu_gnstats.py; folded by the library's own table routine (imh_groupnorm with the handed-over
    partials) they give torch's GroupNorm (32 groups of 10 / 20 / 30 / 40 channels) of the output; variants / sizes without the epilogue hand back None"""
    ctx = ctx_for(dtype)
    for (B, H, W, Cin, Cout) in [(2, 16, 16, 64, 320), (1, 8, 32, 128, 640), (3, 16, 8, 64, 960), (2, 32, 32, 64, 1280)]:
        x, w4, bias = _case(B, H, W, Cin, Cout, dtype)
        y, gs = ctx.conv3x3(x, pack_conv(w4), bias=bias, up=2, cfg=cfg, gn_groups=1)
        assert gs is not None and gs.nblk == 4 * H * W // rows and gs.sub == 10 and gs.npart == 10 * rows and gs.C == Cout
        assert_close(y, _ref(x, w4, bias), dtype, f"phase form + gn {cfg} {(B, H, W, Cin, Cout)}")
        what = f"GroupNorm partials of the phase form {cfg} {(B, H, W, Cin, Cout)}"
        _check_partials(gs, _ref_phase_partials(y, B, H, W, rows), y, what)
        _check_groupnorm(ctx, y.view(B * 4 * H * W, Cout), B, 4 * H * W, gs, dtype, what)
        y2, gs2 = ctx.conv3x3(x, pack_conv(w4), bias=bias, up=2, cfg=cfg, gn_groups=1)
        assert torch.equal(y2, y) and torch.equal(gs2.t, gs.t)
    x, w4, bias = _case(1, 12, 20, 64, 320, dtype)           # 240 low-res pixels: no whole blocks
    assert ctx.conv3x3(x, pack_conv(w4), bias=bias, up=2, cfg=cfg, gn_groups=1)[1] is None
    assert ctx.conv3x3(x, pack_conv(w4), bias=bias, up=2, cfg=(5258, 320, 1), gn_groups=1)[1] is None


@pytest.mark.parametrize("dtype", DTYPES)
def test_eager_plan_and_graph_replay_are_bit_identical(L, dtype):
    """the launch has no atomics and no cross-workgroup hand-over: eager == recorded plan == captured graph, replayed 10 times"""
    from imagharmony_amd.ctx import Ctx
    for (B, H, W, C) in [(2, 32, 32, 1280), (2, 64, 64, 640)]:
        x, w4, bias = _case(B, H, W, C, C, dtype)
        ctx = ctx_for(dtype)
        y, gs = ctx.conv3x3(x, pack_conv(w4), bias=bias, up=2, gn_groups=1)
        assert gs is not None
        torch.cuda.synchronize()
        rec = Ctx(DEV, dtype, record=True)
        yr, gr = rec.conv3x3(x, pack_conv(w4), bias=bias, up=2, gn_groups=1)
        rec.run()
        torch.cuda.synchronize()
        assert torch.equal(yr, y) and torch.equal(gr.t, gs.t), "recorded plan != eager"
        yr.zero_(); gr.t.zero_()
        rec.capture()
        for i in range(10):
            rec.replay()
            torch.cuda.synchronize()
            assert torch.equal(yr, y) and torch.equal(gr.t, gs.t), f"graph replay {i} != eager"
            yr.zero_(); gr.t.zero_()
