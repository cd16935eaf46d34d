"""GPU: guarded placement of every kernel family behind the C ABI (tests/guarded.py).  Each case runs its op twice -- placed densely
with a plain Ctx as the other GPU files do, and through GuardCtx with every input place()d in a NaN-sentinel arena, every output
carved from it and every leading dimension the wrapper takes wider than the row -- and asserts
  (a) the dense result meets the bound the op already has against fp32 / fp64 torch (test_gpu_ops.py / _vae / _lnstats / _gnstats /
      _img2img: same helpers, same k),
  (b) the guarded result has the same bits (placement and pitch are not arithmetic),
  (c) no byte outside the operands changed and every output is finite (Arena.check()).
Shapes are the smallest at which an edge tile, a ragged key tile or a pitch can go wrong, not workload shapes.  A load outside an
operand whose value is discarded is invisible to this method (the sentinel shows only reads that reach a result)."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import built, ref_row_stats
from guarded import GuardDamage, run_dense_and_guarded
from test_gpu_ops import BIG_VARIANTS, DEV, DTYPES, EPS, L, assert_close, geglu_ref, make_vt, rnd, sdpa_ref, vt_unpermute  # noqa: F401

pytestmark = pytest.mark.gpu

# an upper bound of the row pitch of every view a case below places or carves (the widest are the packed [Q|K|V] rows of the 33-head
# self-attention, 3 * 33 * 64 + 64 elements of 2 bytes, and the 4096-wide LayerNorm rows); tests/test_guarded_host.py holds the
# guard-size rule at this pitch
MAX_ROW_PITCH_BYTES = 4096 * 4

# real tile rows of every variant code (include/imh.h imh_gemm_args.bm)
TILE_ROWS = {64: 64, 128: 128, 256: 256, 3064: 64, 3128: 128, 4064: 64, 4128: 128, 5064: 64, 5258: 256, 6128: 128, 6064: 64, 8256: 256,
             9128: 128, 9256: 256, 1464: 64, 2464: 64, 24128: 128, 23256: 256, 22128: 128, 26256: 256}


def settle(dense, guarded, arena, what, bits=True):
    """(c) guards intact and outputs finite, (b) same bits as the dense run -- both reported together"""
    problems = []
    try:
        arena.check()
    except GuardDamage as e:
        problems.append(str(e))
    if bits:
        for i, (d, g) in enumerate(zip(dense, guarded)):
            assert d.shape == g.shape and d.dtype == g.dtype
            if not torch.equal(d, g):
                problems.append(f"result {i}: {int((d != g).sum())} of {d.numel()} elements differ from the dense run")
    assert not problems, f"{what}: " + " | ".join(problems)


def run(dtype, body, what, bits=True):
    dense, guarded, arena = run_dense_and_guarded(DEV, dtype, body)
    settle(dense, guarded, arena, what, bits)
    return dense


def _norm(K):
    norm = torch.nn.LayerNorm(K, eps=1e-5)
    with torch.no_grad():
        norm.weight.copy_(1 + 0.2 * torch.randn(K, generator=torch.Generator().manual_seed(3)))
        norm.bias.copy_(0.3 * torch.randn(K, generator=torch.Generator().manual_seed(4)))
    return norm


def _folded(w, K, dtype):
    from imagharmony_amd.attention_processor import fold_ln
    from imagharmony_amd.ctx import Ctx
    norm = _norm(K)
    return norm, fold_ln(w, norm, Ctx(DEV, dtype))


def test_arena_notices_a_stray_store_on_the_device():
    """the audit itself on device memory: one element written (by torch, inside the arena) just past a carved output is found"""
    from guarded import Arena
    a = Arena(DEV, 8 << 20)
    v = a.carve((6, 10), torch.bfloat16, ld=16, name="victim")
    v.fill_(1)
    a.check()
    torch.as_strided(v, (1,), (1,), v.storage_offset() + 5 * 16 + 10).fill_(2)
    with pytest.raises(GuardDamage, match=r"victim: after, bytes \[180, 181\]"):
        a.check()


# ------------------------------------------------------------------------------------ GEMM
PLAIN = [(bm, bn, sp) for bm in (64, 128) for bn in (64, 128) for sp in (1, 2, 4)]


def _gemm_shapes(cfg):
    bm, bn = TILE_ROWS[cfg[0]], cfg[1]
    return [(2, 8, 64), (bm + 2, bn + 8, 128), (2 * bm - 6, 2 * bn - 8, 192)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg", PLAIN + built(BIG_VARIANTS))
def test_gemm_edge_tiles(L, dtype, cfg):
    """bias + residual (ldr > N) + a row-add that is a column slice of a wider table, ldx / ldw / ldy wider than the rows, on one
    row x one column tile's worth of edge, just past one tile and just short of two"""
    for (M, N, K) in _gemm_shapes(cfg):
        x, w = rnd(M, K, dtype=dtype, seed=1), rnd(N, K, dtype=dtype, seed=2, scale=K ** -0.5)
        b, r = rnd(N, dtype=dtype, seed=3), rnd(M, N, dtype=dtype, seed=4)
        rpb = (M + 2) // 3
        nb = (M + rpb - 1) // rpb
        ra_full = rnd(nb, N + 64, dtype=dtype, seed=5)

        def body(ctx, put, out):
            ra = put(ra_full)[:, 32:32 + N]
            o = out((M, N), dtype, ld=N + 24)
            ctx.gemm(put(x, ld=K + 64), put(w, ld=K + 8), out=o, bias=put(b), residual=put(r, ld=N + 16), rowadd=ra,
                     rows_per_batch=rpb, ldra=N + 64, cfg=cfg)
            return o
        what = f"gemm {cfg} {(M, N, K)}"
        ref = x.float() @ w.float().t() + b.float() + r.float() + ra_full[:, 32:32 + N].float()[torch.arange(M, device=DEV) // rpb]
        dense, guarded, arena = run_dense_and_guarded(DEV, dtype, body)
        assert_close(dense[0], ref, dtype, what)
        settle(dense, guarded, arena, what)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("flags", ["ln", "ln_geglu"])
def test_gemm_sixteen_wave_tile(L, dtype, flags):
    """26256 x 320 accepts whole tiles with the row-form folded LayerNorm only: one tile and 2 x 2 tiles, statistics from the guarded
    row-statistics launch"""
    fl = L.GF_LN_ROW | (L.GF_GEGLU if flags == "ln_geglu" else 0)
    for (M, N, K) in [(256, 320, 64), (512, 640, 128)]:
        x = (rnd(M, K, dtype=dtype, seed=1) * 1.5 + 3.0).contiguous()
        w = rnd(N, K, dtype=torch.float32, seed=2, scale=K ** -0.5)
        norm, (wg, s, c) = _folded(w, K, dtype)
        ref = (F.layer_norm(x.float().cpu(), (K,), norm.weight, norm.bias, 1e-5) @ w.cpu().t()).to(DEV)

        def body(ctx, put, out):
            xx = put(x, ld=K + 64)
            st = ctx.row_stats(xx)
            o = out((M, N // 2 if fl & L.GF_GEGLU else N), dtype, ld=N + 24)
            ctx.gemm(xx, put(wg, ld=K + 8), out=o, flags=fl, ln=(put(s), put(c), 1e-5, st), cfg=(26256, 320, 1))
            return o, st[0]
        dense = run(dtype, body, f"26256 {flags} {(M, N, K)}")
        assert_close(dense[0], geglu_ref(ref) if fl & L.GF_GEGLU else ref, dtype, f"26256 {flags} {(M, N, K)}", k=8.0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_geglu_vt_perm_f32_act(L, dtype):
    from imagharmony_amd.unet import geglu_interleave
    # GEGLU, ragged on both sides of a 128 x 128 tile
    M, K, inner = 130, 128, 72
    x = rnd(M, K, dtype=dtype, seed=1)
    w, b = rnd(2 * inner, K, dtype=dtype, seed=2, scale=K ** -0.5), rnd(2 * inner, dtype=dtype, seed=3)
    r = rnd(M, inner, dtype=dtype, seed=4)
    wi, bi = geglu_interleave(w), geglu_interleave(b)

    def geglu(ctx, put, out):
        o = out((M, inner), dtype, ld=inner + 24)
        ctx.gemm(put(x, ld=K + 64), put(wi, ld=K + 8), out=o, bias=put(bi), residual=put(r, ld=inner + 16), flags=L.GF_GEGLU, cfg=(128, 128, 1))
        return o
    full = x.float() @ w.float().t() + b.float()
    assert_close(run(dtype, geglu, "geglu")[0], full[:, :inner] * F.gelu(full[:, inner:]) + r.float(), dtype, "geglu")
    # V^T permutation: [C, n] with n a whole number of 16-key groups, ragged against the 64 x 128 tile
    C_, n, K = 72, 144, 64
    wv, xk = rnd(C_, K, dtype=dtype, seed=1, scale=K ** -0.5), rnd(n, K, dtype=dtype, seed=2)

    def vt(ctx, put, out):
        o = out((C_, n), dtype, ld=n + 16)
        ctx.gemm(put(wv, ld=K + 8), put(xk, ld=K + 64), out=o, flags=L.GF_VT_PERM, cfg=(64, 128, 1))
        return o
    assert_close(vt_unpermute(run(dtype, vt, "V^T")[0].contiguous()), wv.float() @ xk.float().t(), dtype, "V^T")
    # fp32 output and the activations
    M, N, K = 66, 72, 128
    x, w, b = rnd(M, K, dtype=dtype, seed=1), rnd(N, K, dtype=dtype, seed=2, scale=K ** -0.5), rnd(N, dtype=dtype, seed=3)
    ref = x.float() @ w.float().t()
    for fl, want, odt in ((L.GF_OUT_F32, ref, torch.float32), (L.GF_ACT_SILU, F.silu(ref + b.float()), dtype), (L.GF_ACT_GELU, F.gelu(ref + b.float()), dtype)):
        def act(ctx, put, out):
            o = out((M, N), odt, ld=N + 24)
            ctx.gemm(put(x, ld=K + 64), put(w, ld=K + 8), out=o, bias=None if fl == L.GF_OUT_F32 else put(b), flags=fl, cfg=(64, 64, 1))
            return o
        y = run(dtype, act, f"flags {fl}")[0]
        assert y.dtype == odt
        assert_close(y, want, dtype, f"flags {fl}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg", [(2464, 160, 1), (128, 128, 1), (5258, 320, 1)])
def test_gemm_row_statistics_out(L, dtype, cfg):
    """stats_out on a variant with the statistics epilogue (ragged M: the epilogue must not emit rows >= M) and on two without (the
    row-statistics launch over the strided y)"""
    from test_gpu_lnstats import _check_stats
    M, N, K = 70, 160, 128
    x, w = rnd(M, K, dtype=dtype, seed=1), rnd(N, K, dtype=dtype, seed=2, scale=K ** -0.5)
    b, r = rnd(N, dtype=dtype, seed=5), (rnd(M, N, dtype=dtype, seed=6) * 1.5 + 0.5).contiguous()

    def body(ctx, put, out):
        o = out((M, N), dtype, ld=N + 24)
        y, (st, slots) = ctx.gemm(put(x, ld=K + 64), put(w, ld=K + 8), out=o, bias=put(b), residual=put(r, ld=N + 16), cfg=cfg, stats_out=True)
        wd = ctx.lib.imh_gemm_stats_slot_width(cfg[0], cfg[1])
        assert slots == (N // wd if wd and N % wd == 0 else 1)        # (128 x 128: 64-wide slots do not divide N = 160 -> the row-statistics launch)
        return y, st
    y, st = run(dtype, body, f"stats_out {cfg}")
    assert_close(y, x.float() @ w.float().t() + b.float() + r.float(), dtype, f"stats_out {cfg}")
    _check_stats(st, st.shape[1], y.contiguous(), f"stats_out {cfg}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg,rows", built([((2464, 160, 1), 32), ((23256, 160, 1), 64)]))
def test_gemm_groupnorm_partials_out(L, dtype, cfg, rows):
    from imagharmony_amd.ctx import GnStats
    from test_gpu_gnstats import _check_partials, _ref_partials
    B, hw, N, K = 3, 64, 160, 128
    M = B * hw                                               # 192: ragged against the 256-row tile, three samples in it
    x, w = rnd(M, K, dtype=dtype, seed=1), rnd(N, K, dtype=dtype, seed=2, scale=K ** -0.5)
    b, r = rnd(N, dtype=dtype, seed=5), (rnd(M, N, dtype=dtype, seed=6) * 1.5 + 0.5).contiguous()

    def body(ctx, put, out):
        y, gs = ctx.gemm(put(x, ld=K + 64), put(w, ld=K + 8), bias=put(b), residual=put(r, ld=N + 16), cfg=cfg, gn_out=hw)
        assert gs is not None and gs.nblk == hw // rows
        return y, gs.t
    y, t = run(dtype, body, f"gn_out {cfg}")
    assert_close(y, x.float() @ w.float().t() + b.float() + r.float(), dtype, f"gn_out {cfg}")
    _check_partials(GnStats(t, hw // rows, 10, 10 * rows, N), _ref_partials(y, B, hw, hw // rows, 10), y, f"gn_out {cfg}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg", [(2464, 160, 1), (23256, 160, 1)])
def test_gemm_one_launch_qkv_transposed_v(L, dtype, cfg):
    """yt=: [Q|K] row-major with ldy > 2C, V transposed into a V^T buffer with ldyt > M (whole tiles only)"""
    B, Lq, C_ = 1, 256, 320
    M = B * Lq
    x = (rnd(M, C_, dtype=dtype, seed=1) * 1.5 + 2.0).contiguous()
    w3 = rnd(3 * C_, C_, dtype=torch.float32, seed=2, scale=C_ ** -0.5)
    norm, f3 = _folded(w3, C_, dtype)
    st80 = ref_row_stats(x.float(), C_ // 80).to(DEV)

    def body(ctx, put, out):
        vt = out((C_, M), dtype, ld=M + 64)
        qk = out((M, 2 * C_), dtype, ld=2 * C_ + 64)
        ctx.gemm(put(x, ld=C_ + 64), put(f3[0], ld=C_ + 8), out=qk, flags=L.GF_LN_ROW, ln=(put(f3[1]), put(f3[2]), 1e-5, (put(st80), C_ // 80)),
                 cfg=cfg, yt=(vt, 2 * C_))
        return qk, vt
    qk, vt = run(dtype, body, f"yt {cfg}")
    ref = (F.layer_norm(x.float().cpu(), (C_,), norm.weight, norm.bias, 1e-5) @ w3.cpu().t()).to(DEV)
    assert_close(qk, ref[:, :2 * C_], dtype, f"[Q|K] {cfg}", k=6.0)
    assert_close(vt_unpermute(vt), ref[:, 2 * C_:].t(), dtype, f"V^T {cfg}", k=6.0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg", [(64, 64, 1), (128, 128, 1), (2464, 160, 1), (23256, 160, 1)])
def test_gemm_two_source_operand(L, dtype, cfg):
    M, C1, C2, N = 70, 128, 64, 168
    a, b2 = rnd(M, C1, dtype=dtype, seed=1), rnd(M, C2, dtype=dtype, seed=2)
    w, bias = rnd(N, C1 + C2, dtype=dtype, seed=7, scale=(C1 + C2) ** -0.5), rnd(N, dtype=dtype, seed=4)

    def body(ctx, put, out):
        o = out((M, N), dtype, ld=N + 24)
        ctx.gemm(put(a, ld=C1 + 64), put(w, ld=C1 + C2 + 8), out=o, bias=put(bias), x2=put(b2), cfg=cfg)       # (x2 must be dense: Ctx.gemm)
        return o
    assert_close(run(dtype, body, f"x2 {cfg}")[0], torch.cat([a, b2], 1).float() @ w.float().t() + bias.float(), dtype, f"x2 {cfg}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg", [(64, 64), (128, 128)])
def test_gemm_dual(L, dtype, cfg):
    """the [Q|K] (row form) + V^T (column form, V^T layout) pair in one launch, statistics from the guarded row-statistics launch"""
    M, N, K = 80, 136, 128
    x = (rnd(M, K, dtype=dtype, seed=1) * 1.5 + 3.0).contiguous()
    w = rnd(N, K, dtype=torch.float32, seed=2, scale=K ** -0.5)
    norm, (wg, s, c) = _folded(w, K, dtype)

    def body(ctx, put, out):
        xx, ww, ss, cc = put(x, ld=K + 64), put(wg, ld=K + 8), put(s), put(c)
        y, yt = out((M, N), dtype, ld=N + 24), out((N, M), dtype, ld=M + 16)
        ctx.gemm_dual(dict(x=xx, w=ww, out=y, flags=L.GF_LN_ROW, ln=(ss, cc, 1e-5)),
                      dict(x=ww, w=xx, out=yt, flags=L.GF_LN_COL | L.GF_VT_PERM, ln=(ss, cc, 1e-5)), cfg=cfg)
        return y, yt
    y, yt = run(dtype, body, f"gemm_dual {cfg}")
    ref = (F.layer_norm(x.float().cpu(), (K,), norm.weight, norm.bias, 1e-5) @ w.cpu().t()).to(DEV)
    assert_close(y, ref, dtype, f"dual row form {cfg}", k=6.0)
    assert_close(vt_unpermute(yt.contiguous()), ref.t(), dtype, f"dual column form {cfg}", k=6.0)


# ------------------------------------------------------------------------------------ conv3x3
CONV_VARIANTS = [(128, 64, 1), (64, 128, 2), (256, 128, 1), (4128, 64, 1), (5258, 320, 1), (1464, 160, 1), (2464, 160, 1), (24128, 160, 1), (23256, 160, 1),
                 (22128, 160, 1), (7128, 320, 1), (7128, 160, 1), (7128, 80, 1), (7256, 160, 1), (7356, 160, 1), (7328, 160, 1), (7428, 160, 1), (7564, 160, 1)]
HALO = (7128, 7564, 7328, 7428, 7256, 7356)


def _conv_case(dtype, cfg, B, H, W, Cin, Cout, stride=1, up=0, pad=0):
    x = rnd(B, H, W, Cin, dtype=dtype, seed=1)
    w4 = rnd(Cout, Cin, 3, 3, dtype=dtype, seed=2, scale=(9 * Cin) ** -0.5)
    b = rnd(Cout, dtype=dtype, seed=3)
    wp = w4.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin).contiguous()
    xin = x.float().permute(0, 3, 1, 2)
    if up:
        xin = F.interpolate(xin, scale_factor=2.0, mode="nearest")
    if pad:
        ref = F.conv2d(F.pad(xin, (0, 1, 0, 1)), w4.float(), b.float(), stride=2).permute(0, 2, 3, 1)
    else:
        ref = F.conv2d(xin, w4.float(), b.float(), stride=stride, padding=1).permute(0, 2, 3, 1)
    extras = up != 2
    temb = rnd(B, Cout + 64, dtype=dtype, seed=4)
    res = rnd(*ref.shape, dtype=dtype, seed=5)

    def body(ctx, put, out):
        kw = dict(rowadd=put(temb)[:, 32:32 + Cout], ldra=Cout + 64, residual=put(res).view(-1, Cout)) if extras else {}
        return ctx.conv3x3(put(x), put(wp), bias=put(b), stride=stride, up=up, pad=pad, cfg=cfg, **kw)
    what = f"conv {cfg} {(B, H, W, Cin, Cout)} stride {stride} up {up} pad {pad}"
    y = run(dtype, body, what)[0]
    assert y.shape == ref.shape
    assert_close(y, ref + (temb[:, 32:32 + Cout].float()[:, None, None, :] + res.float() if extras else 0.0), dtype, what)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg", built(CONV_VARIANTS))
def test_conv3x3_ragged_geometries(L, dtype, cfg):
    """a 3 x 5 image, a 2 x 12 x 20 one (ragged against the 4 / 8 / 16-row patches and every implicit-GEMM row tile) and Cout = bn + 8,
    with the row-add (a column slice of a wider table) and the residual of test_conv3x3"""
    _conv_case(dtype, cfg, 1, 3, 5, 64, 8)
    _conv_case(dtype, cfg, 2, 12, 20, 64, cfg[1] + 8)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg", built(CONV_VARIANTS))
def test_conv3x3_stride_up_pad(L, dtype, cfg):
    from imagharmony_amd.ctx import Ctx
    if cfg[0] not in HALO:
        _conv_case(dtype, cfg, 2, 11, 9, 64, 72, stride=2)
        if Ctx._variant_ok(cfg[0], cfg[2], 0, 1, 2, False, pad=1):
            _conv_case(dtype, cfg, 2, 11, 9, 64, 72, stride=2, pad=1)
    _conv_case(dtype, cfg, 1, 6, 10, 64, 72, up=1)
    if (cfg[0], cfg[1]) in Ctx._PHASE:
        _conv_case(dtype, cfg, 2, 5, 7, 64, cfg[1], up=2)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg", built([(7128, 320, 1), (7128, 160, 1), (7128, 80, 1), (7256, 160, 1), (7356, 160, 1), (7328, 160, 1), (7428, 160, 1), (7564, 160, 1)]))
def test_conv3x3_fused_groupnorm_and_two_sources(L, dtype, cfg):
    """the LDS-halo front end on a ragged image: GroupNorm (+ SiLU) applied in the halo staging from a guarded table, and the channel
    concat read from two guarded producers"""
    from test_gpu_gnstats import G, _gn_conv_ref, pack_conv
    B, H, W, C1, C2, Cout = 2, 13, 19, 256, 64, 168
    Cin = C1 + C2
    a = (rnd(B, H, W, C1, dtype=dtype, seed=1) * 1.2 + 0.3).contiguous()
    b2 = (rnd(B, H, W, C2, dtype=dtype, seed=2) * 0.7 - 0.2).contiguous()
    w4 = rnd(Cout, Cin, 3, 3, dtype=dtype, seed=3, scale=(9 * Cin) ** -0.5)
    bias = rnd(Cout, dtype=dtype, seed=4)
    gamma, beta = rnd(Cin, dtype=dtype, seed=11) * 0.2 + 1.0, rnd(Cin, dtype=dtype, seed=12) * 0.3

    def body(ctx, put, out):
        aa, bb = put(a), put(b2)
        tab = ctx.gn_table([ctx.gn_stats(aa.view(B, H * W, C1), sub=2), ctx.gn_stats(bb.view(B, H * W, C2), sub=2)], put(gamma), put(beta), G, 1e-5, H * W)
        return ctx.conv3x3(aa, put(pack_conv(w4)), bias=put(bias), cfg=cfg, gn=(tab, True), x2=bb), tab
    y = run(dtype, body, f"fused GroupNorm two-source conv {cfg}")[0]
    assert_close(y.view(B * H * W, Cout), _gn_conv_ref(torch.cat([a, b2], -1), gamma, beta, w4, bias), dtype, f"fused GroupNorm two-source conv {cfg}", k=6.0)


# ------------------------------------------------------------------------------------ attention
def _self_attention(L, dtype, B, H, Lq, Lk, Lk_pad, what):
    """Q rows [B, Lq], K rows [B, Lk_pad] with rows >= Lk finite padding (30.0: an unmasked key would show), V^T padding columns zero,
    as include/imh.h makes them part of the operand; packed [Q|K|.] rows of 3 H 64 columns when Lq == Lk_pad"""
    C_ = H * 64
    packed = Lq == Lk_pad
    q = rnd(B * Lq, C_, dtype=dtype, seed=1)
    k = rnd(B, Lk_pad, C_, dtype=dtype, seed=3)
    k[:, Lk:] = 30.0
    v = rnd(B, Lk, C_, dtype=dtype, seed=2)
    vt = make_vt(v, Lk_pad)
    qkv = torch.cat([q, k.view(B * Lk_pad, C_), rnd(B * Lq, C_, dtype=dtype, seed=4)], 1) if packed else None

    def body(ctx, put, out):
        if packed:
            t = put(qkv, ld=3 * C_ + 64)
            qq, kk = t[:, :C_], t[:, C_:2 * C_]
        else:
            qq, kk = put(q, ld=C_ + 64), put(k.view(B * Lk_pad, C_), ld=2 * C_)
        o = out((B * Lq, C_), dtype, ld=C_ + 64)
        vv = put(vt, ld=B * Lk_pad + 64)
        ctx.attention(qq, kk, vv, o, B, H, Lq, Lk, Lk_pad, qq.stride(0), kk.stride(0), vv.stride(0), o.stride(0), 0.125)
        return o
    o = run(dtype, body, what)[0]
    assert_close(o.view(B, Lq, C_), sdpa_ref(q.view(B, Lq, C_), k[:, :Lk], v, H), dtype, what, k=6.0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("B,H,Lq", [(1, 1, 64), (2, 1, 100), (1, 2, 192), (1, 3, 320)])
def test_attention_self(L, dtype, mode, B, H, Lq):
    assert L.load().imh_debug_set(4, mode) == 0
    try:
        _self_attention(L, dtype, B, H, Lq, Lq, (Lq + 63) // 64 * 64, f"self attention mode {mode} {(B, H, Lq)}")
    finally:
        L.load().imh_debug_set(4, 0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("Lk,Lk_pad", [(1, 64), (63, 64), (100, 128), (988, 1024)])
def test_attention_self_masked_keys(L, dtype, mode, Lk, Lk_pad):
    assert L.load().imh_debug_set(4, mode) == 0
    try:
        _self_attention(L, dtype, 1, 2, Lk_pad, Lk, Lk_pad, f"masked keys mode {mode} {(Lk, Lk_pad)}")
    finally:
        L.load().imh_debug_set(4, 0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_key_quarter_workgroups(L, dtype):
    _self_attention(L, dtype, 1, 33, 1024, 1024, 1024, "key-quarter workgroups (1, 33, 1024)")


def _pad64(n):
    return (n + 63) // 64 * 64


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Lq,nt,nip", [(100, 77, 4), (64, 130, 0), (128, 77, 32)])
def test_attention_cross_ip(L, dtype, Lq, nt, nip):
    B, H = 2, 2
    C_ = H * 64
    q = rnd(B * Lq, C_, dtype=dtype, seed=1)
    k, v = rnd(B, nt, C_, dtype=dtype, seed=2), rnd(B, nt, C_, dtype=dtype, seed=3)
    kp = torch.zeros(B, _pad64(nt), C_, dtype=dtype, device=DEV)
    kp[:, :nt] = k
    ref = sdpa_ref(q.view(B, Lq, C_), k, v, H)
    if nip:
        k2, v2 = rnd(B, nip, C_, dtype=dtype, seed=4), rnd(B, nip, C_, dtype=dtype, seed=5)
        k2p = torch.zeros(B, _pad64(nip), C_, dtype=dtype, device=DEV)
        k2p[:, :nip] = k2
        ref = ref + 0.7 * sdpa_ref(q.view(B, Lq, C_), k2, v2, H)

    def body(ctx, put, out):
        kw = {}
        if nip:
            vt2 = put(make_vt(v2, _pad64(nip)), ld=B * _pad64(nip) + 16)
            kk2 = put(k2p.view(-1, C_), ld=C_ + 64)
            kw = dict(k2=kk2, vt2=vt2, Lk2=nip, Lk2_pad=_pad64(nip), ldk2=kk2.stride(0), ldvt2=vt2.stride(0), scale2=0.7)
        qq, kk, vt = put(q, ld=C_ + 64), put(kp.view(-1, C_), ld=C_ + 64), put(make_vt(v, _pad64(nt)), ld=B * _pad64(nt) + 16)
        o = out((B * Lq, C_), dtype, ld=C_ + 64)
        ctx.attention(qq, kk, vt, o, B, H, Lq, nt, _pad64(nt), qq.stride(0), kk.stride(0), vt.stride(0), o.stride(0), 0.125, **kw)
        return o
    assert_close(run(dtype, body, f"cross attention {(Lq, nt, nip)}")[0].view(B, Lq, C_), ref, dtype, "cross attention", k=6.0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", [1, 10])
@pytest.mark.parametrize("ln", [0, 1, 2])
@pytest.mark.parametrize("Lq,nt,nip", [(100, 77, 4), (64, 130, 0), (128, 77, 32)])
def test_fused_cross_attention(L, dtype, mode, ln, Lq, nt, nip):
    """csrc/xattn.hip, one head per workgroup (mode 1) and the wide five-head form (10): to_q (+ folded LayerNorm, statistics from a
    guarded row-statistics launch or handed over in a guarded tensor) + text (+ image-prompt) attention.  The wide form takes whole
    128-query blocks only (IMH_ERR_SHAPE otherwise), so it runs the same key counts at Lq = 128"""
    if mode == 10:
        Lq = 128
    B, H = 2, 5
    C_ = H * 64
    x = (rnd(B * Lq, C_, dtype=dtype, seed=1) * 1.3 + (0.7 if ln else 0.0)).contiguous()
    wq = rnd(C_, C_, dtype=torch.float32, seed=6, scale=C_ ** -0.5)
    k, v = rnd(B, nt, C_, dtype=dtype, seed=2), rnd(B, nt, C_, dtype=dtype, seed=3)

    def make_k(kk, n_pad):
        kp = torch.zeros(B, n_pad, C_, dtype=dtype, device=DEV)
        kp[:, :kk.shape[1]] = kk
        return kp.view(B, n_pad, C_ // 16, 4, 4)[:, :, :, [0, 2, 1, 3], :].reshape(B * n_pad, C_).contiguous()
    if ln:
        norm, (wg, s_, c_) = _folded(wq, C_, dtype)
        q_ref = (F.layer_norm(x.float(), (C_,), norm.weight.to(DEV), norm.bias.to(DEV), 1e-5) @ wq.to(DEV).t()).to(dtype)
    else:
        wg = wq.to(DEV, dtype)
        q_ref = (x.float() @ wg.float().t()).to(dtype)
    ref = sdpa_ref(q_ref.view(B, Lq, C_), k, v, H)
    if nip:
        k2, v2 = rnd(B, nip, C_, dtype=dtype, seed=4), rnd(B, nip, C_, dtype=dtype, seed=5)
        ref = ref + 0.7 * sdpa_ref(q_ref.view(B, Lq, C_), k2, v2, H)

    def body(ctx, put, out):
        xx = put(x, ld=C_ + 64)
        lnq = None
        if ln:
            st = None if ln == 1 else (put(ref_row_stats(x.float(), C_ // 32).to(DEV)), C_ // 32)
            lnq = (put(s_), put(c_), 1e-5, st)
        kw = {}
        if nip:
            kk2, vt2 = put(make_k(k2, _pad64(nip)), ld=C_ + 64), put(make_vt(v2, _pad64(nip)), ld=B * _pad64(nip) + 16)
            kw = dict(k2=kk2, vt2=vt2, Lk2=nip, Lk2_pad=_pad64(nip), ldk2=kk2.stride(0), ldvt2=vt2.stride(0), scale2=0.7)
        kk, vt = put(make_k(k, _pad64(nt)), ld=C_ + 64), put(make_vt(v, _pad64(nt)), ld=B * _pad64(nt) + 16)
        o = out((B * Lq, C_), dtype, ld=C_ + 64)
        ctx.cross_attention(xx, put(wg, ld=C_ + 8), kk, vt, o, B, H, Lq, nt, _pad64(nt), kk.stride(0), vt.stride(0), 0.125, ln=lnq, **kw)
        return o
    assert L.load().imh_debug_set(3, mode) == 0
    try:
        o = run(dtype, body, f"fused cross attention mode {mode} ln {ln} {(Lq, nt, nip)}")[0]
    finally:
        L.load().imh_debug_set(3, 0)
    assert_close(o.view(B, Lq, C_), ref, dtype, f"fused cross attention mode {mode} ln {ln} {(Lq, nt, nip)}", k=8.0)


# ------------------------------------------------------------------------------------ attention_small
def _small_need(Lk, dq, dv):
    """LDS bytes of the K^T / V-resident kernel, as attention_small_launch computes them"""
    LkP = (Lk + 63) & ~63
    return (dq * LkP + Lk * dv) * 2 + (4 * LkP + 4 * dq) * 4


def _small_lk_above_threshold(dq, dv):
    return next(lk for lk in range(1, 8193) if _small_need(lk, dq, dv) > 150 * 1024)


def _small_ref(q, k, v, B, H, Lq, Lk, dq, dv, scale):
    qh = q.float().view(B, Lq, H, dq).transpose(1, 2)
    kh = k.float().view(B, Lk, H, dq).transpose(1, 2)
    vh = v.float().view(B, Lk, H, dv).transpose(1, 2)
    return F.scaled_dot_product_attention(qh, kh, vh, scale=scale).transpose(1, 2).reshape(B * Lq, H * dv)


def _small_case(dtype, B, H, Lq, Lk, dq, dv, ldkv_extra=0):
    """K and V are the two column ranges of ONE [B Lk, H dq + H dv] buffer (modules.py hands to_kv's output over like this)"""
    scale = dq ** -0.5
    q = rnd(B * Lq, H * dq, dtype=dtype, seed=1)
    kv = rnd(B * Lk, H * (dq + dv), dtype=dtype, seed=2)

    def body(ctx, put, out):
        t = put(kv, ld=H * (dq + dv) + ldkv_extra)
        o = out((B * Lq, H * dv), dtype, ld=H * dv + 24)
        return ctx.attention_small(put(q, ld=H * dq + 40), t[:, :H * dq], t[:, H * dq:], B, H, Lq, Lk, dq, dv, scale, out=o)
    return body, _small_ref(q, kv[:, :H * dq], kv[:, H * dq:], B, H, Lq, Lk, dq, dv, scale)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(1, 8, 8, 77, 40, 64), (2, 12, 16, 273, 64, 64), (1, 2, 5, 1, 8, 8), (1, 1, 3, 64, 128, 128), (1, 1, 3, 65, 128, 128),
                                   (1, 2, 5, 77, 36, 64), "threshold"])
def test_attention_small(L, dtype, shape):
    """imh_attention_small against fp32 SDPA with dq != dv: the LDS-resident kernel (key counts on both sides of a 64-key tile), and the
    fallback kernel reached by dq = 36 (not a multiple of 8) and by the smallest Lk whose K^T + V exceed the 150 KB threshold"""
    if shape == "threshold":
        shape = (1, 1, 3, _small_lk_above_threshold(64, 64), 64, 64)
        assert 64 < shape[3] <= 8192 and _small_need(shape[3] - 1, 64, 64) <= 150 * 1024
    body, ref = _small_case(dtype, *shape, ldkv_extra=64)
    assert_close(run(dtype, body, f"attention_small {shape}")[0], ref, dtype, f"attention_small {shape}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_small_kernels_agree(L, dtype):
    """one shape that both kernels accept: ldk / ldv multiples of 8 -> the LDS-resident kernel; a pitch that is not (the one place where
    a leading dimension legitimately changes the dispatch) -> the fallback.  Different summation orders, so (a) holds for each and the
    two agree within the same bound; no bit equality between them"""
    shape = (2, 4, 9, 77, 40, 64)
    body_lds, ref = _small_case(dtype, *shape, ldkv_extra=64)
    body_fb, _ = _small_case(dtype, *shape, ldkv_extra=4)
    y_lds = run(dtype, body_lds, "attention_small, LDS-resident")[0]
    dense, guarded, arena = run_dense_and_guarded(DEV, dtype, body_fb)
    settle(dense, guarded, arena, "attention_small, fallback by pitch", bits=False)
    assert_close(y_lds, ref, dtype, "LDS-resident kernel")
    assert_close(guarded[0], ref, dtype, "fallback kernel")
    assert_close(guarded[0], y_lds, dtype, "the two kernels")


def test_attention_small_error_codes(L):
    lib = L.load()
    t = torch.zeros(64, 128, dtype=torch.bfloat16, device=DEV)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(Lk=8, dtype=L.IMH_DT_BF16):
        a = L.SmallAttnArgs()
        a.Q, a.K, a.V, a.O = t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr()
        a.B, a.H, a.Lq, a.Lk, a.dq, a.dv = 1, 1, 4, Lk, 64, 64
        a.ldq = a.ldk = a.ldv = a.ldo = 128
        a.scale, a.dtype = 0.125, dtype
        return lib.imh_attention_small(C.byref(a), s)
    assert call(Lk=8193) == -2 and b"unsupported shape" in lib.imh_last_error()        # IMH_ERR_SHAPE, nothing launched
    assert call(dtype=7) == -3 and b"unknown dtype" in lib.imh_last_error()            # IMH_ERR_DTYPE
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------ norms
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,HW,C_", [(1, 15, 64), (2, 100, 320), (1, 1030, 2560)])
def test_groupnorm_every_mode(L, dtype, B, HW, C_):
    """IMH_GN_ALL (workspace carved at exactly imh_groupnorm_workspace_bytes), IMH_GN_STATS -> IMH_GN_TABLE -> IMH_GN_APPLY and
    IMH_GN_TABLE_APPLY, every buffer between them guarded"""
    from imagharmony_amd.ctx import GnSpec
    x = rnd(B, HW, C_, dtype=dtype, seed=1) + 0.5
    g, b = rnd(C_, dtype=dtype, seed=2) * 0.1 + 1, rnd(C_, dtype=dtype, seed=3) * 0.1

    def body(ctx, put, out):
        xx, gg, bb = put(x), put(g), put(b)
        y0 = ctx.groupnorm(xx, gg, bb, 32, 1e-5, True)
        gs = ctx.gn_stats(xx, sub=2)
        tab = ctx.gn_table(gs, gg, bb, 32, 1e-5, HW)
        y1 = ctx.gn_apply(xx, tab, True)
        y2 = ctx.gn_table_apply(xx, GnSpec(gs, gg, bb, 32, 1e-5), True)
        return y0, y1, y2, gs.t, tab
    y0, y1, y2, _, _ = run(dtype, body, f"groupnorm {(B, HW, C_)}")
    ref = F.silu(F.group_norm(x.float().transpose(1, 2), 32, g.float(), b.float(), 1e-5)).transpose(1, 2)
    for y, what in ((y0, "all-in-one"), (y1, "stats + table + apply"), (y2, "table-apply")):
        assert_close(y, ref, dtype, f"groupnorm {what} {(B, HW, C_)}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,C_", [(3, 64), (7, 2048), (5, 4096)])
def test_layernorm(L, dtype, rows, C_):
    x = rnd(rows, C_, dtype=dtype, seed=1) * 2 + 0.3
    g, b = rnd(C_, dtype=dtype, seed=2) * 0.1 + 1, rnd(C_, dtype=dtype, seed=3) * 0.1
    y = run(dtype, lambda ctx, put, out: ctx.layernorm(put(x), put(g), put(b), 1e-5), f"layernorm {(rows, C_)}")[0]
    assert_close(y, F.layer_norm(x.float(), (C_,), g.float(), b.float(), 1e-5), dtype, "layernorm")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows", [1, 5, 130])
def test_row_stats_strided_rows(L, dtype, rows):
    from test_gpu_lnstats import _check_stats
    C_ = 320
    x = (rnd(rows, C_, dtype=dtype, seed=1) * 1.5 + 2.0).contiguous()
    st = run(dtype, lambda ctx, put, out: ctx.row_stats(put(x, ld=C_ + 72))[0], f"row_stats {rows}")[0]
    _check_stats(st, 1, x, f"row_stats {rows}")


# ------------------------------------------------------------------------------------ elementwise
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", [64, 256, 320])
def test_ew_timestep(L, dtype, dim):
    t = torch.tensor([958.0, 1.0, 500.0], device=DEV)

    def body(ctx, put, out):
        return ctx.ew(L.EW_TIMESTEP, out((3, dim), dtype), a=put(t), n=3, i=(dim, 0, 0, 0, 0, 0))
    half = dim // 2
    a = t[:, None] * torch.exp(-math.log(10000.0) * torch.arange(half, device=DEV, dtype=torch.float32) / half)[None]
    assert_close(run(dtype, body, f"timestep {dim}")[0], torch.cat([a.cos(), a.sin()], -1), dtype, "timestep", k=2.0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [8, 2056])
def test_ew_flat_ops(L, dtype, n):
    """EW_ADD (k = 2, silu's bound), EW_SILU, EW_CONCAT, EW_CAST_F32 (exact), EW_STEP_ROW (exact; first and last row of the table) and
    EW_STEP_SET with the counter one int inside the arena"""
    a, b = rnd(n, dtype=dtype, seed=1), rnd(n, dtype=dtype, seed=2)
    rows = 5
    tab = rnd(rows, n, dtype=dtype, seed=3)

    def body(ctx, put, out):
        aa, bb = put(a), put(b)
        y_add = ctx.ew(L.EW_ADD, out((n,), dtype), a=aa, b=bb, n=n)
        y_silu = ctx.silu(aa)
        y_cat = ctx.concat(aa.view(n // 8, 8), bb.view(n // 8, 8))
        y_f32 = ctx.ew(L.EW_CAST_F32, out((n,), torch.float32), a=aa, n=n)
        step = out((1,), torch.int32)
        tt = put(tab)
        ctx.ew(L.EW_STEP_SET, step, i=(0, 1, 0, 0, 0, 0))
        y_first = ctx.ew(L.EW_STEP_ROW, out((n,), dtype), a=tt, step=step, n=n)
        ctx.ew(L.EW_STEP_SET, step, i=(rows - 2, 1, 0, 0, 0, 0))
        ctx.ew(L.EW_STEP_SET, step, i=(0, 0, 0, 0, 0, 0))                    # + 1 -> the last row
        y_last = ctx.ew(L.EW_STEP_ROW, out((n,), dtype), a=tt, step=step, n=n)
        return y_add, y_silu, y_cat, y_f32, y_first, y_last, step
    y_add, y_silu, y_cat, y_f32, y_first, y_last, step = run(dtype, body, f"flat elementwise ops n={n}")
    assert_close(y_add, a.float() + b.float(), dtype, "add", k=2.0)
    assert_close(y_silu, F.silu(a.float()), dtype, "silu", k=2.0)
    assert torch.equal(y_cat, torch.cat([a.view(n // 8, 8), b.view(n // 8, 8)], -1))
    assert torch.equal(y_f32, a.float())
    assert torch.equal(y_first, tab[0]) and torch.equal(y_last, tab[rows - 1]) and step.item() == rows - 1


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("chan", [4, 9])
@pytest.mark.parametrize("C0", [8, 64, 320])
@pytest.mark.parametrize("H,W", [(3, 5), (16, 12)])
def test_ew_conv_in(L, dtype, chan, C0, H, W):
    S = 2
    lat = torch.randn(S, 4, H, W, generator=torch.Generator().manual_seed(1)).to(DEV)
    x2 = torch.randn(S, 5, H, W, generator=torch.Generator().manual_seed(2)).to(DEV)
    w, bias = rnd(C0, chan, 3, 3, dtype=dtype, seed=3, scale=1 / 6), rnd(C0, dtype=dtype, seed=4)

    def body(ctx, put, out):
        kw = dict(x2=put(x2)) if chan == 9 else {}
        return ctx.ew(L.EW_CONV_IN, out((2 * S, H, W, C0), dtype), a=put(lat), w=put(w), bias=put(bias), i=(S, H, W, C0, 2 * S, chan if chan == 9 else 0),
                      f=(0.5, 0, 0, 0), **kw)
    xin = (lat * 0.5).to(dtype).float()
    if chan == 9:
        xin = torch.cat([xin, x2.to(dtype).float()], 1)
    ref = F.conv2d(torch.cat([xin, xin]), w.float(), bias.float(), padding=1).permute(0, 2, 3, 1)
    assert_close(run(dtype, body, f"conv_in {chan} ch C0={C0} {H}x{W}")[0], ref, dtype, "conv_in")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("HW", [1, 60, 1024])
def test_ew_cfg_rescale(L, dtype, HW):
    """against oracle.pipeline.rescale_noise_cfg's factor in fp64, relative 1e-5 (the kernel accumulates in double: anything looser
    would hide a wrong N - 1)"""
    from oracle.pipeline import rescale_noise_cfg
    S, gs_, gr = 3, 5.0, 0.7
    npred = rnd(2 * S, HW, 4, dtype=dtype, seed=5)

    def body(ctx, put, out):
        return ctx.ew(L.EW_CFG_RESCALE, out((S,), torch.float32), a=put(npred), i=(S, HW, 0, 0, 0, 0), f=(0, 0, gs_, gr))
    y = run(dtype, body, f"cfg_rescale HW={HW}")[0]
    n = npred.double().cpu().view(2, S, HW * 4)
    # the kernel forms the guided prediction in fp32 (the value CFG_STEP applies); its std is then taken in double
    cfg = (n[0].float() + gs_ * (n[1].float() - n[0].float())).double()
    out = rescale_noise_cfg(cfg, n[1], gr)
    i = cfg.abs().argmax(dim=1, keepdim=True)
    factor = (out.gather(1, i) / cfg.gather(1, i)).squeeze(1)
    rel = ((y.double().cpu() - factor).abs() / factor.abs()).max().item()
    assert rel <= 1e-5, f"cfg_rescale HW={HW}: relative error {rel:.3e}"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cols", [4, 1000, 1028])
def test_ew_softmax_strided(L, dtype, cols):
    rows = 5
    a = torch.randn(rows, cols, generator=torch.Generator().manual_seed(2)).mul(3.0).to(DEV)
    a[2, min(7, cols - 1)] = 40.0                                 # one dominant score

    def body(ctx, put, out):
        aa, y = put(a, ld=cols + 12), out((rows, cols), dtype, ld=cols + 20)
        return ctx.ew(L.EW_SOFTMAX, y, a=aa, i=(rows, cols, aa.stride(0), y.stride(0), 0, 0), f=(0.25, 0.0, 0.0, 0.0))
    y = run(dtype, body, f"softmax {cols}")[0]
    ref = torch.softmax(a * 0.25, dim=-1)
    assert torch.allclose(y.float(), ref, atol=4e-3 if dtype == torch.bfloat16 else 5e-4, rtol=2e-2)
    assert torch.allclose(y.float().sum(-1), torch.ones(rows, device=DEV), atol=2e-2)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", ["plain", "w", "b", "tables", "blend1", "blendS"])
def test_ew_cfg_step(L, dtype, form):
    """CFG combine + scheduler step (fp32 latents): plain, with the per-sample rescale factor `w`, with the `b` side output, with
    per-step tables + step, and the masked blend with a mask batch of 1 and of S"""
    S, HW = 2, 60
    lat = torch.randn(S, 4, HW, generator=torch.Generator().manual_seed(1)).to(DEV)
    npred = rnd(2 * S, HW, 4, dtype=dtype, seed=5)
    n = npred.float().view(2, S, HW, 4).permute(0, 1, 3, 2)
    eps = n[0] + 5.0 * (n[1] - n[0])
    ca, cb = 0.9, -0.3
    wf = torch.tensor([0.8, 1.1], device=DEV)
    tab = torch.tensor([[0.5, 0.1], [0.9, -0.3], [0.7, 0.2]], device=DEV)
    z, noise = torch.randn(S, 4, HW, generator=torch.Generator().manual_seed(2)).to(DEV), torch.randn(S, 4, HW, generator=torch.Generator().manual_seed(3)).to(DEV)
    nm = 1 if form == "blend1" else S
    mask = (torch.rand(nm, HW, generator=torch.Generator().manual_seed(4)) > 0.5).float().to(DEV)
    btab = torch.tensor([[0.3, 0.4], [0.6, 0.2], [1.0, 0.0]], device=DEV)

    def body(ctx, put, out):
        y = out((S, 4, HW), torch.float32)
        y.copy_(lat)
        kw, i, f = {}, [S, HW, 0, 1, 0, 0], (ca, cb, 5.0, 0)
        if form == "w":
            kw["w"] = put(wf)
        if form in ("tables", "blend1", "blendS"):
            step = out((1,), torch.int32)
            ctx.ew(L.EW_STEP_SET, step, i=(1, 1, 0, 0, 0, 0))
            kw.update(tab=put(tab), step=step)
        if form.startswith("blend"):
            kw.update(x2=put(z), noise=put(noise), mask=put(mask), blend_tab=put(btab))
            i[4] = nm
        side = out((S, 4, HW), torch.float32) if form == "b" else None
        ctx.ew(L.EW_CFG_STEP, y, a=put(npred), b=side, i=tuple(i), f=f, **kw)
        return (y, side) if form == "b" else y
    res = run(dtype, body, f"cfg_step {form}")
    y = res[0]
    if form == "b":
        assert (res[1] - eps).abs().max().item() < 1e-6, "the guided prediction handed out through `b`"
    e = eps * (wf[:, None, None] if form == "w" else 1.0)
    ref = ca * lat + cb * e
    if form.startswith("blend"):
        m = mask[torch.arange(S) % nm][:, None, :]
        ref = (1 - m) * (btab[1, 0] * z + btab[1, 1] * noise) + m * ref
    assert (y - ref).abs().max().item() < 1e-5, f"cfg_step {form}: {(y - ref).abs().max().item():.3e}"


# ------------------------------------------------------------------------------------ fp32 kernels (csrc/f32.hip)
@pytest.mark.parametrize("exact", [1, 0])
def test_f32_gemm_and_conv(L, exact):
    """the f32_gemm shapes of test_f32_ops_against_torch (the ldw slice included) and f32_conv3x3 with up, stride 2 and pad 1, in both
    arithmetic modes, same bounds"""
    from oracle.detfill import det_randn
    lib = L.load()
    tol = 1.0 if exact else 4.0
    lib.imh_debug_set(10, exact)
    try:
        for (M, N, K) in [(300, 200, 64), (128, 3, 1152), (1000, 129, 16), (64, 512, 512)]:
            x, w = det_randn((M, K), 1).to(DEV), det_randn((N, K), 2).to(DEV)
            b, r = det_randn((N,), 3).to(DEV), det_randn((M, N), 4).to(DEV)

            def body(ctx, put, out):
                return ctx.f32_gemm(put(x, ld=K + 16), put(w, ld=K + 4), bias=put(b), residual=put(r, ld=N + 5), out=out((M, N), torch.float32, ld=N + 3))
            y = run(torch.bfloat16, body, f"f32_gemm {(M, N, K)} exact={exact}")[0]
            assert (y.double() - (x.double() @ w.double().t() + b.double() + r.double())).abs().max() < tol * 2e-5 * K ** 0.5 * 4, (M, N, K, tol)
        vt, pr = det_randn((32, 3 * 128), 5).to(DEV), det_randn((128, 128), 6).to(DEV)
        y = run(torch.bfloat16, lambda ctx, put, out: ctx.f32_gemm(put(pr), put(vt)[:, 128:256], N=32, K=128, ldw=384), f"f32_gemm ldw slice exact={exact}")[0]
        assert (y.double() - pr.double() @ vt[:, 128:256].double().t()).abs().max() < tol * 1e-3
        for (B, H, W, Cin, Cout) in [(2, 9, 7, 16, 40), (1, 8, 8, 32, 3)]:
            for kw in (dict(), dict(up=1), dict(stride=2), dict(stride=2, pad=1)):
                x = det_randn((B, Cin, H, W), 7).to(DEV)
                w = (det_randn((Cout, Cin, 3, 3), 8) * (9 * Cin) ** -0.5).to(DEV)
                b = det_randn((Cout,), 9).to(DEV)
                xin = F.interpolate(x, scale_factor=2.0, mode="nearest") if kw.get("up") else x
                if kw.get("pad"):
                    ref = F.conv2d(F.pad(xin.double(), (0, 1, 0, 1)), w.double(), b.double(), stride=2)
                else:
                    ref = F.conv2d(xin.double(), w.double(), b.double(), stride=kw.get("stride", 1), padding=1)
                ref = ref.permute(0, 2, 3, 1)
                res = det_randn(tuple(ref.shape), 10).to(DEV)
                xh, wh = x.permute(0, 2, 3, 1).contiguous(), w.permute(0, 2, 3, 1).reshape(Cout, -1).contiguous()
                y = run(torch.bfloat16, lambda ctx, put, out: ctx.f32_conv3x3(put(xh), put(wh), bias=put(b), residual=put(res).view(-1, Cout), **kw),
                        f"f32_conv3x3 {(B, H, W, Cin, Cout)} {kw} exact={exact}")[0]
                assert (y.double() - (ref + res.double())).abs().max() < tol * 5e-5, (B, H, W, Cin, Cout, kw, tol)
    finally:
        lib.imh_debug_set(10, 0)


def test_f32_groupnorm_softmax_img2img_init(L):
    from oracle.detfill import det_randn
    for (B, HW, Cc, silu, off) in [(3, 70, 32, True, -40.0), (1, 1024, 512, False, 300.0)]:
        x = (det_randn((B, HW, Cc), 11) * 0.7 + off).to(DEV)
        g, be = (1 + 0.2 * det_randn((Cc,), 12)).to(DEV), (0.3 * det_randn((Cc,), 13)).to(DEV)
        y = run(torch.bfloat16, lambda ctx, put, out: ctx.f32_groupnorm(put(x), put(g), put(be), 32, 1e-6, silu=silu), f"f32_groupnorm {(B, HW, Cc)}")[0]
        ref = F.group_norm(x.double().permute(0, 2, 1), 32, g.double(), be.double(), 1e-6).permute(0, 2, 1)
        ref = F.silu(ref) if silu else ref
        assert (y.double() - ref).abs().max() < 2e-3, (B, HW, Cc, (y.double() - ref).abs().max().item())
    a = (det_randn((130, 1000), 14) * 30.0).to(DEV)

    def softmax(ctx, put, out):
        aa = put(a.clone(), ld=1012)                               # (the in-place call below overwrites it)
        o = ctx.f32_softmax(aa, out((130, 1000), torch.float32, ld=1004), 0.25)
        ctx.f32_softmax(aa, aa, 0.25)                               # in place, as the decode uses it
        return o, aa
    o, inplace = run(torch.bfloat16, softmax, "f32_softmax")
    assert (o.double() - torch.softmax(a.double() * 0.25, -1)).abs().max() < 2e-6
    assert torch.equal(o, inplace)
    for (M, N, S) in [(1, 1, 1), (2, 2, 6)]:
        h, w = 5, 7
        mom, n1, n2 = det_randn((M, h, w, 8), 21).to(DEV), det_randn((N, 4, h, w), 22).to(DEV), det_randn((S, 4, h, w), 23).to(DEV)
        y = run(torch.bfloat16, lambda ctx, put, out: ctx.img2img_init(out((S, 4, h, w), torch.float32), put(mom), put(n1), put(n2), 0.13025, 0.8, 0.6),
                f"img2img_init {(M, N, S)}")[0]
        md = mom.double()[torch.arange(S) % M].permute(0, 3, 1, 2)
        z = 0.13025 * (md[:, :4] + torch.exp(0.5 * md[:, 4:].clamp(-30, 20)) * n1.double()[torch.arange(S) % N])
        assert torch.allclose(y.double(), 0.8 * z + 0.6 * n2.double(), rtol=1e-5, atol=1e-5)
