"""GPU: every finite value of bf16 and of fp16 through every activation and pointwise site, against float64 (criterion, allowances and
layouts: tests/pointwise_values.py; their CPU side: tests/test_pointwise_values_host.py).

The nonlinear half of a launch was held by assert_close's k * EPS * max|ref| on randn inputs (test_gpu_ops.py), which says nothing about
small outputs: negative tails, fp16 subnormal results, inputs near 0 or past the fit range, one lane position of a vectorised epilogue.
Here a stored y passes iff round_T(f(x) - e(x)) <= y <= round_T(f(x) + e(x)) with f in float64 and e derived from the kernel's
instruction sequence -- away from near-ties one T value.

Sites: the GEMM epilogues (SiLU, erf-GELU, quick-GELU, GEGLU) on every variant Ctx approves, splits 2 / 4 (the reduce kernel's epilogue)
included, at N = 320 (vector path), N = 200 / 208 (ragged last vector) and with an output pitch that is no multiple of 8 (scalar path);
GEGLU behind the folded LayerNorm on the sixteen-wave tile and a wave-specialised tile; Ctx.silu, Ctx.relu, Ctx.gn_apply, EW_CAST_F32;
the fused GroupNorm (+ SiLU) front end of every LDS-halo conv3x3 variant; the tiny VAE head's 3 tanh(u / 3); the timestep sinusoid.
A value reaches a GEMM / conv epilogue exactly: the weight is one-hot, so the fp32 accumulator holds the input value itself.

Exclusion: the matrix unit reads bf16 subnormals as zero, so a site that passes the value through it is not asked the 254 bf16 patterns
with 0 < |x| < 2^-126 (of the value that enters the MFMA: the staged value for the fused front ends).  Every launch runs in the guard
arena of tests/dispatch_matrix.py with the guards checked; every site asserts how many distinct values it compared; the first variant of
each family is also compared with ONE faulted statement, which the comparator must refuse on the kernel's own output."""
import collections

import pytest
import torch
import torch.nn.functional as F

import dispatch_matrix as dm
import exact_operands as exo
import pointwise_values as pv
from conftest import built
from imagharmony_amd.ctx import Ctx
from test_gpu_exact_gemm import SPLIT_K
from test_gpu_gnstats import pack_conv
from test_gpu_ops import BIG_VARIANTS, DEV, DTYPES, L  # noqa: F401

pytestmark = pytest.mark.gpu

GEMM_V = dm.gemm_variants(built(BIG_VARIANTS + SPLIT_K))
HALO_V = dm.conv_variants([])
M, K = pv.GEMM_M, pv.GEMM_K
ODD_PITCH = 3                         # ldy = N + 3: not a multiple of 8 (nor of 2) -> epilogue_fast() is false in every lane, the scalar path stores
COMPARED = collections.OrderedDict()  # (site, dtype) -> distinct values compared (test_zz prints the table)
_REF = {}

STATEMENTS = {"silu": (pv.f_silu, pv.e_silu), "gelu": (pv.f_gelu, pv.e_gelu), "qgelu": (pv.f_qgelu, pv.e_qgelu)}


def ref(name, dtype):
    """(values of T, statement, allowance) on the device, float64, computed once per function and type"""
    if (name, dtype) not in _REF:
        v = pv.values(dtype)
        f, e = STATEMENTS[name]
        _REF[name, dtype] = (v.to(DEV), f(v).to(DEV), e(v).to(DEV))
    return _REF[name, dtype]


def faulted(name, x):
    """one wrong statement per function: what a subtly wrong kernel would compute"""
    x = x.double()
    if name == "silu":
        return x * torch.sigmoid(x).to(torch.bfloat16).double()               # the sigmoid rounded to 8 bits before the multiply
    if name == "qgelu":
        return pv.f_silu(x)                                                    # another activation
    return F.gelu(x, approximate="tanh")                                       # gelu / geglu: the tanh form


def record(site, dtype, idx, mask, n_values, skipped=0):
    """the distinct values a site compared: all of T's finite ones, less the stated exclusion"""
    n = int(torch.unique(idx[mask]).numel())
    assert n == n_values - skipped, f"{site} {dtype}: {n} distinct values compared, expected {n_values} - {skipped}"
    COMPARED[site, str(dtype).replace("torch.", "")] = n
    return n


def skipped_by_mfma(dtype):
    return pv.MFMA_SKIPPED_BF16 if dtype == torch.bfloat16 else 0


def launch(dtype):
    arena = dm.fresh_arena()
    return arena, dm.ArenaCtx(arena, dtype)


def done(arena):
    torch.cuda.synchronize()
    arena.check()


# ------------------------------------------------------------------------------------------------ GEMM epilogues
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("act", ["silu", "gelu", "qgelu"])
def test_gemm_activation_epilogue_every_value(L, dtype, act):
    """x [1030, 64] holds the value set, w[n, (n + n // 64) % 64] = 1: y[m, n] = act(x[m, src(n)]) on every approved variant"""
    flag = {"silu": L.GF_ACT_SILU, "gelu": L.GF_ACT_GELU, "qgelu": L.GF_ACT_QGELU}[act]
    v, fv, ev = ref(act, dtype)
    idx = pv.value_index(M * K, v.numel()).view(M, K).to(DEV)
    x = v[idx]
    failures, ran, odd_refused = [], collections.Counter(), []
    for N, pitch in ((320, 24), (200, 24), (320, ODD_PITCH)):
        src = pv.act_source(N).to(DEV)
        w = pv.onehot(N, K, src.cpu(), dtype).to(DEV)
        io = idx[:, src]
        xs, f, e = v[io], fv[io], ev[io]
        mask = pv.through_mfma(xs, dtype)
        record(f"gemm {act} N={N} ld=N+{pitch}", dtype, io, mask, v.numel(), skipped_by_mfma(dtype))
        for cfg in GEMM_V:
            if not Ctx._variant_ok(cfg[0], cfg[2], flag, 0, 1, False, M, N, False):
                continue
            arena, ctx = launch(dtype)
            out = arena.carve((M, N), dtype, ld=N + pitch)
            try:
                ctx.gemm(arena.place(x, ld=K + 64), arena.place(w, ld=K + 8), out=out, flags=flag, cfg=cfg)
            except L.ImhError as err:
                if pitch != ODD_PITCH or not dm.is_library_refusal(err) or cfg[0] <= 128:
                    raise
                odd_refused.append(cfg)              # (the library may ask a vector-aligned pitch of a big tile: recorded, the plain tiles must run)
                continue
            done(arena)
            what = f"{act} N={N} ld={N + pitch} {cfg}"
            try:
                assert pv.check(xs, out, f, e, what, mask=mask) == int(mask.sum())
            except AssertionError as err:
                failures.append(str(err))
            ran[cfg] += 1
            if cfg == GEMM_V[0] and pitch != ODD_PITCH:
                with pytest.raises(AssertionError, match="outside the rounded interval"):
                    pv.check(xs, out, faulted(act, xs), e, "control: " + what, mask=mask)
    print(f"\n[values] gemm {act} {dtype}: shapes run per variant {dict(ran)}")
    print(f"[values]   refused at ld = N + {ODD_PITCH}: {odd_refused or 'none'}")
    assert all(ran[cfg] + odd_refused.count(cfg) == 3 for cfg in GEMM_V if cfg[0] not in Ctx._W16), dict(ran)
    assert {1, 2, 4} <= {cfg[2] for cfg in ran}
    assert not failures, f"{len(failures)} launches:\n" + "\n".join(failures[:20])


def _geglu_case(dtype, N, mult):
    """x [M, 128] = [values | multipliers], w one-hot in (value, value, gate, gate) quads -> (x, w, gate index, gate value, val, f, e, mask)"""
    v, fv, ev = ref("gelu", dtype)
    Mx = mult.shape[0]
    idx = pv.value_index(Mx * K, v.numel()).view(Mx, K).to(DEV)
    x = torch.cat([v[idx], mult.to(DEV)[:, None].expand(-1, K)], 1).contiguous()
    pre, gate = pv.geglu_sources(N)
    w = pv.onehot(N, 2 * K, pre, dtype).to(DEV)
    io = idx[:, gate.to(DEV)]
    val = mult.to(DEV).double()[:, None].expand(-1, N // 2)
    f = val * fv[io]
    e = val.abs() * ev[io] + 2.0 ** -22 * f.abs()
    return x, w, io, v[io], val, f, e, pv.through_mfma(v[io], dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mult", ["one", "full_mantissa"])
def test_gemm_geglu_epilogue_every_value(L, dtype, mult):
    """GF_GEGLU, K = 128: the swept value in both gate slots of a quad, the multiplier (1, or one full-mantissa value per row) in both
    value slots; out = val * gelu(gate) with e = |val| e_gelu(gate) + 2^-22 |out|"""
    m = torch.ones(M, dtype=dtype) if mult == "one" else pv.multipliers(M, dtype)
    failures, ran, odd_refused = [], collections.Counter(), []
    for N, pitch in ((320, 24), (208, 24), (320, ODD_PITCH)):
        x, w, io, xs, val, f, e, mask = _geglu_case(dtype, N, m)
        record(f"gemm geglu ({mult}) N={N} ld=N/2+{pitch}", dtype, io, mask, pv.N_FINITE[dtype], skipped_by_mfma(dtype))
        for cfg in GEMM_V:
            if not Ctx._variant_ok(cfg[0], cfg[2], L.GF_GEGLU, 0, 1, False, M, N, False):
                continue
            arena, ctx = launch(dtype)
            out = arena.carve((M, N // 2), dtype, ld=N // 2 + pitch)
            try:
                ctx.gemm(arena.place(x, ld=2 * K + 64), arena.place(w, ld=2 * K + 8), out=out, flags=L.GF_GEGLU, cfg=cfg)
            except L.ImhError as err:
                if pitch != ODD_PITCH or not dm.is_library_refusal(err) or cfg[0] <= 128:
                    raise
                odd_refused.append(cfg)
                continue
            done(arena)
            what = f"geglu ({mult}) N={N} ld={N // 2 + pitch} {cfg}"
            try:
                assert pv.check(xs, out, f, e, what, mask=mask) == int(mask.sum())
            except AssertionError as err:
                failures.append(str(err))
            ran[cfg] += 1
            if cfg == GEMM_V[0] and pitch != ODD_PITCH:
                with pytest.raises(AssertionError, match="outside the rounded interval"):
                    pv.check(xs, out, val * faulted("gelu", xs), e, "control: " + what, mask=mask)
    print(f"\n[values] gemm geglu ({mult}) {dtype}: shapes run per variant {dict(ran)}")
    print(f"[values]   refused at ld = N + {ODD_PITCH}: {odd_refused or 'none'}")
    assert all(ran[cfg] + odd_refused.count(cfg) == 3 for cfg in GEMM_V if cfg[0] not in Ctx._W16), dict(ran)
    assert {1, 2, 4} <= {cfg[2] for cfg in ran}
    assert not failures, f"{len(failures)} launches:\n" + "\n".join(failures[:20])


@pytest.mark.parametrize("dtype", DTYPES)
def test_folded_layernorm_geglu_every_value(L, dtype):
    """GF_LN_ROW | GF_GEGLU (the ff.net.0 launch: the own GEGLU code of gemm_w16.hip and of gemm_ring.hip's lean epilogue) on the
    sixteen-wave tile and one wave-specialised tile, M = 1024, N = 640.  Statistics handed in as (sum 0, M2 = K (1 - eps)) with s = c = 0:
    mean = 0, rstd = rsqrt(1 - eps + eps) -- the fold is the identity to two fp32 ulps of the gate and of the value, which the allowance
    covers (e_gelu's fit term leaves 0.9e-6 |x| / 2 beside the documented fit error; 2^-22 |out| is four ulps of the product)"""
    Mx, N, eps = 1024, 640, 1e-5
    ws = [c for c in dm.WS_SET if c in GEMM_V][:1]
    cfgs = [(26256, 320, 1)] + ws
    assert len(cfgs) == 2 and all(c in GEMM_V for c in cfgs)
    x, w, io, xs, val, f, e, mask = _geglu_case(dtype, N, pv.multipliers(Mx, dtype))
    record("folded-LN geglu N=640", dtype, io, mask, pv.N_FINITE[dtype], skipped_by_mfma(dtype))
    flags = L.GF_LN_ROW | L.GF_GEGLU
    stats = torch.tensor([0.0, 2 * K * (1.0 - eps)], dtype=torch.float32).expand(Mx, 1, 2).contiguous().to(DEV)
    zeros = torch.zeros(N, dtype=torch.float32, device=DEV)
    failures = []
    for cfg in cfgs:
        assert Ctx._variant_ok(cfg[0], cfg[2], flags, 0, 1, True, Mx, N, False), cfg
        arena, ctx = launch(dtype)
        out = arena.carve((Mx, N // 2), dtype, ld=N // 2 + 24)
        ln = (arena.place(zeros), arena.place(zeros), eps, (arena.place(stats), 1))
        ctx.gemm(arena.place(x, ld=2 * K + 64), arena.place(w, ld=2 * K + 8), out=out, flags=flags, ln=ln, cfg=cfg)
        done(arena)
        try:
            assert pv.check(xs, out, f, e, f"folded-LN geglu {cfg}", mask=mask) == int(mask.sum())
        except AssertionError as err:
            failures.append(str(err))
        if cfg == cfgs[0]:
            with pytest.raises(AssertionError, match="outside the rounded interval"):
                pv.check(xs, out, val * faulted("gelu", xs), e, f"control: folded-LN geglu {cfg}", mask=mask)
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------ elementwise sites
@pytest.mark.parametrize("dtype", DTYPES)
def test_silu_relu_cast_every_value(L, dtype):
    v, fv, ev = ref("silu", dtype)
    n = v.numel()
    idx = torch.arange(n, device=DEV)
    everything = torch.ones(n, dtype=torch.bool, device=DEV)
    # Ctx.silu
    arena, ctx = launch(dtype)
    y = ctx.silu(arena.place(v.view(-1, 64)))
    done(arena)
    assert pv.check(v, y.view(-1), fv, ev, "ctx.silu") == n
    with pytest.raises(AssertionError, match="outside the rounded interval"):
        pv.check(v, y.view(-1), faulted("silu", v), ev, "control: ctx.silu")
    record("ctx.silu", dtype, idx, everything, n)
    # Ctx.relu: value equality
    arena, ctx = launch(dtype)
    y = ctx.relu(arena.place(v.view(-1, 64)))
    done(arena)
    assert pv.check(v, y.view(-1), pv.f_relu(v), pv.zero(v), "ctx.relu") == n
    with pytest.raises(AssertionError, match="outside the rounded interval"):
        pv.check(v, y.view(-1), v.double().abs(), pv.zero(v), "control: ctx.relu")
    record("ctx.relu", dtype, idx, everything, n)
    # EW_CAST_F32 widens T to fp32 (csrc/elementwise.hip cast_f32_kernel): its input IS a T value, so the fp32 neighbours and the
    # midpoints between T values have no form as inputs of this op; every T value must arrive unchanged, sign of zero included
    arena, ctx = launch(dtype)
    y = ctx.ew(L.EW_CAST_F32, ctx.new(n // 64, 64, dtype=torch.float32), a=arena.place(v.view(-1, 64)), n=n)
    done(arena)
    exo.assert_equal(y, v.float().view(-1, 64), "EW_CAST_F32")
    assert torch.equal(torch.signbit(y), torch.signbit(v.view(-1, 64)))
    record("EW_CAST_F32", dtype, idx, everything, n)


def _gn_case(v, dtype, B, HW, C, affine):
    """x [B, HW, C] holding the value set and its [B, C, 2] table: identity, or the affine grid of exact_operands' gn_affine (scales
    0.5 / 1 / 2, shifts k / 16) with every value whose double leaves T's range in a channel of scale <= 1"""
    n = B * HW * C
    if affine:
        tab = exo.conv_operands("gn_affine", (B, 1, 1, C, 8), dtype)["table"]
        scale_of_slot = tab[:, None, :, 0].expand(B, HW, C).reshape(-1)
        idx = pv.place_for_scales(v.cpu(), n, scale_of_slot, dtype).to(DEV)
    else:
        tab = torch.tensor([1.0, 0.0]).expand(B, C, 2).contiguous()
        idx = pv.value_index(n, v.numel()).to(DEV)
    idx = idx.view(B, HW, C)
    tab = tab.to(DEV)
    x = v[idx]
    u = pv.f_affine(x, tab[:, None, :, 0], tab[:, None, :, 1])
    return x, tab, idx, u


def _gn_statement(u, silu):
    """silu: the SiLU allowance at u = x scale + shift (its second term covers the fp32 rounding of the fma, which enters like the
    rounding of the exponent's argument); else e = 0 (test_exact_affine_in_fp32_rounds_once: the fp32 fma adds no second rounding)"""
    return (pv.f_silu(u), pv.e_silu(u)) if silu else (u, pv.zero(u))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,C", [(5, 64), (1, 320)])
def test_gn_apply_every_value(L, dtype, B, C):
    """Ctx.gn_apply with hand-made tables, SiLU on and off; HW = 204 = 4 * 51: the four-pixel unroll and (C = 320, one pixel per pass and
    thread) its tail"""
    v = pv.values(dtype).to(DEV)
    HW = 204
    assert B * HW * C == 65280
    for affine in (False, True):
        x, tab, idx, u = _gn_case(v, dtype, B, HW, C, affine)
        for silu in (False, True):
            f, e = _gn_statement(u, silu)
            arena, ctx = launch(dtype)
            y = ctx.gn_apply(arena.place(x), arena.place(tab), silu)
            done(arena)
            what = f"gn_apply C={C} {'affine' if affine else 'identity'}{' + SiLU' if silu else ''}"
            assert pv.check(x, y, f, e, what) == x.numel()
            record(what, dtype, idx, torch.ones_like(idx, dtype=torch.bool), v.numel())
            if not affine:
                with pytest.raises(AssertionError, match="outside the rounded interval"):
                    pv.check(x, y, faulted("silu", u) if silu else u * (1 - 2.0 ** -6), e, "control: " + what)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("affine", [False, True])
def test_conv_fused_groupnorm_front_end_every_value(L, dtype, affine):
    """conv3x3(gn=(table, silu)) over [1, 32, 32, 64] holding the value set, centre-tap one-hot weights (the staged value passes the
    MFMAs unchanged), on every LDS-halo variant that fuses the front end: the criterion, and equality with gn_apply's output (csrc/
    imh_halo_norm.h: the in-kernel transform and the apply pass give the same bits; the sign of a zero is lost in the accumulator)"""
    v = pv.values(dtype).to(DEV)
    B, H, W, Cin, Cout = 1, 32, 32, 64, 160
    x, tab, idx, u = _gn_case(v, dtype, B, H * W, Cin, affine)
    src = pv.act_source(Cout).to(DEV)
    w4 = torch.zeros(Cout, Cin, 3, 3, dtype=dtype, device=DEV)
    w4[torch.arange(Cout, device=DEV), src, 1, 1] = 1.0
    wp = pack_conv(w4)
    bias = torch.zeros(Cout, dtype=dtype, device=DEV)         # (acc + 0: the value unchanged)
    probe = Ctx(DEV, dtype)
    cfgs = [c for c in HALO_V if Ctx._variant_ok(c[0], c[2], 0, 1, 1, False, B * H * W, Cout)
            and probe.conv_fuses_gn(B * H * W, Cout, 9 * Cin, cfg=c)]
    assert cfgs, "no LDS-halo variant fuses the front end at this shape"
    failures = []
    for silu in (False, True):
        arena, ctx = launch(dtype)
        staged = ctx.gn_apply(arena.place(x), arena.place(tab), silu).clone()          # [B, HW, Cin]: what the conv stages in LDS
        done(arena)
        f, e = _gn_statement(u, silu)
        io, xo, fo, eo, so = idx[..., src], x[..., src], f[..., src], e[..., src], staged[..., src]
        mask = pv.through_mfma(so, dtype)
        what = f"conv3x3 front end {'affine' if affine else 'identity'}{' + SiLU' if silu else ''}"
        # (bf16: the staged value enters the matrix unit, so its subnormals are the ones left out -- e.g. silu(x) = x / 2 for the
        # smallest normals; the count of distinct inputs compared is printed, not pinned to 65 026)
        COMPARED[what, str(dtype).replace("torch.", "")] = int(torch.unique(io[mask]).numel())
        assert COMPARED[what, str(dtype).replace("torch.", "")] >= v.numel() - 3 * skipped_by_mfma(dtype)
        for cfg in cfgs:
            arena, ctx = launch(dtype)
            y = ctx.conv3x3(arena.place(x.view(B, H, W, Cin)), arena.place(wp.view(9 * Cout, Cin)).view(Cout, 9 * Cin),
                            bias=arena.place(bias), gn=(arena.place(tab), silu), cfg=cfg).view(B, H * W, Cout)
            done(arena)
            try:
                assert pv.check(xo, y, fo, eo, f"{what} {cfg}", mask=mask) == int(mask.sum())
                same = (y.double() == so.double()) | ~mask
                assert bool(same.all()), f"{what} {cfg}: {int((~same).sum())} values differ from gn_apply's"
            except AssertionError as err:
                failures.append(str(err))
            if cfg == cfgs[0] and not affine:
                with pytest.raises(AssertionError, match="outside the rounded interval"):
                    pv.check(xo, y, faulted("silu", xo) if silu else xo.double() * (1 - 2.0 ** -6), eo, "control: " + what, mask=mask)
    print(f"\n[values] conv3x3 front end {dtype}: variants {cfgs}")
    assert not failures, f"{len(failures)} launches:\n" + "\n".join(failures[:20])


# ------------------------------------------------------------------------------------------------ tiny VAE head
@pytest.mark.parametrize("dtype", DTYPES)
def test_tinyvae_head_clamp_every_value(L, dtype):
    """tinyvae_conv(head=True): fp32 NCHW input, 3 tanh(u / 3) rounded to T in the staging, then the conv -- one-hot centre-tap weights
    pass the staged value on.  Inputs: every T value upcast and 4 096 fp32 values between them"""
    v = pv.values(dtype)
    g = torch.Generator().manual_seed(17)
    between = torch.cat([(torch.rand(3072, generator=g) * 24 - 12), torch.randn(1024, generator=g) * 1e-3])
    H = W = 132
    n = 4 * H * W
    u = torch.cat([v.float(), between])
    n_in = u.numel()
    assert n_in == v.numel() + 4096 and n >= n_in
    idx = pv.value_index(n, n_in).to(DEV)
    u = u.to(DEV)[idx].view(1, 4, H, W).contiguous()
    # the head's ReLU is part of the launch (csrc/tinyvae.hip: relu = head || flag), so a weight of +1 shows the non-negative staged
    # values and a weight of -1 the non-positive ones: column n reads channel (n + n // 16) % 4 with sign +1 (n < 32) or -1
    ch = (torch.arange(64) + torch.arange(64) // 16) % 4
    sign = torch.where(torch.arange(64) < 32, 1.0, -1.0)
    assert {(int(c), float(s)) for c, s in zip(ch, sign)} == {(c, s) for c in range(4) for s in (1.0, -1.0)}
    w = torch.zeros(64, 36, dtype=dtype)
    w[torch.arange(64), 16 + ch] = sign.to(dtype)             # K index = (ky * 3 + kx) * 4 + c: the centre tap of channel c
    arena, ctx = launch(dtype)
    y = ctx.tinyvae_conv(arena.place(u), arena.place(w.to(DEV)), head=True)
    done(arena)
    sg = sign.to(DEV).double()
    uo = u[0].permute(1, 2, 0)[..., ch.to(DEV)]               # [H, W, 64]: the input each output element was computed from
    io = idx.view(4, H, W).permute(1, 2, 0)[..., ch.to(DEV)]
    t, e = pv.f_tanh3(uo), pv.e_tanh3(uo)
    shown = sg * t >= 0                                       # where the ReLU passes the staged value on (elsewhere the output is 0)
    f = (sg * t).clamp_min(0.0)
    assert bool((y[0].double()[~shown] == 0).all())
    mask = pv.through_mfma(pv.round_T(t, dtype), dtype) & shown          # the staged value enters the matrix unit
    n_cmp = pv.check(uo, y[0], f, e, "tinyvae head 3 tanh(u / 3)", dtype=dtype, mask=mask)
    assert n_cmp == int(mask.sum())
    COMPARED["tinyvae head", str(dtype).replace("torch.", "")] = int(torch.unique(io[mask]).numel())
    assert COMPARED["tinyvae head", str(dtype).replace("torch.", "")] >= n_in - 2 * skipped_by_mfma(dtype)
    with pytest.raises(AssertionError, match="outside the rounded interval"):
        pv.check(uo, y[0], (sg * uo.double().clamp(-3, 3)).clamp_min(0.0), e, "control: hard clamp", dtype=dtype, mask=mask)


# ------------------------------------------------------------------------------------------------ timestep embedding
def timesteps_under_test():
    """every integer t in 0 .. 999, the timestep tables the product builds (Euler, 30 steps; DPM-Solver++ with Karras sigmas, 30 steps)
    and fractional ones: the 30-step linspace spacing of diffusers' Euler default"""
    from imagharmony_amd.schedulers import DPMSolverMultistepScheduler, EulerDiscreteScheduler
    eu = EulerDiscreteScheduler()
    eu.set_timesteps(30)
    ka = DPMSolverMultistepScheduler(use_karras_sigmas=True)
    ka.set_timesteps(30)
    frac = torch.linspace(0, 999, 30, dtype=torch.float64).flip(0).float()
    assert bool((frac != frac.round()).any())
    return torch.cat([torch.arange(1000, dtype=torch.float32), eu.tables()["timesteps"].float(), ka.timesteps.float(), frac])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", [320, 256])
def test_timestep_embedding_every_timestep(L, dtype, dim):
    t = timesteps_under_test().to(DEV)
    n = t.numel()
    f, e = pv.f_timestep(t, dim), pv.e_timestep(t, dim)
    x = t[:, None].expand(-1, dim)
    arena, ctx = launch(dtype)
    y = ctx.ew(L.EW_TIMESTEP, ctx.new(n, dim), a=arena.place(t), n=n, i=(dim, 0, 0, 0, 0, 0))
    done(arena)
    assert pv.check(x, y, f, e, f"timestep dim={dim}") == n * dim
    with pytest.raises(AssertionError, match="outside the rounded interval"):
        pv.check(x, y, torch.cat([f[:, dim // 2:], f[:, :dim // 2]], -1), e, "control: sin and cos swapped")
    COMPARED[f"timestep dim={dim}", str(dtype).replace("torch.", "")] = n
    # through the step indirection (t = table[*step] for every row): a handful of steps, two rows each
    for s in (0, 1, 500, 999, 1015, n - 1):
        arena, ctx = launch(dtype)
        step = arena.place(torch.tensor([s], dtype=torch.int32, device=DEV))
        y = ctx.ew(L.EW_TIMESTEP, ctx.new(2, dim), a=arena.place(t), step=step, n=2, i=(dim, 0, 0, 0, 0, 0))
        done(arena)
        assert pv.check(x[s:s + 1].expand(2, -1), y, f[s:s + 1].expand(2, -1), e[s:s + 1].expand(2, -1), f"timestep dim={dim} step={s}") == 2 * dim


def test_zz_values_compared_per_site(L):
    """printed for the record: distinct values compared per site in this process"""
    print("\n[values] distinct values compared per site:")
    for (site, dt), n in COMPARED.items():
        print(f"[values]   {site:58s} {dt:9s} {n}")
    for (site, dt), n in COMPARED.items():
        if site.startswith(("gemm", "folded", "ctx.", "EW_", "gn_apply")):
            full = pv.N_FINITE[getattr(torch, dt)]
            assert n == full - (pv.MFMA_SKIPPED_BF16 if dt == "bfloat16" and site.startswith(("gemm", "folded")) else 0), (site, dt, n)
