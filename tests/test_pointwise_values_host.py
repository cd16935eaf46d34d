"""CPU: the every-value criterion of tests/pointwise_values.py, before it is asked of a kernel (tests/test_gpu_pointwise_values.py).

For every function and both 16-bit types: an fp32 restatement of the kernel's formula (coefficients read from csrc/imh_common.h) passes at
every finite value; the share of inputs whose interval holds more than one T value stays under the cap (1 % for SiLU / quick-GELU / tanh,
5 % for GELU: the criterion decides all but those by a single T value); the header's polynomial meets its documented bounds at every T
value.  Then the faults the k * EPS * max|ref| bound lets through -- a tanh-form GELU, a sigmoid rounded to T before the multiply, small
results flushed, another activation, one wrong column in sixteen, one wrong row in sixty-four -- are each refused, in both types."""
import math

import pytest
import torch
import torch.nn.functional as F

import pointwise_values as pv

DTYPES = [torch.bfloat16, torch.float16]
FUNCS = {
    # name: (statement, allowance, fp32 restatement, cap on the ambiguous share)
    "silu": (pv.f_silu, pv.e_silu, pv.k32_silu, 0.01),
    "qgelu": (pv.f_qgelu, pv.e_qgelu, lambda x: pv.k32_silu(x, pv.QGELU_A), 0.01),
    "gelu": (pv.f_gelu, pv.e_gelu, pv.k32_gelu, 0.05),
    "tanh3": (pv.f_tanh3, pv.e_tanh3, pv.k32_tanh3, 0.01),
}
_CACHE = {}


def table(name, dtype):
    """(values, statement, allowance) of one function and type, computed once"""
    if (name, dtype) not in _CACHE:
        v = pv.values(dtype)
        _CACHE[name, dtype] = (v, FUNCS[name][0](v), FUNCS[name][1](v))
    return _CACHE[name, dtype]


def refused(x, y, f, e, what):
    """the comparator raises; -> the number of offenders it counted"""
    with pytest.raises(AssertionError, match="outside the rounded interval") as info:
        pv.check(x, y, f, e, what)
    return int(str(info.value).split(": ")[1].split(" of ")[0])


# ------------------------------------------------------------------------------------------------ the value set and the rounding
def test_value_set_is_every_finite_pattern():
    for dtype, n, subn in ((torch.bfloat16, 65280, 254), (torch.float16, 63488, 2046)):
        v = pv.values(dtype)
        assert v.numel() == n and v.view(torch.int16).unique().numel() == n and bool(torch.isfinite(v).all())
        assert int((v == 0).sum()) == 2 and int(torch.signbit(v[v == 0]).sum()) == 1
        sub = (v.double().abs() < pv.MIN_NORMAL[dtype]) & (v != 0)
        assert int(sub.sum()) == subn
    assert pv.MFMA_SKIPPED_BF16 == 254 and int((~pv.through_mfma(pv.values(torch.bfloat16), torch.bfloat16)).sum()) == 254
    assert bool(pv.through_mfma(pv.values(torch.float16), torch.float16).all())


def test_round_T_rounds_once():
    """torch's float64 -> fp16 goes through fp32 and rounds twice; round_T does not"""
    x = torch.tensor([1 + 2.0 ** -11 + 2.0 ** -30, 1 + 2.0 ** -11, 1 + 2.0 ** -11 - 2.0 ** -40, -(1 + 3 * 2.0 ** -11 - 2.0 ** -40)], dtype=torch.float64)
    assert x.to(torch.float16).tolist() == [1.0, 1.0, 1.0, -(1 + 2.0 ** -9)]          # the first and the last are wrong
    assert pv.round_T(x, torch.float16).tolist() == [1 + 2.0 ** -10, 1.0, 1.0, -(1 + 2.0 ** -10)]
    # exact fp32 values pass unchanged, zeros keep their sign, a value below fp32's range keeps its side of zero
    v = torch.tensor([0.0, -0.0, 3.0, -2.0 ** -149, 1e-60, -1e-60], dtype=torch.float64)
    r = pv.round_to_odd_f32(v)
    assert r[:4].tolist() == v[:4].tolist() and bool(torch.signbit(r[1])) and r[4] == 2.0 ** -149 and r[5] == -2.0 ** -149
    # against exact rational arithmetic on random float64 values near fp16 / bf16 ties
    g = torch.Generator().manual_seed(3)
    for dtype, mant in ((torch.float16, 10), (torch.bfloat16, 7)):
        base = (1 + torch.randint(0, 2 ** mant, (4096,), generator=g).double() * 2.0 ** -mant)          # T values in [1, 2)
        off = (torch.randint(-3, 4, (4096,), generator=g).double() * 2.0 ** -45)
        x = base + 2.0 ** -(mant + 1) + off                                                           # a midpoint, +- a few 2^-45
        up = (off > 0) | ((off == 0) & ((base * 2.0 ** mant) % 2 == 1))
        want = torch.where(up, base + 2.0 ** -mant, base)
        assert torch.equal(pv.round_T(x, dtype).double(), want)


def test_layouts_reach_every_source_and_both_slots():
    for N in (200, 320):
        src = pv.act_source(N)
        assert src.unique().numel() == 64
    src = pv.act_source(320)
    for k in range(64):
        cols = (src == k).nonzero().flatten()
        assert set((cols % 4).tolist()) == {0, 1, 2, 3} and len(set((cols % 16).tolist())) >= 4
    for N in (208, 320):
        pre, gate = pv.geglu_sources(N)
        n = torch.arange(N)
        assert bool((pre[n % 4 < 2] >= 64).all()) and bool((pre[n % 4 >= 2] < 64).all())
        o = (n // 4) * 2 + n % 2
        assert torch.equal(pre[n % 4 >= 2], gate[o[n % 4 >= 2]]) and gate.unique().numel() == 64
    pre, gate = pv.geglu_sources(320)
    for k in range(64):
        assert set(((gate == k).nonzero().flatten() % 2).tolist()) == {0, 1}                          # both gate slots of a quad
    for dtype in DTYPES:
        m = pv.multipliers(pv.GEMM_M, dtype)
        assert bool((m.abs() >= 0.5).all()) and bool((m.abs() <= 1).all()) and m.unique().numel() > 100
        v = pv.values(dtype)
        scale = torch.tensor([0.5, 1.0, 2.0])[torch.arange(65280) % 3]
        idx = pv.place_for_scales(v, 65280, scale, dtype)
        assert idx.unique().numel() == v.numel()
        assert bool(torch.isfinite((v[idx].double() * scale.double() + 1.0).to(dtype)).all())


# ------------------------------------------------------------------------------------------------ the restatements pass, the caps hold
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(FUNCS))
def test_fp32_restatement_passes_and_few_inputs_are_ambiguous(name, dtype):
    v, f, e = table(name, dtype)
    y32 = FUNCS[name][2](v)
    assert pv.check(v, y32.to(dtype), f, e, f"{name} restated in fp32") == pv.N_FINITE[dtype]
    ratio = (y32.double() - f).abs() / e
    amb = pv.ambiguous(f, e, dtype)
    print(f"\n[values] {name} {dtype}: worst err / e {float(ratio.max()):.3f} at x = {float(v[ratio.argmax()])!r}, "
          f"{amb} of {v.numel()} inputs ambiguous ({100.0 * amb / v.numel():.2f} %)")
    assert float(ratio.max()) <= 1.0
    assert amb <= FUNCS[name][3] * v.numel()


def test_reciprocal_flush_needs_the_scaled_denominator():
    """v_rcp_f32 returns 0 for a denormal result: x * rcp(1 + 2^t) is -0 from t = 126 on, and silu(-87.5) = -8.7e-37 is a normal bf16 value
    above the allowance's floor -- the unscaled form is refused at exactly that input (found on the MI355X), the scaled form of silu_f
    passes; quick-GELU is below the floor where its reciprocal flushes, and fp16 has no value that small"""
    v, f, e = table("silu", torch.bfloat16)
    y = pv.k32_silu(v, scaled=False).to(torch.bfloat16)
    assert refused(v, y, f, e, "unscaled SiLU") == 1
    bad, _, _ = pv.offenders(v, y, f, e, torch.bfloat16)
    assert v[bad].tolist() == [-87.5] and y[bad].tolist() == [0.0]
    v, f, e = table("silu", torch.float16)
    assert pv.check(v, pv.k32_silu(v, scaled=False).to(torch.float16), f, e, "unscaled SiLU, fp16") == v.numel()


@pytest.mark.parametrize("dtype", DTYPES)
def test_header_polynomial_meets_its_documented_bounds(dtype):
    """csrc/imh_common.h: |erf error| <= 5.1e-6, |GELU error| <= 1.2e-5 over all x -- at every T value, the fit evaluated in fp32"""
    v = pv.values(dtype)
    x = v.double()
    erf_k = torch.where(x.abs() >= pv.GELU_XMAX, torch.sign(x), pv.k32_erf_poly(v).double())
    erf_err = (erf_k - torch.special.erf(x / pv.SQRT2)).abs()
    inside = x.abs() < pv.GELU_XMAX
    gelu_err = (pv.k32_gelu(v).double() - pv.f_gelu(v)).abs()
    # beyond the fit range the fp32 result x (or 0) is exact; the half-ulp of the fp32 result is no part of the fit's claim
    gelu_fit_err = torch.where(inside, gelu_err, (0.5 * x * (torch.sign(x) + 1) - pv.f_gelu(v)).abs())
    pos = (x < 0) & (pv.k32_gelu(v) > 0)
    print(f"\n[values] GELU fit {dtype}: max |erf error| {float(erf_err.max()):.3e}, max |GELU error| {float(gelu_fit_err.max()):.3e} "
          f"(at x = {float(v[gelu_fit_err.argmax()])!r}); positive for {int(pos.sum())} negative inputs"
          + (f", at most {float(pv.k32_gelu(v)[pos].max()):.2e}" if bool(pos.any()) else ""))
    assert float(erf_err.max()) <= 5.1e-6
    assert float(gelu_fit_err.max()) <= 1.2e-5
    # for the record, not a failure: GELU(x) < 0 for every x < 0, the fit may come out (slightly) positive
    if bool(pos.any()):
        assert float(pv.k32_gelu(v)[pos].max()) <= 1.2e-5


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_affine_in_fp32_rounds_once(dtype):
    """the GroupNorm apply is fma(x, scale, shift) in fp32, then one rounding to T; over the table grid of exact_operands' gn_affine (scales
    0.5 / 1 / 2, shifts k / 16) the fp32 fma never lands on a T tie it was not on, so the stored value is the ONE rounding of the exact
    x scale + shift and the site is compared with e = 0"""
    v = pv.values(dtype)
    lim = float(torch.finfo(dtype).max) / 2 - 1.0
    worst = 0
    for scale in (0.5, 1.0, 2.0):
        x = v[v.double().abs() <= lim] if scale > 1 else v
        for k in list(range(-16, 0)) + list(range(1, 17)):
            exact = x.double() * scale + k / 16.0
            y = exact.float().to(dtype)
            worst += int((y.double() != pv.round_T(exact, dtype).double()).sum())
    assert worst == 0


# ------------------------------------------------------------------------------------------------ seeded faults are refused
def _tanh_gelu(x):
    return F.gelu(x.double(), approximate="tanh")


@pytest.mark.parametrize("dtype", DTYPES)
def test_seeded_faults_are_refused(dtype):
    counts = {}
    v, f, e = table("gelu", dtype)
    counts["tanh-form GELU"] = refused(v, _tanh_gelu(v).to(dtype), f, e, "tanh-form GELU")
    y = pv.k32_gelu(v)
    counts["GELU = 0 for |x| < 1e-5"] = refused(v, torch.where(v.double().abs() < 1e-5, torch.zeros_like(y), y).to(dtype), f, e, "GELU zeroed near 0")
    v, f, e = table("silu", dtype)
    sig_T = torch.sigmoid(v.double()).to(dtype)
    counts["sigmoid rounded to T"] = refused(v, (v.double() * sig_T.double()).to(dtype), f, e, "sigmoid rounded to T before the multiply")
    if dtype == torch.float16:
        y = pv.k32_silu(v).to(dtype)
        counts["results below 2^-14 flushed"] = refused(v, torch.where(y.double().abs() < 2.0 ** -14, torch.zeros_like(y), y), f, e, "fp16 subnormal results flushed")
    v, f, e = table("qgelu", dtype)
    counts["SiLU for quick-GELU"] = refused(v, pv.k32_silu(v).to(dtype), f, e, "SiLU where quick-GELU was asked")
    v, f, e = table("tanh3", dtype)
    counts["hard clamp for 3 tanh(u / 3)"] = refused(v, v.double().clamp(-3, 3).to(dtype), f, e, "hard clamp")
    print(f"\n[values] seeded faults {dtype}: " + ", ".join(f"{k}: {n}" for k, n in counts.items()))
    assert all(n > 0 for n in counts.values())
    assert counts["tanh-form GELU"] >= 150 and counts["sigmoid rounded to T"] >= 500 and counts["GELU = 0 for |x| < 1e-5"] >= 300
    if dtype == torch.float16:
        assert counts["results below 2^-14 flushed"] >= 4000


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("where", ["column 5 of 16", "row 63 of 64"])
def test_a_fault_in_one_lane_position_is_refused_and_located(dtype, where):
    """the value set laid out as the GEMM sites lay it out ([1030, 320] outputs of [1030, 64] inputs): a sigmoid rounded to T in the
    columns c % 16 == 5 only, or in the rows m % 64 == 63 only, is refused and the report names such a position"""
    v, f, e = table("silu", dtype)
    M, K, N = pv.GEMM_M, pv.GEMM_K, 320
    idx = pv.value_index(M * K, v.numel()).view(M, K)[:, pv.act_source(N)]
    x, fo, eo = v[idx], f[idx], e[idx]
    good = pv.k32_silu(x).to(dtype)
    assert pv.check(x, good, fo, eo, "laid out") == M * N
    wrong = (x.double() * torch.sigmoid(x.double()).to(dtype).double()).to(dtype)
    m, c = torch.meshgrid(torch.arange(M), torch.arange(N), indexing="ij")
    hit = (c % 16 == 5) if where.startswith("column") else (m % 64 == 63)
    y = torch.where(hit, wrong, good)
    with pytest.raises(AssertionError, match="outside the rounded interval") as info:
        pv.check(x, y, fo, eo, where)
    bad, _, _ = pv.offenders(x, y, fo, eo, dtype)
    assert bool(bad.any()) and bool((bad & ~hit).sum() == 0)
    first = tuple(int(i) for i in bad.nonzero()[0])
    assert f"{first} (col % 16 = {first[1] % 16})" in str(info.value)
    assert first[1] % 16 == 5 if where.startswith("column") else first[0] % 64 == 63


@pytest.mark.parametrize("dtype", DTYPES)
def test_geglu_and_timestep_statements(dtype):
    """GEGLU: the product of a full-mantissa multiplier and the fp32 GELU restatement passes, a tanh-form gate is refused; the timestep
    sinusoid: cos / sin of the fp32 angle (as diffusers computes it) passes at every integer timestep and both widths"""
    v, f, e = table("gelu", dtype)
    n = v.numel()
    val = pv.multipliers(n, dtype, seed=5)
    fo, eo = pv.f_geglu(val, v), pv.e_geglu(val, v)
    assert bool(((fo - val.double() * f).abs() == 0).all())
    y = (val.float() * pv.k32_gelu(v)).to(dtype)
    assert pv.check(v, y, fo, eo, "GEGLU restated in fp32") == n
    assert refused(v, (val.double() * _tanh_gelu(v)).to(dtype), fo, eo, "GEGLU with a tanh-form gate") > 0
    t = torch.arange(1000, dtype=torch.float32)
    for dim in (320, 256):
        half = dim // 2
        fr = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float32) / half)
        a = t[:, None] * fr[None]
        y = torch.cat([a.cos(), a.sin()], -1).to(dtype)
        x = t[:, None].expand(-1, dim)
        assert pv.check(x, y, pv.f_timestep(t, dim), pv.e_timestep(t, dim), f"timestep {dim}") == 1000 * dim
        swapped = torch.cat([a.sin(), a.cos()], -1).to(dtype)
        assert refused(x, swapped, pv.f_timestep(t, dim), pv.e_timestep(t, dim), "sin and cos swapped") > 0
