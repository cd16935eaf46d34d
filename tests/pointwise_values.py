"""Every value of a 16-bit type through a pointwise site, against float64 (tests/test_pointwise_values_host.py on the CPU,
tests/test_gpu_pointwise_values.py on the device).

A 16-bit type has 65 536 bit patterns; values(T) is every finite one (65 280 for bf16, 63 488 for fp16, +-0 and the subnormals
included).  A site has a float64 statement f and an allowance e(x) >= 0 for the fp32 evaluation inside the kernel; a stored y passes iff

    round_T(f(x) - e(x)) <= y <= round_T(f(x) + e(x))                    (+-0 compare equal, a NaN fails)

i.e. y is the rounding of SOME real within e of the true value -- away from near-ties a single T value, so the criterion has no slack in
T.  The allowances are derived from the instruction sequences of csrc/imh_common.h (module docstring of each e_* below), not fitted to
what a kernel returns.

round_T is ONE rounding from float64: torch converts float64 -> bf16 / fp16 through fp32, which rounds twice (1 + 2^-11 + 2^-30 becomes
1.0 in fp16, not 1 + 2^-10), so the float64 value is first brought to fp32 with round-to-odd -- after which the rounding to T
(exact_operands.expected, round-to-nearest-even from an fp32-exact value) is the correct single rounding.

A plain helper module: no GPU needed to import it, no fixtures, no pytest settings."""
import math
import os
import re

import torch

import exact_operands as exo

SQRT2 = math.sqrt(2.0)
FLOOR = 2.0 ** -120                 # absolute floor of every allowance (exp2 overflow for bf16 x <= -88.7: the kernel returns -0, the truth is <= 2.6e-37)
QGELU_A = 1.702
N_FINITE = {torch.bfloat16: 65280, torch.float16: 63488}
MFMA_SKIPPED_BF16 = 254             # bf16 subnormal inputs (|x| < 2^-126, x != 0): not asked of sites that pass the value through the matrix unit
MIN_NORMAL = {torch.bfloat16: 2.0 ** -126, torch.float16: 2.0 ** -14}


# ------------------------------------------------------------------------------------------------ the value set
def values(dtype):
    """every finite bit pattern of T in bit order (positive half first), as a CPU tensor of dtype T"""
    bits = torch.arange(0, 65536, dtype=torch.int32).to(torch.int16)          # wraps: 0 .. 0x7fff, then 0x8000 .. 0xffff
    v = bits.view(dtype)
    v = v[torch.isfinite(v)].clone()
    assert v.numel() == N_FINITE[dtype]
    return v


def through_mfma(x, dtype):
    """mask of the inputs asked of a site that passes the value through the matrix unit: all but the bf16 subnormals"""
    if dtype == torch.bfloat16:
        return (x.double().abs() >= MIN_NORMAL[dtype]) | (x.double() == 0)
    return torch.ones_like(x, dtype=torch.bool)


def tile_values(v, n):
    """n >= len(v) slots holding every value of v; the extra slots repeat values (from the start of v)"""
    assert n >= v.numel()
    reps = (n + v.numel() - 1) // v.numel()
    return v.repeat(reps)[:n].clone()


# ------------------------------------------------------------------------------------------------ the header's constants
def header_constants():
    """GELU_Q0 .. GELU_Q10 (Q(u) = sum_i Q_i u^i) and GELU_XMAX as the fp32 values csrc/imh_common.h compiles"""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "imagharmony_amd", "csrc", "imh_common.h")
    src = open(path).read()
    q = {}
    for m in re.finditer(r"#define\s+GELU_Q(\d+)\s+(-?[0-9.eE+-]+)f", src):
        q[int(m.group(1))] = float(torch.tensor(float(m.group(2)), dtype=torch.float32))
    assert sorted(q) == list(range(11)), sorted(q)
    m = re.search(r"constexpr\s+float\s+GELU_XMAX\s*=\s*([0-9.eE+-]+)f", src)
    assert m
    xmax = float(torch.tensor(float(m.group(1)), dtype=torch.float32))
    return [q[i] for i in range(11)], xmax


GELU_Q, GELU_XMAX = header_constants()


# ------------------------------------------------------------------------------------------------ one rounding from float64
def round_to_odd_f32(v):
    """float64 -> fp32 with round-to-odd (inexact values take the neighbour whose last bit is set): rounding the result to a narrower
    format gives what rounding v itself would have given"""
    assert v.dtype == torch.float64
    a = v.abs()
    r = a.float()
    assert bool(torch.isfinite(r).all()), "beyond fp32"
    d = a - r.double()
    mag = r.view(torch.int32)
    step = torch.where(d > 0, 1, -1).to(torch.int32)
    mag = torch.where((d != 0) & ((mag & 1) == 0), mag + step, mag)
    return torch.copysign(mag.view(torch.float32), v.float()).double() if v.numel() else v


def round_T(v, dtype):
    """the one correctly rounded T value of float64 v"""
    return exo.expected(round_to_odd_f32(v), dtype)


# ------------------------------------------------------------------------------------------------ statements and allowances (float64)
def f_silu(x, a=1.0):
    """x sigma(a x): SiLU (a = 1), quick-GELU (a = 1.702)"""
    x = x.double()
    return x * torch.sigmoid(a * x)


def e_silu(x, a=1.0):
    """silu_f / qgelu_f = x * rcp(1 + exp2(-x a log2 e)): mul, v_exp_f32, add, v_rcp_f32, mul at one ulp each sum to about 2^-22; the first
    term is over 16 times that and still 64 times below fp16's half-ulp.  Second term: the fp32 rounding of the exponent's argument
    (relative 2^-24, i.e. a |x| 2^-24 absolute in the exponent, four times that allowed) weighted by d ln sigma(a x) / d(a x) = sigma(-a x)"""
    x = x.double()
    return (2.0 ** -18 + a * x.abs() * 2.0 ** -22 * torch.sigmoid(-a * x)) * f_silu(x, a).abs() + FLOOR


def f_qgelu(x):
    return f_silu(x, QGELU_A)


def e_qgelu(x):
    return e_silu(x, QGELU_A)


def f_gelu(x):
    """0.5 x (1 + erf(x / sqrt 2)); through erfc for x < -3, where 1 + erf cancels and float64 would lose the tail"""
    x = x.double()
    return torch.where(x < -3.0, 0.5 * x * torch.special.erfc(-x / SQRT2), 0.5 * x * (1.0 + torch.special.erf(x / SQRT2)))


def e_gelu(x):
    """inside the fit range the documented erf-fit error (5.1e-6, allowed 6e-6) times x / 2, plus the Horner and final-fma rounding;
    beyond it erf is set to +-1 exactly, so the error is x / 2 erfc(|x| / sqrt 2) by construction"""
    x = x.double()
    ax = x.abs()
    fit = torch.where(ax < GELU_XMAX, torch.full_like(ax, 6e-6), 1.01 * torch.special.erfc(ax / SQRT2))
    return 0.5 * ax * fit + 2.0 ** -20 * f_gelu(x).abs() + FLOOR


def f_geglu(val, gate):
    return val.double() * f_gelu(gate)


def e_geglu(val, gate):
    return val.double().abs() * e_gelu(gate) + 2.0 ** -22 * f_geglu(val, gate).abs()


def f_tanh3(u):
    u = u.double()
    return 3.0 * torch.tanh(u / 3.0)


def e_tanh3(u, rel=2.0 ** -18):
    return rel * f_tanh3(u).abs() + FLOOR


def f_relu(x):
    return x.double().clamp_min(0.0)


def f_affine(x, scale, shift):
    return x.double() * scale.double() + shift.double()


def zero(x):
    return torch.zeros_like(x, dtype=torch.float64)


def timestep_angles(t, dim):
    """(a [n, half], relative weight [half]) of diffusers Timesteps(dim, flip_sin_to_cos=True, shift 0) in float64"""
    half = dim // 2
    j = torch.arange(half, dtype=torch.float64, device=t.device)
    ex = math.log(10000.0) * j / half
    return t.double()[:, None] * torch.exp(-ex)[None], ex


def f_timestep(t, dim):
    a, _ = timestep_angles(t, dim)
    return torch.cat([a.cos(), a.sin()], -1)


def e_timestep(t, dim):
    """|a| (ln(10^4) j / half + 2) 2^-22: the fp32 rounding of the exponent's argument, of expf and of the product t f_j, as an error
    of the angle (|d cos| <= |d angle|) -- it covers the angle as diffusers computes it in fp32 as well"""
    a, ex = timestep_angles(t, dim)
    e = a.abs() * (ex + 2.0)[None] * 2.0 ** -22
    return torch.cat([e, e], -1)


# ------------------------------------------------------------------------------------------------ fp32 restatements of the kernel formulas
def _flushed(r):
    """v_exp_f32 / v_rcp_f32 return zero where the result would be an fp32 denormal"""
    return torch.where(r.abs() < 2.0 ** -126, torch.zeros_like(r), r)


def k32_silu(x, a=1.0, scaled=None):
    """silu_f / qgelu_f in fp32, the transcendentals' denormal results flushed as the hardware flushes them.  scaled (silu_f): the
    denominator carried as (1 + 2^t) / 4, so that the reciprocal stays normal up to t = 128; unscaled (qgelu_f) it is zero from
    t = 126 on"""
    x = x.float()
    scaled = (a == 1.0) if scaled is None else scaled
    c = torch.tensor(-a * 1.4426950408889634, dtype=torch.float64).float()
    if scaled:
        t = (x.double() * c.double() - 2.0).float()
        return x * (0.25 * _flushed(1.0 / (0.25 + _flushed(torch.exp2(t)))))
    return x * _flushed(1.0 / (1.0 + _flushed(torch.exp2(x * c))))


def k32_erf_poly(x):
    """the clamped fit xc Q(u(xc^2)) of gelu_erf_f, Horner in fp32 (each fma as a float64 product-sum rounded once)"""
    x = x.float()
    xmax = torch.tensor(GELU_XMAX, dtype=torch.float32)
    xc = torch.minimum(torch.maximum(x, -xmax), xmax)
    ua = (torch.tensor(2.0, dtype=torch.float32) / (xmax * xmax))
    fma = lambda p, q, r: (p.double() * q.double() + r.double()).float()
    u = fma(xc * xc, ua, torch.tensor(-1.0))
    q = torch.full_like(x, GELU_Q[10])
    for i in range(9, -1, -1):
        q = fma(q, u, torch.tensor(GELU_Q[i], dtype=torch.float32))
    return xc * q


def k32_gelu(x):
    x = x.float()
    e = torch.where(x.abs() >= GELU_XMAX, torch.copysign(torch.ones_like(x), x), k32_erf_poly(x))
    h = 0.5 * x
    return (h.double() * e.double() + h.double()).float()


def k32_tanh3(u):
    u = u.float()
    return 3.0 * torch.tanh(u / 3.0)


# ------------------------------------------------------------------------------------------------ the comparator
def offenders(x, y, f, e, dtype):
    """bool mask of the stored y outside [round_T(f - e), round_T(f + e)]"""
    f, e = f.double(), e.double()
    assert tuple(y.shape) == tuple(f.shape) == tuple(e.shape), (tuple(y.shape), tuple(f.shape), tuple(e.shape))
    assert y.dtype == dtype and bool((e >= 0).all())
    lo, hi = round_T(f - e, dtype).double(), round_T(f + e, dtype).double()
    yd = y.double()
    return ~((yd >= lo) & (yd <= hi)), lo, hi


def check(x, y, f, e, what, dtype=None, mask=None):
    """x: the value each element was computed from (same shape as y, for the report); mask: the elements asked (None: all).
    -> the number of elements compared; raises AssertionError with the count and the first offenders (index, column residue mod 16)"""
    dtype = dtype or y.dtype
    bad, lo, hi = offenders(x, y, f, e, dtype)
    if mask is not None:
        bad &= mask.to(bad.device)
    n = int(bad.sum())
    asked = int(mask.sum()) if mask is not None else y.numel()
    if n:
        rows = []
        for ix in bad.nonzero()[:6]:
            ix = tuple(int(i) for i in ix)
            rows.append(f"{ix} (col % 16 = {ix[-1] % 16}): x = {float(x[ix])!r}, got {float(y[ix])!r}, allowed [{float(lo[ix])!r}, {float(hi[ix])!r}]")
        raise AssertionError(f"{what}: {n} of {asked} values outside the rounded interval; first: " + "; ".join(rows))
    return asked


def ambiguous(f, e, dtype, floor=2.0 ** -110):
    """how many inputs have an interval that holds more than one T value while |f| > 2^-110"""
    f, e = f.double(), e.double()
    return int(((round_T(f - e, dtype).double() != round_T(f + e, dtype).double()) & (f.abs() > floor)).sum())


# ------------------------------------------------------------------------------------------------ layouts of the GEMM sites
GEMM_M, GEMM_K = 1030, 64            # 1024 rows hold the value set; 1030 is ragged against every tile height, the extra rows repeat values


def value_index(n_slots, n_values):
    """index into values(T) of every slot: the whole set in order, then repeats"""
    assert n_slots >= n_values
    return torch.arange(n_slots) % n_values


def act_source(N):
    """source column of every output column under w[n, (n + n // 64) % 64] = 1: each of the 64 sources at all four residues mod 4 and at
    several mod 16 once N reaches 256"""
    n = torch.arange(N)
    return (n + n // 64) % 64


def onehot(N, K, src, dtype):
    w = torch.zeros(N, K, dtype=dtype)
    w[torch.arange(N), src] = 1.0
    return w


def geglu_sources(N):
    """GF_GEGLU reads its N pre-activation columns in (value, value, gate, gate) quads and writes N / 2 outputs: output o = 2 k + s takes
    value column 4 k + s and gate column 4 k + 2 + s.  -> (source column in [0, 128) of every pre-activation column, gate source in
    [0, 64) of every output column): gate sources are act_source over the output index, so a swept value that sits in the first gate slot
    of a quad in the first 64 outputs sits in the second in the next 64; value columns read the multiplier half, 64 + the same index"""
    assert N % 4 == 0
    n = torch.arange(N)
    o = (n // 4) * 2 + (n % 2)
    src = (o + o // 64) % 64
    return torch.where(n % 4 < 2, src + 64, src), act_source(N // 2)


def multipliers(M, dtype, seed=9):
    """one multiplier per row with every mantissa bit of T in use, 0.5 <= |m| <= 1: the product with the largest finite gate stays finite"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    m = (0.5 + 0.5 * torch.rand(M, generator=g)).to(dtype)
    return torch.where(torch.rand(M, generator=g) < 0.5, -m, m)


def place_for_scales(v, n_slots, scale_of_slot, dtype):
    """index into v of every slot such that every value whose double would leave T's range sits in a slot with scale <= 1"""
    lim = float(torch.finfo(dtype).max) / 2 - 1.0
    big = (v.double().abs() > lim).nonzero().flatten()
    rest = (v.double().abs() <= lim).nonzero().flatten()
    safe = (scale_of_slot <= 1).nonzero().flatten()
    other = (scale_of_slot > 1).nonzero().flatten()
    assert safe.numel() >= big.numel()
    pad = n_slots - v.numel()
    order = torch.cat([big, rest, rest[:pad]])
    idx = torch.empty(n_slots, dtype=torch.long)
    idx[torch.cat([safe, other])] = order
    return idx
