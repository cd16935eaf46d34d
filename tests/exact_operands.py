"""Operands for which a GEMM or conv3x3 launch has ONE right answer (tests/test_gpu_exact_gemm.py, test_gpu_exact_conv.py, the exact mode of
the cells of tests/dispatch_matrix.py; the conditions on these inputs are checked on the CPU by tests/test_exact_operands_host.py).

Weights are integers of [-32, 32] over 32, activations integers of [-64, 64] over 32 (with [-32, 32] the sums of a K = 128 launch stay so
small that fp16 holds 62 % of them exactly; the wider range brings the share that is rounded above one half for every K >= 128), the bias
integers of [-128, 128] over 1024, the residual and the row-add integers of [-128, 128] over 16: every value is exact in bf16 and in fp16,
every product is a multiple of 2^-10, and as long as 2 K + 16.125 < 2^12 every partial sum of the launch -- in any order, split-K partials
and the epilogue's adds included -- is a multiple of 2^-10 below 2^12: at most 22 significant bits, exact in fp32 with two bits to spare for
however the MFMA aligns its addends.  The fp32 accumulator therefore holds the float64 statement exactly, the kernel's one rounding to T has one correct result (torch's round-to-nearest-even), and the comparison is
equality: nothing is measured, so there is no tolerance to choose.  assert_exact_in_fp32 is the premise as an assert on the operands
themselves; every exact case calls it, so a shape that breaks the premise fails on the premise and not on the kernel.

(float64 -> T in torch goes through fp32; the statement's values are exact in fp32, so that is still one rounding.)

A plain helper module: no GPU needed to import it, no fixtures, no pytest settings."""
import torch
import torch.nn.functional as F

ACT_N, BIAS_N, ADD_N = 32, 1024, 16          # grids: activations / weights k / 32, bias k / 1024, residual and row-add k / 16 ...
ACT_K, BIAS_K, ADD_K = 64, 128, 128          # ... activations with |k| <= 64 (weights <= 32), the latter two with |k| <= 128
LSB, TOP = 10, 12                            # every partial sum: a multiple of 2^-LSB below 2^TOP

# K_DEEP: more K tiles (of 64) than twice the deepest operand ring of any variant -- four slots (gemm_ring.hip: the wave-specialised 64 x 160 and
# 128 x 160 tiles and the 4064 / 6064 rings; gemm_pp.hip and gemm_w16.hip hold two buffers) -> nine tiles
K_DEEP = 576
GEMM_SHAPES = [(512, 640, 128), (300, 200, 192), (2, 320, 64), (192, 160, K_DEEP)]
GEMM_FEATURES = ["none", "bias", "residual", "residual_inplace", "bias_residual", "rowadd", "out_f32", "vt_perm", "x2"]
CONV_FEATURES = ["s1", "s2", "pad1", "up1", "up2", "residual", "rowadd", "x2", "gn_affine"]
TINY_PATCH = (1, 3, 5, 64, 8)                # [B, H, W, Cin, Cout]: smaller than any tile


def gemm_shapes(feat):
    """the four shapes under the feature's own rule: the V^T layout permutes whole 16-key groups (N = 208 for 200), two token sources are
    at least 64 columns each (K = 128 for 64)"""
    out = []
    for M, N, K in GEMM_SHAPES:
        if feat == "vt_perm" and N % 16:
            N = (N + 15) // 16 * 16
        if feat == "x2" and K < 128:
            K = 128
        out.append((M, N, K))
    return out


# ------------------------------------------------------------------------------------------------ generators
def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def grid(shape, n=ACT_N, seed=0, dtype=torch.float64, kmax=None):
    """integers of [-kmax, kmax] (kmax = n unless given) over n, n a power of two: exact in bf16 and fp16 for kmax <= 256"""
    assert n & (n - 1) == 0 and (kmax or n) <= 256
    kmax = n if kmax is None else kmax
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    k = torch.randint(-kmax, kmax + 1, shape, generator=_gen(seed))
    return (k.double() / n).to(dtype)


def bias_grid(shape, seed, dtype):
    return grid(shape, BIAS_N, seed, dtype, kmax=BIAS_K)


def add_grid(shape, seed, dtype):
    return grid(shape, ADD_N, seed, dtype, kmax=ADD_K)


def full_mantissa(shape, seed, dtype):
    """normals that use every mantissa bit of T, none closer to zero than 2^-8 (normal in fp16, where a tile may flush a subnormal)"""
    x = torch.randn(tuple(shape), generator=_gen(seed))
    x = torch.where(x.abs() < 2.0 ** -8, torch.copysign(torch.tensor(2.0 ** -8), x), x)
    return x.to(dtype)


def channel_map(n_out, n_in, seed):
    """source channel of every output channel: a permutation where n_out == n_in, else a permutation repeated / cut to n_out"""
    perm = torch.randperm(n_in, generator=_gen(seed))
    return perm.repeat((n_out + n_in - 1) // n_in)[:n_out]


# ------------------------------------------------------------------------------------------------ the premise
def _lsb(t):
    """smallest e with t * 2^e all integers"""
    v = t.detach().double().abs().cpu()
    for e in range(0, 40):
        s = v * 2.0 ** e
        if bool((s == s.floor()).all()):
            return e
    raise AssertionError("operand is not on a binary grid")


def assert_exact_in_fp32(K, x, w, *adds):
    """every possible partial sum of sum_k x[., k] w[., k] (+ adds) over K terms is a multiple of 2^-10 below 2^12 (22 significant bits):
    x, w and every epilogue addend are given as the tensors the launch reads"""
    ex, ew = _lsb(x), _lsb(w)
    assert ex + ew <= LSB, f"products are multiples of 2^-{ex + ew}, finer than 2^-{LSB}"
    top = K * float(x.detach().abs().max()) * float(w.detach().abs().max())
    for t in adds:
        if t is None:
            continue
        assert torch.isfinite(t).all()
        assert _lsb(t) <= LSB, f"an addend is on a grid finer than 2^-{LSB}"
        top += float(t.detach().abs().max())
    assert top < 2.0 ** TOP, f"a partial sum can reach {top}, not below 2^{TOP}"


# ------------------------------------------------------------------------------------------------ expected value, comparison
def expected(ref64, dtype):
    """the one correctly rounded value: torch's round-to-nearest-even (fp32 outputs: ref64.float(), exact under the premise)"""
    assert ref64.dtype == torch.float64
    return ref64.float() if dtype == torch.float32 else ref64.to(dtype)


def ulp(ref, dtype):
    """one unit in the last place of `dtype` at the float64 values `ref`"""
    mant, emin = {torch.float16: (10, -14), torch.bfloat16: (7, -126), torch.float32: (23, -126)}[dtype]
    e = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** emin))).clamp_min(emin)
    return torch.pow(torch.tensor(2.0, dtype=torch.float64, device=ref.device), e - mant)


def unrepresentable(ref64, dtype):
    """fraction of the statement's values that T does not hold: where the one rounding is exercised"""
    return float((ref64.to(dtype).double() != ref64).double().mean())


def assert_equal(y, want, what):
    """value equality of every element (-0 == +0, a NaN fails); the message carries the count, the worst difference in units of the last
    place of `want` and the first differing index -- for a tile bug the row and column"""
    assert tuple(y.shape) == tuple(want.shape) and y.dtype == want.dtype, f"{what}: {tuple(y.shape)} {y.dtype}, expected {tuple(want.shape)} {want.dtype}"
    yd, wd = y.double(), want.double().to(y.device)
    bad = ~(yd == wd)
    n = int(bad.sum())
    if n:
        d = (yd - wd).abs() / ulp(wd, want.dtype)
        d = torch.where(torch.isfinite(d), d, torch.full_like(d, float("inf")))
        idx = tuple(int(i) for i in bad.nonzero()[0])
        last = tuple(int(i) for i in bad.nonzero()[-1])
        raise AssertionError(f"{what}: {n} of {bad.numel()} elements differ, worst {float(d[bad].max()):.1f} ulp, first at {idx} "
                             f"(got {float(yd[idx])!r}, expected {float(wd[idx])!r}), last at {last}")


# ------------------------------------------------------------------------------------------------ float64 statements
def gemm_statement(x, w, bias=None, rowadd=None, rows_per_batch=0, residual=None):
    """x [M, K] w [N, K]^T (+ bias [N]) (+ rowadd [batches, N] by row // rows_per_batch) (+ residual [M, N]) in float64"""
    acc = x.double() @ w.double().t()
    if bias is not None:
        acc = acc + bias.double()
    if rowadd is not None:
        acc = acc + rowadd.double()[torch.arange(x.shape[0], device=x.device) // rows_per_batch]
    if residual is not None:
        acc = acc + residual.double()
    return acc


def conv_statement(x, w4, bias=None, stride=1, up=0, pad=0, fill=None):
    """NHWC x, w4 [Cout, Cin, 3, 3] -> NHWC float64 conv3x3 as explicit padding + im2col + matmul.  up: nearest x2 first; pad = 0: one pixel of
    padding on every side, 1: on the right / bottom only (stride 2); fill [B, Cin]: the value the padding holds (None: zero, the conv's)"""
    xin = x.double().permute(0, 3, 1, 2)
    if up:
        xin = xin.repeat_interleave(2, 2).repeat_interleave(2, 3)
    B, C, H, W = xin.shape
    lo = 0 if pad else 1
    p = torch.zeros(B, C, H + lo + 1, W + lo + 1, dtype=torch.float64, device=x.device)
    if fill is not None:
        p += fill.double()[:, :, None, None]
    p[:, :, lo:lo + H, lo:lo + W] = xin
    cols = F.unfold(p, 3, padding=0, stride=stride)
    Ho, Wo = (H + lo - 2) // stride + 1, (W + lo - 2) // stride + 1
    y = (w4.double().reshape(w4.shape[0], -1) @ cols).view(B, w4.shape[0], Ho, Wo)
    if bias is not None:
        y = y + bias.double()[None, :, None, None]
    return y.permute(0, 2, 3, 1)


def taps_inside(n_in, stride=1, up=0, pad=0):
    """per output index along one axis, how many of the three taps fall inside the image: positions stride * o + k - lo, k = 0 .. 2, of
    an axis of n_in << up pixels -> int64 [n_out]"""
    nv = n_in << (1 if up else 0)
    lo = 0 if pad else 1
    n_out = (nv + lo - 2) // stride + 1
    o = torch.arange(n_out)
    return sum((((stride * o + k - lo) >= 0) & ((stride * o + k - lo) < nv)).long() for k in range(3))


def affine(x, table, dtype):
    """fma(x, scale, shift) per (sample, channel) of a [B, Cin, 2] table over NHWC x, in float64, stored in T (exact by construction)"""
    v = x.double() * table[:, None, None, :, 0].double() + table[:, None, None, :, 1].double()
    assert bool((v.to(dtype).double() == v).all())
    return v.to(dtype)


# ------------------------------------------------------------------------------------------------ operands of the cells
def gemm_operands(feat, shape, dtype):
    """CPU operands of one exact GEMM cell (seeds as the cells': x 1, w 2, bias 3, residual 4, row-add 5): dict with x, w and where the
    feature has them bias [N], residual [M, N], rowadd [3, N + 64] (the launch reads columns 32 .. 32 + N) and rows_per_batch"""
    M, N, K = shape
    o = dict(x=grid((M, K), ACT_N, 1, dtype, kmax=ACT_K), w=grid((N, K), ACT_N, 2, dtype), bias=None, residual=None, rowadd=None, rows_per_batch=0)
    if feat in ("bias", "bias_residual"):
        o["bias"] = bias_grid(N, 3, dtype)
    if feat in ("residual", "residual_inplace", "bias_residual"):
        o["residual"] = add_grid((M, N), 4, dtype)
    if feat == "rowadd":
        o["rowadd"], o["rows_per_batch"] = add_grid((3, N + 64), 5, dtype), (M + 2) // 3
    return o


def gemm_operands_statement(o):
    N = o["w"].shape[0]
    return gemm_statement(o["x"], o["w"], o["bias"], None if o["rowadd"] is None else o["rowadd"][:, 32:32 + N], o["rows_per_batch"], o["residual"])


def conv_geometry(feat):
    """(stride, up, pad) of a conv feature (up: the statement's, nearest x2 or not)"""
    return (2 if feat in ("s2", "pad1") else 1), int(feat in ("up1", "up2")), int(feat == "pad1")


def conv_operands(feat, shape, dtype):
    """CPU operands of one exact conv cell: x NHWC, w4 [Cout, Cin, 3, 3], bias, and residual [B, Ho, Wo, Cout] / rowadd [B, Cout + 64] /
    table [B, Cin, 2] fp32 where the feature has them.  gn_affine: x on k / 16, scales of {0.5, 1, 2}, nonzero shifts k / 16 with |k| <= 16,
    both different from channel to channel and from sample to sample -- the staged halo fma(x, scale, shift) is on k / 32 below 3, exact in T"""
    if feat == "x2" and shape[3] < 128:
        shape = shape[:3] + (128,) + shape[4:]
    B, H, W, Cin, Cout = shape
    stride, up, pad = conv_geometry(feat)
    o = dict(shape=shape, x=grid((B, H, W, Cin), ACT_N, 1, dtype, kmax=ACT_K), w4=grid((Cout, Cin, 3, 3), ACT_N, 2, dtype), bias=bias_grid(Cout, 3, dtype),
             residual=None, rowadd=None, table=None)
    lo = 0 if pad else 1
    Ho, Wo = ((H << up) + lo - 2) // stride + 1, ((W << up) + lo - 2) // stride + 1
    if feat == "residual":
        o["residual"] = add_grid((B, Ho, Wo, Cout), 5, dtype)
    if feat == "rowadd":
        o["rowadd"] = add_grid((B, Cout + 64), 4, dtype)
    if feat == "gn_affine":
        o["x"] = grid((B, H, W, Cin), 16, 1, dtype)
        scale = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (B, Cin), generator=_gen(11))]
        k = torch.randint(1, 17, (B, Cin), generator=_gen(12)) * (torch.randint(0, 2, (B, Cin), generator=_gen(13)) * 2 - 1)
        o["table"] = torch.stack([scale, k.float() / 16], -1).contiguous()
    return o


def conv_operands_statement(feat, o, dtype):
    """-> (float64 statement, the activations the MFMAs read: x, or the staged halo of gn_affine)"""
    stride, up, pad = conv_geometry(feat)
    xin = o["x"] if o["table"] is None else affine(o["x"], o["table"], dtype)
    ref = conv_statement(xin, o["w4"], o["bias"], stride, up, pad)
    if o["residual"] is not None:
        ref = ref + o["residual"].double()
    if o["rowadd"] is not None:
        ref = ref + o["rowadd"][:, 32:32 + o["w4"].shape[0]].double()[:, None, None, :]
    return ref, xin


# the fp32 tail (csrc/f32.hip): ragged M and N, N = 3, K = 16 .. 1152; [B, H, W, Cin, Cout, up, stride, pad]
F32_GEMM_SHAPES = [(300, 200, 64), (128, 3, 1152), (1000, 129, 16)]
F32_CONV_CASES = [(1, 8, 8, 32, 3, 1, 1, 0), (2, 9, 7, 16, 40, 0, 2, 1), (1, 16, 12, 64, 130, 0, 1, 0), (2, 9, 7, 16, 40, 1, 1, 0)]


def f32_gemm_operands(shape):
    """fp32 operands on the same grids: representable in bf16, so the hi / lo split of the default arithmetic mode has lo = 0"""
    M, N, K = shape
    f = torch.float32
    return grid((M, K), ACT_N, 1, f, kmax=ACT_K), grid((N, K), ACT_N, 2, f), bias_grid(N, 3, f), add_grid((M, N), 4, f)


def f32_conv_operands(case):
    B, H, W, Cin, Cout, up, stride, pad = case
    f = torch.float32
    lo = 0 if pad else 1
    Ho, Wo = ((H << up) + lo - 2) // stride + 1, ((W << up) + lo - 2) // stride + 1
    return grid((B, H, W, Cin), ACT_N, 7, f, kmax=ACT_K), grid((Cout, Cin, 3, 3), ACT_N, 8, f), bias_grid(Cout, 9, f), add_grid((B, Ho, Wo, Cout), 10, f)


def cancelling_residual(pre64, dtype, seed=5):
    """residual = round_T(noise - pre), noise = +-k 2^-10 with k in 32 .. 96: the sum is the noise plus the residual's own rounding, a
    multiple of 2^-10 -- a kernel that rounds `pre` (acc + bias) to T before it adds the residual is off by up to half a unit of `pre`"""
    g = _gen(seed)
    k = torch.randint(32, 97, tuple(pre64.shape), generator=g).double()
    sign = torch.randint(0, 2, tuple(pre64.shape), generator=g).double() * 2 - 1
    return ((k * sign * 2.0 ** -LSB).to(pre64.device) - pre64).to(dtype)


# ------------------------------------------------------------------------------------------------ negative controls (what a wrong kernel returns)
def control_round_before_residual(pre64, residual, dtype):
    """(a) acc + bias rounded to T before the residual is added"""
    return (pre64.to(dtype).double() + residual.double()).to(dtype)


def control_drop_last_k(ref64, x, w):
    """(b) the last K element dropped, for the last output row only"""
    out = ref64.clone()
    out[-1] -= x[-1, -1].double() * w[:, -1].double()
    return out


def control_swap_taps(ref64, x, w4, bias=None, stride=1, up=0, pad=0):
    """(c) taps (ky, kx) and (kx, ky) swapped, for the first output row only"""
    out = ref64.clone()
    out[:, 0] = conv_statement(x, w4.transpose(2, 3), bias, stride, up, pad)[:, 0]
    return out


def control_shift_in_padding(x, table, w4, bias, dtype):
    """(d) the fused normalisation table's shift also applied to the zero padding"""
    return conv_statement(affine(x, table, dtype), w4, bias, fill=table[:, :, 1])
