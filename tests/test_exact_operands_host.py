"""CPU: the inputs of the exact-operand tests (tests/exact_operands.py; test_gpu_exact_gemm.py, test_gpu_exact_conv.py, the fp32 tail in
test_gpu_vae.py) do what they are for.  For every shape and dtype used there: the premise holds (every partial sum exact in fp32), an fp32
evaluation of the statement on the CPU equals the float64 one, most outputs are NOT representable in T (so the one rounding is exercised),
and each negative control -- what a subtly wrong kernel would return -- is flagged by assert_equal.  These are conditions on the inputs, not
tolerances: a shape that misses one is changed, not the cap."""
import pytest
import torch

import exact_operands as exo

DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
CONV_SHAPES = [(2, 16, 16, 64, 160), (1, 12, 20, 128, 200), (1, 16, 32, 64, 160), exo.TINY_PATCH]      # dispatch_matrix.CONV_SHAPES + the tiny patch
CANCEL_SHAPES = [s for s in exo.GEMM_SHAPES if s[2] >= 128]


def _flagged(got, want, what):
    with pytest.raises(AssertionError, match="elements differ"):
        exo.assert_equal(got, want, what)


def test_conv_shapes_are_the_matrix_shapes():
    """... and the statement the conv cells build (dispatch_matrix.conv_ref64) is the one checked here, for every geometry"""
    import dispatch_matrix as dm
    assert dm.CONV_SHAPES == CONV_SHAPES[:3]
    for feat in ("s1", "s2", "pad1", "up1"):
        o = exo.conv_operands(feat, exo.TINY_PATCH, torch.bfloat16)
        stride, up, pad = exo.conv_geometry(feat)
        assert torch.equal(dm.conv_ref64(o["x"], o["w4"], o["bias"], stride, up, pad), exo.conv_statement(o["x"], o["w4"], o["bias"], stride, up, pad))


def test_grid_values_are_exact_in_both_dtypes():
    for n, kmax in ((exo.ACT_N, None), (exo.BIAS_N, exo.BIAS_K), (exo.ADD_N, exo.ADD_K), (16, None)):
        g = exo.grid((64, 257), n, 3, torch.float64, kmax=kmax)
        lim = (kmax or n) / n
        assert float(g.abs().max()) == lim and g.unique().numel() == 2 * (kmax or n) + 1          # the whole range is used
        for dt in DTYPES:
            assert torch.equal(g.to(dt).double(), g)
            assert torch.equal(exo.grid((64, 257), n, 3, dt, kmax=kmax).double(), g)
    x = exo.full_mantissa((300, 64), 1, torch.float16)
    assert float(x.abs().min()) >= 2.0 ** -8 and torch.isfinite(x).all()
    assert exo.channel_map(64, 64, 7).sort().values.tolist() == list(range(64)) and exo.channel_map(200, 64, 7).max() == 63


def test_premise_assert_refuses_what_breaks_it():
    x, w = torch.ones(8, 64), -torch.ones(8, 64)
    x[0, 0] = w[0, 0] = 2.0 ** -5
    b, r = torch.full((8,), 0.125), torch.full((8, 8), -8.0)
    exo.assert_exact_in_fp32(64, x, w)
    exo.assert_exact_in_fp32(4079, x, w, b, r, None, r)                              # 4095.125
    with pytest.raises(AssertionError, match="finer"):
        exo.assert_exact_in_fp32(64, exo.grid((8, 64), 64, 1), w)                   # products on 2^-11
    with pytest.raises(AssertionError, match="finer"):
        exo.assert_exact_in_fp32(64, x, w, exo.grid(8, 256, 3, kmax=255) / 8)       # a bias on 2^-11
    with pytest.raises(AssertionError, match="not below"):
        exo.assert_exact_in_fp32(4096, x, w)
    with pytest.raises(AssertionError, match="not below"):
        exo.assert_exact_in_fp32(4080, x, w, r, r)
    with pytest.raises(AssertionError, match="finer"):
        exo.assert_exact_in_fp32(64, x / 3, w)


def test_assert_equal_reports_count_ulps_and_index():
    want = torch.tensor([[1.0, -0.0, 2.0], [4.0, 8.0, 16.0]], dtype=torch.bfloat16)
    got = want.clone()
    got[0, 1] = 0.0
    exo.assert_equal(got, want, "signed zeros are equal")
    got[1, 1] = 8.0 + 2 ** -4 * 3                                                  # three units of bf16 at 8
    with pytest.raises(AssertionError, match=r"1 of 6 elements differ, worst 3\.0 ulp, first at \(1, 1\)"):
        exo.assert_equal(got, want, "x")
    got[0, 0] = float("nan")
    with pytest.raises(AssertionError, match=r"2 of 6 elements differ, worst inf ulp, first at \(0, 0\)"):
        exo.assert_equal(got, want, "x")
    with pytest.raises(AssertionError):
        exo.assert_equal(want.float(), want, "dtype")
    assert exo.expected(torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8], dtype=torch.float64), torch.bfloat16).tolist() == [1.0, 1.0 + 2.0 ** -6]   # ties to even
    assert exo.expected(torch.tensor([1.0 + 2.0 ** -20], dtype=torch.float64), torch.float32).dtype == torch.float32


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("feat", exo.GEMM_FEATURES)
def test_gemm_inputs(feat, dtype):
    for shape in exo.gemm_shapes(feat):
        M, N, K = shape
        o = exo.gemm_operands(feat, shape, dtype)
        ra = None if o["rowadd"] is None else o["rowadd"][:, 32:32 + N]
        exo.assert_exact_in_fp32(K, o["x"], o["w"], o["bias"], ra, o["residual"])
        ref = exo.gemm_operands_statement(o)
        y32 = o["x"].float() @ o["w"].float().t()
        if o["bias"] is not None:
            y32 = y32 + o["bias"].float()
        if ra is not None:
            y32 = y32 + ra.float()[torch.arange(M) // o["rows_per_batch"]]
        if o["residual"] is not None:
            y32 = y32 + o["residual"].float()
        assert y32.dtype == torch.float32 and torch.equal(y32.double(), ref), (feat, shape)
        assert torch.equal(exo.expected(ref, torch.float32).double(), ref)
        frac = exo.unrepresentable(ref, dtype)
        print(f"gemm {feat} {shape} {dtype}: {frac:.2f} of the outputs are not representable")
        if K >= 128:
            assert frac >= 0.5, (feat, shape, frac)
        # (b) the last K element dropped in the last output row
        _flagged(exo.expected(exo.control_drop_last_k(ref, o["x"], o["w"]), dtype), exo.expected(ref, dtype), f"{feat} {shape} (b)")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gemm_one_rounding_inputs(dtype):
    """(a) on the plain bias_residual cell, and the cancellation case (with a bias, and without one as the in-place cell runs it)"""
    for shape in exo.gemm_shapes("bias_residual"):
        o = exo.gemm_operands("bias_residual", shape, dtype)
        pre = exo.gemm_statement(o["x"], o["w"], o["bias"])
        want = exo.expected(pre + o["residual"].double(), dtype)
        twice = exo.control_round_before_residual(pre, o["residual"], dtype)
        frac = float((twice != want).double().mean())
        print(f"(a) bias_residual {shape} {dtype}: {frac:.3f} of the elements differ")
        assert frac >= 0.05, (shape, frac)
        _flagged(twice, want, f"{shape} (a)")
    for shape in CANCEL_SHAPES:
        o = exo.gemm_operands("bias_residual", shape, dtype)
        for bias in (o["bias"], None):
            pre = exo.gemm_statement(o["x"], o["w"], bias)
            res = exo.cancelling_residual(pre, dtype)
            exo.assert_exact_in_fp32(shape[2], o["x"], o["w"], bias, res)
            ref = pre + res.double()
            assert float(ref.abs().mean()) < 0.05 * float(pre.abs().mean()) and float(pre.abs().mean()) > 2.0          # the sum is small against what cancels
            y32 = o["x"].float() @ o["w"].float().t() + (0 if bias is None else bias.float()) + res.float()
            assert torch.equal(y32.double(), ref)
            frac = float((exo.control_round_before_residual(pre, res, dtype) != exo.expected(ref, dtype)).double().mean())
            print(f"cancellation {shape} {dtype} bias={bias is not None}: {frac:.3f} of the elements differ under (a)")
            assert frac > 0.25, (shape, frac)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("feat", exo.CONV_FEATURES)
def test_conv_inputs(feat, dtype):
    import torch.nn.functional as F
    for shape in CONV_SHAPES:
        o = exo.conv_operands(feat, shape, dtype)
        B, H, W, Cin, Cout = o["shape"]
        K = 9 * Cin
        stride, up, pad = exo.conv_geometry(feat)
        ref, xin = exo.conv_operands_statement(feat, o, dtype)
        ra = None if o["rowadd"] is None else o["rowadd"][:, 32:32 + Cout]
        exo.assert_exact_in_fp32(K, xin, o["w4"], o["bias"], ra, o["residual"])
        assert K <= 1152
        # fp32 evaluation through torch's own conv (an independent statement of the geometry: padding, stride, the nearest x2)
        xi = xin.float().permute(0, 3, 1, 2)
        if up:
            xi = F.interpolate(xi, scale_factor=2, mode="nearest")
        if pad:
            xi = F.pad(xi, (0, 1, 0, 1))
        y32 = F.conv2d(xi, o["w4"].float(), o["bias"].float(), stride=stride, padding=0 if pad else 1).permute(0, 2, 3, 1)
        if o["residual"] is not None:
            y32 = y32 + o["residual"].float()
        if ra is not None:
            y32 = y32 + ra.float()[:, None, None, :]
        assert y32.dtype == torch.float32 and torch.equal(y32.double(), ref), (feat, shape)
        frac = exo.unrepresentable(ref, dtype)
        print(f"conv {feat} {o['shape']} {dtype}: {frac:.2f} of the outputs are not representable")
        assert frac >= 0.5, (feat, shape, frac)
        want = exo.expected(ref, dtype)
        if feat == "s1":          # (c) taps (ky, kx) and (kx, ky) swapped in the first output row
            _flagged(exo.expected(exo.control_swap_taps(ref, o["x"], o["w4"], o["bias"]), dtype), want, f"{shape} (c)")
        if feat == "gn_affine":   # (d) the shift also in the padding; and the table differs per channel and per sample
            t = o["table"]
            assert bool((t[..., 1] != 0).all()) and set(t[..., 0].unique().tolist()) == {0.5, 1.0, 2.0}
            assert t[0, :, 0].unique().numel() == 3 and t[0, :, 1].unique().numel() > 8 and (B == 1 or not torch.equal(t[0], t[1]))
            _flagged(exo.expected(exo.control_shift_in_padding(o["x"], t, o["w4"], o["bias"], dtype), dtype), want, f"{shape} (d)")
            # a wrong channel or sample index into the table changes the result
            for wrong in (t.roll(1, 1), t.roll(1, 0) if B > 1 else None):
                if wrong is not None:
                    other = exo.conv_statement(exo.affine(o["x"], wrong, dtype), o["w4"], o["bias"])
                    _flagged(exo.expected(other, dtype), want, f"{shape} wrong table index")


def test_all_ones_closed_form_is_the_conv():
    """the integer expectation of the all-ones cases, stated from the tap counts, is what the statement gives -- for every geometry"""
    for feat in ("s1", "s2", "pad1", "up1", "up2"):
        stride, up, pad = exo.conv_geometry(feat)
        for (B, H, W, Cin, Cout) in CONV_SHAPES:
            want = exo.taps_inside(H, stride, up, pad)[:, None] * exo.taps_inside(W, stride, up, pad)[None, :] * Cin
            ref = exo.conv_statement(torch.ones(B, H, W, Cin), torch.ones(Cout, Cin, 3, 3), None, stride, up, pad)
            assert torch.equal(ref, want.double()[None, :, :, None].expand_as(ref)), (feat, H, W)
            for dt in DTYPES:
                assert torch.equal((want.double() / 32).to(dt).double() * 32, want.double())      # exact in T once scaled to the grid
    t = exo.taps_inside(5)
    assert t.tolist() == [2, 3, 3, 3, 2] and exo.taps_inside(5, 2).tolist() == [2, 3, 2] and exo.taps_inside(5, 2, 0, 1).tolist() == [3, 3]
    assert exo.taps_inside(4, 2, 0, 1).tolist() == [3, 2] and exo.taps_inside(2, 1, 1).tolist() == [2, 3, 3, 2]


def test_f32_tail_inputs():
    """the fp32 tail: grid operands are representable in bf16, so the hi / lo split of the default arithmetic mode has lo = 0"""
    for shape in exo.F32_GEMM_SHAPES:
        x, w, b, r = exo.f32_gemm_operands(shape)
        for t in (x, w):
            assert t.dtype == torch.float32 and torch.equal(t.bfloat16().float(), t)
        exo.assert_exact_in_fp32(shape[2], x, w, b, r)
        ref = exo.gemm_statement(x, w, b, residual=r)
        assert torch.equal((x @ w.t() + b + r).double(), ref) and torch.equal(ref.float().double(), ref)
    for case in exo.F32_CONV_CASES:
        x, w4, b, r = exo.f32_conv_operands(case)
        B, H, W, Cin, Cout, up, stride, pad = case
        assert torch.equal(x.bfloat16().float(), x) and torch.equal(w4.bfloat16().float(), w4)
        exo.assert_exact_in_fp32(9 * Cin, x, w4, b, r)
        ref = exo.conv_statement(x, w4, b, stride, up, pad) + r.double()
        assert torch.equal(ref.float().double(), ref) and tuple(ref.shape) == tuple(r.shape)
