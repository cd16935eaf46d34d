"""GPU tests of AutoencoderTiny on csrc/tinyvae.hip: the one conv entry (body, head, tail) against the fp64 expression of
include/imh_tinyvae.h, its exact cases, guarded placement and refusals; the whole decoder against the CPU restatement
(tests/tiny_vae_reference.py); the decode's behaviour (batching, repeatability, 35 launches) and the opt-in wiring (preview_vae=, vae=).

How the one-ulp bound is made sound.  The entry rounds once, so its result is within HALF a unit in the last place of T of the fp32 sum it
formed; the other half unit of the bound is left for the order of the fp32 accumulation.  An fp32 sum of 576 products is off by about
1e-6 of the products' scale, which is more than half a unit of an output that happens to fall within 1e-3 of zero -- a few hundred of
the 1e5 outputs of a random-normal case, for a perfect kernel.  So the one-ulp cases are built from operands on binary grids (activations
and weights k / 64 with |k| <= 64, bias k / 4096, residual k / 16): every product and every partial sum is a multiple of 2^-12 below 2^10,
exact in fp32 in any order, and the bound holds for every element, the ones near zero included; the sums (spread about 8, on a 2^-12
grid) are not representable in either T, so the one rounding is exercised.  The "offset" cases use full-mantissa random operands and a
bias of 16, which keeps every output where an fp32 sum's error is far below its last place."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

from conftest import record_parity, rel_rms
from oracle.detfill import det_fill, det_randn

import tiny_vae_reference as tvr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float16, torch.bfloat16]
IDS = ["fp16", "bf16"]
# [B, H, W]: the degenerate ones, a small ragged one, and one above the kernel's 16 x 32 pixel tile in both extents, a multiple of neither
# (two row tiles x two column tiles; under UP2 three x three)
SHAPES = [(1, 1, 1), (1, 1, 9), (1, 9, 1), (2, 5, 7), (1, 19, 37)]
RAGGED = [(2, 5, 7), (1, 19, 37)]


def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def _ulp(ref, dtype):
    """one unit in the last place of `dtype` at the fp64 values `ref`"""
    mant, emin = (10, -14) if dtype == torch.float16 else (7, -126)
    e = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** emin))).clamp_min(emin)
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - mant)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _grid(shape, lo, hi, step, seed, dtype):
    """integers of [lo, hi] times `step` (a power of two): exact in bf16 and fp16"""
    return (torch.randint(lo, hi + 1, tuple(shape), generator=_gen(seed)).double() * step).to(dtype)


def _grid_operands(B, H, W, up2, dtype, seed=0):
    Ho, Wo = (2 * H, 2 * W) if up2 else (H, W)
    x = _grid((B, H, W, 64), -64, 64, 2.0 ** -6, 100 + seed, dtype)
    w = _grid((64, 576), -64, 64, 2.0 ** -6, 200 + seed, dtype)
    b = _grid((64,), -128, 128, 2.0 ** -12, 300 + seed, dtype)
    r = _grid((B, Ho, Wo, 64), -128, 128, 2.0 ** -4, 400 + seed, dtype)
    return x, w, b, r


def _ref_body(x, w, bias=None, residual=None, up2=False, relu=False):
    """the fp64 expression of the body on the CPU: NHWC in, NHWC out"""
    xi = x.double().cpu().permute(0, 3, 1, 2)
    if up2:
        xi = F.interpolate(xi, scale_factor=2, mode="nearest")
    wt = w.double().cpu().view(w.shape[0], 3, 3, -1).permute(0, 3, 1, 2)
    y = F.conv2d(xi, wt, None if bias is None else bias.double().cpu(), padding=1).permute(0, 2, 3, 1)
    if residual is not None:
        y = y + residual.double().cpu()
    return y.clamp_min(0) if relu else y


def _within_one_ulp(y, ref, dtype, what):
    err = (y.double().cpu() - ref).abs()
    bad = err > _ulp(ref, dtype)
    assert torch.isfinite(y).all() and not bad.any(), f"{what}: {int(bad.sum())} of {bad.numel()} beyond one ulp, worst {float((err / _ulp(ref, dtype)).max()):.2f} ulp"


def _conv(dtype, x, w, **kw):
    from imagharmony_amd.ctx import Ctx
    y = Ctx(DEV, dtype).tinyvae_conv(x.to(DEV), w.to(DEV), **{k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in kw.items()})
    torch.cuda.synchronize()
    return y


# ---------------------------------------------------------------------------------------------------- body against fp64
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_body_within_one_ulp_of_fp64(shape, dtype):
    """every combination of UP2, bias, residual and RELU on grid operands (exact fp32 sums: the docstring of this file)"""
    B, H, W = shape
    for up2 in (False, True):
        x, w, b, r = _grid_operands(B, H, W, up2, dtype)
        for use_b in (False, True):
            for use_r in (False, True):
                for relu in (False, True):
                    kw = dict(bias=b if use_b else None, residual=r if use_r else None, up2=up2, relu=relu)
                    y = _conv(dtype, x, w, **kw)
                    assert y.shape == r.shape and y.dtype == dtype
                    _within_one_ulp(y, _ref_body(x, w, **kw), dtype, f"{shape} {kw.keys()} up2={up2} bias={use_b} residual={use_r} relu={relu}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", RAGGED)
@pytest.mark.parametrize("up2", [False, True])
def test_body_full_mantissa_operands_offset_from_zero(shape, up2, dtype):
    """random-normal operands that use every mantissa bit; a bias of 16 keeps the outputs in [8, 32), where the fp32 sum's error (1e-6) is
    three orders below the last place of T"""
    B, H, W = shape
    Ho, Wo = (2 * H, 2 * W) if up2 else (H, W)
    x, w = det_randn((B, H, W, 64), 21).to(dtype), det_randn((64, 576), 22, 1.0 / 24).to(dtype)
    b, r = (16.0 + det_randn((64,), 23, 0.05)).to(dtype), det_randn((B, Ho, Wo, 64), 24).to(dtype)
    y = _conv(dtype, x, w, bias=b, residual=r, up2=up2, relu=True)
    ref = _ref_body(x, w, b, r, up2, True)
    assert float(ref.min()) > 8.0
    _within_one_ulp(y, ref, dtype, f"{shape} up2={up2}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", RAGGED)
@pytest.mark.parametrize("relu", [False, True])
def test_body_rounds_once_under_cancellation(shape, relu, dtype):
    """residual = -(conv + bias) + noise, rounded to T: the sum is the noise (0.008 .. 0.023) plus the residual's own rounding, exact in fp32.  A
    kernel that rounds conv + bias to T before it adds the residual is off by up to half a unit of the conv result -- hundreds of units of
    the sum -- and fails here."""
    B, H, W = shape
    x, w, b, _ = _grid_operands(B, H, W, False, dtype, seed=1)
    c = _ref_body(x, w, b)
    assert float(c.abs().mean()) > 2.0                                  # the conv result is large against the noise: its T rounding is coarse
    g = _gen(5)
    noise = torch.randint(32, 97, tuple(c.shape), generator=g).double() * (torch.randint(0, 2, tuple(c.shape), generator=g).double() * 2 - 1) * 2.0 ** -12
    r = (noise - c).to(dtype)
    ref = _ref_body(x, w, b, r, False, relu)
    # what a twice-rounding kernel would return misses the bound on most elements: the input does what it is for
    twice = (c.to(dtype).double() + r.double())
    twice = twice.clamp_min(0) if relu else twice
    assert float(((twice.to(dtype).double() - ref).abs() > _ulp(ref, dtype)).double().mean()) > 0.25
    _within_one_ulp(_conv(dtype, x, w, bias=b, residual=r, relu=relu), ref, dtype, f"{shape} relu={relu}")


# ---------------------------------------------------------------------------------------------------- exact cases
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", RAGGED)
@pytest.mark.parametrize("up2", [False, True])
def test_all_ones_proves_the_zero_padding(shape, up2, dtype):
    """ones in, ones as weights: an output counts the taps inside the image times 64 -- 256 at a corner, 384 on an edge, 576 inside;
    the tail turns them into 2 n - 1"""
    B, H, W = shape
    Ho, Wo = (2 * H, 2 * W) if up2 else (H, W)
    x = torch.ones(B, H, W, 64, dtype=dtype)
    ny = 3 - (torch.arange(Ho) == 0).long() - (torch.arange(Ho) == Ho - 1).long()
    nx = 3 - (torch.arange(Wo) == 0).long() - (torch.arange(Wo) == Wo - 1).long()
    want = (ny[:, None] * nx[None, :] * 64).to(torch.float32)
    assert want[0, 0] == 256 and want[0, 1] == 384 and want[1, 1] == 576
    y = _conv(dtype, x, torch.ones(64, 576, dtype=dtype), up2=up2).float().cpu()
    assert torch.equal(y, want[None, :, :, None].expand(B, Ho, Wo, 64))
    if not up2:
        t = _conv(dtype, x, torch.ones(3, 576, dtype=dtype), tail=True).cpu()
        assert t.dtype == torch.float32 and torch.equal(t, (2 * want - 1)[None, None].expand(B, 3, H, W))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("up2", [False, True])
def test_one_tap_permutations_shift_the_input_bit_for_bit(up2, dtype):
    """for each of the nine taps a weight that is a channel permutation at that tap alone: the output is the input, shifted by the tap and
    permuted, bit for bit (every mantissa bit passes) -- the packing [Cout, tap, Cin], the tap order 3 ky + kx and the >> 1 of UP2"""
    for shape in RAGGED:
        B, H, W = shape
        x = det_randn((B, H, W, 64), 41).to(dtype)
        xv = x.repeat_interleave(2, 1).repeat_interleave(2, 2) if up2 else x
        Ho, Wo = xv.shape[1], xv.shape[2]
        perm = torch.randperm(64, generator=_gen(7))
        for tap in range(9):
            ky, kx = divmod(tap, 3)
            w = torch.zeros(64, 9, 64, dtype=dtype)
            w[torch.arange(64), tap, perm] = 1.0
            want = torch.zeros(B, Ho, Wo, 64, dtype=dtype)
            # y[Y, X, co] = xv[Y + ky - 1, X + kx - 1, perm[co]]
            ys, xs = slice(max(0, 1 - ky), Ho - max(0, ky - 1)), slice(max(0, 1 - kx), Wo - max(0, kx - 1))
            yd, xd = slice(max(0, ky - 1), Ho - max(0, 1 - ky)), slice(max(0, kx - 1), Wo - max(0, 1 - kx))
            want[:, ys, xs] = xv[:, yd, xd][..., perm]
            y = _conv(dtype, x, w.view(64, 576), up2=up2).cpu()
            assert torch.equal(_bits(y), _bits(want)), (shape, tap)


# ---------------------------------------------------------------------------------------------------- head and tail
def _ref_head(z, w, b, dtype):
    """round_T(3 tanh(z / 3)) in fp64, conv 4 -> 64 + bias, ReLU: NCHW fp32 in, NHWC fp64 out"""
    t = (3.0 * torch.tanh(z.double() / 3.0)).to(dtype)
    return _ref_body(t.permute(0, 2, 3, 1), w, b, None, False, True), t


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_head_within_one_ulp_of_fp64(shape, dtype):
    B, H, W = shape
    # (a) latents whose clamp lands on the grid k / 16 (z = 3 atanh(g / 3)): a kernel without the tanh, or with another clamp, is far off;
    # the conv's sums (multiples of 2^-13 below 16) are exact in fp32
    g = torch.randint(-40, 41, (B, 4, H, W), generator=_gen(51)).double() / 16
    z = (3.0 * torch.atanh(g / 3.0)).float()
    w, b = _grid((64, 36), -64, 64, 2.0 ** -9, 52, dtype), _grid((64,), -128, 128, 2.0 ** -13, 53, dtype)
    ref, t = _ref_head(z, w, b, dtype)
    assert torch.equal(t.double(), g)
    y = _conv(dtype, z, w, bias=b, head=True)
    assert y.shape == (B, H, W, 64) and y.dtype == dtype
    _within_one_ulp(y, ref, dtype, f"head grid {shape}")
    if H * W > 1:
        assert 0.2 < float((ref > 0).double().mean()) < 0.8               # the ReLU works on both sides
    # (b) the decoder's own latents (normal, scale 3: the clamp bends them) and full-mantissa weights, offset from zero by the bias
    z = tvr.latents(B, H, W)
    w, b = det_randn((64, 36), 54, 1.0 / 6).to(dtype), (16.0 + det_randn((64,), 55, 0.05)).to(dtype)
    ref, _ = _ref_head(z, w, b, dtype)
    assert float(ref.min()) > 4.0                                        # (the sums spread by about 1.6 around the bias)
    _within_one_ulp(_conv(dtype, z, w, bias=b, head=True), ref, dtype, f"head offset {shape}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_tail_against_fp64(shape, dtype):
    """2 (conv + bias) - 1 in fp32, NCHW, never rounded to T: every element within 1e-5 of the output's RMS"""
    B, H, W = shape
    x, w, b = det_randn((B, H, W, 64), 61).to(dtype), det_randn((3, 576), 62, 1.0 / 24).to(dtype), det_randn((3,), 63, 0.05).to(dtype)
    for bias in (b, None):
        ref = (2.0 * _ref_body(x, w, bias) - 1.0).permute(0, 3, 1, 2)
        y = _conv(dtype, x, w, bias=bias, tail=True)
        assert y.shape == (B, 3, H, W) and y.dtype == torch.float32 and y.is_contiguous()
        err = float((y.double().cpu() - ref).abs().max())
        rms = float(ref.pow(2).mean().sqrt())
        assert err <= 1e-5 * rms, (err, rms)


# ---------------------------------------------------------------------------------------------------- guarded placement
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_guarded_placement(shape, dtype):
    """all operands carved from one NaN-sentinel arena: no byte outside the outputs changes, the outputs are finite and equal the dense
    run's bit for bit -- body (plain and UP2 with bias, residual, ReLU), head and tail"""
    from guarded import run_dense_and_guarded
    B, H, W = shape
    z = tvr.latents(B, H, W).to(DEV)
    wh, wt = det_randn((64, 36), 71, 1.0 / 6).to(dtype).to(DEV), det_randn((3, 576), 72, 1.0 / 24).to(dtype).to(DEV)
    bt = det_randn((3,), 73, 0.05).to(dtype).to(DEV)
    for up2 in (False, True):
        x, w, b, r = (t.to(DEV) for t in _grid_operands(B, H, W, up2, dtype))

        def body(ctx, put, out):
            return ctx.tinyvae_conv(put(x), put(w), bias=put(b), residual=put(r), up2=up2, relu=True)
        dense, guarded, arena = run_dense_and_guarded(DEV, dtype, body)
        arena.check()
        assert torch.equal(_bits(dense[0]), _bits(guarded[0]))
    for body in (lambda ctx, put, out: ctx.tinyvae_conv(put(z), put(wh), bias=put(b), head=True),
                 lambda ctx, put, out: ctx.tinyvae_conv(put(x), put(wt), bias=put(bt), tail=True),
                 lambda ctx, put, out: ctx.tinyvae_conv(put(x), put(w))):
        dense, guarded, arena = run_dense_and_guarded(DEV, dtype, body)
        arena.check()
        assert torch.equal(_bits(dense[0]), _bits(guarded[0]))


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals_return_their_status_and_launch_nothing():
    from guarded import Arena
    from imagharmony_amd import lib as L
    l = L.load()
    arena = Arena(DEV, 16 << 20)
    x = arena.place(torch.zeros(1, 4, 4, 64, dtype=torch.bfloat16, device=DEV))
    w = arena.place(torch.zeros(64, 576, dtype=torch.bfloat16, device=DEV))
    b = arena.place(torch.zeros(64, dtype=torch.bfloat16, device=DEV))
    r = arena.place(torch.zeros(1, 8, 8, 64, dtype=torch.bfloat16, device=DEV))
    y = arena.carve((1, 8, 8, 64), torch.bfloat16)                          # room for the UP2 output too
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    H_, T_, U_, R_ = L.TINYVAE_HEAD, L.TINYVAE_TAIL, L.TINYVAE_UP2, L.TINYVAE_RELU

    def call(**kw):
        a = L.TinyVaeArgs()
        a.x, a.w, a.bias, a.residual, a.y = x.data_ptr(), w.data_ptr(), b.data_ptr(), None, y.data_ptr()
        a.B, a.H, a.W, a.flags, a.dtype = 1, 4, 4, R_, L.IMH_DT_BF16
        for k, v in kw.items():
            setattr(a, k, v)
        rc = l.imh_tinyvae_conv(C.byref(a), stream)
        torch.cuda.synchronize()
        assert arena.written() is None, kw                               # the output keeps its sentinel: nothing ran
        return rc
    assert call(x=None) == -1 and call(w=None) == -1 and call(y=None) == -1
    assert call(x=x.data_ptr() + 8) == -1 and call(w=w.data_ptr() + 2) == -1 and call(y=y.data_ptr() + 4) == -1
    assert call(bias=b.data_ptr() + 2) == -1 and call(residual=r.data_ptr() + 8, flags=U_) == -1
    assert call(flags=32) == -1 and call(flags=R_ | 64) == -1
    assert call(dtype=2) == -3 and call(dtype=7) == -3
    assert call(flags=H_ | U_) == -1 and call(flags=T_ | U_) == -1 and call(flags=H_ | T_) == -1
    assert call(flags=H_, residual=r.data_ptr()) == -1 and call(flags=T_, residual=r.data_ptr()) == -1
    assert call(B=0) == -2 and call(H=0) == -2 and call(W=0) == -2 and call(H=-3) == -2
    assert call(B=1 << 9, H=1 << 8, W=1 << 8) == -2                        # 2^31 elements of x and y
    assert call(B=1, H=1 << 12, W=1 << 12, flags=U_) == -2                 # x has 2^30, y 2^32
    assert call(y=x.data_ptr()) == -1 and b"overlap" in l.imh_last_error()
    assert call(residual=y.data_ptr(), flags=U_) == -1 and b"overlap" in l.imh_last_error()
    # ... and the same arguments without a fault are accepted and write y
    a = L.TinyVaeArgs()
    a.x, a.w, a.bias, a.residual, a.y = x.data_ptr(), w.data_ptr(), b.data_ptr(), r.data_ptr(), y.data_ptr()
    a.B, a.H, a.W, a.flags, a.dtype = 1, 4, 4, R_ | U_, L.IMH_DT_BF16
    assert l.imh_tinyvae_conv(C.byref(a), stream) == 0
    torch.cuda.synchronize()
    arena.check()
    assert not y.any()


# ---------------------------------------------------------------------------------------------------- offsets beyond 2^31 bytes
def test_body_addresses_beyond_two_gib():
    """[1, 4100, 4100, 64]: 1.08 G elements, 2.15 GB per operand -- byte offsets that do not fit 31 bits.  The last rows (and the first)
    against fp64 on grid operands"""
    from imagharmony_amd.ctx import Ctx
    dtype, H, W = torch.bfloat16, 4100, 4100
    g = torch.Generator(device=DEV).manual_seed(3)
    x = (torch.randint(-8, 9, (1, H, W, 64), generator=g, device=DEV, dtype=torch.int8).to(dtype) * 0.125)
    w, b = _grid((64, 576), -8, 8, 2.0 ** -6, 81, dtype), _grid((64,), -64, 64, 2.0 ** -9, 82, dtype)
    y = Ctx(DEV, dtype).tinyvae_conv(x, w.to(DEV), bias=b.to(DEV), relu=True)
    torch.cuda.synchronize()
    assert y.numel() * 2 > 1 << 31
    for rows in (slice(0, 3), slice(H - 3, H)):
        # rows of the slice that have all their neighbours inside it (or outside the image)
        ref = _ref_body(x[:, rows].cpu(), w, b, None, False, True)
        keep = slice(0, 2) if rows.start == 0 else slice(1, 3)
        _within_one_ulp(y[:, rows][:, keep].cpu(), ref[:, keep], dtype, f"rows {rows}")
    assert torch.isfinite(y[:, ::257].float()).all()


# ---------------------------------------------------------------------------------------------------- the whole decoder
@functools.lru_cache(maxsize=None)
def _product(dtype):
    from imagharmony_amd import AutoencoderTiny
    m = AutoencoderTiny()
    m.load_state_dict(tvr.reference().state_dict(), strict=True)
    return m.to(DEV, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("hw", [(5, 7), (16, 16)])
def test_whole_decoder_against_the_cpu_restatement(hw, dtype):
    """the product's decode against the fp32 restatement with the same T-rounded weights: rel-RMS within 3 x what the restatement run in
    T on the CPU shows against its own fp32 (the rule of the CLIP text and T2I-Adapter parity tests); the baseline is computed here"""
    h, w = hw
    z, ref = tvr.decoded(2, h, w, dtype)
    noise = tvr.own_noise(2, h, w, dtype)
    out = _product(dtype).decode(z.to(DEV)).cpu()
    assert out.shape == (2, 3, 8 * h, 8 * w) and out.dtype == torch.float32 and torch.isfinite(out).all()
    r = rel_rms(out, ref)
    name = f"tiny_vae_decode_{h}x{w}_{IDS[DTYPES.index(dtype)]}"
    print(f"{name}: rel-rms {r:.3e}; the restatement in {dtype} on the CPU: {noise:.3e} (bound 3 x)")
    record_parity(name, r, 3 * noise, cpu_restatement_rel_rms=noise, output_std=float(ref.std()))
    assert 1e-4 < noise < 5e-2                                            # the yardstick itself is in the range seen (7e-3 .. 9e-3 bf16, 1e-3 fp16)
    assert r <= 3 * noise, (r, noise)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_decode_behaviour(dtype, monkeypatch):
    from imagharmony_amd.ctx import Ctx
    from imagharmony_amd.vae import decode_latents, postprocess
    from imagharmony_amd.pipeline import decode_output
    m = _product(dtype)
    z = tvr.latents(2, 5, 7).to(DEV)
    calls = []
    real = Ctx.tinyvae_conv
    monkeypatch.setattr(Ctx, "tinyvae_conv", lambda self, *a, **kw: (calls.append(kw.get("descr")), real(self, *a, **kw))[1])
    n0 = m.launches
    both = m.decode(z)
    assert m.launches - n0 == 35 == len(calls) and len(set(calls)) == 35   # head, 33 body convs, tail: one launch each, nothing else
    assert calls[0] == "tiny_vae.layers.0" and calls[-1] == "tiny_vae.layers.18" and "tiny_vae.layers.6" in calls
    # a batch of two is two batches of one; a second decode gives the same bits
    assert torch.equal(both[0:1], m.decode(z[0:1])) and torch.equal(both[1:2], m.decode(z[1:2]))
    assert torch.equal(both, m.decode(z)) and torch.equal(both, m.decode(z, precision="native"))
    # the VAE helpers take the class unchanged (scaling_factor 1.0)
    assert torch.equal(decode_latents(m, z), both)
    assert torch.equal(decode_output(m, None, z, "pt"), postprocess(both, "pt"))
    # a 1 x 1 latent decodes (every h, w >= 1)
    one = m.decode(tvr.latents(1, 1, 1).to(DEV))
    assert one.shape == (1, 3, 8, 8) and torch.isfinite(one).all()
    # the packed weights are cached per weight version: an in-place update rebuilds them
    conv = m.decoder.layers[18]
    p0 = conv.packed(Ctx(DEV, dtype))[0]
    assert conv.packed(Ctx(DEV, dtype))[0] is p0
    keep = conv.weight.detach().clone()
    conv.weight.mul_(0.5)
    try:
        assert conv.packed(Ctx(DEV, dtype))[0] is not p0 and not torch.equal(m.decode(z), both)
    finally:
        conv.weight.copy_(keep)
    assert torch.equal(m.decode(z), both)
    # a recording context refuses the entry: it is no plan kind
    from imagharmony_amd import lib as L
    with pytest.raises(L.ImhError, match="no plan kind"):
        real(Ctx(DEV, dtype, record=True), z, conv.packed(Ctx(DEV, dtype))[0], head=True)


# ---------------------------------------------------------------------------------------------------- wiring
SEEDS = [3, 9, 27, 81]


def _spy(obj, log):
    real = obj.decode

    def decode(z, *a, **kw):
        log.append(int(z.shape[0]))
        return real(z, *a, **kw)
    obj.decode = decode
    return real


def test_pns_previews_through_the_tiny_vae_and_pipeline_vae():
    from test_gpu_clip_preprocess import _tower
    from test_gpu_inpaint import build_pair, build_vae_pair
    from imagharmony_amd import AutoencoderTiny, StableDiffusionXLCustomPipeline
    from imagharmony_amd import schedulers as hs
    from imagharmony_amd.ip_adapter import IPAdapterXL
    from imagharmony_amd.modules import HarmonyAttention
    from imagharmony_amd.vae import postprocess
    dtype = torch.bfloat16
    enc, _ = _tower(dtype)
    _, hu, ocfg = build_pair(dtype, 4)
    _, hv = build_vae_pair()
    tiny = AutoencoderTiny().init_random_(5).to(DEV, dtype)
    pipe = StableDiffusionXLCustomPipeline(hu, scheduler=hs.DDIMScheduler(), device=DEV, dtype=dtype, vae=hv)
    cd, dim = ocfg.cross_attention_dim, enc.config.projection_dim
    ha = det_fill(HarmonyAttention(image_hidden_size=dim, text_context_dim=cd, inter_dim=512, cross_heads=8, reshape_blocks=8, cross_value_dim=64), 3)
    ip = IPAdapterXL(pipe, None, None, DEV, num_tokens=4, inference=True, number_class_crossattention=ha, dtype=dtype,
                     clip_embeddings_dim=dim, image_encoder=enc)
    det_fill(ip.image_proj_model, 5)
    embeds4 = (det_randn((1, 77, cd), 1), det_randn((1, 77, cd), 2), det_randn((1, ocfg.pooled_dim), 3), det_randn((1, ocfg.pooled_dim), 4))
    kw = dict(clip_image_embeds=det_randn((1, dim), 5), prompt_embeds=embeds4, extra_prompt_embeds=det_randn((1, 77, cd), 6), scale=0.8,
              guidance_scale=5.0, preview_steps=2, num_inference_steps=3, batch=2)
    t_log, v_log = [], []
    t_real, v_real = _spy(tiny, t_log), _spy(hv, v_log)
    try:
        r = ip.generate_pns(SEEDS, preview_vae=tiny, judge_preprocess="hip", output_type="pt", **kw)
        # the judge saw every preview through tiny.decode, in stacks of `batch`; pipe.vae decoded the winner alone
        assert t_log == [2, 2] and v_log == [1]
        assert r["scores"].shape == (4,) and torch.isfinite(r["scores"]).all() and r["scores"].unique().numel() == 4
        assert r["images"].shape == (1, 3, 256, 256)
        # the winner's latents are, as without a preview VAE, the pipe's own call with that seed's generator
        fused = ip.fused_clip_embeds(None, kw["clip_image_embeds"], kw["extra_prompt_embeds"])
        ipe, uipe = ip._g(ip.image_proj_model)(fused), ip._g(ip.image_proj_model)(torch.zeros_like(fused))
        call = dict(prompt_embeds=torch.cat([embeds4[0].to(DEV, dtype), ipe], 1), negative_prompt_embeds=torch.cat([embeds4[1].to(DEV, dtype), uipe], 1),
                    pooled_prompt_embeds=embeds4[2], negative_pooled_prompt_embeds=embeds4[3], num_inference_steps=3, guidance_scale=5.0)
        direct = pipe(output_type="latent", generator=[torch.Generator("cpu").manual_seed(int(r["best_seed"]))], **call).images
        assert torch.equal(direct.float(), r["latents"].to(DEV).float())
        # the scores are the judge's over tiny.decode of the previews: another preview VAE, other scores
        t_log.clear(); v_log.clear()
        r0 = ip.generate_pns(SEEDS, preview_vae=None, judge_preprocess="hip", output_type="latent", **kw)
        assert t_log == [] and v_log == [2, 2]                              # preview_vae=None never touches the tiny module
        assert not torch.equal(r0["scores"], r["scores"])
        r1 = ip.generate_pns(SEEDS, judge_preprocess="hip", output_type="latent", **kw)
        assert torch.equal(r1["scores"], r0["scores"]) and torch.equal(r1["latents"], r0["latents"]) and t_log == []
        # a text-to-image pipe whose vae is the tiny one decodes its output with it
        t_log.clear()
        pipe.vae = tiny
        lat = pipe(output_type="latent", generator=[torch.Generator("cpu").manual_seed(3)], **call).images
        img = pipe(output_type="pt", generator=[torch.Generator("cpu").manual_seed(3)], **call).images
        assert t_log == [1] and torch.equal(img, postprocess(t_real(lat.float()), "pt")) and img.shape == (1, 3, 256, 256)
        assert float(img.min()) >= 0.0 and float(img.max()) <= 1.0 and float(img.std()) > 0.0
    finally:
        tiny.decode, hv.decode, pipe.vae = t_real, v_real, hv
