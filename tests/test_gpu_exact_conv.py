"""GPU: every conv3x3 tile variant against the ONE correctly rounded value of its float64 statement, element for element -- the scheme of
tests/test_gpu_exact_gemm.py over the conv variants: the tile list of test_gpu_ops.test_conv3x3 and of the guarded-placement tests, the plain
64 x 64 tile, and every built LDS-halo code (dispatch_matrix.conv_variants).

Shapes: dispatch_matrix.CONV_SHAPES plus (1, 3, 5, 64, 8), a patch smaller than any tile: Cin <= 128, K = 9 Cin <= 1152, partial sums below
2^12 on the 2^-10 grid (ConvCell(exact=True) asserts it on the operands it places).  Features: stride 1 / 2, the right-bottom padding mode, the
fused nearest x2 in both forms (up = 1, and up = 2: the phase form), residual, row-add, two sources, and gn_affine: the fused normalisation
front end fed a hand-made (scale, shift) table whose fma is exact in T -- a wrong channel or sample index into the table, or a shift applied
to the zero padding, changes the result (the controls of tests/test_exact_operands_host.py).

A cell runs on a variant iff cell.variant_ok(cfg); a refusal of an approved cell is a failure."""
import collections

import pytest
import torch

import dispatch_matrix as dm
import exact_operands as exo
from conftest import built
from test_gpu_guarded_ops import CONV_VARIANTS
from test_gpu_ops import DTYPES, L  # noqa: F401

pytestmark = pytest.mark.gpu

# the cfg= of the cases of test_gpu_ops.test_conv3x3
TEST_CONV3X3 = [(128, 128, 2), (5258, 320, 1), (6128, 320, 1), (4128, 64, 1), (7128, 320, 1), (7128, 160, 1), (7328, 160, 1), (7428, 160, 1),
                (7256, 160, 1), (7356, 160, 1), (7564, 160, 1), (7564, 320, 1), (7128, 80, 1), (1464, 160, 1), (2464, 160, 1), (2464, 160, 2),
                (24128, 160, 1), (22128, 160, 1), (24128, 128, 1)]
CONV_V = dm.conv_variants([(64, 64, 1)] + built(TEST_CONV3X3) + built(CONV_VARIANTS))
HALO_V = [v for v in CONV_V if v[0] in dm.Ctx._HALO]
SHAPES = dm.CONV_SHAPES + [exo.TINY_PATCH]
UP2_WIDE = (1, 6, 10, 64, 320)          # up2 only: the one width of these at which the 320-wide phase tile (5258 x 320) has whole column tiles
RAN = collections.Counter()


def shapes_of(feat):
    return SHAPES + ([UP2_WIDE] if feat == "up2" else [])


def _run(cell, cfg, dtype, what, failures):
    arena = dm.fresh_arena()
    ctx = dm.ArenaCtx(arena, dtype)
    out, side = cell.call(ctx, cfg=cfg)
    torch.cuda.synchronize()
    arena.check()
    try:
        cell.check(out, side, what, cfg_used=cfg)
    except AssertionError as e:
        failures.append(str(e))
    return out


def _report(failures):
    assert not failures, f"{len(failures)} cells differ from the correctly rounded statement:\n" + "\n".join(failures[:40])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("feat", exo.CONV_FEATURES)
def test_conv_variant_equals_the_rounded_statement(L, dtype, feat):
    failures = []
    counts = {cfg: 0 for cfg in CONV_V}
    for shape in shapes_of(feat):
        cell = dm.ConvCell(feat, shape, dtype, exact=True)
        for cfg in CONV_V:
            if not cell.variant_ok(cfg):
                continue
            out = _run(cell, cfg, dtype, f"exact conv {feat} {cell.shape} {cfg}", failures)
            counts[cfg] += 1
            RAN[cfg] += 1
            # the comparison has teeth on the kernel's own output: controls (c) swapped taps in the first output row, (d) the shift in the padding
            wrong = None
            if feat == "s1" and cfg == CONV_V[0]:
                wrong = exo.control_swap_taps(cell.ref, cell.x, cell.w4, cell.bias)
            if feat == "gn_affine" and cfg == HALO_V[0]:
                wrong = exo.control_shift_in_padding(cell.x, cell.table, cell.w4, cell.bias, dtype)
            if wrong is not None:
                with pytest.raises(AssertionError, match="elements differ"):
                    exo.assert_equal(out, exo.expected(wrong, dtype), "control")
    print(f"\n[exact] conv {feat} {dtype}: shapes run per variant {counts}")
    if feat == "s1":
        assert all(n == len(SHAPES) for n in counts.values()), counts            # every conv variant runs the plain stride-1 conv
    if feat in ("x2", "gn_affine"):
        assert all(counts[cfg] == len(SHAPES) for cfg in CONV_V if cfg[0] in dm.Ctx._HALO), counts                # the front end: every LDS-halo code
    if feat in ("s2", "pad1"):
        assert all(counts[cfg] == len(SHAPES) for cfg in CONV_V if cfg[0] not in dm.Ctx._HALO), counts
    if feat == "up2":
        assert all(counts[cfg] > 0 for cfg in CONV_V if cfg[:2] in dm.Ctx._PHASE and cfg[2] == 1), counts
    assert sum(counts.values()) > 0
    _report(failures)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(1, 12, 20, 64, 200), exo.TINY_PATCH])
def test_conv_one_tap_channel_maps_shift_the_input_bit_for_bit(L, dtype, shape):
    """for each of the nine taps a weight that is a channel map at that tap alone, x = full-mantissa normals: the output is the input shifted
    by the tap with its channels mapped, bit for bit (every mantissa bit passes), zero where the tap reads the padding -- the packing
    [Cout, tap, Cin], the tap order 3 ky + kx and the halo offsets of every variant"""
    failures = []
    B, H, W, Cin, Cout = shape
    cell = dm.ConvCell("s1", shape, dtype, exact=True)
    src = exo.channel_map(Cout, Cin, 7).to(dm.DEV)
    cell.x = exo.full_mantissa((B, H, W, Cin), 41, dtype).to(dm.DEV)
    cell.bias = torch.zeros(Cout, dtype=dtype, device=dm.DEV)
    for tap in range(9):
        ky, kx = divmod(tap, 3)
        cell.w4 = torch.zeros(Cout, Cin, 3, 3, dtype=dtype, device=dm.DEV)
        cell.w4[torch.arange(Cout, device=dm.DEV), src, ky, kx] = 1.0
        want = torch.zeros(B, H, W, Cout, dtype=dtype, device=dm.DEV)
        # y[Y, X, co] = x[Y + ky - 1, X + kx - 1, src[co]]
        ys, xs = slice(max(0, 1 - ky), H - max(0, ky - 1)), slice(max(0, 1 - kx), W - max(0, kx - 1))
        yd, xd = slice(max(0, ky - 1), H - max(0, 1 - ky)), slice(max(0, kx - 1), W - max(0, 1 - kx))
        want[:, ys, xs] = cell.x[:, yd, xd][..., src]
        cell.ref = want.double()
        for cfg in CONV_V:
            assert cell.variant_ok(cfg)
            _run(cell, cfg, dtype, f"one tap {tap} {shape} {cfg}", failures)
    _report(failures)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("feat", ["s1", "s2", "pad1", "up1", "up2"])
def test_conv_all_ones_proves_the_zero_padding(L, dtype, feat):
    """ones in, 1 / 32 as every weight, no bias: an output is Cin / 32 times the number of taps inside the image -- ny nx with ny, nx the
    count of k in 0 .. 2 with 0 <= stride o + k - lo < extent (lo = 1, or 0 in the right-bottom padding mode; extent doubled by the nearest
    x2): 4 Cin / 32 at a corner, 6 Cin / 32 on an edge, 9 Cin / 32 inside for stride 1.  Integers times a power of two, exact in T"""
    failures = []
    stride, up, pad = exo.conv_geometry(feat)
    ran = 0
    for shape in shapes_of(feat):
        B, H, W, Cin, Cout = shape
        cell = dm.ConvCell(feat, shape, dtype, exact=True)
        cell.x = cell.xin = torch.ones(B, H, W, Cin, dtype=dtype, device=dm.DEV)
        cell.w4 = torch.full((Cout, Cin, 3, 3), 1.0 / 32, dtype=dtype, device=dm.DEV)
        cell.bias = torch.zeros(Cout, dtype=dtype, device=dm.DEV)
        ny, nx = exo.taps_inside(H, stride, up, pad), exo.taps_inside(W, stride, up, pad)
        if feat == "s1":
            assert ny[0] == 2 and ny[1] == 3 and ny[-1] == 2
        want = (ny[:, None] * nx[None, :] * Cin).double() / 32
        cell.ref = want[None, :, :, None].expand(B, len(ny), len(nx), Cout).contiguous().to(dm.DEV)
        assert cell.ref.shape[1:3] == (cell.M // B // len(nx), len(nx))
        cell.assert_premise()
        for cfg in CONV_V:
            if cell.variant_ok(cfg):
                _run(cell, cfg, dtype, f"all ones {feat} {shape} {cfg}", failures)
                ran += 1
    assert ran >= (len(CONV_V) if feat in ("s1", "up1") else 3)
    _report(failures)


def test_zz_cells_run_per_variant(L):
    """printed for the record: the exact (feature, shape, dtype) cells each conv variant ran in this process; none is left out"""
    print("\n[exact] conv cells run per variant: " + ", ".join(f"{cfg}: {RAN[cfg]}" for cfg in CONV_V))
    assert (64, 64, 1) in CONV_V and len(HALO_V) >= 4
    assert not RAN or all(RAN[cfg] > 0 for cfg in CONV_V), dict(RAN)
