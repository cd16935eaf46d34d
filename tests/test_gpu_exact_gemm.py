"""GPU: every GEMM tile variant against the ONE correctly rounded value of its float64 statement, element for element.

Operands sit on the binary grids of tests/exact_operands.py, so every fp32 partial sum of a launch is exact in any order (split-K partials and
the epilogue's adds included; GemmCell(exact=True) asserts the premise on the operands it places), the accumulator holds the statement exactly
and the one rounding to T has one right result.  A dropped K element in one ragged edge row, a second rounding of acc + bias before the residual
add, a stale ring slot: each changes some element, and equality sees it -- where the k * EPS * max|ref| bound of test_gpu_ops.assert_close
passes all three.  out_f32 is the bit-exact proof of every variant's accumulator.

Variants: dispatch_matrix.gemm_variants(built(BIG_VARIANTS + SPLIT_K)) -- the plain tiles at splits 1 / 2 / 4, every ring / KG2 / ping-pong
variant, the wave-specialised set, the sixteen-wave tile, and split-K off the plain tiles: BIG_VARIANTS holds the wave-specialised
(2464, 160, 2), SPLIT_K adds one ring and one KG2 variant at splits = 2 (the split-K range and the fp32 slab store inside those three
pipelines: 512 x 640 x 128 gives one K tile per split, 300 x 200 x 192 a 2 + 1 split with ragged edges).  A cell runs on a variant iff cell.variant_ok(cfg) (Ctx's own gate); a refusal of an approved cell is a failure.  The sixteen-wave tile (26256 x 320) serves folded-LayerNorm launches only, whose arithmetic is inexact by nature: Ctx approves
none of the exact features for it, the test asserts exactly that, and its accumulator stays under test_gemm_sixteen_wave_256x320_tile.

Shapes (exact_operands.GEMM_SHAPES): whole tiles, ragged M and N, fewer rows than one MFMA with one K tile, and K_DEEP = 576: nine K tiles, more
than twice the deepest operand ring of any variant -- FOUR slots (gemm_ring.hip: the wave-specialised 64 x 160 / 128 x 160 tiles and the 4064 /
6064 rings; gemm_pp.hip and gemm_w16.hip hold two buffers), so every slot is refilled at least twice.

Placement is the cells': padded leading dimensions in the guard arena (tests/guarded.py), checked after every launch."""
import collections

import pytest
import torch

import dispatch_matrix as dm
import exact_operands as exo
from conftest import built
from test_gpu_ops import BIG_VARIANTS, DTYPES, L  # noqa: F401

pytestmark = pytest.mark.gpu

SPLIT_K = [(5064, 64, 2), (3064, 64, 2)]                            # ring, KG2 at splits = 2 (the wave-specialised (2464, 160, 2) is in BIG_VARIANTS)
assert (2464, 160, 2) in BIG_VARIANTS
GEMM_V = dm.gemm_variants(built(BIG_VARIANTS + SPLIT_K))
NO_EXACT_FORM = [v for v in GEMM_V if v[0] in dm.Ctx._W16]          # folded-LayerNorm launches only
RAN = collections.Counter()                                          # cfg -> (feature, shape, dtype) cells run
CANCEL_SHAPES = [s for s in exo.GEMM_SHAPES if s[2] >= 128]
PERM_M = 200                                                         # ragged against every tile height, several 64-row blocks


def _run(cell, cfg, dtype, what, failures):
    """one approved cell on one variant: placed in a fresh arena, launched, guards checked, compared; a refusal propagates"""
    arena = dm.fresh_arena()
    ctx = dm.ArenaCtx(arena, dtype)
    res = cell.call(ctx, cfg=cfg)
    torch.cuda.synchronize()
    arena.check()
    try:
        cell.check(*res, what)
    except AssertionError as e:
        failures.append(str(e))
    return res


def _report(failures):
    assert not failures, f"{len(failures)} cells differ from the correctly rounded statement:\n" + "\n".join(failures[:40])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("feat", exo.GEMM_FEATURES)
def test_gemm_variant_equals_the_rounded_statement(L, dtype, feat):
    """every approved (variant, shape) cell of the feature; the fourth shape has K = 576, nine K tiles against a deepest ring of four slots"""
    failures = []
    counts = collections.Counter({cfg: 0 for cfg in GEMM_V})
    for shape in exo.gemm_shapes(feat):
        cell = dm.GemmCell(feat, shape, dtype, exact=True)
        for cfg in GEMM_V:
            if not cell.variant_ok(cfg):
                continue
            res = _run(cell, cfg, dtype, f"exact gemm {feat} {shape} {cfg}", failures)
            counts[cfg] += 1
            RAN[cfg] += 1
            if cfg == GEMM_V[0]:
                # the comparison has teeth on the kernel's own output: control (b), one K element dropped in the last row, is flagged
                right, cell.ref = cell.ref, exo.control_drop_last_k(cell.ref, cell.x, cell.w)
                with pytest.raises(AssertionError, match="elements differ"):
                    cell.check(*res, "control (b)")
                cell.ref = right
    counts = dict(counts)
    print(f"\n[exact] gemm {feat} {dtype}: shapes run per variant {counts}")
    for cfg in GEMM_V:
        if cfg in NO_EXACT_FORM:
            assert counts[cfg] == 0
        elif feat in ("none", "out_f32"):
            assert counts[cfg] >= 3, f"{cfg} ran {feat} on {counts[cfg]} of the four shapes"
    assert sum(counts.values()) > 0, f"{feat}: no variant ran it"
    _report(failures)


def test_only_the_sixteen_wave_tile_has_no_exact_form(L):
    """every built variant but the folded-LayerNorm-only tile is approved for `none` and `out_f32` on at least three of the four shapes"""
    assert NO_EXACT_FORM == [(26256, 320, 1)] and len(GEMM_V) >= 20
    for feat in exo.GEMM_FEATURES:
        cells = [dm.GemmCell(feat, s, torch.bfloat16, exact=True) for s in exo.gemm_shapes(feat)]
        for cfg in GEMM_V:
            n = sum(c.variant_ok(cfg) for c in cells)
            if cfg in NO_EXACT_FORM:
                assert n == 0, (cfg, feat, n)
            elif feat in ("none", "out_f32"):
                assert n >= 3, (cfg, feat, n)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("feat", ["bias_residual", "residual_inplace"])
def test_gemm_rounds_once_under_cancellation(L, dtype, feat):
    """residual = round_T(noise - (x w^T + bias)), noise = +-k 2^-10 with k in 32 .. 96: the sum is the noise plus the residual's own rounding,
    exact in fp32.  A kernel that rounds acc + bias to T before it adds the residual is off by up to half a unit of acc -- hundreds of units
    of the sum; control (a) shows on the CPU that such a kernel would fail on more than a quarter of the elements.  Every variant that takes
    a residual, out of place (with a bias) and in place."""
    failures = []
    ran = collections.Counter()
    for shape in CANCEL_SHAPES:
        cell = dm.GemmCell(feat, shape, dtype, exact=True)
        pre = exo.gemm_statement(cell.x, cell.w, cell.bias)
        cell.res = exo.cancelling_residual(pre, dtype)
        cell.ref = pre + cell.res.double()
        cell.assert_premise()
        twice = exo.control_round_before_residual(pre, cell.res, dtype)
        assert float((twice != exo.expected(cell.ref, dtype)).double().mean()) > 0.25
        for cfg in GEMM_V:
            if cell.variant_ok(cfg):
                _run(cell, cfg, dtype, f"cancellation {feat} {shape} {cfg}", failures)
                ran[cfg] += 1
    print(f"\n[exact] gemm cancellation {feat} {dtype}: shapes run per variant {dict(ran)}")
    assert all(ran[cfg] == len(CANCEL_SHAPES) for cfg in GEMM_V if cfg not in NO_EXACT_FORM), dict(ran)
    _report(failures)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("feat", ["none", "x2"])
@pytest.mark.parametrize("n", [128, 192])
def test_gemm_permutation_passes_every_mantissa_bit(L, dtype, feat, n):
    """w = a one-hot permutation matrix (N = K = n), x = full-mantissa normals: y is x[:, perm] bit for bit, on every variant (the plain
    tiles at splits 1, 2 and 4 and the split wave-specialised tile among them), from one token source and from two"""
    failures = []
    cell = dm.GemmCell(feat, (PERM_M, n, n), dtype, exact=True)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(7)).to(dm.DEV)
    cell.x = exo.full_mantissa((PERM_M, n), 41, dtype).to(dm.DEV)
    cell.w = torch.zeros(n, n, dtype=dtype, device=dm.DEV)
    cell.w[torch.arange(n, device=dm.DEV), perm] = 1.0
    cell.ref = cell.x.double()[:, perm]
    assert torch.equal(exo.expected(cell.ref, dtype), cell.x[:, perm])
    ran = [cfg for cfg in GEMM_V if cell.variant_ok(cfg)]
    for cfg in ran:
        _run(cell, cfg, dtype, f"permutation {feat} n={n} {cfg}", failures)
    assert {1, 2, 4} <= {cfg[2] for cfg in ran}
    if feat == "none":
        assert set(ran) == set(GEMM_V) - set(NO_EXACT_FORM)
    _report(failures)


def test_zz_cells_run_per_variant(L):
    """printed for the record: how many (feature, shape) cells each variant ran exactly in this process (0 == nothing selected before this test)"""
    print("\n[exact] gemm cells run per variant: " + ", ".join(f"{cfg}: {RAN[cfg]}" for cfg in GEMM_V))
    assert not RAN or all(RAN[cfg] > 0 for cfg in GEMM_V if cfg not in NO_EXACT_FORM), dict(RAN)
