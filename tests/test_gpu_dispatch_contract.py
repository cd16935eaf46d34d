"""GPU: the dispatch contract.  Every kernel sits behind two gatekeepers written by hand in two languages -- the launch validators of
csrc/ (gemm_launch, gemm_w16_launch, conv_halo_launch, conv_hws_launch, gemm_pp_launch) and their mirror in imagharmony_amd/ctx.py
(_variant_ok, _config, the stats_out condition, the x2 / yt fallbacks, _gn_epilogue, conv_fuses_gn, conv_up_phase_cfg).  This module
sweeps variant x feature and holds them to one statement: Ctx never approves a launch the library refuses.

  forced (cfg=V):  the call matches float64, or raises ImhError with the output and every side output bit-untouched -- eagerly and while
                   recording, where the refusal comes at the recording call; where Ctx._variant_ok(V, ...) is True the library accepts
  auto (cfg=None): V is the tuning-table entry of the shape; no refusal reaches the caller, the result matches float64, the launch ran on
                   V or on a fallback; a request no variant serves is a Python-side ImhError naming the rule, before anything is emitted
  conv_fuses_gn:   True  =>  the fused launch runs and is right, across the LDS limit of both kernel families

References: matmul / F.layer_norm / F.group_norm / GEGLU / SiLU / im2col conv in float64 on the device; bounds are those of the existing
tests of the same op and dtype (test_gpu_ops assert_close k = 4, folded LayerNorm 6, + GEGLU 8, fused GroupNorm conv 6; _check_stats,
_check_partials)."""
import collections

import pytest
import torch

import dispatch_matrix as dm
from conftest import built
from test_gpu_guarded_ops import CONV_VARIANTS
from test_gpu_ops import BIG_VARIANTS, DTYPES, L  # noqa: F401

pytestmark = pytest.mark.gpu

GEMM_V = dm.gemm_variants(built(BIG_VARIANTS))
CONV_V = dm.conv_variants(built(CONV_VARIANTS))
HALO_V = [v for v in CONV_V if v[0] in dm.Ctx._HALO]
COUNTS = collections.Counter()          # cells per part, refusals, "library would accept, Python declines" (printed; the PR summary quotes them)
DECLINED = []


def _known_good(ctx, dtype):
    """after a refusal the same context runs one plain launch correctly"""
    from test_gpu_ops import assert_close
    x, w = dm.rnd(64, 64, dtype=dtype, seed=7), dm.rnd(64, 64, dtype=dtype, seed=8, scale=0.125)
    y = torch.empty(64, 64, dtype=dtype, device=dm.DEV)
    n = ctx.lib.imh_plan_size(ctx.plan) if ctx.record else 0
    ctx.gemm(x, w, out=y, cfg=(64, 64, 1))
    if ctx.record:
        assert ctx.lib.imh_plan_size(ctx.plan) == n + 1
        ctx.run()
    torch.cuda.synchronize()
    assert_close(y, x.double() @ w.double().t(), dtype, "known-good launch after a refusal")


def _forced(cell, cfg, dtype, record, what, part):
    """one forced cell -> True (accepted and right) / False (cleanly refused)"""
    arena = dm.fresh_arena()
    ctx = dm.ArenaCtx(arena, dtype, record=record)
    ok = cell.variant_ok(cfg)
    try:
        res = cell.call(ctx, cfg=cfg)
    except dm.L.ImhError as e:
        torch.cuda.synchronize()
        assert not ok, f"{what}: Ctx._variant_ok approves what the call refuses: {e}"
        clean, where = dm.outputs_untouched(arena)
        assert clean, f"{what}: refused ({e}) but {where} was written"
        if record:          # the refusal came at the recording call: nothing of the launch is in the plan, and what is there replays
            assert not [t for t in ctx.tags if t[1] == dm.L.OP_GEMM], f"{what}: the refused launch reached the plan"
            ctx.run()
            torch.cuda.synchronize()
        _known_good(ctx, dtype)
        COUNTS[part + " refused"] += 1
        return False
    if record:
        ctx.run()
    torch.cuda.synchronize()
    arena.check()
    cell.check(*res, what) if isinstance(cell, dm.GemmCell) else cell.check(*res, what, cfg_used=cfg)
    if not ok:
        COUNTS[part + " library accepts, Python declines"] += 1
        DECLINED.append(what)
    COUNTS[part + " accepted"] += 1
    return True


# ------------------------------------------------------------------------------------ 5: the matrix tests something (library rules, no GPU work)
def _lib_rule_gemm(cfg, feat, shape=dm.WHOLE):
    """does gemm_launch / the variant's launcher take `feat` on cfg at `shape`?  (csrc/gemm.hip gemm_launch, gemm_w16.hip gemm_w16_launch,
    gemm_pp.hip gemm_pp_launch restated once, for the honesty check and for the requests no variant serves: the GPU tests decide by running)"""
    bm, bn, sp = cfg
    M, N, K = shape
    plain, ws, pp, w16 = bm <= 128, bm in (1464, 2464, 24128, 23256, 22128), bm in (8256, 9128, 9256), bm == 26256
    if w16:
        return feat in ("ln_row", "ln_row_stats", "ln_geglu") and M % 256 == 0 and N % 320 == 0
    if feat in ("ln_row", "ln_row_stats", "ln_geglu", "ln_stats_out"):
        return sp == 1 and (plain or ws)
    if feat == "ln_col":
        return sp == 1 and plain
    if feat == "vt_perm":
        return plain
    if feat == "x2":
        return plain or ws
    if feat == "yt":          # whole tiles, and col0 = N / 2 a multiple of bn (at N = 640: not 23256 x 128)
        rows = 256 if bm == 23256 else 128 if bm in (24128, 22128) else 64
        return ws and (bn == 160 or (bm, bn) == (23256, 128)) and sp == 1 and M % rows == 0 and N % bn == 0 and (N // 2) % bn == 0
    return not (pp and sp > 1)


def _lib_rule_conv(cfg, feat, shape):
    """the same for conv3x3 (csrc/api.hip do_gemm: pad mode 1 and the phase form; gemm.hip gemm_launch: the phase variants, the fused GroupNorm
    front end and the second source on the LDS-halo kernels only; conv_halo.hip conv_halo_launch: stride 1, no split-K, the LDS limit;
    gemm_pp.hip / gemm_w16.hip: no conv; the plain tiles and the ring family take every stride, pad mode and up = 1).  The LDS-halo family is
    whatever the library's own byte count knows as one"""
    bm, bn, sp = cfg
    B, H, W, Cin, Cout = shape
    lib = dm.L.load()
    if bm in (8256, 9128, 9256, 26256):
        return False
    if feat == "up2":
        ws = bm in (1464, 2464, 24128, 23256)
        return sp == 1 and ((ws and bn == 160) or (bm, bn) in ((23256, 128), (5258, 320))) and Cout % bn == 0 and Cout % 8 == 0 and Cin % 64 == 0
    front = feat in ("gn_table", "gn_spec", "x2")
    if front and feat == "x2":
        Cin = max(Cin, 128)          # (ConvCell: two sources of at least 64 channels each)
    if lib.imh_conv_halo_lds_bytes(bm, bn, Cin, 0) < 0:          # not an LDS-halo variant
        return not front
    if feat in ("s2", "pad1") or sp != 1 or Cin % 64:
        return False
    return lib.imh_conv_halo_lds_bytes(bm, bn, Cin, int(feat != "x2" and front)) <= 160 * 1024


def test_matrix_is_not_vacuous():
    """every variant has an accepted forced cell and every feature is accepted by some variant, from the library's rules"""
    assert len(GEMM_V) >= 20 and len(HALO_V) >= 4 and len(CONV_V) > len(HALO_V), (GEMM_V, CONV_V)
    for v in GEMM_V:
        assert any(_lib_rule_gemm(v, f, s) for f in dm.GEMM_FEATURES for s in dm.gemm_shapes(f)), v
    for f in dm.GEMM_FEATURES:
        assert any(_lib_rule_gemm(v, f, s) for v in GEMM_V for s in dm.gemm_shapes(f)), f
    for v in CONV_V:
        assert any(_lib_rule_conv(v, f, s) for f in dm.CONV_FEATURES for s in dm.CONV_SHAPES), v
        assert any(_lib_rule_conv(v, "s1", s) for s in dm.CONV_SHAPES), v
    for f in dm.CONV_FEATURES:
        assert any(_lib_rule_conv(v, f, s) for v in CONV_V for s in dm.CONV_SHAPES), f
    # the families the library's rules tell apart are all there: LDS-halo (the fused front end), the phase tiles (up = 2), the rest (stride 2, pad 1)
    assert {v[0] for v in HALO_V} == {v[0] for v in CONV_V if dm.L.load().imh_conv_halo_lds_bytes(v[0], v[1], 64, 0) > 0}


# ------------------------------------------------------------------------------------ 4: forced variant, right or cleanly refused
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("feat", dm.GEMM_FEATURES)
def test_forced_gemm_variant_is_right_or_cleanly_refused(L, dtype, feat):
    accepted = collections.Counter()
    for shape in dm.gemm_shapes(feat):
        cell = dm.GemmCell(feat, shape, dtype)
        for cfg in GEMM_V:
            for record in (False, True):
                what = f"forced gemm {feat} {shape} {cfg} {'record' if record else 'eager'}"
                accepted[cfg] += _forced(cell, cfg, dtype, record, what, "4 gemm")
                COUNTS["4 gemm cells"] += 1
    assert any(accepted.values()), f"{feat}: no variant accepted it"
    for cfg in GEMM_V:
        if _lib_rule_gemm(cfg, feat):
            assert accepted[cfg], f"{feat}: the library's rules take it on {cfg}, no cell was accepted"
    print(f"\n[dispatch] forced gemm {feat}: {dict(COUNTS)}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("feat", dm.CONV_FEATURES)
def test_forced_conv_variant_is_right_or_cleanly_refused(L, dtype, feat):
    accepted = collections.Counter()
    for shape in dm.CONV_SHAPES:
        cell = dm.ConvCell(feat, shape, dtype)
        for cfg in CONV_V:
            for record in (False, True):
                what = f"forced conv {feat} {shape} {cfg} {'record' if record else 'eager'}"
                accepted[cfg] += _forced(cell, cfg, dtype, record, what, "4 conv")
                COUNTS["4 conv cells"] += 1
    assert any(accepted.values()), f"{feat}: no variant accepted it"
    for cfg in CONV_V:
        if any(_lib_rule_conv(cfg, feat, shape) for shape in dm.CONV_SHAPES):
            assert accepted[cfg], f"{feat}: the library's rules take it on {cfg}, no cell was accepted"
    print(f"\n[dispatch] forced conv {feat}: {dict(COUNTS)}")


# ------------------------------------------------------------------------------------ 1: auto-dispatch, GEMM
def _last_gemm_cfg(ctx):
    return [t[6]["cfg"] for t in ctx.tags if t[1] == dm.L.OP_GEMM and t[6] and "cfg" in t[6]][-1]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("feat", dm.GEMM_FEATURES)
def test_auto_dispatch_gemm(L, dtype, feat):
    for shape in dm.gemm_shapes(feat):
        cell = dm.GemmCell(feat, shape, dtype)
        M, N, K = shape
        unservable = not any(_lib_rule_gemm(v, feat, shape) for v in GEMM_V)          # (the ragged yt cell: whole tiles only)
        for cfg in GEMM_V:
            what = f"auto gemm {feat} {shape} table entry {cfg}"
            arena = dm.fresh_arena()
            ctx = dm.ArenaCtx(arena, dtype, record=True)
            ctx.tuning = dict(ctx.tuning)
            ctx.tuning[(M, N, K, 0)] = ctx.tuning[(M, N, K, 0, 1)] = cfg
            if unservable:
                with pytest.raises(dm.L.ImhError, match="Yt .*whole tiles") as ei:
                    cell.call(ctx)
                assert not dm.is_library_refusal(ei.value), f"{what}: ended in a library refusal: {ei.value}"
                assert not [t for t in ctx.tags if t[1] == dm.L.OP_GEMM and t[2] == "gemm"], f"{what}: something was emitted before the refusal"
                COUNTS["1 python-side refusals"] += 1
                COUNTS["1 cells"] += 1
                continue
            try:
                res = cell.call(ctx)
            except dm.L.ImhError as e:
                raise AssertionError(f"{what}: a legal request was refused: {e}") from e
            used = _last_gemm_cfg(ctx)
            ctx.run()
            torch.cuda.synchronize()
            arena.check()
            cell.check(*res, what + f" (ran on {used})")
            assert tuple(used) == cfg or used[0] <= 128 or (used[0], used[1]) in dm.YT_OK, f"{what}: ran on {used}, neither the entry nor a fallback"
            if cell.variant_ok(cfg) and feat not in ("x2", "yt"):
                assert tuple(used) == cfg, f"{what}: _variant_ok approves the entry, the launch ran on {used}"
            COUNTS["1 on the entry" if tuple(used) == cfg else "1 on a fallback"] += 1
            COUNTS["1 cells"] += 1
    print(f"\n[dispatch] auto gemm {feat}: {dict(COUNTS)}")


# ------------------------------------------------------------------------------------ 2: auto-dispatch, conv3x3
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("feat", dm.CONV_FEATURES)
def test_auto_dispatch_conv(L, dtype, feat):
    for shape in dm.CONV_SHAPES:
        cell = dm.ConvCell(feat, shape, dtype)
        B, H, W, Cin, Cout = cell.shape
        for cfg in CONV_V:
            what = f"auto conv {feat} {shape} table entry {cfg}"
            arena = dm.fresh_arena()
            ctx = dm.ArenaCtx(arena, dtype, record=True)
            ctx.tuning = dict(ctx.tuning)
            for key in ((cell.M, Cout, cell.K, 1), (B * H * W, 4 * Cout, 4 * Cin, 1)):
                for k5 in ((), (2,), (3,), (4,)):
                    ctx.tuning[key + k5] = cfg
            try:
                if feat == "up2" and ctx.conv_up_phase_cfg(B, H, W, Cin, Cout) is None:
                    cell1 = dm.ConvCell("up1", shape, dtype)           # unet.py: the up = 1 form when the phase form does not qualify
                    res = cell1.call(ctx)
                    how = "2 up=2 run as up=1"
                elif feat in ("gn_table", "gn_spec", "x2"):
                    fused = ctx.conv_fuses_gn(cell.M, Cout, cell.K)
                    res = cell.call(ctx, fused=fused)
                    how = "2 fused" if fused else "2 as passes"
                else:
                    res = cell.call(ctx)
                    how = "2 plain"
            except dm.L.ImhError as e:
                raise AssertionError(f"{what}: a legal request was refused: {e}") from e
            used = _last_gemm_cfg(ctx)
            ctx.run()
            torch.cuda.synchronize()
            arena.check()
            cell.check(*res, what + f" (ran on {used})", cfg_used=used)
            assert tuple(used) == cfg or used[0] <= 128 or (used[0], used[1]) in dm.Ctx._PHASE, f"{what}: ran on {used}, neither the entry nor a fallback"
            COUNTS[how] += 1
            COUNTS["2 cells"] += 1
    print(f"\n[dispatch] auto conv {feat}: {dict(COUNTS)}")


# ------------------------------------------------------------------------------------ 3: conv_fuses_gn against the library's LDS limit
def _lds_cins(cfg):
    """Cin in steps of 64 across the limit of BOTH kernel families of the variant (the table is 8 Cin bytes of the 160 KB; imh_debug_set
    key 5: 0 = the default routing, 6 = the lock-step kernels for every variant), plus the widths named by the issue: 2240 .. 2560 for the
    16-row patch, 4288 .. 4416 for 7128 x 160"""
    lib = dm.L.load()
    cins = set()
    try:
        for mode in (0, 6):
            lib.imh_debug_set(5, mode)
            lim = (160 * 1024 - lib.imh_conv_halo_lds_bytes(cfg[0], cfg[1], 0, 1)) // 8 // 64 * 64
            cins |= {lim - 64, lim, lim + 64}
    finally:
        lib.imh_debug_set(5, 0)
    if cfg[0] in (7256, 7356):
        cins |= {2240, 2304, 2368, 2560}
    if cfg[:2] == (7128, 160):
        cins |= {4288, 4352, 4416}
    return sorted(c for c in cins if c >= 128)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg", HALO_V)
def test_conv_fuses_gn_agrees_with_the_library_lds_limit(L, dtype, cfg):
    from imagharmony_amd.ctx import Ctx
    missed = []
    B, H, W, Cout = 1, 16, 16, 160
    lib = dm.L.load()
    try:
        for Cin in _lds_cins(cfg):
            for two in (0, Cin // 2 // 64 * 64):
                cell = dm.ConvCell("gn_table", (B, H, W, Cin, Cout), dtype, two_source=two or None)
                for feat in ("gn_table", "gn_spec"):
                    cell.feat = feat
                    for mode in (0, 6):
                        assert lib.imh_debug_set(5, mode) == 0
                        what = f"conv_fuses_gn {cfg} halo mode {mode} Cin {Cin} ({'two sources' if two else 'one source'}, {feat})"
                        arena = dm.fresh_arena()
                        ctx = dm.ArenaCtx(arena, dtype)
                        fuses = Ctx.conv_fuses_gn(ctx, cell.M, Cout, cell.K, cfg=cfg)
                        try:
                            res = cell.call(ctx, cfg=cfg)
                        except dm.L.ImhError as e:
                            torch.cuda.synchronize()
                            assert not fuses, f"{what}: conv_fuses_gn says True, the launch is refused: {e}"
                            assert not dm.is_library_refusal(e), f"{what}: the refusal came from the library: {e}"
                            ctx.conv_fuses_gn = lambda *a, **k: True              # past Python's gate: the library must refuse too, cleanly
                            arena = ctx.arena = dm.fresh_arena()
                            try:
                                res = cell.call(ctx, cfg=cfg)
                            except dm.L.ImhError as e2:
                                torch.cuda.synchronize()
                                assert dm.is_library_refusal(e2) and dm.outputs_untouched(arena)[0], f"{what}: {e2}"
                                COUNTS["3 refused by both"] += 1
                                COUNTS["3 cells"] += 1
                                continue
                            missed.append(what)
                            COUNTS["3 missed fusions"] += 1
                        assert fuses or missed and missed[-1] == what
                        torch.cuda.synchronize()
                        arena.check()
                        cell.check(*res, what)
                        COUNTS["3 fused and right" if fuses else "3 missed fusions and right"] += 1
                        COUNTS["3 cells"] += 1
    finally:
        lib.imh_debug_set(5, 0)
    print(f"\n[dispatch] conv_fuses_gn {cfg}: {dict(COUNTS)}; missed fusions: {missed}")


def test_zz_report():
    """the tallies of the module (cells per part, refusals, cells the library would take and Python declines) add up: every cell of every part
    that ran ended in exactly one of the outcomes its part knows; nothing was left out on the way.  (Counts are of the tests that ran before
    this one in the same process; with none of them selected every identity reads 0 == 0.)"""
    print("\n[dispatch] totals: " + ", ".join(f"{k}: {v}" for k, v in sorted(COUNTS.items())))
    print("[dispatch] library accepts, Python declines: " + "; ".join(sorted(set(w.rsplit(" ", 1)[0] for w in DECLINED))))
    c = COUNTS
    assert c["1 cells"] == c["1 on the entry"] + c["1 on a fallback"] + c["1 python-side refusals"]
    assert c["2 cells"] == c["2 plain"] + c["2 fused"] + c["2 as passes"] + c["2 up=2 run as up=1"]
    assert c["3 cells"] == c["3 fused and right"] + c["3 refused by both"] + c["3 missed fusions and right"]
    assert c["3 missed fusions"] == c["3 missed fusions and right"]
    for part in ("4 gemm", "4 conv"):
        assert c[part + " cells"] == c[part + " accepted"] + c[part + " refused"]
        assert c[part + " library accepts, Python declines"] <= c[part + " accepted"]
    assert len(DECLINED) == c["4 gemm library accepts, Python declines"] + c["4 conv library accepts, Python declines"]
