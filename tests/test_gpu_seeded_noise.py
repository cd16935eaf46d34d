"""GPU: the seeded step noise -- the stand-alone fill (imh_randn_seeded), the seeded step (imh_step_seeded) and the device-resident loop
under a seeded schedule (DenoiseEngine.set_schedule(seeded_noise=True)).

1. the fill's raw words equal the numpy restatement bit for bit, dense and under guarded placement;
2. the fill's normals against the float64 restatement;          3. a sample's noise does not depend on its place in the batch;
4. the statistics of one fill;                                   5. the seeded step equals the bank step fed the fill's row, bit for bit;
6. seeded trajectories are the bank trajectories (and match the oracle);   7. image-to-image / inpainting read rows t_start ..;
8. a seed reproduces its latents;   9. the CFG-split pair;   10. two-stage PNS with the step noise derived from the candidate seed."""
import itertools

import numpy as np
import pytest
import torch

from conftest import record_parity, rel_rms
from guarded import run_dense_and_guarded
from oracle.detfill import det_randn
from oracle.pipeline import denoise as oracle_denoise
from test_gpu_multistep import HW32, STEPS, _inputs, _pair, _product_scheduler, _reference_scheduler
from test_seeded_noise_host import CEILING, moments_ok

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_CACHE = {}

# 2. max |z_gpu - z_ref| over the 2^20-normal fill of (seed 42, lane 0, row 0), measured on an MI355X: 4.768e-7 = 2^-21 (one fp32 ulp at
# |z| in [4, 8)).
# The test holds 4 x that, and never more than the ceiling 1e-5 = 29 ulps at the largest magnitude 5.77 -- several times what
# ulp-accurate log / sqrt / sincospi can produce, so that a fast intrinsic cannot hide.
FILL_MEASURED = 4.768e-7
FILL_BOUND = CEILING if FILL_MEASURED is None else min(4 * FILL_MEASURED, CEILING)


def _rows(seeds, lanes=None):
    from imagharmony_amd import noise
    return torch.from_numpy(noise.seed_rows(seeds, lanes).view(np.int32)).to(DEV)


def _ctx(dtype=torch.bfloat16):
    from imagharmony_amd.ctx import Ctx
    if ("ctx", dtype) not in _CACHE:
        _CACHE["ctx", dtype] = Ctx(DEV, dtype)
    return _CACHE["ctx", dtype]


def _fill(seeds, lanes, HW, row, raw=False):
    """a fresh tensor (not pool memory) [S, 4, HW]"""
    out = torch.empty(len(seeds), 4, HW, dtype=torch.int32 if raw else torch.float32, device=DEV)
    return _ctx().randn_seeded(_rows(seeds, lanes), HW, row=row, raw=raw, out=out)


def _big_fill():
    """the 2^20 normals of (42, lane 0, row 0), S = 1, HW = 262144: one launch shared by tests 2 and 4"""
    if "big" not in _CACHE:
        _CACHE["big"] = _fill([42], None, 262144, 0).cpu().numpy()
    return _CACHE["big"]


# ------------------------------------------------------------------------------------ 1. raw words
@pytest.mark.parametrize("HW", [35, 1024])
def test_fill_words_equal_the_restatement_dense_and_guarded(HW):
    """S = 2: (42, lane 0) and (2^63 + 5, lane 3).  HW = 35: 140 elements per sample, quads straddle the channel boundaries, one partial
    block; HW = 1024: 2048 quads, several blocks.  The row as an immediate and through *step, rows 0 and 3."""
    from imagharmony_amd import lib as L
    from imagharmony_amd import noise
    from test_gpu_guarded_ops import settle
    seeds, lanes = [42, 2 ** 63 + 5], [0, 3]
    rows = _rows(seeds, lanes)
    for via_step, row in itertools.product((False, True), (0, 3)):
        def body(ctx, put, out):
            y = out((2, 4, HW), torch.int32)
            step = None
            if via_step:
                step = out((1,), torch.int32)
                ctx.ew(L.EW_STEP_SET, step, i=(row, 1, 0, 0, 0, 0))
            ctx.randn_seeded(put(rows), HW, row=17 if via_step else row, step=step, raw=True, out=y)
            return y
        what = f"randn_seeded raw HW={HW} row={row} via_step={via_step}"
        dense, guarded, arena = run_dense_and_guarded(DEV, torch.bfloat16, body)
        settle(dense, guarded, arena, what)
        want = noise.seeded_words(seeds, row, (4, HW), lanes)
        assert np.array_equal(dense[0].cpu().numpy().view(np.uint32), want), what


# ------------------------------------------------------------------------------------ 2. normals
def test_fill_normals_match_the_float64_restatement():
    from imagharmony_amd import noise
    z = _big_fill()
    ref = noise.seeded_randn([42], 0, (4, 262144))
    err = float(np.abs(z.astype(np.float64) - ref.astype(np.float64)).max())
    print(f"seeded_noise.fill: max |z_gpu - z_ref| over 2^20 normals = {err:.3e} (bound {FILL_BOUND:.3e}, ceiling {CEILING:g})")
    record_parity("seeded_noise.fill.max_abs", err, FILL_BOUND, ceiling=CEILING, n=int(z.size))
    assert np.isfinite(z).all() and FILL_BOUND <= CEILING and err <= FILL_BOUND, err


# ------------------------------------------------------------------------------------ 3. position independence
def test_a_samples_noise_does_not_depend_on_its_place_in_the_batch():
    for HW in (35, 1024):
        alone = _fill([42], [0], HW, 3)
        pair = _fill([7, 42], [0, 0], HW, 3)
        assert torch.equal(alone[0], pair[1]) and not torch.equal(pair[0], pair[1])
        # lane and row are part of the function
        assert not torch.equal(_fill([42], [1], HW, 3), alone) and not torch.equal(_fill([42], [0], HW, 2), alone)


# ------------------------------------------------------------------------------------ 4. statistics
def test_fill_statistics():
    """the conditions of the CPU test (5 sigma of each statistic at N = 2^20) on one GPU fill, and its rows / seeds uncorrelated"""
    from test_seeded_noise_host import PROD_TOL
    z = _big_fill()
    ok, (m, dv, m4) = moments_ok(z)
    print(f"GPU fill seed 42 row 0: mean {m:.2e}, var - 1 {dv:.2e}, E z^4 {m4:.4f}")
    assert ok, (m, dv, m4)
    a = z.astype(np.float64).ravel()
    b = _fill([42], None, 262144, 1).cpu().numpy().astype(np.float64).ravel()
    c = _fill([43], None, 262144, 0).cpu().numpy().astype(np.float64).ravel()
    assert abs((a * b).mean()) <= PROD_TOL and abs((a * c).mean()) <= PROD_TOL


# ------------------------------------------------------------------------------------ 5. the seeded step == the bank step
@pytest.mark.parametrize("blend", [0, 1, 2], ids=["plain", "blend1", "blend2"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_seeded_step_equals_bank_step_bit_for_bit(dtype, blend):
    """IMH_EW_CFG_MSTEP fed the fill's row as its bank (every other bank row NaN) against imh_step_seeded on the same operands: CFG, rescale
    factor and history on / off, rows 0, 1, 3, HW = 35 and 1024, S = 2 with lanes (0, 3).  x' and h' bit-equal; the seeded run also under
    guarded placement (guards intact, same bits).  At row 3 without the rescale factor cn is 0 -- the row that generates nothing."""
    from imagharmony_amd import lib as L
    from imagharmony_amd.ctx import Ctx
    from test_gpu_guarded_ops import settle
    ctx = Ctx(DEV, dtype)
    S, NR, G = 2, 4, 4.0
    seeds, lanes = [42, 2 ** 63 + 5], [0, 3]
    rows = _rows(seeds, lanes)
    nan = float("nan")
    for k, (HW, cfg, use_w, use_h, row) in enumerate(itertools.product((35, 1024), (1, 0), (False, True), (True, False), (0, 1, 3))):
        g = torch.Generator().manual_seed(1000 * blend + k)
        rn = lambda *s: torch.randn(*s, generator=g)
        lat, h0, z, nz = (rn(S, 4, HW).to(DEV) for _ in range(4))
        npred = rn((2 if cfg else 1) * S, HW, 4).to(dtype).to(DEV)
        wf = torch.tensor([0.8, 1.1], device=DEV)
        tab = torch.full((NR, 6), nan)
        tab[row] = torch.tensor([0.9, -0.3, 0.45, 0.7, 1.6, -1.2]) + 0.1 * rn(6)
        if row == 3 and not use_w:
            tab[row, 3] = 0.0
        tab = tab.to(DEV)
        btab = torch.full((NR, 2), nan)
        btab[row] = torch.tensor([0.6, 0.8])
        btab = btab.to(DEV)
        mask = (torch.rand(max(blend, 1), HW, generator=g) > 0.5).float().to(DEV)
        bank = torch.full((NR, S, 4, HW), nan, device=DEV)
        bank[row] = _fill(seeds, lanes, HW, row)
        step = torch.full((1,), row, dtype=torch.int32, device=DEV)
        common = dict(i=(S, HW, 0, int(cfg), blend, 0), f=(0.0, 0.0, G, 0.0))
        y_b, h_b = lat.clone(), h0.clone() if use_h else None
        kw = dict(x2=z, noise=nz, mask=mask, blend_tab=btab) if blend else {}
        ctx.ew(L.EW_CFG_MSTEP, y_b, a=npred, w=wf if use_w else None, tab=tab, step=step, hist=h_b, bank=bank, **common, **kw)

        def body(c, put, out):
            y = out((S, 4, HW), torch.float32)
            y.copy_(lat)
            hist = None
            if use_h:
                hist = out((S, 4, HW), torch.float32)
                hist.copy_(h0)
            bkw = dict(x2=put(z), noise=put(nz), mask=put(mask), blend_tab=put(btab)) if blend else {}
            c.ew(L.EW_CFG_MSTEP, y, a=put(npred), w=put(wf) if use_w else None, tab=put(tab), step=put(step), hist=hist, seeds=put(rows),
                 **common, **bkw)
            return (y, hist) if use_h else y
        what = f"step_seeded {dtype} blend={blend} HW={HW} cfg={cfg} w={use_w} h={use_h} row={row}"
        dense, guarded, arena = run_dense_and_guarded(DEV, dtype, body)
        settle(dense, guarded, arena, what)
        assert torch.equal(dense[0], y_b) and not torch.equal(y_b, lat), what + ": x'"
        if use_h:
            assert torch.equal(dense[1], h_b) and not torch.equal(h_b, h0), what + ": h'"
    with pytest.raises(L.ImhError, match="seeds"):                               # the bank and the seeds exclude each other
        ctx.ew(L.EW_CFG_MSTEP, lat.clone(), a=npred, tab=tab, step=step, bank=bank, seeds=rows, **common)
    with pytest.raises(L.ImhError, match="seeds"):
        ctx.ew(L.EW_CFG_STEP, lat.clone(), a=npred, seeds=rows, **common)


# ------------------------------------------------------------------------------------ 6. trajectories
SEED = 42


def _fill_rows(seeds, lanes, first=0):
    """[STEPS - first, S, 4, HW32, HW32]: rows first .. STEPS - 1 of the fill, what a bank engine is fed"""
    return torch.stack([_fill(seeds, lanes, HW32 * HW32, r).view(len(seeds), 4, HW32, HW32) for r in range(first, STEPS)], 0)


def _oracle_seeded(kind):
    """the fp32 oracle trajectory with the restatement's rows as the scheduler's noise: once per scheduler"""
    from imagharmony_amd import noise
    if ("oracle", kind) not in _CACHE:
        ou, _, ocfg = _pair(torch.float16)
        lat, pe, ne, po, no = _inputs(ocfg)
        rows = torch.from_numpy(np.stack([noise.seeded_randn([SEED], r, (4, HW32, HW32)) for r in range(STEPS)], 0))
        with torch.no_grad():
            _CACHE["oracle", kind] = oracle_denoise(ou, _reference_scheduler(kind, noise=rows), lat, pe, ne, po, no, HW32 * 8, HW32 * 8,
                                                    num_inference_steps=STEPS, guidance_scale=5.0)
    return _CACHE["oracle", kind]


def _engine(dtype, graph=True, role=None):
    from imagharmony_amd.denoise import DenoiseEngine
    _, hu, ocfg = _pair(dtype)
    lat, pe, ne, po, no = _inputs(ocfg)
    eng = DenoiseEngine(hu, DEV, dtype, use_graph=graph)
    eng.set_conditioning(pe.to(DEV), ne.to(DEV), po.to(DEV), no.to(DEV), HW32 * 8, HW32 * 8, guidance_scale=5.0, cfg_role=role)
    return eng, lat


# the bounds tests/test_gpu_multistep.py holds for these samplers: the seeded noise differs from a bank's by at most
# the fill's ceiling, so they carry over.          measured on an MI355X with the seeded rows
ORACLE_BOUND = {("sde-dpmpp2m", torch.float16): 6.2e-3,     # 3.161e-3 (graph and eager)
                ("sde-dpmpp2m", torch.bfloat16): 5.0e-2,    # 2.474e-2
                ("euler-a", torch.float16): 6.5e-3,         # 3.288e-3
                ("euler-a", torch.bfloat16): 5.6e-2}        # 2.794e-2


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("kind", ["euler-a", "sde-dpmpp2m"])
def test_seeded_trajectory_is_the_bank_trajectory(kind, dtype, graph):
    """text-to-image, 4 steps, tiny UNet: the seeded engine's latents equal, bit for bit, those of the bank plan of the same engine fed the
    fill's rows; same launch count, the last tags cfg+mstep+seeded / step++, no bank allocated; the two plans coexist in the cache.
    Against the fp32 oracle driven by the restatement's rows: the bounds test_gpu_multistep.py holds for these samplers."""
    eng, lat = _engine(dtype, graph)
    sch = _product_scheduler(kind)
    eng.set_schedule(sch, STEPS, seeded_noise=True)
    out = eng.denoise(lat, step_seeds=[SEED]).clone()
    plan_s = eng.plan
    tags = [t[2] for t in plan_s.tags]
    size = plan_s.lib.imh_plan_size(plan_s.plan)
    assert tags[-2:] == ["cfg+mstep+seeded", "step++"] and size == len(tags)
    assert plan_s.lib.imh_plan_get_kind(plan_s.plan, size - 2) == 10
    assert eng.seeded and eng.st.noise_bank is None and tuple(eng.st.seed_rows.shape) == (1, 4)
    assert (eng.st.hist is not None) == (kind == "sde-dpmpp2m")
    eng.set_schedule(sch, STEPS)
    bank = eng.denoise(lat, step_noise=_fill_rows([SEED], None)).clone()
    plan_b = eng.plan
    tb = [t[2] for t in plan_b.tags]
    assert plan_b is not plan_s and tb[-2:] == ["cfg+mstep", "step++"] and tb[:-2] == tags[:-2]
    assert plan_b.lib.imh_plan_size(plan_b.plan) == size and eng.st.noise_bank is not None and eng.st.seed_rows is None
    assert torch.isfinite(out).all() and torch.equal(out, bank)
    eng.set_schedule(sch, STEPS, seeded_noise=True)                      # back: the cached plan, the same bits
    assert eng.plan is plan_s and torch.equal(eng.denoise(lat, step_seeds=[SEED]), out)
    r = rel_rms(out.float().cpu(), _oracle_seeded(kind))
    bound = ORACLE_BOUND[kind, dtype]
    name = f"seeded_noise.t2i.{kind}.{str(dtype).split('.')[-1]}.{'graph' if graph else 'eager'}"
    print(f"{name}: rel-rms vs oracle {r:.3e} (bound {bound:g})")
    record_parity(name, r, bound)
    assert r < bound, (name, r)


# ------------------------------------------------------------------------------------ 7. start row
@pytest.mark.parametrize("mode", ["img2img", "inpaint"])
def test_an_edit_reads_the_rows_from_t_start_on(mode):
    """Euler ancestral; image-to-image from t_start = 2 of 4, the inpainting blend from t_start = 1: the device step counter is the
    row, so the seeded run equals the bank engine fed the fill's rows t_start .. 3 -- and differs from one fed rows 0 .."""
    dtype = torch.float16
    eng, lat = _engine(dtype)
    sch = _product_scheduler("euler-a")
    t_start = 2 if mode == "img2img" else 1
    kw = dict(t_start=t_start, inpaint=mode == "inpaint")
    moments, n1, n2 = det_randn((1, HW32, HW32, 8), 31), det_randn((1, 4, HW32, HW32), 32), det_randn((1, 4, HW32, HW32), 33)
    mask = torch.zeros(1, 1, HW32, HW32)
    mask[..., 8:24, 8:24] = 1

    def run(**noise_kw):
        if mode == "inpaint":
            eng.prepare_inpaint(moments, n1, n2, 0.13025, *sch.add_noise_coefficients(t_start), mask)
            return eng.denoise(None, **noise_kw).clone()
        return eng.denoise(lat, **noise_kw).clone()
    eng.set_schedule(sch, STEPS, seeded_noise=True, **kw)
    out = run(step_seeds=[SEED])
    assert [t[2] for t in eng.plan.tags][-2] == ("cfg+mstep+seeded+blend" if mode == "inpaint" else "cfg+mstep+seeded")
    assert eng.t_start == t_start and eng.st.noise_bank is None
    eng.set_schedule(sch, STEPS, **kw)
    right = run(step_noise=_fill_rows([SEED], None, first=t_start))
    wrong = run(step_noise=_fill_rows([SEED], None)[:STEPS - t_start])
    assert torch.isfinite(out).all() and torch.equal(out, right) and not torch.equal(out, wrong)


# ------------------------------------------------------------------------------------ 8. reproducibility
def test_a_seed_reproduces_its_latents():
    eng, lat = _engine(torch.float16)
    eng.set_schedule(_product_scheduler("sde-dpmpp2m"), STEPS, seeded_noise=True)
    a = eng.denoise(lat, step_seeds=[SEED]).clone()
    assert torch.equal(eng.denoise(lat, step_seeds=[SEED]), a)
    other = eng.denoise(lat, step_seeds=[SEED + 1]).clone()
    assert not torch.equal(other, a)
    assert torch.equal(eng.denoise(lat, step_seeds=[SEED]), a)             # after an interleaved denoise of another seed
    assert not torch.equal(eng.denoise(lat, step_seeds=[SEED], step_lanes=[1]), a)
    fk = eng.fork()
    assert fk.seeded and fk.st.seed_rows is not None and fk.st.seed_rows is not eng.st.seed_rows and fk.st.noise_bank is None
    assert torch.equal(fk.denoise(lat, step_seeds=[SEED]), a)
    from imagharmony_amd import lib as L
    with pytest.raises(L.ImhError, match="step_seeds"):
        eng.denoise(lat)
    with pytest.raises(L.ImhError, match="generator"):
        eng.denoise(lat, generator=torch.Generator().manual_seed(1), step_seeds=[SEED])


# ------------------------------------------------------------------------------------ 9. CFG split
# the tolerances of test_denoise_cfg_split_over_two_engines_matches_the_fused_step (tests/test_gpu_pipeline.py), borrowed; measured here
# on an MI355X (rel-RMS of the pair against the fused seeded engine): 0 in fp16 and in bf16 (at
# this size the batch-1 halves and the fused batch-2 forward give the same bits)
@pytest.mark.parametrize("dtype,tol", [(torch.float16, 6e-3), (torch.bfloat16, 4e-2)], ids=["fp16", "bf16"])
def test_cfg_split_pair_under_euler_ancestral_with_seeds(dtype, tol):
    """two engines with cfg_role 0 / 1 under a seeded Euler-ancestral schedule: each generates the identical noise from the seed, so
    the latents of the two stay bit-equal without an exchanged bank; `a` runs the blocking entry (denoise_cfg_split(step_seeds=...)),
    whose exchange steps `b` in lockstep on the same GPU"""
    from imagharmony_amd import lib as L
    sch = _product_scheduler("euler-a")
    fused_eng, lat = _engine(dtype)
    fused_eng.set_schedule(sch, STEPS, seeded_noise=True)
    fused = fused_eng.denoise(lat, step_seeds=[SEED]).float().cpu().clone()
    (a, _), (b, _) = _engine(dtype, role=0), _engine(dtype, role=1)
    for e in (a, b):
        e.set_schedule(sch, STEPS)
        with pytest.raises(NotImplementedError, match="stochastic"):          # a bank schedule is still refused
            e.denoise_cfg_split(lat, None, step_seeds=[SEED])
        e.set_schedule(sch, STEPS, seeded_noise=True)
    b._record()
    b.st.latents.copy_(lat.to(DEV, torch.float32) * b.init_noise_sigma)
    b._start_general_step(step_seeds=[SEED])
    b.eager.ew(L.EW_STEP_SET, b.st.step, i=(0, 1, 0, 0, 0, 0), descr="step=0")
    equal = []

    def exchange(mine):
        b.plan.replay()
        un, co = mine.clone(), b.noise_pred.clone()
        b.np_full[0].copy_(un); b.np_full[1].copy_(co)
        b.plan_tail.replay()
        equal.append(None)
        return un, co
    out = a.denoise_cfg_split(lat, exchange, step_seeds=[SEED])
    assert len(equal) == STEPS and torch.equal(out, b.st.latents)
    assert [t[2] for t in a.plan_tail.tags] == ["cfg+mstep+seeded", "step++"] and a.st.noise_bank is None
    r = rel_rms(out.float().cpu(), fused)
    print(f"seeded CFG-split pair {dtype}: rel-rms vs the fused seeded engine {r:.3e} (tolerance {tol:g})")
    record_parity(f"seeded_noise.cfg_split.{str(dtype).split('.')[-1]}", r, tol)
    assert torch.isfinite(out).all() and r < tol


# ------------------------------------------------------------------------------------ 10. PNS
def test_two_stage_pns_with_step_noise_from_the_candidate_seed():
    from imagharmony_amd import pns
    eng, _ = _engine(torch.float16)
    sch = _product_scheduler("euler-a")
    shape = (1, 4, HW32, HW32)
    preview, final = pns.two_stage_fns(eng, sch, preview_steps=2, final_steps=STEPS, step_noise="seed")
    runs = [pns.run_pns(preview, [3, 9, 27], shape, device=DEV, final_fn=final, batch=1, pass_seeds=True) for _ in range(2)]
    assert torch.equal(runs[0]["scores"], runs[1]["scores"]) and runs[0]["best_seed"] == runs[1]["best_seed"]
    assert torch.equal(runs[0]["latents"], runs[1]["latents"]) and torch.isfinite(runs[0]["latents"]).all()
    assert len(set(runs[0]["scores"].tolist())) == 3
    best = runs[0]["best_seed"]
    eng.set_schedule(sch, STEPS, seeded_noise=True)
    direct = eng.denoise(pns.seed_latents(best, shape), step_seeds=[best])
    assert torch.equal(direct.float(), runs[0]["latents"].to(DEV))
    with pytest.raises(ValueError, match="pass_seeds"):                       # the seeds must reach the stage functions
        pns.run_pns(preview, [3], shape, device=DEV)
