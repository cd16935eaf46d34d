"""CPU: the multistep and ancestral schedulers (schedulers.DPMSolverMultistepScheduler, EulerAncestralDiscreteScheduler) and the host
logic of the engine around them -- no GPU.

1. the six-column table form (what EW_CFG_MSTEP evaluates) equals the sequential restatement of tests/multistep_reference.py;
2. exactness on a model whose data prediction is constant;
3. order of convergence on the analytic Gaussian-data model;
4. plan keys, blend table, noise-bank draw order, the binding of the new op."""
import itertools
import os
import re

import pytest
import torch

from multistep_reference import RefDPMSolverMultistep, RefEulerAncestral

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OPTIONS = [dict(algorithm_type=alg, solver_order=so, lower_order_final=lof, euler_at_final=eaf, use_karras_sigmas=kar, timestep_spacing=sp)
           for alg, so, lof, eaf, kar, sp in itertools.product(("dpmsolver++", "sde-dpmsolver++"), (2, 1), (True, False), (False, True),
                                                               (False, True), ("leading", "trailing"))]


def _rel(a, b):
    return float((a - b).norm() / b.norm())


def _table_walk(tab, x, eps, noise, t_start):
    """the kernel's arithmetic on the host in float64: x' = cx x + ce eps + ch h + cn z, h' = hx x + he eps, h zeroed before the loop"""
    h = torch.zeros_like(x)
    out = []
    for i in range(t_start, tab.shape[0]):
        c = tab[i]
        x, h = c[0] * x + c[1] * eps[i] + c[2] * h + c[3] * noise[i], c[4] * x + c[5] * eps[i]
        out.append(x)
    return out


# ------------------------------------------------------------------------------------ 1. table form == sequential form
@pytest.mark.parametrize("n", [4, 10, 20, 30])
def test_table_form_equals_sequential_form(n):
    """float64, random eps sequences, every option combination, t_start in {0, 1, n - 1}, the noise rows shared.  An algebraic identity:
    relative error <= 1e-9 per step (float64 rounding times the 1 / alpha <= ~15 amplification leaves orders of magnitude of room).
    The product's own host-side ``step`` is held to the same sequence."""
    from imagharmony_amd import schedulers as hs
    g = torch.Generator().manual_seed(n)
    worst = 0.0
    cases = [(hs.DPMSolverMultistepScheduler, RefDPMSolverMultistep, kw) for kw in OPTIONS] + [(hs.EulerAncestralDiscreteScheduler, RefEulerAncestral, {})]
    for prod, ref, kw in cases:
        p = prod(**kw)
        p.set_timesteps(n)
        for t_start in (0, 1, n - 1):
            x0 = torch.randn(24, generator=g, dtype=torch.float64)
            eps = torch.randn(n, 24, generator=g, dtype=torch.float64)
            noise = torch.randn(n, 24, generator=g, dtype=torch.float64)
            r = ref(t_start=t_start, noise=noise, **kw)
            r.set_timesteps(n)
            assert torch.equal(p.sigmas, r.sigmas) and torch.equal(p.timesteps.double(), r.all_timesteps.double()), (kw, "schedule")
            assert len(r.timesteps) == n - t_start
            tab = p.tables(t_start)
            assert tab["coef6"].dtype == torch.float32 and tuple(tab["coef6"].shape) == (n, 6) and tab["coef"] is None
            c6 = p.table_f64(t_start)
            assert torch.equal(tab["coef6"], c6.float()) and torch.isfinite(tab["coef6"]).all()
            walked = _table_walk(c6, x0, eps, noise, t_start)
            p.set_begin_index(t_start)
            xr, xh = x0, x0
            for k, i in enumerate(range(t_start, n)):
                xr = r.step(eps[i], r.timesteps[k], xr)[0]
                xh = p.step(eps[i], p.timesteps[i], xh, noise=noise[i])[0]
                e = max(_rel(walked[k], xr), _rel(xh, xr))
                worst = max(worst, e)
                assert e <= 1e-9, (kw, t_start, i, e)
            # what the rows must look like: no history term in the first row that runs, noise only where the sampler is stochastic
            assert c6[t_start, 2] == 0.0
            if not p.stochastic:
                assert (c6[:, 3] == 0).all()
            if p.needs_history and n >= 4 and t_start == 0:
                assert (c6[1:n - 1, 2] != 0).all() and c6[n - 1, 2] == 0.0
    print(f"n = {n}: worst relative error {worst:.2e}")


def test_image_to_image_start_changes_exactly_the_first_row_that_runs():
    from imagharmony_amd import schedulers as hs
    p = hs.DPMSolverMultistepScheduler()
    p.set_timesteps(10)
    t0, t3 = p.tables(0)["coef6"], p.tables(3)["coef6"]
    differ = [i for i in range(10) if not torch.equal(t0[i], t3[i])]
    assert differ == [3]
    # a single-order sampler has one table whatever the start
    for q in (hs.DPMSolverMultistepScheduler(solver_order=1), hs.EulerAncestralDiscreteScheduler()):
        q.set_timesteps(10)
        assert torch.equal(q.tables(0)["coef6"], q.tables(3)["coef6"])
    # refused configurations are errors, not silently something else
    for bad in (dict(algorithm_type="dpmsolver"), dict(solver_order=3), dict(solver_type="heun"), dict(final_sigmas_type="sigma_min"),
                dict(timestep_spacing="linspace")):
        with pytest.raises(NotImplementedError):
            hs.DPMSolverMultistepScheduler(**bad)


def test_schedules_follow_the_stated_rules():
    """leading spacing (arange(0, n + 1) * (1000 // (n + 1))).round()[::-1][:-1] + 1; Karras: rho 7 between the first and the last
    training sigma; Euler ancestral: the existing Euler class's schedule"""
    import numpy as np
    from imagharmony_amd import schedulers as hs
    p = hs.DPMSolverMultistepScheduler()
    p.set_timesteps(4)
    assert p.timesteps.tolist() == [801, 601, 401, 201] and p.init_noise_sigma == 1.0 and p.order == 1
    p.set_timesteps(30)
    assert p.timesteps.tolist() == [32 * k + 1 for k in range(30, 0, -1)]
    assert p.sigmas.shape == (31,) and p.sigmas[-1] == 0 and (p.sigmas[:-1] > p.sigmas[1:]).all()
    t = hs.DPMSolverMultistepScheduler(timestep_spacing="trailing")
    t.set_timesteps(4)
    assert t.timesteps.tolist() == [999, 749, 499, 249]
    k = hs.DPMSolverMultistepScheduler(use_karras_sigmas=True)
    k.set_timesteps(20)
    assert abs(float(k.sigmas[0]) - float(k.all_sigmas[-1])) < 1e-5 and abs(float(k.sigmas[19]) - float(k.all_sigmas[0])) < 1e-6
    inv = k.sigmas[:-1].double() ** (1 / 7.0)
    assert float((inv[1:] - inv[:-1]).std() / (inv[1:] - inv[:-1]).mean().abs()) < 1e-5        # equal steps in sigma^(1/7)
    assert k.timesteps[0] == 999 and k.timesteps[-1] == 0 and (k.timesteps[:-1] >= k.timesteps[1:]).all()
    e, a = hs.EulerDiscreteScheduler(), hs.EulerAncestralDiscreteScheduler()
    e.set_timesteps(10)
    a.set_timesteps(10)
    assert torch.equal(e.sigmas, a.sigmas) and torch.equal(e.timesteps, a.timesteps) and e.init_noise_sigma == a.init_noise_sigma
    assert torch.equal(e.tables()["in_scale"], a.tables()["in_scale"])
    assert a.add_noise_coefficients(3) == (1.0, float(a.sigmas[3]))
    al, s = p.add_noise_coefficients(5)
    sg = float(p.sigmas[5])
    assert abs(al - 1 / np.sqrt(sg * sg + 1)) < 1e-12 and abs(s - sg * al) < 1e-12
    assert hs.get_timesteps(p, 30, 0.5)[1] == 15


# ------------------------------------------------------------------------------------ 2. exactness
@pytest.mark.parametrize("kw", [dict(), dict(use_karras_sigmas=True), dict(solver_order=1), dict(timestep_spacing="trailing"),
                                dict(lower_order_final=False, euler_at_final=True)], ids=str)
@pytest.mark.parametrize("n", [4, 10, 20])
def test_constant_data_prediction_is_integrated_exactly(kw, n):
    """a model whose data prediction is the constant x0*: eps = (x - alpha x0*) / s.  Every deterministic step lands on alpha_{i+1} x0* +
    s_{i+1} eps, and the last step returns x0* (float64, 1e-9): pins the signs, the indices and the sigma -> 0 limit"""
    from imagharmony_amd import schedulers as hs
    p = hs.DPMSolverMultistepScheduler(**kw)
    p.set_timesteps(n)
    g = torch.Generator().manual_seed(1)
    x0s = torch.randn(16, generator=g, dtype=torch.float64)
    x = torch.randn(16, generator=g, dtype=torch.float64)
    sg = p.sigmas.double()
    al = 1 / (sg * sg + 1).sqrt()
    s = sg * al
    tab = p.table_f64()
    xt, h = x.clone(), torch.zeros_like(x)
    for i in range(n):
        eps = (x - al[i] * x0s) / s[i]
        want = al[i + 1] * x0s + s[i + 1] * eps
        x = p.step(eps, p.timesteps[i], x)[0]
        assert _rel(x, want) <= 1e-9, (i, _rel(x, want))
        et = (xt - al[i] * x0s) / s[i]
        c = tab[i]
        xt, h = c[0] * xt + c[1] * et + c[2] * h, c[4] * xt + c[5] * et
        assert _rel(xt, want) <= 1e-9 and _rel(h, x0s) <= 1e-9, i
    assert _rel(x, x0s) <= 1e-9 and _rel(xt, x0s) <= 1e-9


# ------------------------------------------------------------------------------------ 3. order of convergence
def _gaussian_endpoint_error(n, solver_order, c):
    """data ~ N(0, c^2) per element: with x = alpha (x0 + sigma n) the ideal prediction is eps(x, sigma) = sigma (x / alpha) / (c^2 +
    sigma^2), and the probability-flow solution is (x / alpha)(sigma) = (x / alpha)(sigma_0) sqrt((c^2 + sigma^2) / (c^2 + sigma_0^2)):
    the exact endpoint at sigma = 0 is closed-form"""
    from imagharmony_amd import schedulers as hs
    p = hs.DPMSolverMultistepScheduler(solver_order=solver_order, use_karras_sigmas=True)
    p.set_timesteps(n)
    sg = p.sigmas.double()
    x = torch.tensor([1.0, -0.5, 2.0], dtype=torch.float64)
    a0 = 1 / (sg[0] ** 2 + 1).sqrt()
    exact = x / a0 * c / (c * c + sg[0] ** 2).sqrt()
    for i in range(n):
        a = 1 / (sg[i] ** 2 + 1).sqrt()
        x = p.step(sg[i] * (x / a) / (c * c + sg[i] ** 2), p.timesteps[i], x)[0]
    return _rel(x, exact)


@pytest.mark.parametrize("c", [0.5, 1.0, 2.0])
def test_order_of_convergence_on_gaussian_data(c):
    """doubling n from 10 to 20 cuts the endpoint error of DPM++ 2M by more than 3x and that of first order by less than 3x.  Karras
    sigmas: they reach the smallest training sigma, so the closing first-order step to sigma = 0 is negligible; on the linear timestep
    grid that one step (from sigma(t ~ 1000 / (n + 1))) dominates the endpoint error of either order and hides the order of the rest.
    A second-order step with a wrong r0 or without its history term fails this."""
    e = {(n, o): _gaussian_endpoint_error(n, o, c) for n in (10, 20) for o in (1, 2)}
    print(f"c = {c}: first order {e[10, 1]:.3e} -> {e[20, 1]:.3e} (x{e[10, 1] / e[20, 1]:.2f}), 2M {e[10, 2]:.3e} -> {e[20, 2]:.3e} "
          f"(x{e[10, 2] / e[20, 2]:.2f})")
    assert e[10, 2] / e[20, 2] > 3.0
    assert e[10, 1] / e[20, 1] < 3.0
    assert e[20, 2] < e[20, 1]


# ------------------------------------------------------------------------------------ 4. host logic
def _cpu_engine(S=1, H=8, W=8):
    """a DenoiseEngine as set_conditioning leaves it, without a device: set_schedule builds tables and keys with plain torch"""
    from imagharmony_amd.denoise import DenoiseEngine
    from imagharmony_amd.unet import StepState

    class _U:
        attn_processors = {}

        class config:
            in_channels = 4
    e = DenoiseEngine(_U(), "cpu")
    e.st, e.S, e.H, e.W, e.max_cached_plans = StepState(), S, H, W, 3
    return e


def test_plan_keys_fingerprint_the_table_the_plan_reads():
    from imagharmony_amd import schedulers as hs
    e = _cpu_engine()

    def key(s, n=10, **kw):
        e.set_schedule(s, n, **kw)
        return e._sched_key
    k_ddim, k_dpm = key(hs.DDIMScheduler()), key(hs.DPMSolverMultistepScheduler())
    assert k_ddim != k_dpm and k_ddim[8] != k_dpm[8]                   # the fingerprint itself, not only the class name
    assert not e.stochastic and e.general and e.st.coef_tab is None and tuple(e.st.coef6_tab.shape) == (10, 6)
    assert tuple(e.st.hist.shape) == (1, 4, 8, 8) and e.st.noise_bank is None
    assert key(hs.DPMSolverMultistepScheduler()) == k_dpm
    # same class name, another table -> another key
    assert key(hs.DPMSolverMultistepScheduler(use_karras_sigmas=True))[8] != k_dpm[8]
    assert key(hs.DPMSolverMultistepScheduler(algorithm_type="sde-dpmsolver++"))[8] != k_dpm[8]
    assert e.stochastic and tuple(e.st.noise_bank.shape) == (10, 1, 4, 8, 8)
    # an image-to-image start: the row at t_start is first order, the table differs, so does the key
    assert key(hs.DPMSolverMultistepScheduler(), t_start=3)[8] != k_dpm[8]
    assert e.st.coef6_tab[3, 2] == 0 and e.st.coef6_tab[4, 2] != 0      # first order at the start, second order behind it
    # ... and where the table does not depend on the start the plan is shared, as for DDIM and Euler
    ea = hs.EulerAncestralDiscreteScheduler()
    assert key(ea, t_start=3) == key(ea)
    assert e.st.hist is None and tuple(e.st.noise_bank.shape) == (10, 1, 4, 8, 8) and e.st.in_scale_tab is not None
    assert key(hs.DDIMScheduler(), t_start=3) == k_ddim
    assert not e.general and e.st.coef6_tab is None and e.st.hist is None and e.st.noise_bank is None and e.st.coef_tab is not None


@pytest.mark.parametrize("kind", ["dpm", "dpm-karras", "sde", "euler-a"])
def test_blend_table_rows_are_add_noise_coefficients(kind):
    from imagharmony_amd import schedulers as hs
    from imagharmony_amd.denoise import DenoiseEngine
    s = {"dpm": hs.DPMSolverMultistepScheduler, "dpm-karras": lambda: hs.DPMSolverMultistepScheduler(use_karras_sigmas=True),
         "sde": lambda: hs.DPMSolverMultistepScheduler(algorithm_type="sde-dpmsolver++"), "euler-a": hs.EulerAncestralDiscreteScheduler}[kind]()
    N = 8
    s.set_timesteps(N)
    for n in (N, 6):
        tab = DenoiseEngine.blend_table(s, N, n)
        assert tab.dtype == torch.float32 and tuple(tab.shape) == (N, 2)
        for r in range(N):
            want = s.add_noise_coefficients(r + 1) if r < n - 1 else (1.0, 0.0)
            assert torch.equal(tab[r], torch.tensor(want, dtype=torch.float32)), (n, r)
    sg = s.sigmas.double()
    for r in (0, 3, N - 1):
        a, b = s.add_noise_coefficients(r)
        if kind == "euler-a":
            assert (a, b) == (1.0, float(s.sigmas[r]))
        else:
            al = float(1 / (sg[r] ** 2 + 1).sqrt())
            assert abs(a - al) < 1e-12 and abs(b - float(sg[r]) * al) < 1e-12


@pytest.mark.parametrize("as_list", [False, True])
def test_noise_bank_draw_order_reproduces_per_step_randn_latents(as_list):
    """after the initial-latents draw: one randn_latents call per step that runs, in step order"""
    from imagharmony_amd.denoise import DenoiseEngine
    from imagharmony_amd.pipeline import randn_latents
    S, shape, m = 2, (2, 4, 5, 7), 3
    gen = lambda: [torch.Generator().manual_seed(10 + s) for s in range(S)] if as_list else torch.Generator().manual_seed(10)
    g = gen()
    lat = randn_latents(shape, g)
    bank = DenoiseEngine.draw_step_noise(shape, m, g)
    g = gen()
    assert torch.equal(lat, randn_latents(shape, g))
    for r in range(m):
        assert torch.equal(bank[r], randn_latents(shape, g)), r
    assert bank.dtype == torch.float32 and tuple(bank.shape) == (m,) + shape


def test_engine_fills_bank_rows_of_the_steps_that_run_and_zeroes_the_history():
    from imagharmony_amd import lib as L
    from imagharmony_amd import schedulers as hs
    e = _cpu_engine(S=2, H=5, W=7)
    e.set_schedule(hs.DPMSolverMultistepScheduler(algorithm_type="sde-dpmsolver++"), 6, t_start=2, denoising_end=None)
    assert (e.t_start, e.steps) == (2, 6)
    e.st.hist.fill_(float("nan"))
    e._start_general_step(generator=torch.Generator().manual_seed(4))
    want = e.draw_step_noise((2, 4, 5, 7), 4, torch.Generator().manual_seed(4))
    assert torch.equal(e.st.noise_bank[2:], want) and (e.st.noise_bank[:2] == 0).all() and (e.st.hist == 0).all()
    given = torch.randn(4, 2, 4, 5, 7)
    e._start_general_step(step_noise=given)
    assert torch.equal(e.st.noise_bank[2:], given)
    with pytest.raises(L.ImhError, match="step_noise"):
        e._start_general_step(step_noise=given[:3])
    e.set_schedule(hs.DPMSolverMultistepScheduler(), 6)
    with pytest.raises(L.ImhError, match="step_noise"):
        e._start_general_step(step_noise=given)
    # the two-rank tail refuses a stochastic scheduler before any work
    e.set_schedule(hs.EulerAncestralDiscreteScheduler(), 6)
    e.cfg_role, e.do_cfg = 0, True
    with pytest.raises(NotImplementedError, match="stochastic"):
        e.denoise_cfg_split(torch.zeros(2, 4, 5, 7), None)


def test_new_op_is_bound_without_growing_the_argument_struct():
    """IMH_EW_CFG_MSTEP is the next free op number; imh_ew_args and the ABI version stay: the history buffer and the noise bank travel
    in the fields `b` and `bias`.  The header's Memory sentence says which rows the op reads.  Bad arguments are status codes."""
    from imagharmony_amd import lib
    import imagharmony_amd
    hdr = open(os.path.join(ROOT, "include", "imh.h")).read()
    body = re.search(r"enum imh_ew_op \{(.*?)\n\};", hdr, re.S).group(1)
    names = re.findall(r"^\s*(IMH_EW_[A-Z0-9_]+)", re.sub(r"/\*.*?\*/", "", body, flags=re.S), re.M)
    assert names[-2:] == ["IMH_EW_GATHER_ROWS", "IMH_EW_CFG_MSTEP"] and len(names) == 14
    assert lib.EW_CFG_MSTEP == 13 == lib.EW_GATHER_ROWS + 1 and lib.EW_CFG_STEP == 4
    mem = re.search(r"/\* Memory: every elementwise op.*?\*/", hdr, re.S).group(0)
    assert "IMH_EW_CFG_MSTEP" in mem and "row *step only" in mem
    assert [f[0] for f in lib.EwArgs._fields_][-4:] == ["x2", "noise", "mask", "blend_tab"]
    l = lib.load()
    e = lib.EwArgs()
    e.y = e.a = 64
    e.i0, e.i1 = 1, 64
    assert l.imh_elementwise(lib.EW_CFG_MSTEP, lib.C.byref(e), None) == -1 and b"cfg_mstep" in l.imh_last_error()
    e.tab = e.step = e.mask = 64
    assert l.imh_elementwise(lib.EW_CFG_MSTEP, lib.C.byref(e), None) == -1 and b"blend" in l.imh_last_error()
    for name in ("DPMSolverMultistepScheduler", "EulerAncestralDiscreteScheduler", "DDIMScheduler", "EulerDiscreteScheduler"):
        assert getattr(imagharmony_amd, name).__module__ == "imagharmony_amd.schedulers"
