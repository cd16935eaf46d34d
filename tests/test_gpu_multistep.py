"""GPU: the general CFG + scheduler step (IMH_EW_CFG_MSTEP) and the device-resident loop under the multistep and ancestral samplers.

5. the op alone against a float64 evaluation of its formula, operands placed with tests/guarded.py, every other table / bank row NaN;
6. text-to-image trajectories against oracle.pipeline.denoise driven by the test-local schedulers of tests/multistep_reference.py;
7. image-to-image and the inpainting blend under DPM++ 2M and Euler ancestral;
8. DDIM and Euler plans are the launches they were, and the new op with a two-term row reproduces them bit for bit."""
import itertools

import pytest
import torch
import torch.nn.functional as F

from conftest import record_parity, rel_rms
from guarded import run_dense_and_guarded
from multistep_reference import RefDPMSolverMultistep, RefEulerAncestral
from oracle.detfill import det_randn
from oracle.pipeline import denoise as oracle_denoise

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24


# ------------------------------------------------------------------------------------ 5. the op alone
def _op_case(dtype, blend, cfg, use_w, use_h, use_z, row, seed):
    """one launch, dense and guarded -> (y, h') of the dense run, the float64 reference and the per-element bound of each"""
    from imagharmony_amd import lib as L
    from test_gpu_guarded_ops import settle
    S, HW, NR, G = 2, 35, 4, 4.0                       # 5 x 7 pixels: ragged against the 256-thread block; four table rows, `row` of them read
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    lat, h0, z, noise = rn(S, 4, HW), rn(S, 4, HW), rn(S, 4, HW), rn(S, 4, HW)
    npred = rn((2 if cfg else 1) * S, HW, 4).to(dtype)
    wf = torch.tensor([0.8, 1.1])
    nan = float("nan")
    tab = torch.full((NR, 6), nan)
    tab[row] = torch.tensor([0.9, -0.3, 0.45, 0.7, 1.6, -1.2]) + 0.1 * rn(6)
    bank = torch.full((NR, S, 4, HW), nan)
    bank[row] = rn(S, 4, HW)
    btab = torch.full((NR, 2), nan)
    btab[row] = torch.tensor([0.6, 0.8])
    mask = (torch.rand(max(blend, 1), HW, generator=g) > 0.5).float()

    def body(ctx, put, out):
        y = out((S, 4, HW), torch.float32)
        y.copy_(lat)
        hist = None
        if use_h:
            hist = out((S, 4, HW), torch.float32)
            hist.copy_(h0)
        step = out((1,), torch.int32)
        ctx.ew(L.EW_STEP_SET, step, i=(row, 1, 0, 0, 0, 0))
        kw = dict(x2=put(z.to(DEV)), noise=put(noise.to(DEV)), mask=put(mask.to(DEV)), blend_tab=put(btab.to(DEV))) if blend else {}
        ctx.ew(L.EW_CFG_MSTEP, y, a=put(npred.to(DEV)), w=put(wf.to(DEV)) if use_w else None, tab=put(tab.to(DEV)), step=step,
               hist=hist, bank=put(bank.to(DEV)) if use_z else None, i=(S, HW, 0, int(cfg), blend, 0), f=(0.0, 0.0, G, 0.0), **kw)
        return (y, hist) if use_h else y
    what = f"cfg_mstep {dtype} blend={blend} cfg={cfg} w={use_w} h={use_h} z={use_z} row={row}"
    dense, guarded, arena = run_dense_and_guarded(DEV, dtype, body)
    settle(dense, guarded, arena, what)
    # the guided prediction as the kernel forms it in fp32: with a power-of-two guidance scale every operation rounds at most once,
    # whether or not the compiler contracts it -> reproducible to the bit on the host
    n = npred.float().view(-1, S, HW, 4).permute(0, 1, 3, 2)
    eps = (n[0] + G * (n[1] - n[0])) if cfg else n[0]
    if use_w:
        eps = eps * wf[:, None, None]
    c = tab[row].double()
    terms = [c[0] * lat.double(), c[1] * eps.double()] + ([c[2] * h0.double()] if use_h else []) + ([c[3] * bank[row].double()] if use_z else [])
    ref, mag = sum(terms), sum(t.abs() for t in terms)
    if blend:
        m = mask[torch.arange(S) % blend][:, None, :].double().expand(S, 4, HW)
        bt = [btab[row, 0].double() * z.double(), btab[row, 1].double() * noise.double()]
        ref, mag = torch.where(m == 1, ref, sum(bt)), torch.where(m == 1, mag, sum(t.abs() for t in bt))
    out = [(dense[0].cpu(), ref, mag)]
    if use_h:
        ht = [c[4] * lat.double(), c[5] * eps.double()]
        out.append((dense[1].cpu(), sum(ht), sum(t.abs() for t in ht)))
    return what, out


@pytest.mark.parametrize("blend", [0, 1, 2], ids=["plain", "blend1", "blend2"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_general_step_op_matches_float64_formula(dtype, blend):
    """S = 2, HW = 35, both eps dtypes; CFG, rescale factor, history, noise on / off; no blend, mask batch 1 and 2; *step at rows 0, 1 and
    last.  Per element |y - ref| <= 8 * 2^-24 * sum |c_k v_k| over the terms of that element -- the summation-error bound of four fp32
    products, nothing measured -- for x' and for h'.  Every row of the table, the bank and the blend table but row *step is NaN, and all
    operands sit between NaN guard bands: a read of another row, or outside the operand, shows in the result."""
    worst = 0.0
    for k, (cfg, use_w, use_h, use_z, row) in enumerate(itertools.product((1, 0), (False, True), (True, False), (True, False), (0, 1, 3))):
        what, outs = _op_case(dtype, blend, cfg, use_w, use_h, use_z, row, seed=100 * blend + k)
        for name, (y, ref, mag) in zip(("x'", "h'"), outs):
            assert torch.isfinite(y).all(), f"{what}: {name} not finite"
            ratio = ((y.double() - ref).abs() / (8 * U * mag).clamp_min(1e-300)).max().item()
            worst = max(worst, ratio)
            assert ratio <= 1.0, f"{what}: {name} error / bound = {ratio:.3f}"
    print(f"cfg_mstep {dtype} blend={blend}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("blend", [0, 2], ids=["plain", "blend2"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_general_step_with_a_two_term_row_equals_cfg_step_bit_for_bit(dtype, blend):
    """ch = cn = 0, no history buffer, no bank: the bits of EW_CFG_STEP on the same inputs (CFG, rescale factor, table row 1)"""
    from imagharmony_amd import lib as L
    from imagharmony_amd.ctx import Ctx
    ctx = Ctx(DEV, dtype)
    S, HW = 2, 35
    g = torch.Generator().manual_seed(7 + blend)
    lat, z, noise = (torch.randn(S, 4, HW, generator=g).to(DEV) for _ in range(3))
    npred = torch.randn(2 * S, HW, 4, generator=g).to(dtype).to(DEV)
    wf = torch.tensor([0.8, 1.1], device=DEV)
    tab2 = torch.tensor([[0.5, 0.1], [0.9371, -0.3127], [0.7, 0.2]], device=DEV)
    tab6 = torch.cat([tab2, torch.zeros(3, 2, device=DEV), torch.tensor([[1.3, -0.8]] * 3, device=DEV)], 1).contiguous()
    mask = (torch.rand(blend or 1, HW, generator=g) > 0.5).float().to(DEV)
    btab = torch.tensor([[0.3, 0.4], [0.6, 0.2], [1.0, 0.0]], device=DEV)
    step = torch.ones(1, dtype=torch.int32, device=DEV)
    kw = dict(x2=z, noise=noise, mask=mask, blend_tab=btab) if blend else {}
    for w in (None, wf):
        old, new = lat.clone(), lat.clone()
        ctx.ew(L.EW_CFG_STEP, old, a=npred, w=w, tab=tab2, step=step, i=(S, HW, 0, 1, blend, 0), f=(0.0, 0.0, 5.0, 0.0), **kw)
        ctx.ew(L.EW_CFG_MSTEP, new, a=npred, w=w, tab=tab6, step=step, i=(S, HW, 0, 1, blend, 0), f=(0.0, 0.0, 5.0, 0.0), **kw)
        assert torch.equal(old, new) and not torch.equal(old, lat)
    with pytest.raises(L.ImhError, match=r"status -1\)"):                       # the table and the step counter are required
        ctx.ew(L.EW_CFG_MSTEP, lat.clone(), a=npred, i=(S, HW, 0, 1, 0, 0), f=(0.0, 0.0, 5.0, 0.0))
    with pytest.raises(L.ImhError, match="hist / bank"):
        ctx.ew(L.EW_CFG_STEP, lat.clone(), a=npred, hist=lat.clone(), i=(S, HW, 0, 1, 0, 0), f=(0.9, -0.3, 5.0, 0.0))


# ------------------------------------------------------------------------------------ 6. the loop
_CACHE = {}
HW32, STEPS = 32, 4


def _pair(dtype):
    from smoke_impl import build_pair
    if ("pair", dtype) not in _CACHE:
        _CACHE["pair", dtype] = build_pair(DEV, dtype)
    return _CACHE["pair", dtype]


def _inputs(ocfg, S=1):
    cd = ocfg.cross_attention_dim
    return (det_randn((S, 4, HW32, HW32), 3), det_randn((S, 81, cd), 4), det_randn((S, 81, cd), 5),
            det_randn((S, ocfg.pooled_dim), 6), det_randn((S, ocfg.pooled_dim), 7))


KINDS = {"dpmpp2m": dict(), "dpmpp2m-karras": dict(use_karras_sigmas=True), "sde-dpmpp2m": dict(algorithm_type="sde-dpmsolver++"), "euler-a": None}


def _product_scheduler(kind):
    from imagharmony_amd import schedulers as hs
    return hs.EulerAncestralDiscreteScheduler() if kind == "euler-a" else hs.DPMSolverMultistepScheduler(**KINDS[kind])


def _reference_scheduler(kind, **kw):
    return RefEulerAncestral(**kw) if kind == "euler-a" else RefDPMSolverMultistep(**KINDS[kind], **kw)


def _step_noise(seed, m, S=1):
    """what the engine draws for a stochastic scheduler from torch.Generator().manual_seed(seed) when the latents are handed over"""
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randn((S, 4, HW32, HW32), generator=g) for _ in range(m)], 0)


def _oracle_t2i(kind, guidance=5.0, solver_order=None):
    """the fp32 oracle trajectory (the same for every compute dtype of the HIP side): computed once per scheduler and shared"""
    key = ("t2i", kind, guidance, solver_order)
    if key not in _CACHE:
        ou, _, ocfg = _pair(torch.float16)
        lat, pe, ne, po, no = _inputs(ocfg)
        kw = dict(noise=_step_noise(21, STEPS)) if kind in ("sde-dpmpp2m", "euler-a") else {}
        if solver_order is not None:
            kw["solver_order"] = solver_order
        with torch.no_grad():
            _CACHE[key] = oracle_denoise(ou, _reference_scheduler(kind, **kw), lat, pe, ne, po, no, HW32 * 8, HW32 * 8,
                                         num_inference_steps=STEPS, guidance_scale=guidance)
    return _CACHE[key]


# rel-RMS against the oracle measured on an MI355X, and the bound = 2 x measured (the project's convention; the margin covers the
# box-to-box rounding-order differences of the UNet).  Caps: 2 x the bounds of the existing 3-step DDIM trajectories, 2e-2 fp16 / 8e-2 bf16.
# Every sampler runs in fp16 and in bf16.  The "first-order oracle lies more than 5 x the bound away" assertion is made on the fp16
# rows: the gap is a property of the fp32 oracle trajectories (0.10 - 0.18 rel-RMS here), the bf16 trajectory error is about a
# seventh of it, so with bound = 2 x measured the factor 5 cannot hold in bf16; there the parity bound alone is asserted, and the op
# test above holds the history term to 8 ulps in both dtypes.
#    scheduler         dtype          graph  CFG  bound        measured on an MI355X
T2I = [
    ("dpmpp2m", torch.float16, True, 5.0, 5.1e-3),          # 2.543e-3
    ("dpmpp2m", torch.float16, False, 5.0, 5.1e-3),         # 2.543e-3 (eager == graph, to the digit)
    ("dpmpp2m", torch.bfloat16, True, 5.0, 4.0e-2),         # 1.992e-2
    ("dpmpp2m-karras", torch.float16, True, 5.0, 6.0e-3),   # 3.010e-3
    ("dpmpp2m-karras", torch.bfloat16, True, 5.0, 4.8e-2),  # 2.386e-2
    ("sde-dpmpp2m", torch.float16, True, 5.0, 6.2e-3),      # 3.076e-3
    ("sde-dpmpp2m", torch.bfloat16, True, 5.0, 5.0e-2),     # 2.480e-2
    ("euler-a", torch.float16, True, 5.0, 6.5e-3),          # 3.251e-3
    ("euler-a", torch.bfloat16, True, 5.0, 5.6e-2),         # 2.784e-2
]


@pytest.mark.parametrize("kind,dtype,graph,guidance,bound", T2I,
                         ids=[f"{k}-{str(d).split('.')[-1]}-{'graph' if g else 'eager'}-cfg{c:g}" for k, d, g, c, _ in T2I])
def test_text_to_image_trajectory_matches_oracle(kind, dtype, graph, guidance, bound):
    """tiny UNet, 32 x 32 latents, CFG 5, 4 steps: a first-order start, two second-order steps, the first-order final step.  The
    stochastic samplers read the same noise rows on both sides.  For the second-order samplers the oracle's first-order-only
    trajectory (solver_order = 1) lies more than 5 x the fp16 bound away from its 2M trajectory (0.103 / 0.178 / 0.137 rel-RMS for 2M /
    2M Karras / SDE 2M on these inputs, computed on the CPU): a kernel that drops the history term cannot pass the fp16 rows.
    The bf16 rows assert the parity bound alone (see the comment above T2I).
    Measured rel-RMS on an MI355X / bound = 2 x measured (also in DESIGN.md's parity table), fp16: DPM++ 2M 2.543e-3 / 5.1e-3 (graph
    and eager), 2M Karras 3.010e-3 / 6.0e-3, SDE 2M 3.076e-3 / 6.2e-3, Euler a 3.251e-3 / 6.5e-3; bf16: DPM++ 2M 1.992e-2 / 4.0e-2,
    2M Karras 2.386e-2 / 4.8e-2, SDE 2M 2.480e-2 / 5.0e-2, Euler a 2.784e-2 / 5.6e-2."""
    from imagharmony_amd.pipeline import StableDiffusionXLCustomPipeline
    ou, hu, ocfg = _pair(dtype)
    lat, pe, ne, po, no = _inputs(ocfg)
    ref = _oracle_t2i(kind, guidance)
    pipe = StableDiffusionXLCustomPipeline(hu, scheduler=_product_scheduler(kind), device=DEV, dtype=dtype, use_graph=graph)
    out = pipe(prompt_embeds=pe, negative_prompt_embeds=ne, pooled_prompt_embeds=po, negative_pooled_prompt_embeds=no, height=HW32 * 8,
               width=HW32 * 8, num_inference_steps=STEPS, guidance_scale=guidance, latents=lat, generator=torch.Generator().manual_seed(21),
               output_type="latent").images.float().cpu()
    r = rel_rms(out, ref)
    name = f"multistep.t2i.{kind}.{str(dtype).split('.')[-1]}.{'graph' if graph else 'eager'}.cfg{guidance:g}"
    print(f"{name}: rel-rms {r:.3e} (bound {bound:g})")
    record_parity(name, r, bound)
    descr = [t[2] for t in pipe.engine.plan.tags]
    assert descr[-2:] == ["cfg+mstep", "step++"]
    assert torch.isfinite(out).all() and r < bound, (name, r)
    if kind != "euler-a" and dtype == torch.float16:
        gap = rel_rms(_oracle_t2i(kind, guidance, solver_order=1), ref)
        print(f"{name}: first-order oracle vs 2M oracle rel-rms {gap:.3e}")
        assert gap > 5 * bound, (gap, bound)
    # a second call on the same pipeline re-records nothing under an unchanged conditioning and reproduces the bits (the history is
    # zeroed and the bank refilled before the loop)
    eng = pipe.engine
    plan = eng.plan
    eng.set_schedule(pipe.scheduler, STEPS)
    again = eng.denoise(lat, generator=torch.Generator().manual_seed(21)).float().cpu()
    assert eng.plan is plan and torch.equal(again, out)


def test_preview_final_alternation_rerecords_nothing_and_forks_own_their_state():
    """pns.two_stage_fns under DPM++ 2M: the second image's preview and final schedules come back from the plan cache with their
    history buffers; a fork has a history slot and a noise bank of its own"""
    from imagharmony_amd import pns
    from imagharmony_amd import schedulers as hs
    from imagharmony_amd.denoise import DenoiseEngine
    dtype = torch.float16
    ou, hu, ocfg = _pair(dtype)
    lat, pe, ne, po, no = _inputs(ocfg)
    eng = DenoiseEngine(hu, DEV, dtype)
    eng.set_conditioning(pe, ne, po, no, HW32 * 8, HW32 * 8, guidance_scale=5.0)
    sch = hs.DPMSolverMultistepScheduler()
    preview, final = pns.two_stage_fns(eng, sch, preview_steps=2, final_steps=3)
    p1 = preview(lat); plan_p, hist_p = eng.plan, eng.st.hist
    f1 = final(lat); plan_f, hist_f = eng.plan, eng.st.hist
    assert plan_p is not plan_f and hist_p is not hist_f
    p2 = preview(lat)
    assert eng.plan is plan_p and eng.st.hist is hist_p and torch.equal(p1, p2)
    f2 = final(lat)
    assert eng.plan is plan_f and eng.st.hist is hist_f and torch.equal(f1, f2)
    fk = eng.fork()
    assert fk.general and fk.st.hist is not eng.st.hist and fk.st.coef6_tab is eng.st.coef6_tab and fk.st.noise_bank is None
    assert torch.equal(fk.denoise(lat), f1)
    eng.set_schedule(hs.EulerAncestralDiscreteScheduler(), 3)
    fk = eng.fork()
    assert fk.stochastic and fk.st.hist is None and fk.st.noise_bank is not None and fk.st.noise_bank is not eng.st.noise_bank
    noise = _step_noise(5, 3)
    assert torch.equal(fk.denoise(lat, step_noise=noise), eng.denoise(lat, step_noise=noise))


def test_ipadapter_generate_and_its_preview_final_alternation_under_the_new_samplers():
    """IPAdapterXL takes the scheduler from the pipe: generate() under Euler ancestral equals the direct pipeline call with the seed's
    generator (the step noise comes from it), and generate_pns() under DPM++ 2M records two plans for three previews and the final
    denoise -- the preview / final alternation re-records nothing after the first candidate."""
    from smoke_impl import build_pair
    from imagharmony_amd import schedulers as hs
    from imagharmony_amd.ip_adapter import IPAdapterXL
    from imagharmony_amd.modules import HarmonyAttention
    from imagharmony_amd.pipeline import StableDiffusionXLCustomPipeline
    from imagharmony_amd.utils import get_generator
    from oracle.detfill import det_fill
    dtype = torch.float16
    _, hu, ocfg = build_pair(DEV, dtype)                 # a UNet of its own: IPAdapterXL installs its processors
    cd = ocfg.cross_attention_dim
    pipe = StableDiffusionXLCustomPipeline(hu, scheduler=hs.EulerAncestralDiscreteScheduler(), device=DEV, dtype=dtype)
    ha = det_fill(HarmonyAttention(image_hidden_size=128, text_context_dim=cd, inter_dim=512, cross_heads=8, reshape_blocks=8,
                                   cross_value_dim=64), 3)
    ip = IPAdapterXL(pipe, None, None, DEV, num_tokens=4, inference=True, number_class_crossattention=ha, dtype=dtype,
                     clip_embeddings_dim=128)
    det_fill(ip.image_proj_model, 5)
    embeds4 = (det_randn((1, 77, cd), 1), det_randn((1, 77, cd), 2), det_randn((1, ocfg.pooled_dim), 3), det_randn((1, ocfg.pooled_dim), 4))
    kw = dict(clip_image_embeds=det_randn((1, 128), 5), prompt_embeds=embeds4, extra_prompt_embeds=det_randn((1, 77, cd), 6))
    seen = {}

    class Spy:
        def __getattr__(self, k):
            return getattr(pipe, k)

        def __call__(self, **a):
            seen.update(a)
            return pipe(**a)
    ip.pipe = Spy()
    lat = ip.generate(output_type="latent", num_samples=1, seed=42, num_inference_steps=STEPS, guidance_scale=5.0, **kw)
    ip.pipe = pipe
    assert pipe.engine.stochastic and [t[2] for t in pipe.engine.plan.tags][-2] == "cfg+mstep" and torch.isfinite(lat).all()
    assert torch.equal(lat, pipe(**{**seen, "generator": get_generator(42, "cpu")}).images)
    assert not torch.equal(lat, pipe(**{**seen, "generator": get_generator(43, "cpu")}).images)
    pipe.scheduler = hs.DPMSolverMultistepScheduler()
    eng = pipe.engine
    records, record = [], eng._record

    def counted():
        records.append(eng.steps)
        return record()
    eng._record = counted
    r = ip.generate_pns([1, 2, 3], preview_steps=2, num_inference_steps=3, guidance_scale=5.0, batch=1, output_type="latent", **kw)
    del eng._record
    assert records == [2, 3], records
    assert r["best_seed"] in (1, 2, 3) and r["latents"].shape == (1, 4, HW32, HW32) and torch.isfinite(r["latents"]).all()
    assert eng.general and eng.st.hist is not None


# ------------------------------------------------------------------------------------ 7. image-to-image and inpainting
def _add_noise_pair(ref, row):
    s = ref.sigmas[row].double()
    if isinstance(ref, RefEulerAncestral):
        return 1.0, float(s)
    a = 1 / (s * s + 1).sqrt()
    return float(a), float(s * a)


@torch.no_grad()
def _oracle_edit(kind, strength, inpaint, seed=11, nine=False):
    """diffusers 0.30 img2img / inpaint (4-channel UNet) __call__ over the oracle modules with the test-local scheduler, fp32, S = 1: the
    sequence tests/test_gpu_inpaint.py compares with.  Draws in upstream's order from one generator: posterior noise, add-noise noise,
    (nine: the 9-channel UNet -- posterior noise of the masked image, no blend,) then one draw per step that runs for a stochastic
    scheduler."""
    key = ("edit", kind, strength, inpaint, nine)
    if key in _CACHE:
        return _CACHE[key]
    from test_gpu_inpaint import IMG, build_vae_pair, centred_mask, embeds
    ou, _, ocfg = _pair(torch.float16)               # this file's own pair: other files' cached UNets get new processors along the way
    if nine:
        from test_gpu_inpaint import build_pair as build_pair_cin
        ou, _, ocfg = build_pair_cin(torch.float16, 9)
    ov, _ = build_vae_pair()
    img, mask = IMG(), centred_mask(256, 256)
    emb = embeds(ocfg, 1)
    t_start = STEPS - min(int(STEPS * strength), STEPS)
    g = torch.Generator().manual_seed(seed)
    h = w = HW32
    n1 = torch.randn((1, 4, h, w), generator=g)
    n2 = torch.randn((1, 4, h, w), generator=g)
    n3 = torch.randn((1, 4, h, w), generator=g) if nine else None
    bank = torch.zeros(STEPS, 1, 4, h, w)
    if kind == "euler-a":
        for r in range(t_start, STEPS):
            bank[r] = torch.randn((1, 4, h, w), generator=g)
    sch = _reference_scheduler(kind, t_start=t_start, **(dict(noise=bank) if kind == "euler-a" else {}))
    sch.set_timesteps(STEPS)
    mean, logvar = ov.quant_conv(ov.encoder(img)).chunk(2, 1)
    z = (mean + torch.exp(0.5 * logvar.clamp(-30, 20)) * n1) * ov.config.scaling_factor
    a, b = _add_noise_pair(sch, t_start)
    x = a * z + b * n2
    if nine:
        mm, ml = ov.quant_conv(ov.encoder(img * (mask < 0.5))).chunk(2, 1)
        mz = (mm + torch.exp(0.5 * ml.clamp(-30, 20)) * n3) * ov.config.scaling_factor
    if not inpaint:
        ref = oracle_denoise(ou, sch, x, emb["prompt_embeds"], emb["negative_prompt_embeds"], emb["pooled_prompt_embeds"],
                             emb["negative_pooled_prompt_embeds"], 256, 256, num_inference_steps=STEPS, guidance_scale=5.0)
    else:
        m = F.interpolate(mask, size=(h, w))
        pe, ne, po, no = (emb[k] for k in ("prompt_embeds", "negative_prompt_embeds", "pooled_prompt_embeds", "negative_pooled_prompt_embeds"))
        ids = torch.tensor([[256, 256, 0, 0, 256, 256]], dtype=pe.dtype).repeat(2, 1)
        ehs, text = torch.cat([ne, pe], 0), torch.cat([no, po], 0)
        ts = sch.timesteps
        for i, t in enumerate(ts):
            xin = sch.scale_model_input(torch.cat([x] * 2), t)
            if nine:
                xin = torch.cat([xin, torch.cat([m] * 2), torch.cat([mz] * 2)], 1)
            eps = ou(xin, t, encoder_hidden_states=ehs, added_cond_kwargs={"text_embeds": text, "time_ids": ids})[0]
            u, c = eps.chunk(2)
            x = sch.step(u + 5.0 * (c - u), t, x)[0]
            if not nine:
                p = z
                if i < len(ts) - 1:
                    a, b = _add_noise_pair(sch, t_start + i + 1)
                    p = a * z + b * n2
                x = (1 - m) * p + m * x
        ref = x
    _CACHE[key] = ref
    return ref


#    scheduler  mode  strength  dtype  bound                           measured on an MI355X
EDIT = [
    ("dpmpp2m", "img2img", 0.5, torch.float16, 6.8e-3),      # 3.423e-3
    ("euler-a", "img2img", 0.5, torch.float16, 8.0e-3),      # 4.000e-3
    ("dpmpp2m", "inpaint", 0.75, torch.float16, 6.4e-3),     # 3.206e-3
    ("euler-a", "inpaint", 0.75, torch.float16, 8.3e-3),     # 4.136e-3
    ("dpmpp2m", "inpaint", 0.75, torch.bfloat16, 5.3e-2),    # 2.646e-2
    ("dpmpp2m", "inpaint9", 0.75, torch.float16, 7.5e-3),    # 3.740e-3
    ("euler-a", "inpaint9", 0.75, torch.float16, 8.3e-3),    # 4.166e-3
]


@pytest.mark.parametrize("kind,mode,strength,dtype,bound", EDIT, ids=[f"{k}-{m}-{str(d).split('.')[-1]}" for k, m, _, d, _ in EDIT])
def test_image_to_image_and_inpaint_blend_match_oracle(kind, mode, strength, dtype, bound):
    """image-to-image at strength 0.5 of 4 steps (t_start = 2: the first step that runs is first order, the table row differs from the
    text-to-image one) and the inpainting blend at strength 0.75 (t_start = 1: first order, second order, first-order final; the
    blend's add_noise pair comes from add_noise_coefficients) under DPM++ 2M and Euler ancestral; inpaint9: the same call on the
    9-channel inpainting UNet (conv_in reads [mask | masked-image latents], no blend).  Same tiny sizes and the same bound
    rule as the text-to-image trajectories, bound = 2 x the rel-RMS measured on an MI355X: image-to-image fp16 2M 3.423e-3 / 6.8e-3,
    Euler a 4.000e-3 / 8.0e-3; inpainting fp16 2M 3.206e-3 / 6.4e-3, Euler a 4.136e-3 / 8.3e-3, bf16 2M 2.646e-2 / 5.3e-2; 9-channel
    inpainting fp16 2M 3.740e-3 / 7.5e-3, Euler a 4.166e-3 / 8.3e-3."""
    from imagharmony_amd.pipeline import StableDiffusionXLImg2ImgCustomPipeline, StableDiffusionXLInpaintCustomPipeline
    from test_gpu_inpaint import IMG, build_pair as build_pair_cin, build_vae_pair, centred_mask, embeds
    ou, hu, ocfg = build_pair_cin(dtype, 9) if mode == "inpaint9" else _pair(dtype)
    _, hv = build_vae_pair()
    ref = _oracle_edit(kind, strength, mode != "img2img", nine=mode == "inpaint9")
    kw = dict(image=IMG(), strength=strength, num_inference_steps=STEPS, guidance_scale=5.0, generator=torch.Generator().manual_seed(11),
              output_type="latent", **embeds(ocfg, 1))
    if mode != "img2img":
        pipe = StableDiffusionXLInpaintCustomPipeline(hu, scheduler=_product_scheduler(kind), device=DEV, dtype=dtype, vae=hv)
        out = pipe(mask_image=centred_mask(256, 256), **kw).images.float().cpu()
    else:
        pipe = StableDiffusionXLImg2ImgCustomPipeline(hu, scheduler=_product_scheduler(kind), device=DEV, dtype=dtype, vae=hv)
        out = pipe(**kw).images.float().cpu()
    eng = pipe.engine
    assert eng.t_start == STEPS - int(STEPS * strength) and eng.steps == STEPS
    assert [t[2] for t in eng.plan.tags][-2] == ("cfg+mstep+blend" if mode == "inpaint" else "cfg+mstep")
    assert eng.inpaint == {"img2img": None, "inpaint": "blend", "inpaint9": "concat"}[mode]
    if kind == "dpmpp2m":
        assert eng.st.coef6_tab[eng.t_start, 2] == 0                          # the first-order row of this start
    r = rel_rms(out, ref)
    name = f"multistep.{mode}.{kind}.{str(dtype).split('.')[-1]}"
    print(f"{name}: rel-rms {r:.3e} (bound {bound:g})")
    record_parity(name, r, bound)
    assert torch.isfinite(out).all() and r < bound, (name, r)
    if mode == "inpaint":                                                      # outside the mask: the image latents, to the bit
        keep = (F.interpolate(centred_mask(256, 256), size=(HW32, HW32)) == 0).expand_as(out)
        assert torch.equal(out[keep], eng.st.inp_z.float().cpu()[keep])


# ------------------------------------------------------------------------------------ 8. unchanged paths
class _TwoTermAsGeneral:
    """DDIM / Euler handed to the engine through the general step: the same two coefficients in a six-column row, no history, no bank"""
    general_step, needs_history, stochastic = True, False, False

    def __init__(self, inner):
        self.inner = inner
        self.num_train_timesteps = inner.num_train_timesteps

    def set_timesteps(self, n, device=None):
        self.inner.set_timesteps(n)

    def tables(self, t_start=0):
        t = dict(self.inner.tables())
        t["coef6"] = torch.cat([t["coef"], torch.zeros(t["coef"].shape[0], 4)], 1)
        t["coef"] = None
        return t


# launches of one recorded step of the tiny pair (forward + cfg+step + step++; one more with guidance rescale): the count DESIGN.md
# section 4 records for the plan as it was before the general step existed
LAUNCHES_PER_STEP = 304


@pytest.mark.parametrize("sched", ["ddim", "euler"])
@pytest.mark.parametrize("rescale", [0.0, 0.7])
def test_ddim_and_euler_plans_are_unchanged(sched, rescale):
    """DDIM and Euler still end with EW_CFG_STEP: [cfg.rescale,] cfg+step, step++ behind the forward, the launch count of the multistep
    plan of the same shape (the new op replaces one launch, it adds none).  With the new path switched off that is all there is to run;
    switched on for the same two coefficients (_TwoTermAsGeneral) it gives the same latents bit for bit."""
    from imagharmony_amd import schedulers as hs
    from imagharmony_amd.denoise import DenoiseEngine
    dtype = torch.bfloat16
    ou, hu, ocfg = _pair(dtype)
    lat, pe, ne, po, no = _inputs(ocfg)
    eng = DenoiseEngine(hu, DEV, dtype)
    eng.set_conditioning(pe, ne, po, no, HW32 * 8, HW32 * 8, guidance_scale=5.0, guidance_rescale=rescale)
    new = lambda: hs.DDIMScheduler() if sched == "ddim" else hs.EulerDiscreteScheduler()
    eng.set_schedule(new(), 3)
    old = eng.denoise(lat).clone()
    descr = [t[2] for t in eng.plan.tags]
    size = eng.plan.lib.imh_plan_size(eng.plan.plan)
    tail = (["cfg.rescale"] if rescale else []) + ["cfg+step", "step++"]
    assert descr[-len(tail):] == tail and "cfg+mstep" not in descr and size == len(descr)
    print(f"{sched} rescale {rescale}: {size} launches per step")
    assert size == LAUNCHES_PER_STEP + (1 if rescale else 0)
    assert not eng.general and eng.st.hist is None and eng.st.noise_bank is None and eng.st.coef6_tab is None
    eng.set_schedule(_TwoTermAsGeneral(new()), 3)
    via_new = eng.denoise(lat).clone()
    d2 = [t[2] for t in eng.plan.tags]
    assert d2[-2:] == ["cfg+mstep", "step++"] and d2[:-2] == descr[:-2] and eng.plan.lib.imh_plan_size(eng.plan.plan) == size
    assert torch.equal(old, via_new)
    eng.set_schedule(hs.DPMSolverMultistepScheduler(), 3)
    eng.denoise(lat)
    assert eng.plan.lib.imh_plan_size(eng.plan.plan) == size
