"""CPU (no GPU): the float64 restatement of imh_clip_preprocess (imagharmony_amd/imageops.py) against torch -- ClipPreferenceJudge.preprocess
in fp32 plus the im2col of CLIPVisionEncoder.forward --, the structure of its filter tables, the derived geometry, the ABI additions, and
the host contract of edit-mode PNS (pns.edit_two_stage_fns / edit_prepare_fn / IPAdapterXL.generate_pns) on a fake engine."""
import ctypes as C
import os
import re
import socket
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import clip_pre_cases as cases
from imagharmony_amd import imageops, pns
from imagharmony_amd import schedulers as hs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- restatement vs torch
@pytest.mark.parametrize("hw", cases.SHAPES + [cases.FULL[:2]], ids=lambda s: "%dx%d" % s)
def test_restatement_matches_torch_cpu(hw):
    size, patch, S = (cases.FULL[2], cases.FULL[3], 1) if hw == cases.FULL[:2] else (cases.SIZE, cases.PATCH, 3)
    c = cases.case(hw[0], hw[1], size, patch, S)
    rows = cases.torch_rows(c["x"], size, patch).double()
    d = float((rows - c["ref"]).abs().max())
    bound = cases.HOST_BOUND["full" if size == 224 else "small"]
    print(f"restatement vs torch CPU fp32 {hw} -> {size}: max abs diff {d:.3e} (bound {bound:.3e})")
    assert rows.shape == c["ref"].shape == (S * (size // patch) ** 2, 3 * patch * patch)
    assert d <= bound


def test_identity_size_is_the_identity_resize():
    """28 x 28 -> 28: every output has the taps of its own pixel only (cubic(0) = 1, cubic(+-1) = 0)"""
    m = imageops.aa_matrix(28, 28)
    assert np.array_equal(m, np.eye(28))


# ---------------------------------------------------------------------------------------------- filter structure
@pytest.mark.parametrize("n_in,n_out", [(56, 39), (40, 28), (31, 28), (50, 45), (72, 50), (16, 28), (24, 42), (28, 28), (1024, 224), (7, 28)])
def test_filter_tables(n_in, n_out):
    first, count, wts = imageops.aa_tables(n_in, n_out)
    assert first.shape == count.shape == (n_out,) and wts.shape[0] == n_out
    assert np.allclose(wts.sum(1), 1.0, rtol=0, atol=1e-14)                     # normalised per output pixel
    assert (first >= 0).all() and (count >= 1).all() and (first + count <= n_in).all()      # the tap windows stay inside the image
    assert (np.diff(first) >= 0).all() and (np.diff(first + count) >= 0).all()  # and move monotonically (the kernel's window = first .. last)
    for i in range(n_out):
        assert (wts[i, count[i]:] == 0).all()
    scale = n_in / n_out
    support = 2 * scale if scale >= 1 else 2.0
    assert count.max() <= 2 * support + 1
    # the FORMULA of the launcher's LDS bounds holds for every patch position of the axis.  imageops.clip_tap_bounds restates
    # axis_bounds() of csrc/image.hip; this covers the formula only, not that the two stay the same text -- the kernel itself is held to
    # the restatement on the GPU (tests/test_gpu_clip_preprocess.py), where a table or window cut short by a wrong bound shows as an error
    for patch in (14, 16):
        cols, taps = imageops.clip_tap_bounds(n_in, n_out, patch)
        assert count.max() <= taps
        for i0 in range(0, n_out - patch + 1):
            assert first[i0 + patch - 1] + count[i0 + patch - 1] - first[i0] <= cols
    # a constant image stays constant; the dense matrix is the table
    m = imageops.aa_matrix(n_in, n_out)
    assert np.allclose(m @ np.ones(n_in), 1.0, atol=1e-14)


def test_cubic_kernel_values():
    assert imageops.cubic(0.0) == 1.0 and imageops.cubic(1.0) == 0.0 and imageops.cubic(2.0) == 0.0 and imageops.cubic(-2.5) == 0.0
    assert imageops.cubic(0.5) == pytest.approx(0.5625) and imageops.cubic(-1.5) == pytest.approx(-0.0625)


# ---------------------------------------------------------------------------------------------- derived geometry
@pytest.mark.parametrize("hw", cases.SHAPES + [(1024, 1024), (260, 300), (300, 260), (225, 224)], ids=lambda s: "%dx%d" % s)
def test_geometry_is_the_judges(hw, monkeypatch):
    size = 224 if max(hw) > 100 else cases.SIZE
    seen = {}
    real = torch.nn.functional.interpolate

    def spy(x, size=None, **kw):
        seen["size"] = tuple(size)
        return real(x, size=size, **kw)
    monkeypatch.setattr(torch.nn.functional, "interpolate", spy)
    j = pns.ClipPreferenceJudge.__new__(pns.ClipPreferenceJudge)
    j.image_size = size
    x = torch.zeros(1, 3, *hw)
    x[0, :, :, :] = torch.linspace(-1, 1, hw[1])                               # a horizontal ramp: a shifted crop would show
    out = j.preprocess(x)
    nh, nw, top, left = imageops.clip_geometry(hw[0], hw[1], size)
    assert seen["size"] == (nh, nw) and out.shape[-2:] == (size, size)
    assert (top, left) == ((nh - size) // 2, (nw - size) // 2) and min(nh, nw) == size
    patch = 14
    ref = imageops.clip_preprocess_reference(x.numpy(), size, patch)
    g = size // patch
    rows = out.reshape(1, 3, g, patch, g, patch).permute(0, 2, 4, 1, 3, 5).reshape(g * g, -1).double().numpy()
    assert np.abs(rows - ref).max() <= cases.HOST_BOUND["full" if size == 224 else "small"]


# ---------------------------------------------------------------------------------------------- the ABI addition
def test_abi_addition():
    from imagharmony_amd import lib as L
    hdr = open(os.path.join(ROOT, "include", "imh.h")).read()
    l = L.load()
    assert any(s[0] == "imh_clip_preprocess" for s in L.SYMBOLS) and hasattr(l, "imh_clip_preprocess")
    assert re.search(r"#define IMH_OP_CLIP_PREPROCESS 13\b", hdr) and L.OP_CLIP_PREPROCESS == 13
    assert re.search(r"#define IMH_CLIP_DT_F32 2\b", hdr) and L.CLIP_DT_F32 == 2
    body = re.search(r"typedef struct imh_clip_preprocess_args \{(.*?)\} imh_clip_preprocess_args;", hdr, re.S).group(1)
    names = []
    for decl in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";"):
        parts = decl.strip().replace("*", " ").split(",")
        if parts[0]:
            names.append(parts[0].split()[-1])
            names.extend(p.strip() for p in parts[1:])
    assert names == [f[0] for f in L.ClipPreprocessArgs._fields_]
    before = hdr[:hdr.index("int imh_clip_preprocess(")]
    assert "Memory:" in before[-2500:]
    # refusals are status codes, and never a launch (stream NULL, bogus pointers: nothing may be dereferenced)
    a = L.ClipPreprocessArgs()
    assert l.imh_clip_preprocess(None, None) == -1
    assert l.imh_clip_preprocess(C.byref(a), None) == -1 and b"null" in l.imh_last_error()
    a.x, a.y, a.S, a.H, a.W, a.nh, a.nw, a.size, a.patch, a.ldp = 64, 64, 1, 40, 56, 28, 39, 28, 14, 588
    a.left = 5
    a.std0 = a.std1 = a.std2 = 1.0
    for kw, rc in ((dict(size=30), -2), (dict(nh=27), -2), (dict(left=12), -2), (dict(top=-1), -2), (dict(ldp=587), -2), (dict(dtype=7), -1),
                   (dict(std2=0.0), -1), (dict(W=0), -2), (dict(patch=0), -2), (dict(y=66, dtype=L.CLIP_DT_F32), -1)):
        b = L.ClipPreprocessArgs.from_buffer_copy(a)
        for k, v in kw.items():
            setattr(b, k, v)
        assert l.imh_clip_preprocess(C.byref(b), None) == rc and b"imh_clip_preprocess" in l.imh_last_error(), kw
    p = l.imh_plan_create()
    assert l.imh_plan_add(p, L.OP_CLIP_PREPROCESS, C.byref(a), 0, 5) == 0 and l.imh_plan_get_kind(p, 0) == 13 and l.imh_plan_get_tag(p, 0) == 5
    assert l.imh_plan_add(p, 12, C.byref(a), 0, 0) == -1 and l.imh_plan_add(p, 14, C.byref(a), 0, 0) == -1
    l.imh_plan_destroy(p)


def test_judge_backend_argument():
    enc = types.SimpleNamespace(config=types.SimpleNamespace(image_size=28))
    t = torch.randn(1, 8)
    assert pns.ClipPreferenceJudge(None, enc, t).preprocess_backend == "torch"
    with pytest.raises(ValueError, match="CLIPVisionEncoder"):
        pns.ClipPreferenceJudge(None, enc, t, preprocess_backend="hip")
    with pytest.raises(ValueError):
        pns.ClipPreferenceJudge(None, enc, t, preprocess_backend="cuda")
    enc.embed_decoded = lambda images: types.SimpleNamespace(image_embeds=images.mean((2, 3)).repeat(1, 3)[:, :8])
    enc.device = torch.device("cpu")
    j = pns.ClipPreferenceJudge(lambda z: z[:, :3], enc, t, preprocess_backend="hip")
    s = j(torch.randn(5, 4, 6, 6))
    assert s.shape == (5,) and float(s.abs().max()) <= 1.0 + 1e-6


# ---------------------------------------------------------------------------------------------- edit-PNS on a fake engine
H8 = 4          # latent side of the fake


class FakeEngine:
    """records what the stage functions ask for; its "denoise" is a deterministic function of the prepared latents, the steps that run
    and (seeded) the step seeds -- per candidate, so stacking must not mix them"""

    def __init__(self, stochastic=False):
        self.calls, self.stochastic, self.seeded, self.lat = [], stochastic, False, None

    def set_conditioning(self, pe, *a, **k):
        self.calls.append(("conditioning", pe.shape[0]))

    def set_schedule(self, scheduler, steps, **kw):
        self.calls.append(("schedule", int(steps), dict(kw)))
        self.steps, self.t_start = int(steps), int(kw.get("t_start", 0))
        self.seeded = bool(kw.get("seeded_noise")) and self.stochastic

    def prepare_img2img(self, moments, n1, n2, scaling, a, b):
        self.calls.append(("img2img", n1.clone(), n2.clone(), float(a), float(b)))
        self.lat = a * scaling * (moments + n1) + b * n2

    def prepare_inpaint(self, moments, n1, n2, scaling, a, b, mask, strength_max=False, masked_moments=None, n3=None):
        self.calls.append(("inpaint", n1.clone(), n2.clone(), None if n3 is None else n3.clone(), bool(strength_max), moments is None))
        self.lat = n2.clone() if strength_max else a * scaling * (moments + n1) + b * n2
        if n3 is not None:
            self.lat = self.lat + 0.25 * (masked_moments + n3)

    def denoise(self, latents, step_seeds=None, **kw):
        assert latents is None
        self.calls.append(("denoise", None if step_seeds is None else list(step_seeds)))
        out = self.lat * (0.5 + 0.1 * (self.steps - self.t_start))
        if step_seeds is not None:
            out = out + torch.tensor([float(s % 7) for s in step_seeds]).view(-1, 1, 1, 1)
        return out


def _fake_fns(stochastic=False, strength=0.6, step_noise="global", inpaint=False, concat=False, preview=4, final=6):
    eng, sch = FakeEngine(stochastic), hs.DDIMScheduler()
    moments = torch.full((1, 4, H8, H8), 0.25)
    mask = torch.ones(1, 1, H8, H8) if inpaint else None
    mm = torch.full((1, 4, H8, H8), -0.5) if concat else None
    prepare = pns.edit_prepare_fn(eng, sch, 0.5, None if (concat and strength == 1.0) else moments, H8, H8, strength, mask=mask,
                                  masked_moments=mm, concat=concat)
    pre, fin = pns.edit_two_stage_fns(eng, sch, prepare, strength, preview, final, step_noise=step_noise, inpaint=inpaint)
    return eng, sch, pre, fin


def _draws(seed, n):
    g = torch.Generator("cpu").manual_seed(seed)
    return [torch.randn(1, 4, H8, H8, generator=g) for _ in range(n)]


SEEDS = [11, 7, 3, 19, 5]
SHAPE = (1, 4, H8, H8)


def test_edit_stage_functions_draw_per_seed_in_the_pipelines_order():
    eng, sch, pre, fin = _fake_fns()
    r = pns.run_pns(pre, SEEDS, SHAPE, final_fn=fin, batch=2, pass_seeds=True)
    sched = [c for c in eng.calls if c[0] == "schedule"]
    prep = [c for c in eng.calls if c[0] == "img2img"]
    # 5 seeds, batch 2 -> three preview groups, then the final of the winner
    assert [c[1] for c in sched] == [4, 4, 4, 6]
    # t_start per stage, as get_timesteps truncates: 4 steps x 0.6 -> init 2 -> t_start 2;  6 x 0.6 -> init 3 -> t_start 3
    assert [c[2]["t_start"] for c in sched] == [2, 2, 2, 3] and all(c[2]["inpaint"] is False and "seeded_noise" not in c[2] for c in sched)
    groups = [SEEDS[0:2], SEEDS[2:4], SEEDS[4:5], [r["best_seed"]]]
    for call, grp, steps, t0 in zip(prep, groups, (4, 4, 4, 6), (2, 2, 2, 3)):
        for k, s in enumerate(grp):
            d = _draws(s, 2)
            assert torch.equal(call[1][k:k + 1], d[0]) and torch.equal(call[2][k:k + 1], d[1])      # posterior noise first, add-noise noise second
        sch.set_timesteps(steps)
        assert (call[3], call[4]) == tuple(float(v) for v in sch.add_noise_coefficients(t0))
    assert [c[1] for c in eng.calls if c[0] == "denoise"] == [None] * 4                               # a deterministic sampler: no step seeds
    # scores do not depend on the stacking
    r1 = pns.run_pns(_fake_fns()[2], SEEDS, SHAPE, final_fn=_fake_fns()[3], batch=1, pass_seeds=True)
    assert torch.equal(r1["scores"], r["scores"]) and r1["best_seed"] == r["best_seed"] and torch.equal(r1["latents"], r["latents"])
    with pytest.raises(ValueError, match="pass_seeds"):
        pns.run_pns(pre, SEEDS, SHAPE)


@pytest.mark.parametrize("strength", [0.6, 1.0])
def test_edit_stage_functions_inpainting_draws(strength):
    for concat in (False, True):
        eng, sch, pre, fin = _fake_fns(strength=strength, inpaint=True, concat=concat)
        pre(torch.zeros(2, 4, H8, H8), seeds=[7, 3])
        call = [c for c in eng.calls if c[0] == "inpaint"][0]
        for k, s in enumerate([7, 3]):
            d = _draws(s, 3)
            assert torch.equal(call[1][k:k + 1], d[0]) and torch.equal(call[2][k:k + 1], d[1])
            assert (call[3] is None) if not concat else torch.equal(call[3][k:k + 1], d[2])           # the third draw: 9 channels only
        assert call[4] == (strength == 1.0)                                                           # is_strength_max
        assert call[5] == (concat and strength == 1.0)                                                # the skipped encoder pass
        assert [c for c in eng.calls if c[0] == "schedule"][0][2]["inpaint"] is True


def test_edit_stage_functions_seeded_step_noise_and_refusals():
    eng, sch, pre, fin = _fake_fns(stochastic=True, step_noise="seed")
    pre(None, seeds=[7, 3])
    assert [c for c in eng.calls if c[0] == "schedule"][0][2]["seeded_noise"] is True
    assert [c[1] for c in eng.calls if c[0] == "denoise"] == [[7, 3]]
    eng, sch, pre, fin = _fake_fns(stochastic=False, step_noise="seed")                               # a deterministic sampler ignores the flag
    pre(None, seeds=[7, 3])
    assert [c[1] for c in eng.calls if c[0] == "denoise"] == [None]
    with pytest.raises(ValueError, match="step_noise"):
        _fake_fns(step_noise="generator")
    # a stage whose truncated schedule has no step: the pipelines' ValueError, before the engine is touched
    eng, sch, pre, fin = _fake_fns(strength=0.3, preview=2, final=6)
    with pytest.raises(ValueError, match="no denoising step"):
        pre(None, seeds=[7])
    assert eng.calls == []
    assert fin(None, seeds=[7]).shape == (1, 4, H8, H8)                                               # 6 x 0.3 -> one step: runs


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        eng, sch, pre, fin = _fake_fns(stochastic=True, step_noise="seed")
        r = pns.run_pns(pre, SEEDS, SHAPE, final_fn=fin, batch=2, pass_seeds=True)
        seen = [s for c in eng.calls if c[0] == "denoise" for s in c[1]]
        q.put((rank, r["best_seed"], r["scores"].tolist(), r["latents"].sum().item(), r["owner"], seen))
    finally:
        dist.destroy_process_group()


def test_edit_pns_world2_matches_single_process():
    eng, sch, pre, fin = _fake_fns(stochastic=True, step_noise="seed")
    single = pns.run_pns(pre, SEEDS, SHAPE, final_fn=fin, batch=2, pass_seeds=True)
    assert single["scores"].unique().numel() == len(SEEDS)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in range(2))
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    best = single["best_seed"]
    for rank, b, scores, lat_sum, owner, seen in res:
        assert b == best and scores == single["scores"].tolist() and owner == SEEDS.index(best) % 2
        assert abs(lat_sum - single["latents"].sum().item()) < 1e-5
        mine = pns.shard(SEEDS, rank, 2)
        assert seen == mine + ([best] if rank == owner else [])                                       # its shard's previews; the final on the owner only


# ---------------------------------------------------------------------------------------------- IPAdapterXL.generate_pns, host side
def _bare_adapter(pipe_cls=None):
    """an IPAdapterXL without its constructor: just what generate_pns touches on a fake text-to-image pipe"""
    from imagharmony_amd.ip_adapter import IPAdapterXL
    ip = IPAdapterXL.__new__(IPAdapterXL)
    eng = types.SimpleNamespace(calls=[])
    eng.set_conditioning = lambda pe, *a, **k: eng.calls.append(("conditioning", pe.shape[0]))
    eng.set_schedule = lambda sch, steps, **kw: eng.calls.append(("schedule", steps))
    eng.denoise = lambda noise, **kw: noise * 0.5 + noise.mean(dim=(1, 2, 3), keepdim=True)
    unet = types.SimpleNamespace(attn_processors={}, config=types.SimpleNamespace(in_channels=4))
    ip.pipe = types.SimpleNamespace(unet=unet, engine=eng, scheduler=hs.DDIMScheduler(), vae=None, vae_decode=None, default_sample_size=4,
                                    vae_scale_factor=8)
    ip.device, ip.dtype, ip.image_encoder, ip.clip_image_processor, ip.number_class_crossattention = "cpu", torch.float32, None, None, None
    ip.image_proj_model = torch.nn.Linear(8, 2 * 6)
    ip._g = lambda m: (lambda x: m(x).view(x.shape[0], 2, 6))
    return ip, eng


def test_generate_pns_host_contract():
    ip, eng = _bare_adapter()
    kw = dict(clip_image_embeds=torch.randn(1, 8), prompt_embeds=(torch.randn(1, 3, 6), torch.randn(1, 3, 6), torch.randn(1, 5), torch.randn(1, 5)),
              preview_steps=2, num_inference_steps=3, output_type="latent")
    want = ip.generate_pns([3, 9, 27, 81, 5], **kw)
    assert want["scores"].shape == (5,) and want["scores"].unique().numel() == 5
    # a generator passed as `seeds` still yields all candidates (it used to be consumed by the batch-size count)
    got = ip.generate_pns((s for s in [3, 9, 27, 81, 5]), **kw)
    assert torch.equal(got["scores"], want["scores"]) and got["best_seed"] == want["best_seed"] and torch.equal(got["latents"], want["latents"])
    # judge_preprocess="hip" without the HIP tower: ValueError before any (GPU) work
    n = len(eng.calls)
    with pytest.raises(ValueError, match="hip"):
        ip.generate_pns([3, 9], judge_preprocess="hip", **kw)
    ip.image_encoder = torch.nn.Linear(2, 2)                                     # some other encoder
    with pytest.raises(ValueError, match="hip"):
        ip.generate_pns([3, 9], judge_preprocess="hip", **kw)
    with pytest.raises(ValueError, match="judge_preprocess"):
        ip.generate_pns([3, 9], judge_preprocess="triton", **kw)
    ip.image_encoder = None
    with pytest.raises(ValueError, match="image-to-image or inpainting"):
        ip.generate_pns([3, 9], image=torch.zeros(1, 3, 32, 32), **kw)            # edit arguments on a text-to-image pipe
    assert len(eng.calls) == n
