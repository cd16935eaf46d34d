"""CPU (no GPU): FreeU.  The float64 specification (imagharmony_amd/freeu.py) against a torch.fft restatement of diffusers'
fourier_filter (tests/freeu_reference.py) and against analytic planes; the public surface (UNet and every pipeline class); what the
dry-recorded forward gains with FreeU enabled and that disabling it restores the recording launch for launch and argument for
argument; the plan key; the header (ABI 13, fourteen element-wise ops, the plan kinds) and the C entry's refusals."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import freeu_reference as FRf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SDXL = (0.6, 0.4, 1.1, 1.2)          # s1, s2, b1, b2: the published SDXL values


def _tool(name):
    """a private copy of a trace tool (its model cache is then this module's own: enabling FreeU here never shows elsewhere)"""
    spec = importlib.util.spec_from_file_location(f"freeu_{name}", os.path.join(ROOT, "tools", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


FT = _tool("forward_trace")
ET = _tool("engine_trace")


# ------------------------------------------------------------------------------------------------------------------ the specification
@pytest.mark.parametrize("H,W", [(2, 2), (2, 6), (3, 5), (6, 10), (8, 8), (32, 32)])
def test_closed_form_equals_the_fft_restatement(H, W):
    from imagharmony_amd import freeu
    g = torch.Generator().manual_seed(100 * H + W)
    x = torch.randn(2, 5, H, W, dtype=torch.float64, generator=g)
    for s in (0.6, 0.2, 1.7):
        ref = FRf.fourier_filter(x, 1, s, work=torch.float64).permute(0, 2, 3, 1).numpy()
        got = freeu.fourier_filter(x.permute(0, 2, 3, 1).numpy(), s)
        assert got.shape == ref.shape
        assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max(), (H, W, s)


def test_analytic_needles():
    from imagharmony_amd import freeu
    s = 0.4
    for H, W in ((2, 2), (3, 5), (6, 10), (8, 8)):
        const = np.full((1, H, W, 2), 3.25)
        np.testing.assert_allclose(freeu.fourier_filter(const, s), s * const, rtol=1e-13)
        y = np.arange(H, dtype=np.float64)[:, None, None]
        plane = np.broadcast_to(np.cos(2 * np.pi * y / H), (H, W, 1))[None].copy()
        want = s * plane if H == 2 else plane * (1 + (s - 1) / 2)          # the asymmetric mask: frequency -1 is scaled, +1 is not
        np.testing.assert_allclose(freeu.fourier_filter(plane, s), want, rtol=1e-12, atol=1e-14)
        x = np.random.default_rng(H * W).standard_normal((2, H, W, 3))
        np.testing.assert_allclose(freeu.fourier_filter(x, 1.0), x, rtol=0, atol=0)       # s = 1: the identity
    with pytest.raises(ValueError):
        freeu.fourier_filter(np.zeros((1, 1, 4, 8)), s)


def test_whole_concat_spec_is_apply_freeu_then_cat():
    from imagharmony_amd import freeu
    g = torch.Generator().manual_seed(5)
    h, r = torch.randn(2, 16, 6, 10, dtype=torch.float64, generator=g), torch.randn(2, 24, 6, 10, dtype=torch.float64, generator=g)
    hh = h.clone()
    hh[:, :8] = hh[:, :8] * 1.2
    ref = torch.cat([hh, FRf.fourier_filter(r, 1, 0.4, work=torch.float64)], 1).permute(0, 2, 3, 1).numpy()
    got = freeu.freeu_concat(h.permute(0, 2, 3, 1).numpy(), r.permute(0, 2, 3, 1).numpy(), 8, 1.2, 0.4)
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    assert freeu.unet_settings(SDXL, 0) == (1.1, 0.6) and freeu.unet_settings(SDXL, 1) == (1.2, 0.4)
    assert freeu.unet_settings(SDXL, 2) is None and freeu.unet_settings(None, 0) is None


# ------------------------------------------------------------------------------------------------------------------ the public surface
def test_enable_and_disable_exist_on_the_unet_and_on_every_pipeline_class():
    import inspect
    from imagharmony_amd import pipeline as P
    from imagharmony_amd.controlnet import ControlNetModel
    from imagharmony_amd.unet import UNet2DConditionModel
    assert list(inspect.signature(UNet2DConditionModel.enable_freeu).parameters) == ["self", "s1", "s2", "b1", "b2"]
    assert callable(UNet2DConditionModel.disable_freeu) and not hasattr(ControlNetModel, "enable_freeu")
    pipes = [c for n, c in vars(P).items() if inspect.isclass(c) and n.startswith("StableDiffusionXL") and n.endswith("Pipeline")]
    assert len(pipes) >= 7
    for c in pipes:
        assert list(inspect.signature(c.enable_freeu).parameters) == ["self", "s1", "s2", "b1", "b2"], c
        assert callable(c.disable_freeu), c
    u = ET.unet()
    pipe = P.StableDiffusionXLCustomPipeline(u, device="cpu")
    try:
        assert u.freeu is None
        pipe.enable_freeu(*SDXL)
        assert u.freeu == SDXL
        pipe.disable_freeu()
        assert u.freeu is None
    finally:
        u.disable_freeu()


# ------------------------------------------------------------------------------------------------------------------ the recorded forward
def _record_tiny(u, S=1, Hl=32, Wl=32):
    from imagharmony_amd.ctx import Ctx
    B = 2 * S
    ctx = Ctx("cpu", torch.bfloat16, record=True, dry=True)
    st = u.prepare_conditioning(ctx, torch.zeros(B, 81, 256), torch.zeros(B, 128), torch.zeros(B, 6))
    st.t_value = torch.zeros(B)
    st.latents = torch.zeros(S, 4, Hl, Wl)
    u.emit_forward(ctx, st, S, Hl, Wl, cfg_dup=True)
    return ctx


def _hist(ctx):
    h = {}
    for t in ctx.tags:
        h[(t[0], t[2])] = h.get((t[0], t[2]), 0) + 1
    return h


def _delta(a, b):
    ha, hb = _hist(a), _hist(b)
    return {k: hb.get(k, 0) - ha.get(k, 0) for k in set(ha) | set(hb) if ha.get(k, 0) != hb.get(k, 0)}


def _scalars(a):
    """every non-pointer field of a recorded argument struct (both structs of a two-problem launch)"""
    structs = list(a) if isinstance(a, C.Array) else [a]
    return [getattr(s, n) for s in structs for n, t in s._fields_ if t is not C.c_void_p and not (isinstance(t, type) and issubclass(t, C.Structure))]


def _rows(ctx, tags):
    return [(t[0], t[1], t[2], t[5], sorted(t[6].items()) if isinstance(t[6], dict) else t[6], _scalars(o[1]))
            for t, o in zip(ctx.tags, ctx._ops) if t[0] in tags]


def test_disabling_restores_the_recorded_forward_launch_for_launch():
    u = ET.unet()
    try:
        before = _record_tiny(u)
        u.enable_freeu(*SDXL)
        with_fu = _record_tiny(u)
        u.disable_freeu()
        after = _record_tiny(u)
    finally:
        u.disable_freeu()
    assert FT.describe(before) == FT.describe(after)                       # op for op, with the buffer aliasing
    assert FT.args_digest(before) == FT.args_digest(after)                 # argument for argument
    assert FT.describe(before)["sha1"] != FT.describe(with_fu)["sha1"]


def test_enabled_trace_on_the_tiny_unet():
    """tiny widths, latent 32 x 32, UNet batch 2: the FreeU regions are 8 x 8 (hidden 256; skips 256, 256, 128) and 16 x 16 (hidden 256,
    128, 128; skips 128, 128, 64).  At these widths no conv runs on the LDS-halo kernel, so the plain forward already materialises its
    six concats: the FreeU launches take their place, launch for launch.  The statistics passes change hands -- a ResNet's norm1 reads
    one pass over the concatenated tensor instead of its two producers' partials -- which at these widths comes to one pass less in
    up block 1 (seven become six) and as many as before in up block 0.  Up block 2 and the output convs are what they were."""
    from imagharmony_amd import lib as L
    u = ET.unet()
    try:
        plain = _record_tiny(u)
        u.enable_freeu(*SDXL)
        fu = _record_tiny(u)
    finally:
        u.disable_freeu()
    assert _delta(plain, fu) == {(40, "freeu.concat"): 3, (40, "skip.concat"): -3, (41, "freeu.concat"): 3, (41, "skip.concat"): -3,
                                (41, "gn_stats"): -1}
    assert len(fu.tags) - len(plain.tags) == -1
    got = [(t[0], o[1].n, o[1].i0, o[1].i1, o[1].i2, o[1].i3, o[1].i4, o[1].i5, o[1].f0, o[1].f1)
           for t, o in zip(fu.tags, fu._ops) if t[2] == "freeu.concat"]
    f32 = lambda v: float(np.float32(v))
    b1, s1, b2, s2 = f32(1.1), f32(0.6), f32(1.2), f32(0.4)
    assert got == [(40, 128, 256, 256, 8, 8, 128, 0, b1, s1), (40, 128, 256, 256, 8, 8, 128, 0, b1, s1), (40, 128, 256, 128, 8, 8, 128, 0, b1, s1),
                   (41, 512, 256, 128, 16, 16, 128, 0, b2, s2), (41, 512, 128, 128, 16, 16, 64, 0, b2, s2), (41, 512, 128, 64, 16, 16, 64, 0, b2, s2)]
    assert all(t[1] == L.OP_EW for t in fu.tags if t[2] == "freeu.concat")
    # every plain concat that is left belongs to up block 2, and that block and the output are unchanged launch for launch
    assert {t[0] for t in fu.tags if t[2] == "skip.concat"} == {42}
    assert _rows(plain, (42, 60)) == _rows(fu, (42, 60)) and len(_rows(fu, (42,))) > 6
    # down path, mid block: untouched
    assert _rows(plain, (1, 2, 10, 11, 12, 20, 21, 22, 30, 31)) == _rows(fu, (1, 2, 10, 11, 12, 20, 21, 22, 30, 31))


def test_enabled_trace_at_full_width_grows_by_the_concats_and_their_statistics_passes():
    """SDXL widths at 1024^2 (UNet batch 2): the plain step reads every up-block concat from its two producers; with FreeU the six
    concats of up blocks 0 and 1 are launches, each followed by the statistics pass of the tensor it wrote -- 745 -> 757 launches and
    nothing else changes"""
    import forward_recordings as FR
    u = FR.sdxl_unet_meta()
    plain = FR.record_forward(u, 1, 128, 128)
    u.enable_freeu(*SDXL)
    fu = FR.record_forward(u, 1, 128, 128)
    assert _delta(plain, fu) == {(40, "freeu.concat"): 3, (40, "gn_stats"): 3, (41, "freeu.concat"): 3, (41, "gn_stats"): 3}
    assert len(plain.tags) == 745 and len(fu.tags) == 757
    got = [(o[1].n, o[1].i0, o[1].i1, o[1].i2, o[1].i3, o[1].i4) for t, o in zip(fu.tags, fu._ops) if t[2] == "freeu.concat"]
    assert got == [(2048, 1280, 1280, 32, 32, 640), (2048, 1280, 1280, 32, 32, 640), (2048, 1280, 640, 32, 32, 640),
                   (8192, 1280, 640, 64, 64, 640), (8192, 640, 640, 64, 64, 320), (8192, 640, 320, 64, 64, 320)]
    assert _rows(plain, (42, 60)) == _rows(fu, (42, 60))
    by = {t[2]: t[4] for t in fu.tags if t[2] == "freeu.concat"}
    assert by["freeu.concat"] > 0                                          # nbytes is accounted


# ------------------------------------------------------------------------------------------------------------------ the plan key
def test_plan_key_carries_freeu_only_where_it_is_enabled():
    from imagharmony_amd.denoise import PlanKey
    base = ("DDIMScheduler", 1000, 4, 0.0, 1.0, None, 1.0, 4, "abc")
    kw = dict(controlnet=None, inpaint=None, adapter=None, seeded=False)
    k0 = PlanKey(*base, **kw)
    assert PlanKey(*base, **kw, freeu=None) == k0 and len(k0) == 13 and type(k0) is PlanKey and k0.freeu is None and k0.regions is None
    ka, kb = PlanKey(*base, **kw, freeu=SDXL), PlanKey(*base, **kw, freeu=(0.9, 0.2, 1.2, 1.4))
    assert ka != kb and ka != k0 and kb != k0 and len({k0, ka, kb}) == 3
    assert ka.freeu == SDXL and ka.regions is None and ka[:13] == k0 and ka == PlanKey(*base, **kw, freeu=list(SDXL))
    kr = PlanKey(*base, **kw, regions="digest")
    krf = PlanKey(*base, **kw, regions="digest", freeu=SDXL)
    assert kr.freeu is None and krf.regions == "digest" and krf.freeu == SDXL and len({k0, ka, kr, krf}) == 4


def test_toggling_freeu_rerecords_once_and_toggling_back_hits_the_cache():
    def run():
        eng = ET.engine()
        u = eng.unet
        cond_ctx, kv, aug = eng._cond_ctx, eng.st.kv, eng.st.aug_emb
        try:
            eng.set_schedule(ET.hs.DDIMScheduler(), 4)
            key_plain = eng._sched_key
            assert eng.plan is None and len(key_plain) == 13
            eng._record()
            plain = eng.plan
            u.enable_freeu(*SDXL)
            eng.set_schedule(ET.hs.DDIMScheduler(), 4)
            assert eng.plan is None and eng._sched_key != key_plain and eng._sched_key.freeu == SDXL and eng._sched_key[:13] == key_plain
            eng._record()
            fu = eng.plan
            assert fu is not plain and sum(t[2] == "freeu.concat" for t in fu.tags) == 6
            assert not any(t[2] == "freeu.concat" for t in plain.tags)
            u.disable_freeu()
            eng.set_schedule(ET.hs.DDIMScheduler(), 4)
            assert eng.plan is plain and eng._sched_key == key_plain
            u.enable_freeu(*SDXL)
            eng.set_schedule(ET.hs.DDIMScheduler(), 4)
            assert eng.plan is fu
            u.enable_freeu(0.9, 0.2, 1.2, 1.4)                              # other values: a third plan
            eng.set_schedule(ET.hs.DDIMScheduler(), 4)
            assert eng.plan is None and len(eng._plans) == 2
            # no re-conditioning: the caches are the ones set_conditioning made
            assert eng._cond_ctx is cond_ctx and eng.st.kv is kv and eng.st.aug_emb is aug
        finally:
            u.disable_freeu()
    ET.dry(run)()


# ------------------------------------------------------------------------------------------------------------------ header and refusals
def test_header_keeps_abi_13_and_the_c_entry_refuses():
    from imagharmony_amd import lib
    hdr = open(os.path.join(ROOT, "include", "imh.h")).read()
    l = lib.load()
    assert l.imh_abi_version() == lib.ABI_VERSION == 13 and re.search(r"#define IMH_ABI_VERSION 13\b", hdr)
    body = re.search(r"enum imh_ew_op \{(.*?)\n\};", hdr, re.S).group(1)
    names = re.findall(r"^\s*(IMH_EW_[A-Z0-9_]+)", re.sub(r"/\*.*?\*/", "", body, flags=re.S), re.M)
    assert len(names) == 14 and names[2] == "IMH_EW_CONCAT" and lib.EW_CONCAT == 2
    assert [f[0] for f in lib.EwArgs._fields_][-4:] == ["x2", "noise", "mask", "blend_tab"] and len(lib.EwArgs._fields_) == 23
    kinds = re.findall(r"(IMH_OP_[A-Z_]+) = (\d+)", re.search(r"enum imh_op_kind \{(.*?)\};", hdr, re.S).group(1))
    assert len(kinds) == 12 and len(lib.OPS) == len({k for k in lib.OPS})
    assert "i2 > 0" in body and "fourier_filter" in body                  # the FreeU form is documented at the op
    mem = hdr[hdr.index("/* Memory: every elementwise op"):hdr.index("int imh_elementwise")]
    assert "IMH_EW_CONCAT" in mem and "n * (i0 + i1)" in mem

    def call(**kw):
        e = lib.EwArgs()
        e.a = e.b = e.y = 64                                               # never dereferenced: every case is refused before a launch
        e.n, e.i0, e.i1, e.i2, e.i3, e.i4, e.f0, e.f1, e.dtype = 128, 16, 16, 8, 8, 8, 1.1, 0.6, lib.IMH_DT_BF16
        for k, v in kw.items():
            setattr(e, k, v)
        return l.imh_elementwise(lib.EW_CONCAT, C.byref(e), None), l.imh_last_error() or b""
    for kw in (dict(i4=24), dict(i4=-1), dict(n=100), dict(i2=1, n=128), dict(i3=1), dict(i0=12), dict(i1=20), dict(i2=40000, i3=2, n=80000)):
        rc, msg = call(**kw)
        assert rc in (-1, -2) and b"concat" in msg, (kw, rc, msg)
