"""CPU (no GPU): perturbed-attention guidance.  Which self-attention layers a pattern chooses; the header (ABI 13, fourteen element-wise
ops, 23 fields, twelve plan kinds: the new launches are forms of ops that exist) and the C entry's and Ctx.ew's refusals of malformed
new-form arguments; every combination that is not built, refused before a launch; what the dry-recorded forward and step gain with
PAG on, and that PAG off records what it always did, tag for tag and argument for argument; the plan key and the switch of modes."""
import ctypes as C
import importlib.util
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    """a private copy of a trace tool (its model cache is then this module's own: choosing PAG layers here never shows elsewhere)"""
    spec = importlib.util.spec_from_file_location(f"pag_{name}", os.path.join(ROOT, "tools", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


FT = _tool("forward_trace")
ET = _tool("engine_trace")


# ------------------------------------------------------------------------------------------------------------------ layer matching
def test_patterns_choose_attn1_layers_as_diffusers_does():
    from imagharmony_amd.unet import UNet2DConditionModel, UNetConfig
    with torch.device("meta"):
        u = UNet2DConditionModel(UNetConfig())                             # the SDXL layout
    assert u.pag_layers is None and u.pag_layer_names() == []
    u.set_pag_applied_layers("mid")
    names = u.pag_layer_names()
    assert names == [f"mid_block.attentions.0.transformer_blocks.{i}.attn1" for i in range(10)] and u.pag_layers == ("mid",)
    u.set_pag_applied_layers(["down_blocks.2", "up_blocks.0.attentions.1"])
    names = u.pag_layer_names()
    assert len(names) == 2 * 10 + 10 and all(n.endswith(".attn1") for n in names)
    assert sum(n.startswith("down_blocks.2.") for n in names) == 20 and sum(n.startswith("up_blocks.0.attentions.1.") for n in names) == 10
    with pytest.raises(ValueError, match="matches no self-attention layer"):
        u.set_pag_applied_layers(["mid", "down_blocks.0"])                 # down block 0 has no attention
    assert len(u.pag_layer_names()) == 30                                  # a refused call changes nothing
    with pytest.raises(ValueError):
        u.set_pag_applied_layers("attn2")                                  # cross-attention layers are not candidates
    with pytest.raises(ValueError):
        u.set_pag_applied_layers([])
    u.set_pag_applied_layers(".")
    assert len(u.pag_layer_names()) == 70                                  # every attn1 of SDXL
    u.set_pag_applied_layers(None)
    assert u.pag_layers is None and u.pag_layer_names() == []


def test_the_surface_exists_on_every_pipeline_class():
    import inspect
    from imagharmony_amd import pipeline as P
    from imagharmony_amd.denoise import DenoiseEngine
    pipes = [c for n, c in vars(P).items() if inspect.isclass(c) and n.startswith("StableDiffusionXL") and n.endswith("Pipeline")]
    assert len(pipes) >= 7 and all(callable(c.set_pag_applied_layers) for c in pipes)
    for c in (P.StableDiffusionXLCustomPipeline, P.StableDiffusionXLImg2ImgCustomPipeline, P.StableDiffusionXLInpaintCustomPipeline):
        prm = inspect.signature(c.__call__).parameters
        assert prm["pag_scale"].default == 0.0 and prm["pag_adaptive_scale"].default == 0.0, c
    assert inspect.signature(DenoiseEngine.set_conditioning).parameters["pag_scale"].default == 0.0
    u = ET.unet()
    pipe = P.StableDiffusionXLCustomPipeline(u, device="cpu")
    try:
        pipe.set_pag_applied_layers("mid")
        assert u.pag_layers == ("mid",) and len(u.pag_layer_names()) == 2
        pipe.set_pag_applied_layers(None)
        assert u.pag_layers is None
    finally:
        u.set_pag_applied_layers(None)


# ------------------------------------------------------------------------------------------------------------------ header and refusals
def test_header_keeps_its_pins_and_documents_the_forms():
    from imagharmony_amd import lib
    hdr = open(os.path.join(ROOT, "include", "imh.h")).read()
    l = lib.load()
    assert l.imh_abi_version() == lib.ABI_VERSION == 13 and re.search(r"#define IMH_ABI_VERSION 13\b", hdr)
    body = re.search(r"enum imh_ew_op \{(.*?)\n\};", hdr, re.S).group(1)
    names = re.findall(r"^\s*(IMH_EW_[A-Z0-9_]+)", re.sub(r"/\*.*?\*/", "", body, flags=re.S), re.M)
    assert len(names) == 14 and names[-1] == "IMH_EW_CFG_MSTEP" and len(lib.EwArgs._fields_) == 23
    kinds = re.findall(r"(IMH_OP_[A-Z_]+) = (\d+)", re.search(r"enum imh_op_kind \{(.*?)\};", hdr, re.S).group(1))
    assert len(kinds) == 12
    assert "i5 > 0" in body and "identity" in body and "col0" in body      # the identity-attention form, at IMH_EW_CONCAT
    assert body.count("i2 = 1") >= 3 and "(c - p)" in body                 # the three-term form, at the two step ops and the rescale op
    mem = hdr[hdr.index("/* Memory: every elementwise op"):hdr.index("int imh_elementwise")]
    assert "identity-attention form" in mem and "i2 = 1" in mem


def _concat_args(lib, **kw):
    e = lib.EwArgs()
    e.b = e.y = 64                                                         # never dereferenced: every case is refused before a launch
    e.n, e.i0, e.i1, e.i2, e.i3, e.i4, e.i5, e.dtype = 64, 0, 64, 0, 64, 0, 64, lib.IMH_DT_BF16
    for k, v in kw.items():
        setattr(e, k, v)
    return e


BAD_IDENTITY = (dict(n=24), dict(n=0), dict(i4=8), dict(i4=-16), dict(i1=60), dict(i1=0), dict(i5=68), dict(i5=48), dict(i4=16), dict(i3=60),
                dict(i3=56), dict(i0=8), dict(i2=8), dict(b=0), dict(b=72), dict(y=72))


def test_the_c_entry_refuses_malformed_identity_rows_and_step_forms():
    from imagharmony_amd import lib
    l = lib.load()
    for kw in BAD_IDENTITY:
        rc = l.imh_elementwise(lib.EW_CONCAT, C.byref(_concat_args(lib, **kw)), None)
        msg = l.imh_last_error() or b""
        assert rc == -1 and b"concat" in msg and (b"identity" in msg or b"null" in msg), (kw, rc, msg)      # IMH_ERR_ARG, a telling text
    for op, who in ((lib.EW_CFG_STEP, b"cfg_step"), (lib.EW_CFG_MSTEP, b"cfg_mstep"), (lib.EW_CFG_RESCALE, b"cfg_rescale")):
        e = lib.EwArgs()
        e.a = e.y = e.tab = e.step = 64
        e.i0, e.i1, e.i2, e.i3, e.dtype = 1, 16, 2, 1, lib.IMH_DT_BF16
        rc = l.imh_elementwise(op, C.byref(e), None)
        assert rc == -1 and who in (l.imh_last_error() or b"") and b"i2" in l.imh_last_error(), (op, rc, l.imh_last_error())


def test_ctx_refuses_what_the_library_refuses():
    from imagharmony_amd import lib as L
    from imagharmony_amd.ctx import Ctx
    ctx = Ctx("cpu", torch.bfloat16, record=True, dry=True)
    vt, y = torch.zeros(64, 128, dtype=torch.bfloat16), torch.zeros(64, 64, dtype=torch.bfloat16)
    assert vt.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 0
    ok = dict(n=64, i=(0, 64, 0, 64, 0, 128))
    ctx.ew(L.EW_CONCAT, y, b=vt, **ok)                                     # the well-formed launch records
    assert len(ctx.tags) == 1 and ctx.tags[0][1] == L.OP_EW
    for kw in (dict(n=24), dict(n=0), dict(i=(0, 64, 0, 64, 8, 128)), dict(i=(0, 60, 0, 64, 0, 128)), dict(i=(0, 64, 0, 64, 0, 100)),
               dict(i=(0, 64, 0, 64, 80, 128)), dict(i=(0, 64, 0, 60, 0, 128)), dict(i=(0, 64, 0, 56, 0, 128)), dict(i=(8, 64, 0, 64, 0, 128)),
               dict(i=(0, 64, 8, 64, 0, 128))):
        with pytest.raises(L.ImhError, match="identity"):
            ctx.ew(L.EW_CONCAT, y, b=vt, **dict(ok, **kw))
    with pytest.raises(L.ImhError, match="identity"):
        ctx.ew(L.EW_CONCAT, y, b=None, **ok)
    with pytest.raises(L.ImhError, match="identity"):
        ctx.ew(L.EW_CONCAT, y, b=vt[:, 4:], **ok)                          # 8 bytes off
    with pytest.raises(L.ImhError):
        ctx.identity_rows(vt, y[:, :32], 64, 0)                            # out narrower than C
    lat, tab, step = torch.zeros(1, 4, 16), torch.zeros(4, 2), torch.zeros(1, dtype=torch.int32)
    for op in (L.EW_CFG_STEP, L.EW_CFG_RESCALE):
        with pytest.raises(L.ImhError, match="i2"):
            ctx.ew(op, lat, a=torch.zeros(3, 16, 4, dtype=torch.bfloat16), tab=tab, step=step, i=(1, 16, 2, 1, 0, 0))
    with pytest.raises(L.ImhError, match="i2"):
        ctx.ew(L.EW_CFG_STEP, lat, a=None, tab=tab, step=step, i=(1, 16, 1, 1, 0, 0))
    assert len(ctx.tags) == 1                                              # nothing of the refused was recorded


def _embeds(u, S=1):
    cd, pd = u.config.cross_attention_dim, u.config.pooled_dim
    return dict(prompt_embeds=torch.zeros(S, 77 + ET.TOKENS, cd), negative_prompt_embeds=torch.zeros(S, 77 + ET.TOKENS, cd),
                pooled_prompt_embeds=torch.zeros(S, pd), negative_pooled_prompt_embeds=torch.zeros(S, pd))


def test_what_is_not_built_is_refused_before_a_launch():
    from imagharmony_amd import denoise as D
    from imagharmony_amd import pipeline as P
    from imagharmony_amd.ip_adapter import IPAdapterXL
    u = ET.unet()
    launches = []

    class NoLaunch(ET.DryCtx):
        def _emit(self, *a, **kw):
            launches.append(a)
            raise AssertionError("a launch before the refusal")

    def run():
        kw = dict(_embeds(u), output_type="latent", num_inference_steps=2, height=ET.SIDE, width=ET.SIDE)
        pipe = P.StableDiffusionXLCustomPipeline(u, device="cpu")
        with pytest.raises(NotImplementedError, match="pag_adaptive_scale"):
            pipe(**kw, pag_scale=3.0, pag_adaptive_scale=0.1)
        with pytest.raises(NotImplementedError, match="pag_adaptive_scale"):
            pipe(**kw, pag_adaptive_scale=0.1)                             # ... whatever pag_scale is
        with pytest.raises(ValueError, match="pag_scale"):
            pipe(**kw, pag_scale=-1.0)
        with pytest.raises(NotImplementedError, match="regional image prompts"):
            pipe(**kw, pag_scale=3.0, ip_region_masks=[torch.ones(ET.SIDE, ET.SIDE)])
        cn = P.StableDiffusionXLControlNetCustomPipeline(u, ET.controlnet(), device="cpu")
        with pytest.raises(NotImplementedError, match="ControlNet"):
            cn(**kw, image=ET.control_image(), pag_scale=3.0)
        ad = P.StableDiffusionXLAdapterCustomPipeline(u, ET.adapter(), device="cpu")
        with pytest.raises(NotImplementedError, match="T2I-Adapter"):
            ad(**kw, image=ET.control_image(), pag_scale=3.0)
        e = _embeds(u)
        emb = (e["prompt_embeds"], e["negative_prompt_embeds"], e["pooled_prompt_embeds"], e["negative_pooled_prompt_embeds"])
        eng = D.DenoiseEngine(u, "cpu", ET.DTYPE, False)
        with pytest.raises(NotImplementedError, match="cfg_role"):
            eng.set_conditioning(*emb, ET.SIDE, ET.SIDE, cfg_role=1, pag_scale=3.0)
        eng = D.DenoiseEngine(u, "cpu", ET.DTYPE, False)
        eng.set_controlnet(ET.controlnet())
        with pytest.raises(NotImplementedError, match="ControlNet"):
            eng.set_conditioning(*emb, ET.SIDE, ET.SIDE, pag_scale=3.0)
        eng = D.DenoiseEngine(u, "cpu", ET.DTYPE, False)
        eng.set_adapter(ET.adapter())
        with pytest.raises(NotImplementedError, match="T2I-Adapter"):
            eng.set_conditioning(*emb, ET.SIDE, ET.SIDE, pag_scale=3.0)
        with pytest.raises(NotImplementedError, match="generate_pns"):
            IPAdapterXL.generate_pns(types.SimpleNamespace(), [0, 1], pag_scale=3.0)
        # the UNet itself: perturbed samples next to a ControlNet's or an adapter's residuals, or without chosen layers
        from imagharmony_amd import lib as L
        with pytest.raises(NotImplementedError, match="perturbed-attention"):
            u.emit_forward(None, None, 1, 32, 32, control=object(), pag=1)

    import unittest.mock as mock
    try:
        u.set_pag_applied_layers("mid")
        with mock.patch.object(D, "Ctx", NoLaunch), torch.no_grad():
            run()
        u.set_pag_applied_layers(None)
        from imagharmony_amd import lib as L
        with pytest.raises(L.ImhError, match="set_pag_applied_layers"):
            u.emit_forward(None, types.SimpleNamespace(), 1, 32, 32, pag=1)
    finally:
        u.set_pag_applied_layers(None)
    assert not launches


# ------------------------------------------------------------------------------------------------------------------ the recorded forward
def _record_tiny(u, S=1, Hl=32, Wl=32, pag=False, batch3=False):
    """cfg_dup forward over S latents (UNet batch 2S), with pag the perturbed block behind it (3S); batch3: the plain forward at batch 3S"""
    from imagharmony_amd.ctx import Ctx
    B = 3 * S if (pag or batch3) else 2 * S
    ctx = Ctx("cpu", torch.bfloat16, record=True, dry=True)
    st = u.prepare_conditioning(ctx, torch.zeros(B, 81, 256), torch.zeros(B, 128), torch.zeros(B, 6))
    n0 = len(ctx.tags)
    st.t_value = torch.zeros(B)
    if batch3:
        st.latents = torch.zeros(B, 4, Hl, Wl)
        out = u.emit_forward(ctx, st, B, Hl, Wl, cfg_dup=False)
    else:
        st.latents = torch.zeros(S, 4, Hl, Wl)
        out = u.emit_forward(ctx, st, S, Hl, Wl, cfg_dup=True, **({"pag": S} if pag else {}))
    assert out.shape[0] == B
    return ctx, n0


def _hist(ctx, n0):
    h = {}
    for t in ctx.tags[n0:]:
        h[(t[0], t[2])] = h.get((t[0], t[2]), 0) + 1
    return h


@pytest.mark.parametrize("S,Hl,Wl", [(1, 32, 32), (2, 32, 32), (1, 36, 28)])
@pytest.mark.parametrize("layers,chosen", [("mid", {31: 2}), (".", {21: 2, 22: 4, 31: 2, 50: 6, 51: 3})])
def test_recorded_forward_with_pag(S, Hl, Wl, layers, chosen):
    """tiny UNet: 32 x 32 runs the mid block at 64 tokens (the folded path), 36 x 28 at 63 (the ragged path).  With PAG the forward is
    the plain forward at batch 3S plus ONE launch per chosen layer, and in those layers the attention launch runs the first 2S samples"""
    from imagharmony_amd import lib as L
    u = ET.unet()
    try:
        plain3, p0 = _record_tiny(u, S, Hl, Wl, batch3=True)
        u.set_pag_applied_layers(layers)
        pag, n0 = _record_tiny(u, S, Hl, Wl, pag=True)
    finally:
        u.set_pag_applied_layers(None)
    hp, hg = _hist(plain3, p0), _hist(pag, n0)
    delta = {k: hg.get(k, 0) - hp.get(k, 0) for k in set(hp) | set(hg) if hp.get(k, 0) != hg.get(k, 0)}
    assert delta == {(tag, "self.pag_rows"): n for tag, n in chosen.items()}
    assert len(pag.tags) - n0 == len(plain3.tags) - p0 + sum(chosen.values())
    rows = [(t, o[1]) for t, o in zip(pag.tags[n0:], pag._ops[n0:])]
    assert all(t[1] == L.OP_EW and o.i5 > 0 and o.i0 == 0 and o.i2 == 0 for t, o in rows if t[2] == "self.pag_rows")
    # launch order inside a chosen layer: projections, attention over 2S samples, the copy, to_out; elsewhere attention over 3S
    seen = {}
    for k, (t, o) in enumerate(rows):
        if t[2] != "self.attn":
            continue
        nxt = rows[k + 1][0][2]
        if nxt == "self.pag_rows":
            c = rows[k + 1][1]
            assert o.B == 2 * S and c.n == S * o.Lk_pad and c.i4 == 2 * S * o.Lk_pad and c.i5 == o.ldvt == 3 * S * o.Lk_pad and c.i1 == c.i3 == o.ldo
            seen[t[0]] = seen.get(t[0], 0) + 1
        else:
            assert o.B == 3 * S
    assert seen == chosen
    conv_in = [o[1] for t, o in zip(pag.tags, pag._ops) if t[2] == "conv_in"]
    assert len(conv_in) == 1 and conv_in[0].i0 == S and conv_in[0].i4 == 3 * S      # the perturbed block reads latent b % S


def test_pag_off_records_the_forward_it_always_did():
    u = ET.unet()
    try:
        warm = _record_tiny(u)                                             # (the first recording also builds the UNet's derived weights: not the one to compare)
        before, _ = _record_tiny(u)
        u.set_pag_applied_layers("mid")
        chosen_but_unused, _ = _record_tiny(u)                             # layers chosen, no perturbed samples: nothing changes
        with_pag, _ = _record_tiny(u, pag=True)
        u.set_pag_applied_layers(None)
        after, _ = _record_tiny(u)
    finally:
        u.set_pag_applied_layers(None)
    # tag for tag and argument for argument.  (describe()'s sha1_alias is left out: it numbers buffers by address, and the few host
    # tensors a dry recording does not keep alive may get an address again -- which recordings that happens in depends on the heap)
    tags = lambda c: {k: v for k, v in FT.describe(c).items() if k != "sha1_alias"}
    for other in (warm[0], chosen_but_unused, after):
        assert tags(before) == tags(other)
        assert FT.args_digest(before) == FT.args_digest(other)
    assert tags(before)["sha1"] != tags(with_pag)["sha1"]


# ------------------------------------------------------------------------------------------------------------------ the engine
def _tail(plan):
    return [(t[2], o[1]) for t, o in zip(plan.tags, plan._ops) if ET._is_tail(t[2])]


@pytest.mark.parametrize("guidance,rescale", [(5.0, 0.0), (5.0, 0.7), (1.0, 0.0)])
def test_engine_conditions_and_records_the_third_block(guidance, rescale):
    def run():
        u = ET.unet()
        try:
            u.set_pag_applied_layers("mid")
            eng = ET.D.DenoiseEngine(u, "cpu", ET.DTYPE, False)
            cd, pd = u.config.cross_attention_dim, u.config.pooled_dim
            pos, neg = torch.full((1, 77 + ET.TOKENS, cd), 1.0), torch.full((1, 77 + ET.TOKENS, cd), -1.0)
            eng.set_conditioning(pos, neg, torch.full((1, pd), 2.0), torch.full((1, pd), -2.0), ET.SIDE, ET.SIDE, guidance_scale=guidance,
                                 guidance_rescale=rescale, pag_scale=3.0)
            cfg = guidance > 1.0
            B = 3 if cfg else 2
            ehs, text, ids = eng._cond_in
            assert eng.pag and eng.pag_scale == 3.0 and ehs.shape[0] == text.shape[0] == ids.shape[0] == B
            want = [-1.0, 1.0, 1.0] if cfg else [1.0, 1.0]                  # [neg | pos | pos]  /  [pos | pos]
            assert ehs[:, 0, 0].tolist() == want and (text[:, 0] / 2).tolist() == want
            assert eng.st.aug_emb.shape[0] == B and all(kv.k.shape[0] == B and (kv.k2 is None or kv.k2.shape[0] == B) for kv in eng.st.kv.values())
            eng.set_schedule(ET.hs.DDIMScheduler(), 4)
            key = eng._sched_key
            assert len(key) == 14 and key.pag[1] == 3.0 and len(key.pag[0]) == 40 and key.freeu is None and key.regions is None
            eng._record()
            assert eng.noise_pred.shape[0] == B and eng.st.temb_table.shape[1] == B * u.temb_total
            assert sum(t[2] == "self.pag_rows" for t in eng.plan.tags) == 2
            tail = _tail(eng.plan)
            step = tail[-1]
            assert step[0] == "cfg+step+pag" and (step[1].i0, step[1].i2, step[1].i3, step[1].f3) == (1, 1, int(cfg), 3.0)
            if cfg and rescale:
                assert tail[0][0] == "cfg.rescale" and (tail[0][1].i2, tail[0][1].f0, tail[0][1].f3) == (1, 3.0, float(torch.tensor(rescale)))
            else:
                assert len(tail) == 1
            # the general step carries the form too
            eng.set_schedule(ET.hs.DPMSolverMultistepScheduler(), 4)
            eng._record()
            step = _tail(eng.plan)[-1]
            assert step[0] == "cfg+mstep+pag" and (step[1].i2, step[1].f3) == (1, 3.0)
        finally:
            u.set_pag_applied_layers(None)
    ET.dry(run)()


def test_plan_key_carries_pag_only_where_it_is_on():
    from imagharmony_amd.denoise import PlanKey
    base = ("DDIMScheduler", 1000, 4, 0.0, 1.0, None, 1.0, 4, "abc")
    kw = dict(controlnet=None, inpaint=None, adapter=None, seeded=False)
    k0 = PlanKey(*base, **kw)
    assert PlanKey(*base, **kw, pag=None) == k0 and len(k0) == 13 and type(k0) is PlanKey and k0.pag is None
    ka, kb, kc = PlanKey(*base, **kw, pag=("d1", 3.0)), PlanKey(*base, **kw, pag=("d1", 2.0)), PlanKey(*base, **kw, pag=("d2", 3.0))
    assert len({k0, ka, kb, kc}) == 4 and ka.pag == ("d1", 3.0) and ka[:13] == k0 and ka.freeu is None and ka.regions is None
    kf = PlanKey(*base, **kw, freeu=(0.6, 0.4, 1.1, 1.2), pag=("d1", 3))
    assert kf.freeu == (0.6, 0.4, 1.1, 1.2) and kf.pag == ("d1", 3.0) and kf[-1] == kf.pag and len(kf) == 15 and kf.regions is None
    assert PlanKey(*base, **kw, freeu=(0.6, 0.4, 1.1, 1.2)).pag is None and PlanKey(*base, **kw, regions="r").pag is None


def test_switching_pag_records_once_and_switching_back_reuses_the_plan_and_the_caches():
    def run():
        u = ET.unet()
        try:
            # an engine that never meets PAG carries none of its state (the fork and plan goldens see the instance it always was)
            eng = ET.engine()
            assert not ({"pag", "pag_scale", "_cond_fp", "_cond_stash"} & set(vars(eng))) and "pag" not in vars(eng.st)
            # layers chosen, scale 0: conditioned without PAG -- the key and the plan of an engine without the layers
            u.set_pag_applied_layers("mid")
            eng = ET.engine()
            plain_st, plain_kv, plain_ctx = eng.st, eng.st.kv, eng._cond_ctx
            eng.set_schedule(ET.hs.DDIMScheduler(), 4)
            key_plain = eng._sched_key
            eng._record()
            plain = eng.plan
            assert not eng.pag and len(key_plain) == 13 and key_plain.pag is None and not any(t[2] == "self.pag_rows" for t in plain.tags)
            # PAG on: a conditioning of batch 3 and ONE new plan; the plain conditioning is kept aside
            cd, pd = u.config.cross_attention_dim, u.config.pooled_dim
            emb = (torch.zeros(1, 77 + ET.TOKENS, cd), torch.zeros(1, 77 + ET.TOKENS, cd), torch.zeros(1, pd), torch.zeros(1, pd))
            eng.set_conditioning(*emb, ET.SIDE, ET.SIDE, guidance_scale=5.0, pag_scale=3.0)
            assert eng.pag and eng.st is not plain_st and eng._plans == {} and eng.plan is None
            eng.set_schedule(ET.hs.DDIMScheduler(), 4)
            assert eng._sched_key[:13] == key_plain and eng._sched_key.pag is not None
            eng._record()
            on, on_st = eng.plan, eng.st
            assert on is not plain and sum(t[2] == "self.pag_rows" for t in on.tags) == 2 and len(eng._plans) == 1
            assert on_st.latents is plain_st.latents and on_st.step is plain_st.step
            # other layers under the same conditioning: another key, no re-conditioning
            u.set_pag_applied_layers(".")
            eng.set_schedule(ET.hs.DDIMScheduler(), 4)
            assert eng.plan is None and eng._sched_key.pag[0] != on and eng.st is on_st
            u.set_pag_applied_layers("mid")
            eng.set_schedule(ET.hs.DDIMScheduler(), 4)
            assert eng.plan is on
            # PAG off again, same inputs: the earlier conditioning and its plan, nothing projected, nothing recorded
            eng.set_conditioning(*emb, ET.SIDE, ET.SIDE, guidance_scale=5.0)
            assert not eng.pag and eng.st is plain_st and eng.st.kv is plain_kv and eng._cond_ctx is plain_ctx
            eng.set_schedule(ET.hs.DDIMScheduler(), 4)
            assert eng.plan is plain and eng._sched_key == key_plain
            # ... and on again: the PAG conditioning and its plan
            eng.set_conditioning(*emb, ET.SIDE, ET.SIDE, guidance_scale=5.0, pag_scale=3.0)
            eng.set_schedule(ET.hs.DDIMScheduler(), 4)
            assert eng.st is on_st and eng.plan is on
            # another scale, or other inputs, is a new conditioning
            eng.set_conditioning(*emb, ET.SIDE, ET.SIDE, guidance_scale=5.0, pag_scale=2.0)
            assert eng.st is not on_st and eng._plans == {}
            eng.set_conditioning(emb[0] + 1, *emb[1:], ET.SIDE, ET.SIDE, guidance_scale=5.0)
            assert eng.st is not plain_st and not eng.pag
            # the layers cleared under a PAG conditioning: a telling error, not a forward without the copy
            eng.set_conditioning(*emb, ET.SIDE, ET.SIDE, guidance_scale=5.0, pag_scale=2.0)
            u.set_pag_applied_layers(None)
            from imagharmony_amd import lib as L
            with pytest.raises(L.ImhError, match="PAG layers were cleared"):
                eng.set_schedule(ET.hs.DDIMScheduler(), 4)
            # a fingerprint describes the conditioning it was taken for and no later one
            u.set_pag_applied_layers("mid")
            other = ET.engine()
            assert other._cond_fp is not None and other._cond_stash is None
            u.set_pag_applied_layers(None)
            ET.condition(other)
            assert other._cond_fp is None and other._cond_stash is None and not other.pag
        finally:
            u.set_pag_applied_layers(None)
    ET.dry(run)()


def test_pipeline_call_with_scale_zero_or_without_layers_conditions_as_before():
    """what reaches the engine: pag_scale only where PAG is on -- a call with pag_scale = 0, or with no layers chosen, is the call it was"""
    from imagharmony_amd import pipeline as P
    u = ET.unet()
    seen = []

    class Eng:
        seeded = False

        def set_conditioning(self, *a, **kw):
            seen.append(kw)
            raise StopIteration

    pipe = P.StableDiffusionXLCustomPipeline(u, device="cpu")
    pipe.engine = Eng()
    kw = dict(_embeds(u), output_type="latent", num_inference_steps=2, height=ET.SIDE, width=ET.SIDE)
    try:
        for layers, scale, want in ((None, 0.0, None), (None, 3.0, None), ("mid", 0.0, None), ("mid", 3.0, 3.0)):
            u.set_pag_applied_layers(layers)
            with pytest.raises(StopIteration):
                pipe(**kw, pag_scale=scale)
            assert seen[-1].get("pag_scale") == want and ("pag_scale" in seen[-1]) == (want is not None), (layers, scale, seen[-1])
    finally:
        u.set_pag_applied_layers(None)


def test_ip_adapter_generate_forwards_the_pag_arguments():
    """IPAdapterXL.generate and IPAdapterPlusXL.generate reach the pipe's __call__ through one tail, with their keywords as given"""
    from imagharmony_amd.ip_adapter import IPAdapterPlusXL, IPAdapterXL
    seen = []

    class Pipe:
        def __call__(self, **kw):
            seen.append(kw)
            return types.SimpleNamespace(images=["image"])

    for cls, more in ((IPAdapterXL, dict(clip_image_embeds=torch.zeros(1, 8))), (IPAdapterPlusXL, dict(clip_hidden_states=torch.zeros(1, 4, 8)))):
        me = types.SimpleNamespace(pipe=Pipe(), dtype=torch.float32, set_scale=lambda s: None,
                                   get_image_embeds=lambda *a, **k: (torch.zeros(1, 4, 16), torch.zeros(1, 4, 16)))
        me._run = types.MethodType(cls._run, me)
        out = cls.generate(me, prompt_embeds=(torch.zeros(1, 77, 16), torch.zeros(1, 77, 16), torch.zeros(1, 8), torch.zeros(1, 8)),
                           num_samples=1, seed=0, num_inference_steps=2, pag_scale=3.0, pag_adaptive_scale=0.0, **more)
        assert out == ["image"] and seen[-1]["pag_scale"] == 3.0 and seen[-1]["pag_adaptive_scale"] == 0.0, cls
        assert seen[-1]["prompt_embeds"].shape == (1, 81, 16)
