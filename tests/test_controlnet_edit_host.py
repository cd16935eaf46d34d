"""Host-side pins of the ControlNet edit pipelines (no GPU): the two classes, their exports and class relations, every refusal of their
call and of generate_pns's control arguments before a Ctx exists, the ControlNet gate table over truncated schedules, the reference
loop's own consistency, the dry-recorded step of a 9-channel UNet behind the branch, and the unchanged ABI."""
import hashlib
import os
import re

import pytest
import torch

import controlnet_reference as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _classes():
    from imagharmony_amd import pipeline as P
    return {"i2i": (P.StableDiffusionXLControlNetImg2ImgCustomPipeline, P.StableDiffusionXLImg2ImgCustomPipeline),
            "inp": (P.StableDiffusionXLControlNetInpaintCustomPipeline, P.StableDiffusionXLInpaintCustomPipeline)}


def test_classes_exports_and_relations():
    import inspect
    import imagharmony_amd
    from imagharmony_amd import pipeline as P
    for mode, (cls, parent) in _classes().items():
        assert getattr(imagharmony_amd, cls.__name__) is cls and cls.__name__ in imagharmony_amd._PIPELINES
        assert issubclass(cls, parent) and issubclass(cls, P.StableDiffusionXLCustomPipeline)
        assert not issubclass(cls, P.StableDiffusionXLControlNetCustomPipeline)        # (an edit pipe is not the text-to-image ControlNet pipe)
        # the ControlNet parts are shared with the text-to-image class, not restated
        assert cls.__init__ is P.StableDiffusionXLControlNetCustomPipeline.__init__ and cls.to is P.StableDiffusionXLControlNetCustomPipeline.to
        assert cls._run is P.StableDiffusionXLCustomPipeline._run                       # one call skeleton
        ps = inspect.signature(cls.__call__).parameters
        pp = inspect.signature(parent.__call__).parameters
        assert set(pp) <= set(ps)                                                      # everything the parent edit call takes
        for k in pp:
            assert ps[k].default == pp[k].default, k
        for k, d in (("control_image", None), ("controlnet_conditioning_scale", 1.0), ("guess_mode", False), ("controlnet_guidance_start", 0.0),
                     ("controlnet_guidance_end", 1.0), ("control_guidance_start", 0.0), ("control_guidance_end", 1.0), ("step_noise", "generator")):
            assert ps[k].default == d, k
    # the per-call object: one small class over the two existing ones
    assert P._ControlNetEditCall.__mro__[1:4] == (P._ControlNetCall, P._EditCall, P._Call)
    assert {k for k in vars(P._ControlNetEditCall) if not k.startswith("__")} == {"control_arg"}

    class Multi:
        nets = [object(), object()]
    for cls, _ in _classes().values():
        for many in (Multi(), [object(), object()]):
            with pytest.raises(NotImplementedError, match="MultiControlNetModel"):
                cls(None, many)


def _bare(mode):
    """the class without an engine (tests/test_inpaint_host.py's _bare_pipe): whatever reaches for one fails"""
    from imagharmony_amd.schedulers import DDIMScheduler
    from imagharmony_amd.unet import UNetConfig

    class _U:
        config = UNetConfig()
    cls = _classes()[mode][0]
    pipe = cls.__new__(cls)
    pipe.vae = pipe.vae_decode = None
    pipe.scheduler = DDIMScheduler()
    pipe.unet = _U()
    pipe.controlnet = object()
    return pipe


@pytest.mark.parametrize("mode", ["i2i", "inp"])
def test_every_refusal_is_raised_before_a_ctx_exists(mode, monkeypatch):
    from imagharmony_amd import denoise
    from imagharmony_amd.vae import AutoencoderKL, VAEConfig

    def no_ctx(*a, **k):
        raise AssertionError("a Ctx was built before the refusal")
    monkeypatch.setattr(denoise, "Ctx", no_ctx)
    pipe = _bare(mode)
    img, mask, ctrl = torch.rand(1, 3, 64, 64), torch.ones(1, 1, 64, 64), torch.rand(1, 3, 64, 64)
    kw = dict(prompt_embeds=torch.zeros(1, 81, 8), pooled_prompt_embeds=torch.zeros(1, 8), output_type="latent", image=img,
              **({"mask_image": mask} if mode == "inp" else {}))
    # the ControlNet arguments
    with pytest.raises(ValueError, match="control_image"):
        pipe(**kw)
    for window in ((0.6, 0.4), (-0.1, 1.0), (0.0, 1.01)):
        with pytest.raises(ValueError, match="0 <= start <= end <= 1"):
            pipe(control_image=ctrl, controlnet_guidance_start=window[0], controlnet_guidance_end=window[1], **kw)
    with pytest.raises(NotImplementedError, match="guess_mode"):
        pipe(control_image=ctrl, guess_mode=True, **kw)
    with pytest.raises(NotImplementedError, match="list of conditioning scales"):
        pipe(control_image=ctrl, controlnet_conditioning_scale=[1.0, 0.5], **kw)
    kw["control_image"] = ctrl
    # everything the parent edit call refuses
    with pytest.raises(NotImplementedError, match="denoising_start"):
        pipe(denoising_start=0.5, **kw)
    with pytest.raises(NotImplementedError, match="latents="):
        pipe(latents=torch.zeros(1, 4, 8, 8), **kw)
    with pytest.raises(NotImplementedError, match="eta"):
        pipe(eta=0.5, **kw)
    with pytest.raises(NotImplementedError, match="needs a VAE"):
        pipe(**dict(kw, output_type="pil"))
    with pytest.raises(NotImplementedError, match="latent"):
        pipe(**dict(kw, image=torch.rand(1, 4, 8, 8)))
    with pytest.raises(ValueError, match="image"):
        pipe(**dict(kw, image=None))
    with pytest.raises(ValueError, match="strength"):
        pipe(strength=1.5, **kw)
    with pytest.raises(ValueError, match="step_noise"):
        pipe(step_noise="seeded", **kw)                                                # "seeded" without a generator
    if mode == "inp":
        with pytest.raises(NotImplementedError, match="padding_mask_crop"):
            pipe(padding_mask_crop=32, **kw)
        with pytest.raises(NotImplementedError, match="masked_image_latents"):
            pipe(masked_image_latents=torch.zeros(1, 4, 8, 8), **kw)
        with pytest.raises(ValueError, match="mask_image"):
            pipe(**{k: v for k, v in kw.items() if k != "mask_image"})
        with pytest.raises(NotImplementedError, match="resize the image"):
            pipe(height=128, width=128, **kw)
    with pytest.raises(NotImplementedError, match="with_encoder"):
        pipe(**kw)
    pipe.vae = AutoencoderKL(VAEConfig(block_out_channels=(64, 64), layers_per_block=1, sample_size=64), with_encoder=True)
    with pytest.raises(ValueError, match="control image tensor"):                       # not [n, 3, H, W]
        pipe(**dict(kw, control_image=torch.rand(1, 1, 64, 64)))
    with pytest.raises(ValueError, match="control image of type"):
        pipe(**dict(kw, control_image="edges.png"))
    three = dict(kw, prompt_embeds=torch.zeros(3, 81, 8), pooled_prompt_embeds=torch.zeros(3, 8))
    with pytest.raises(ValueError, match="2 control images for 3 samples"):
        pipe(**dict(three, control_image=torch.rand(2, 3, 64, 64)))
    with pytest.raises(ValueError, match="image batch"):
        pipe(**dict(three, image=torch.rand(2, 3, 64, 64)))
    with pytest.raises(ValueError, match="no denoising step"):
        pipe(strength=0.05, num_inference_steps=10, **kw)


# ---------------------------------------------------------------------------------------------------- the gate table
@pytest.mark.parametrize("window", [(0.0, 1.0), (0.0, 0.5), (0.25, 0.75), (0.3, 1.0), (0.0, 0.7), (1.0, 1.0)])
@pytest.mark.parametrize("steps,strength", [(5, 0.8), (4, 0.75), (6, 0.5), (3, 1.0), (30, 0.3), (50, 0.9999)])
def test_gate_table_over_truncated_schedules_is_controlnet_keep(window, steps, strength):
    """the window of the edit pipes counts the m = steps - t_start steps that run (diffusers: controlnet_keep over len(timesteps) after
    get_timesteps); the rows before t_start hold the scale"""
    from imagharmony_amd.denoise import DenoiseEngine
    from imagharmony_amd.schedulers import DDIMScheduler, get_timesteps
    import controlnet_edit_reference as cer
    sch = DDIMScheduler()
    sch.set_timesteps(steps)
    _, t_start = get_timesteps(sch, steps, strength)
    assert t_start == cer.t_start_of(steps, strength)
    m = steps - t_start
    scale = 0.7
    tab = DenoiseEngine.gate_table(steps, t_start, window[0], window[1], scale)
    assert len(tab) == steps and tab[:t_start] == [scale] * t_start
    assert tab[t_start:] == [scale * cr.keep(i, m, *window) for i in range(m)]
    if (steps, strength, window) == (5, 0.8, (0.25, 0.75)):
        assert tab == [scale, 0.0, scale, scale, 0.0]                                  # of the four steps that run: the first and the last are off
        assert DenoiseEngine.gate_table(steps, 0, *window, scale) == [0.0, 0.0, scale, 0.0, 0.0]        # ... not the full list's window


# ---------------------------------------------------------------------------------------------------- generate_pns
def _bare_adapter(pipe):
    from imagharmony_amd.ip_adapter import IPAdapterXL
    ip = IPAdapterXL.__new__(IPAdapterXL)
    ip.pipe, ip.image_encoder = pipe, None
    return ip


def test_generate_pns_control_arguments(monkeypatch):
    import inspect
    from imagharmony_amd import denoise
    from imagharmony_amd import pipeline as P
    from imagharmony_amd.ip_adapter import IPAdapterXL

    def no_ctx(*a, **k):
        raise AssertionError("a Ctx was built before the refusal")
    monkeypatch.setattr(denoise, "Ctx", no_ctx)
    ps = inspect.signature(IPAdapterXL.generate_pns).parameters
    assert ps["control_image"].default is None and ps["controlnet_conditioning_scale"].default == 1.0
    ctrl, img = torch.rand(1, 3, 64, 64), torch.rand(1, 3, 64, 64)
    for mode in ("i2i", "inp"):
        ip = _bare_adapter(_bare(mode))
        with pytest.raises(ValueError, match="control_image"):                         # a ControlNet pipe: required
            ip.generate_pns([1, 2], image=img, output_type="latent")
        with pytest.raises(NotImplementedError, match="list of conditioning scales"):
            ip.generate_pns([1, 2], image=img, control_image=ctrl, controlnet_conditioning_scale=[1.0], output_type="latent")
        with pytest.raises(ValueError, match="0 <= start <= end <= 1"):
            ip.generate_pns([1, 2], image=img, control_image=ctrl, controlnet_guidance_start=0.8, controlnet_guidance_end=0.2, output_type="latent")
        with pytest.raises(NotImplementedError, match="guess_mode"):
            ip.generate_pns([1, 2], image=img, control_image=ctrl, guess_mode=True, output_type="latent")
        with pytest.raises(NotImplementedError, match="EDITS of image="):              # the edit's own refusals follow
            ip.generate_pns([1, 2], control_image=ctrl, output_type="latent")
    # the text-to-image ControlNet pipe: control_image= there too; image= stays refused
    t2i = P.StableDiffusionXLControlNetCustomPipeline.__new__(P.StableDiffusionXLControlNetCustomPipeline)
    t2i.vae = t2i.vae_decode = None
    t2i.controlnet = object()
    ip = _bare_adapter(t2i)
    with pytest.raises(ValueError, match="control_image"):
        ip.generate_pns([1, 2], output_type="latent")
    with pytest.raises(ValueError, match="image= / mask_image= / strength="):
        ip.generate_pns([1, 2], image=img, control_image=ctrl, output_type="latent")
    # a pipe without a ControlNet: refused
    for cls in (P.StableDiffusionXLCustomPipeline, P.StableDiffusionXLImg2ImgCustomPipeline, P.StableDiffusionXLInpaintCustomPipeline):
        plain = cls.__new__(cls)
        plain.vae = plain.vae_decode = None
        with pytest.raises(ValueError, match="control_image= belongs to a ControlNet pipeline"):
            _bare_adapter(plain).generate_pns([1, 2], control_image=ctrl, image=img, output_type="latent")


# ---------------------------------------------------------------------------------------------------- the reference's own consistency
def test_reference_loop_without_a_controlnet_is_the_inpainting_oracle_loop():
    """controlnet_edit_reference.edit_loop(controlnet=None) is the loop tests/test_gpu_inpaint.py holds the plain pipelines to
    (_oracle_inpaint), and a ControlNet whose zero convs are zero changes nothing: what the new reference adds is the branch alone"""
    import copy
    import controlnet_edit_cases as cc
    import controlnet_edit_reference as cer
    from test_gpu_inpaint import _oracle_inpaint
    H = W = 128
    img, mask, ctrl = cc.image(H, W), cc.half_mask(H, W), cc.control_image(H, W)
    emb = cc.embeds(1)
    rz = copy.deepcopy(cc.ref_controlnet())
    with torch.no_grad():
        for conv in rz.zero_convs()[:-1]:                                              # (the hint tower's conv_out may stay: the residuals are zero)
            conv.weight.zero_(); conv.bias.zero_()
    for cin, kind, strength, steps in ((4, "ddim", 0.75, 4), (9, "euler", 0.5, 4), (4, "euler", 1.0, 2)):
        ou, ov = cc.oracle_unet(cin), cc.oracle_vae()
        want, z, m = _oracle_inpaint(ou, ov, kind, img, mask, strength, steps, 1, cc.gens(1, False), emb, guidance=cc.GUIDANCE)
        for net in (None, rz):
            sch = cer.Sched(kind, steps, cer.t_start_of(steps, strength))
            init = cer.prepare(ov, sch, img, 1, cc.gens(1, False), strength, mask=mask, nine=cin == 9)
            got = cer.edit_loop(ou, net, sch, init, emb, H, W, ctrl, guidance_scale=cc.GUIDANCE)
            assert torch.equal(init["z"], z) and torch.equal(init["m"], m)
            assert torch.equal(got, want), (cin, kind, strength, net is not None)


# ---------------------------------------------------------------------------------------------------- dry recording
def test_dry_recorded_step_of_a_nine_channel_unet_behind_the_branch():
    """the ControlNet reads the 4-channel latents; only the UNet's conv_in reads conv_in_extra; the launch list is the 4-channel one"""
    import dataclasses
    from imagharmony_amd import lib as L
    from imagharmony_amd.controlnet import control_state
    from imagharmony_amd.ctx import Ctx
    from imagharmony_amd.ip_adapter import install_ip_processors
    from imagharmony_amd.unet import UNet2DConditionModel
    from oracle.sdxl_unet import tiny_config
    from test_controlnet_host import _controlnet_meta, _product_cfg
    dtype = torch.bfloat16
    cfg4 = _product_cfg(tiny_config())
    cn = _controlnet_meta(cfg4)
    S, Hl, Wl = 2, 32, 36
    lists = {}
    for cin in (4, 9):
        with torch.device("meta"):
            u = UNet2DConditionModel(dataclasses.replace(cfg4, in_channels=cin))
        u = u.to_empty(device="cpu").to(dtype)
        install_ip_processors(u, num_tokens=4, device="cpu", dtype=dtype, init="empty")
        for with_cn in (False, True):
            ctx = Ctx("cpu", dtype, record=True, dry=True)
            B = 2 * S
            ehs, te, ids = torch.zeros(B, 81, cfg4.cross_attention_dim), torch.zeros(B, cfg4.pooled_dim), torch.zeros(B, 6)
            st = u.prepare_conditioning(ctx, ehs, te, ids)
            st.t_table, st.step, st.in_scale_tab = torch.zeros(4), torch.zeros(1, dtype=torch.int32), torch.ones(4)
            st.latents = torch.zeros(S, 4, Hl, Wl)
            if cin == 9:
                st.conv_in_extra = torch.zeros(S, 5, Hl, Wl)
            control = None
            if with_cn:
                cst = control_state(st, cn.prepare_conditioning(ctx, ehs, te, ids))
                assert getattr(cst, "conv_in_extra", None) is None and cst.latents is st.latents
            n0 = len(ctx.tags)
            if with_cn:
                control = cn.emit_forward(ctx, cst, S, Hl, Wl, hint=torch.zeros(1, Hl, Wl, cfg4.block_out_channels[0], dtype=dtype), tab=torch.zeros(4))
            u.emit_forward(ctx, st, S, Hl, Wl, cfg_dup=True, control=control)
            lists[(cin, with_cn)] = [(t[1], t[2], t[5]) for t in ctx.tags[n0:]]
            if with_cn:
                ops = {t[2]: o[1] for t, o in zip(ctx.tags[n0:], ctx._ops[n0:]) if t[2] in ("cn.conv_in", "conv_in")}
                assert not ops["cn.conv_in"].x2 and ops["cn.conv_in"].a == ops["conv_in"].a == st.latents.data_ptr()
                assert bool(ops["conv_in"].x2) == (cin == 9) and (not ops["conv_in"].x2 or ops["conv_in"].x2 == st.conv_in_extra.data_ptr())
                assert sum(k == L.OP_CONTROL_ADD for k, _, _ in lists[(cin, True)]) == 11
    assert lists[(9, True)] == lists[(4, True)] and lists[(9, False)] == lists[(4, False)]
    assert len(lists[(9, True)]) == len(lists[(9, False)]) + (len(lists[(4, True)]) - len(lists[(4, False)]))


# ---------------------------------------------------------------------------------------------------- header / ABI
def test_abi_13_header_and_symbol_list_are_unchanged():
    """the feature adds no kernel and no C symbol: the header's declarations (comments and layout aside) and the bound symbol list are
    what they were when ABI 13 was introduced"""
    from imagharmony_amd import lib as L
    hdr = open(os.path.join(ROOT, "include", "imh.h")).read()
    assert int(re.search(r"#define IMH_ABI_VERSION (\d+)", hdr).group(1)) == 13 == L.ABI_VERSION == L.load().imh_abi_version()
    names = [s[0] for s in L.SYMBOLS]
    assert len(names) == 40 and hashlib.sha1("\n".join(names).encode()).hexdigest() == "e116e35a79d4df2aae0ad48f44a0af4192c1a86c"
    code = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert hashlib.sha1(" ".join(code.split()).encode()).hexdigest() == "e6aa4af1b74e150873170422eca136a3e27f499b"
