"""Host-side pins of the SDXL ControlNet (no GPU): the state-dict schema, the CPU reference's own consistency, the guidance-window gate
table, the dry-recorded launch list with and without the branch, and the ABI of imh_control_add."""
import math
import os
import re

import pytest
import torch

from oracle.detfill import det_fill, det_randn
from oracle.pipeline import install_ip_processors
from oracle.sdxl_unet import UNet2DConditionModel as OracleUNet
from oracle.sdxl_unet import sdxl_config, tiny_config

import controlnet_reference as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENCODER = ("conv_in", "time_embedding", "add_embedding", "down_blocks", "mid_block")


def _product_cfg(ocfg):
    from imagharmony_amd.unet import UNetConfig
    return UNetConfig(**{k: getattr(ocfg, k) for k in UNetConfig.__dataclass_fields__})


def _expected_controlnet_only(boc):
    """the names and shapes of section 1 of the issue, spelled out"""
    c0, c1, c2 = boc
    exp = {"controlnet_cond_embedding.conv_in": (16, 3, 3, 3), "controlnet_cond_embedding.conv_out": (c0, 256, 3, 3)}
    chain = [(16, 16), (32, 16), (32, 32), (96, 32), (96, 96), (256, 96)]
    for i, (co, ci) in enumerate(chain):
        exp[f"controlnet_cond_embedding.blocks.{i}"] = (co, ci, 3, 3)
    for i, c in enumerate([c0, c0, c0, c0, c1, c1, c1, c2, c2]):
        exp[f"controlnet_down_blocks.{i}"] = (c, c, 1, 1)
    exp["controlnet_mid_block"] = (c2, c2, 1, 1)
    out = {}
    for k, shp in exp.items():
        out[k + ".weight"] = shp
        out[k + ".bias"] = (shp[0],)
    return out


@pytest.mark.parametrize("name", ["tiny", "sdxl"])
def test_state_dict_schema(name):
    from imagharmony_amd.controlnet import ControlNetModel
    from imagharmony_amd.unet import UNet2DConditionModel
    cfg = _product_cfg(tiny_config() if name == "tiny" else sdxl_config())
    with torch.device("meta"):
        u, cn = UNet2DConditionModel(cfg), ControlNetModel(cfg)
    usd, csd = u.state_dict(), cn.state_dict()
    enc = [k for k in usd if k.split(".")[0] in ENCODER]
    assert len(enc) > 100
    for k in enc:
        assert k in csd and csd[k].shape == usd[k].shape, k
    only = {k: tuple(v.shape) for k, v in csd.items() if k.split(".")[0] not in ENCODER}
    assert only == _expected_controlnet_only(cfg.block_out_channels)
    # the reference restatement carries the same schema, so one state dict serves both sides of every parity test
    if name == "tiny":
        rsd = cr.RefControlNet(tiny_config()).state_dict()
        assert {k: tuple(v.shape) for k, v in rsd.items()} == {k: tuple(v.shape) for k, v in csd.items()}


def test_from_unet_copies_bit_for_bit_and_leaves_zero_convs_zero():
    from imagharmony_amd.controlnet import ControlNetModel
    from imagharmony_amd.unet import UNet2DConditionModel
    cfg = _product_cfg(tiny_config())
    u = UNet2DConditionModel(cfg)
    u.load_state_dict(det_fill(OracleUNet(tiny_config()), 5).state_dict(), strict=True)
    cn = ControlNetModel.from_unet(u)
    usd, csd = u.state_dict(), cn.state_dict()
    for k, v in usd.items():
        if k.split(".")[0] in ENCODER:
            assert torch.equal(csd[k], v), k
    zero = [k for k in csd if k.startswith(("controlnet_down_blocks", "controlnet_mid_block", "controlnet_cond_embedding.conv_out"))]
    assert len(zero) == 22 and all(not csd[k].any() for k in zero)
    assert all(torch.isfinite(v).all() for v in csd.values()) and csd["controlnet_cond_embedding.conv_in.weight"].abs().max() > 0


def test_refusals_on_the_host():
    from imagharmony_amd.controlnet import ControlNetModel
    from imagharmony_amd.pipeline import StableDiffusionXLControlNetCustomPipeline
    cfg = _product_cfg(tiny_config())
    with torch.device("meta"):
        for kw in (dict(global_pool_conditions=True), dict(class_embed_type="timestep"), dict(num_class_embeds=10)):
            with pytest.raises(NotImplementedError):
                ControlNetModel(cfg, **kw)
        cn = ControlNetModel(cfg)
    with pytest.raises(NotImplementedError, match="guess_mode"):
        cn.emit_forward(None, None, 1, 32, 32, guess_mode=True)

    class Multi:
        nets = [cn, cn]
    for many in (Multi(), [cn, cn]):
        with pytest.raises(NotImplementedError, match="MultiControlNetModel"):
            StableDiffusionXLControlNetCustomPipeline(None, many)


# ---------------------------------------------------------------------------------------------------- the reference's own consistency
@pytest.fixture(scope="module")
def ref_pair():
    ocfg = tiny_config()
    with torch.no_grad():
        ou = det_fill(OracleUNet(ocfg), 5).eval()
        install_ip_processors(ou, num_tokens=4, scale=0.8)
        rc = det_fill(cr.RefControlNet(ocfg), 11).eval()
        rc.set_attn_processor(cr.RefCNAttnProcessor(4))
    x = det_randn((2, 4, 16, 16), 3)
    ehs = det_randn((2, 81, ocfg.cross_attention_dim), 4)
    added = {"text_embeds": det_randn((2, ocfg.pooled_dim), 6), "time_ids": torch.tensor([[128., 128, 0, 0, 128, 128]]).repeat(2, 1)}
    img = det_randn((1, 3, 128, 128), 9).mul(0.25).add(0.5).clamp(0, 1)
    return ou, rc, x, ehs, added, img


def test_reference_with_zero_residuals_is_the_oracle_forward(ref_pair):
    ou, rc, x, ehs, added, img = ref_pair
    import copy
    rz = copy.deepcopy(rc)
    with torch.no_grad():
        for conv in rz.zero_convs():
            conv.weight.zero_(); conv.bias.zero_()
        down, mid = rz(x, torch.tensor(500.0), ehs, img, added_cond_kwargs=added)
        assert all(not d.any() for d in down) and not mid.any()
        a = cr.unet_forward(ou, x, torch.tensor(500.0), ehs, added, down, mid)
        b = ou(x, torch.tensor(500.0), ehs, added_cond_kwargs=added)[0]
        c = cr.unet_forward(ou, x, torch.tensor(500.0), ehs, added)
    assert torch.equal(a, b) and torch.equal(c, b)


def test_reference_residuals_scale_linearly(ref_pair):
    ou, rc, x, ehs, added, img = ref_pair
    with torch.no_grad():
        d1, m1 = rc(x, torch.tensor(500.0), ehs, img, conditioning_scale=1.0, added_cond_kwargs=added)
        d2, m2 = rc(x, torch.tensor(500.0), ehs, img, conditioning_scale=0.5, added_cond_kwargs=added)     # a power of two: exact
    assert len(d1) == 9 and [d.shape[1] for d in d1] == [64, 64, 64, 64, 128, 128, 128, 256, 256]
    assert all(d.abs().max() > 0 for d in d1) and m1.abs().max() > 0
    for a, b in zip(d1 + [m1], d2 + [m2]):
        assert torch.equal(a * 0.5, b)
    # and the control image is visible: another image gives other residuals
    with torch.no_grad():
        d3, _ = rc(x, torch.tensor(500.0), ehs, 1.0 - img, added_cond_kwargs=added)
    assert (d3[0] - d1[0]).abs().max() > 1e-3


# ---------------------------------------------------------------------------------------------------- the gate table
@pytest.mark.parametrize("window", [(0.0, 1.0), (0.0, 0.5), (0.25, 0.75), (1.0, 1.0)])
@pytest.mark.parametrize("steps,t_start", [(4, 0), (10, 0), (10, 3)])
def test_gate_table_is_the_literal_keep_rule(window, steps, t_start):
    from imagharmony_amd.denoise import DenoiseEngine
    start, end = window
    scale = 0.7
    tab = DenoiseEngine.gate_table(steps, t_start, start, end, scale)
    m = steps - t_start
    assert len(tab) == steps
    for i in range(m):
        k = 1.0 - float(i / m < start or (i + 1) / m > end)               # diffusers' controlnet_keep, literally
        assert tab[t_start + i] == scale * k, (i, tab)
        assert k == cr.keep(i, m, start, end)
    if window == (0.25, 0.75) and (steps, t_start) == (4, 0):
        assert tab == [0.0, scale, scale, 0.0]                             # the first and the last step are gated off


# ---------------------------------------------------------------------------------------------------- dry recordings
def _tiny_unet_meta(dtype=torch.bfloat16):
    from imagharmony_amd.ip_adapter import install_ip_processors as product_install
    from imagharmony_amd.unet import UNet2DConditionModel
    with torch.device("meta"):
        u = UNet2DConditionModel(_product_cfg(tiny_config()))
    u = u.to_empty(device="cpu").to(dtype)
    product_install(u, num_tokens=4, device="cpu", dtype=dtype, init="empty")
    return u


def _controlnet_meta(cfg, dtype=torch.bfloat16):
    from imagharmony_amd.attention_processor import CNAttnProcessor2_0
    from imagharmony_amd.controlnet import ControlNetModel
    with torch.device("meta"):
        cn = ControlNetModel(cfg)
    cn = cn.to_empty(device="cpu").to(dtype)
    cn.set_attn_processor(CNAttnProcessor2_0(num_tokens=4))              # ONE object on every layer, as IPAdapter.set_ip_adapter installs it
    return cn


def _record(u, cn, S, Hl, Wl, mode, dtype=torch.bfloat16):
    """mode: 'omitted' (emit_forward without the argument), 'none' (control=None), 'control' (the branch, then the UNet)"""
    from imagharmony_amd.controlnet import control_state
    from imagharmony_amd.ctx import Ctx
    B = 2 * S
    cd, pd = u.config.cross_attention_dim, u.config.pooled_dim
    ctx = Ctx("cpu", dtype, record=True, dry=True)
    ehs, te, ids = torch.zeros(B, 81, cd), torch.zeros(B, pd), torch.zeros(B, 6)
    st = u.prepare_conditioning(ctx, ehs, te, ids)
    st.t_table, st.step = torch.zeros(4), torch.zeros(1, dtype=torch.int32)
    st.latents = torch.zeros(S, 4, Hl, Wl)
    control = None
    if mode == "control":
        cst = control_state(st, cn.prepare_conditioning(ctx, ehs, te, ids))
    n0 = len(ctx.tags)
    if mode == "control":
        hint = torch.zeros(1, Hl, Wl, u.config.block_out_channels[0], dtype=dtype)
        control = cn.emit_forward(ctx, cst, S, Hl, Wl, hint=hint, tab=torch.zeros(4))
    if mode == "omitted":
        u.emit_forward(ctx, st, S, Hl, Wl, cfg_dup=True)
    else:
        u.emit_forward(ctx, st, S, Hl, Wl, cfg_dup=True, control=control)
    return ctx, n0


@pytest.fixture(scope="module")
def recordings():
    from forward_recordings import sdxl_unet_meta
    out = {}
    for name, u, hw in (("tiny", _tiny_unet_meta(), 32), ("sdxl", sdxl_unet_meta(), 128)):
        cn = _controlnet_meta(u.config)
        out[name] = {m: _record(u, cn, 1, hw, hw, m) for m in ("omitted", "none", "control")}
    return out


@pytest.mark.parametrize("name", ["tiny", "sdxl"])
def test_dry_recording_with_the_branch(recordings, name):
    from imagharmony_amd import lib as L
    from test_host_logic import _launcher_refusal
    ctx, n0 = recordings[name]["control"]
    tags, ops = ctx.tags[n0:], ctx._ops[n0:]
    # every GEMM / conv launch of the branch and of the UNet behind it gets a variant its launcher accepts
    n = 0
    for (tag, kind, descr, fl, by_, shape, epi) in tags:
        if kind == L.OP_GEMM and shape is not None:
            why = _launcher_refusal(shape, epi)
            assert why is None, f"{descr} {shape} {epi}: {why}"
            n += 1
    assert n > 100
    adds = [(t, o[1]) for t, o in zip(tags, ops) if t[1] == L.OP_CONTROL_ADD]
    assert len(adds) == 11
    assert [t[2] for t, _ in adds] == ["cn.hint_add"] + ["control.skip"] * 9 + ["control.mid"]
    for t, a in adds:
        B, HW, C_, Br = t[5]
        # imh_control_add's own refusals, restated (api.hip do_control_add / norm.hip control_add_launch)
        assert a.x and a.r and a.y and a.partial and a.y not in (a.x, a.r)
        assert B == 2 and B % Br == 0 and C_ % 8 == 0 and C_ <= 4096 and a.sub >= 1 and C_ % a.sub == 0 and HW > 0
        assert a.sub == math.gcd(C_ // 32, 10)
        assert (t[2] == "cn.hint_add") == (not a.tab) and bool(a.tab) == bool(a.step)
        assert Br == (1 if t[2] == "cn.hint_add" else 2)
    # no statistics pass over a tensor an add wrote: its partials came with it.  (Pool buffers are reused, so "the tensor at x" is what
    # the most recent earlier launch wrote there.)
    def out_ptr(kind, a):
        if kind == L.OP_GEMM:
            return a.Y
        if kind in (L.OP_ATTN, L.OP_XATTN):
            return a.O
        if kind == L.OP_GEMM_DUAL:
            return a[0].Y
        return getattr(a, "y", None)
    last_writer, over_add = {}, []
    for t, o in zip(tags, ops):
        kind, a = o[0], o[1]                 # (the op list's kind: a two-problem launch is tagged as a GEMM)
        if kind == L.OP_GROUPNORM and a.mode == L.GN_STATS:
            if last_writer.get(a.x) == L.OP_CONTROL_ADD:
                over_add.append(t)
            continue
        p = out_ptr(kind, a)
        if p:
            last_writer[p] = kind
        if kind == L.OP_GEMM_DUAL:
            last_writer[a[1].Y] = kind
    assert not over_add
    # ... and every add's partials are read by some GroupNorm consumer (table-building launch) of the up path / the branch's first block
    used = set()
    for t, o in zip(tags, ops):
        a = o[1]
        if o[0] == L.OP_GEMM:
            used.update((a.gn_part, a.gn_part2))
        elif o[0] == L.OP_GROUPNORM:
            used.update((a.partial, a.partial2))
    assert all(a.partial in used for _, a in adds)
    # the plan kinds the library knows
    kinds = {ctx.lib.imh_plan_get_kind(ctx.plan, i) for i in range(ctx.lib.imh_plan_size(ctx.plan))}
    assert L.OP_CONTROL_ADD in kinds


@pytest.mark.parametrize("name", ["tiny", "sdxl"])
def test_dry_recording_without_control_is_unchanged(recordings, name):
    from imagharmony_amd import lib as L
    (a, na), (b, nb) = recordings[name]["omitted"], recordings[name]["none"]
    strip = lambda tags: [(t[0], t[1], t[2], t[5], t[6]) for t in tags]
    assert strip(a.tags[na:]) == strip(b.tags[nb:]) and len(a.tags) - na > 300
    assert not [t for t in a.tags if t[1] == L.OP_CONTROL_ADD]
    # with the branch, the UNet's own launches are the same list plus the ten injections: nothing else moves
    c, nc = recordings[name]["control"]
    unet_part = [t for t in c.tags[nc:] if not t[2].startswith("cn.") and t[0] < 80]
    rest = [t for t in unet_part if t[1] != L.OP_CONTROL_ADD]
    base = [t for t in a.tags[na:]]
    # the statistics passes over the skips no epilogue covers disappear (the injections supply the partials); everything else stays
    drop = lambda tags: [(t[1], t[2], t[5]) for t in tags if t[2] != "gn_stats"]
    assert drop(rest) == drop(base)
    assert sum(t[2] == "gn_stats" for t in rest) <= sum(t[2] == "gn_stats" for t in base)


# ---------------------------------------------------------------------------------------------------- header / ABI
def test_header_declares_and_binds_control_add():
    from imagharmony_amd import lib as L
    l = L.load()
    hdr = open(os.path.join(ROOT, "include", "imh.h")).read()
    assert re.search(r"\bint imh_control_add\(const imh_control_add_args\* a, void\* stream\);", hdr)
    assert any(s[0] == "imh_control_add" for s in L.SYMBOLS) and hasattr(l, "imh_control_add")
    assert int(re.search(r"#define IMH_ABI_VERSION (\d+)", hdr).group(1)) == 13 == L.ABI_VERSION == l.imh_abi_version()
    assert int(re.search(r"#define IMH_OP_CONTROL_ADD (\d+)\b", hdr).group(1)) == 15 == L.OP_CONTROL_ADD     # the next number after 13 that nothing pins as refused
    body = re.search(r"enum imh_op_kind \{(.*?)\};", hdr, re.S).group(1)
    assert "CONTROL_ADD" not in body and len(re.findall(r"IMH_OP_[A-Z_]+ = \d+", body)) == 12
    before = hdr[:hdr.index("int imh_control_add(")]
    assert "Memory:" in before[-2500:]
    # the argument struct and its ctypes mirror, field for field
    sbody = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct imh_control_add_args \{(.*?)\} imh_control_add_args;", hdr, re.S).group(1), flags=re.S)
    names = []
    for decl in sbody.split(";"):
        decl = decl.strip()
        if decl:
            parts = decl.replace("*", " ").split(",")
            names.append(parts[0].split()[-1])
            names.extend(p.strip() for p in parts[1:])
    assert names == [f[0] for f in L.ControlAddArgs._fields_]
    # kinds 12 and 14 stay refused (tests/test_clip_preprocess_host.py pins both), kind 15 is accepted by the plan
    p = l.imh_plan_create()
    a = L.ControlAddArgs()
    import ctypes as C
    assert l.imh_plan_add(p, 12, C.byref(a), 0, 0) < 0 and l.imh_plan_add(p, 14, C.byref(a), 0, 0) < 0
    assert l.imh_plan_add(p, L.OP_CONTROL_ADD, C.byref(a), 0, 0) == 0
    l.imh_plan_destroy(p)
    # argument errors are status codes, not launches: null pointers, and the in-place form
    assert l.imh_control_add(C.byref(a), None) == -1
    buf = (C.c_char * 4096)()
    base = (C.addressof(buf) + 15) & ~15
    a.x, a.r, a.y, a.B, a.Br, a.HW, a.C = base, base + 2048, base, 1, 1, 4, 8
    assert l.imh_control_add(C.byref(a), None) == -1 and b"in-place" in l.imh_last_error()
