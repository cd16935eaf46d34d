"""Host-side (no GPU) tests of the SDXL T2I-Adapter: the model's key schema and parameter count, the strict state-dict round trip with
the CPU reference (tests/t2i_adapter_reference.py), the engine's gate table and plan key, the refusals (all raised before a Ctx
exists) and the header / library checks of the one new entry, imh_adapter_op."""
import ctypes as C
import hashlib
import os
import re

import pytest
import torch

import t2i_adapter_reference as tr
from test_multistep_host import _cpu_engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = (64, 128, 256, 256)


def _expected_keys(channels=(320, 640, 1280, 1280), n=2):
    keys = ["adapter.conv_in"]
    for i in range(4):
        if i in (1, 2):                       # the blocks whose in and out channels differ
            keys.append(f"adapter.body.{i}.in_conv")
        keys += [f"adapter.body.{i}.resnets.{j}.block{k}" for j in range(n) for k in (1, 2)]
    return {f"{k}.{p}" for k in keys for p in ("weight", "bias")}


def test_xl_config_key_schema_and_parameter_count():
    from imagharmony_amd import T2IAdapter
    with torch.device("meta"):
        m = T2IAdapter()
    sd = m.state_dict()
    assert set(sd) == _expected_keys()
    assert sum(v.numel() for v in sd.values()) == 79_028_160
    assert sd["adapter.conv_in.weight"].shape == (320, 3 * 16 * 16, 3, 3)
    assert sd["adapter.body.1.in_conv.weight"].shape == (640, 320, 1, 1) and sd["adapter.body.2.in_conv.weight"].shape == (1280, 640, 1, 1)
    assert sd["adapter.body.3.resnets.1.block1.weight"].shape == (1280, 1280, 3, 3)
    assert sd["adapter.body.3.resnets.1.block2.weight"].shape == (1280, 1280, 1, 1)
    assert [b.down for b in m.adapter.body] == [False, False, True, False] and m.total_downscale_factor == 32
    with torch.device("meta"):
        ref = tr.RefT2IAdapter()
    assert {k: tuple(v.shape) for k, v in ref.state_dict().items()} == {k: tuple(v.shape) for k, v in sd.items()}


def test_strict_round_trip_with_the_reference():
    from imagharmony_amd import T2IAdapter
    from oracle.detfill import det_fill
    ref = det_fill(tr.RefT2IAdapter(channels=TINY), 3)
    m = T2IAdapter(channels=TINY)
    m.load_state_dict(ref.state_dict(), strict=True)
    back = tr.RefT2IAdapter(channels=TINY)
    back.load_state_dict(m.state_dict(), strict=True)
    for k, v in ref.state_dict().items():
        assert torch.equal(back.state_dict()[k], v), k


def test_from_unet_and_init_random():
    from imagharmony_amd import T2IAdapter
    from imagharmony_amd.unet import UNet2DConditionModel, UNetConfig
    cfg = UNetConfig(block_out_channels=(64, 128, 256), transformer_layers_per_block=(1, 1, 1), attention_head_dim=(1, 2, 4), cross_attention_dim=64,
                     addition_time_embed_dim=8, projection_class_embeddings_input_dim=16 + 48)
    unet = UNet2DConditionModel(cfg).to(torch.bfloat16)
    a = T2IAdapter.from_unet(unet)
    assert a.channels == TINY and a.adapter.conv_in.weight.dtype == torch.bfloat16
    assert all(torch.isfinite(p.float()).all() for p in a.parameters())
    b = T2IAdapter(channels=TINY).init_random_(7)
    c = T2IAdapter(channels=TINY).init_random_(7)
    assert all(torch.equal(p, q) for p, q in zip(b.parameters(), c.parameters()))


def test_reference_unet_forward_without_features_is_the_plain_forward():
    """the checker's own walk: with intrablock=None it is the oracle UNet's forward; zero features change nothing; one non-zero
    feature at each point changes the prediction (every injection point is live)"""
    from oracle.detfill import det_fill, det_randn
    from oracle.sdxl_unet import UNet2DConditionModel as OracleUNet
    from oracle.sdxl_unet import tiny_config
    cfg = tiny_config()
    ou = det_fill(OracleUNet(cfg), 5).eval()
    x, ehs = det_randn((2, 4, 16, 16), 3), det_randn((2, 8, cfg.cross_attention_dim), 4)
    added = {"text_embeds": det_randn((2, cfg.pooled_dim), 6), "time_ids": torch.tensor([[128.0, 128, 0, 0, 128, 128]]).repeat(2, 1)}
    with torch.no_grad():
        plain = ou(x, torch.tensor(500.0), ehs, added_cond_kwargs=added)
        plain = plain[0] if isinstance(plain, (tuple, list)) else plain
        mine = tr.unet_forward(ou, x, torch.tensor(500.0), ehs, added)
        assert torch.equal(mine, plain)
        shapes = [(1, 64, 8, 8), (1, 128, 8, 8), (1, 256, 4, 4), (1, 256, 4, 4)]
        zeros = [torch.zeros(s) for s in shapes]
        assert torch.equal(tr.unet_forward(ou, x, torch.tensor(500.0), ehs, added, zeros), plain)
        for k in range(4):
            feats = [torch.zeros(s) for s in shapes]
            feats[k] = det_randn(shapes[k], 20 + k)
            assert not torch.allclose(tr.unet_forward(ou, x, torch.tensor(500.0), ehs, added, feats), plain, atol=1e-4), k


# ---------------------------------------------------------------------------------------------------- the gate table and the plan key
def test_gate_table_rows():
    from imagharmony_amd.denoise import DenoiseEngine
    g = DenoiseEngine.adapter_gate_table
    assert g(30, 0, 0.5) == [1.0] * 15 + [0.0] * 15
    assert g(30, 0, 1.0) == [1.0] * 30
    assert g(30, 0, 0.0) == [0.0] * 30
    assert g(7, 0, 0.5) == [1.0] * 3 + [0.0] * 4                       # int(3.5) = 3, as upstream's int(num_inference_steps * factor)
    # t_start the way gate_table has it: the m = n - t_start steps that run are counted from row t_start, the rows before hold the value
    assert g(10, 4, 0.5) == [1.0] * 4 + [1.0] * 3 + [0.0] * 3
    assert [bool(v) for v in g(10, 4, 1.0)] == [bool(v) for v in DenoiseEngine.gate_table(10, 4, 0.0, 1.0, 1.0)]


class _FakeAdapter:
    prepare_features = None

    def check_image(self, image, height=None, width=None):
        pass


def test_schedule_builds_the_table_and_keys_it():
    from imagharmony_amd import lib as L
    from imagharmony_amd import schedulers as hs
    e = _cpu_engine(S=1, H=8, W=8)
    sch = hs.DDIMScheduler()
    e.set_schedule(sch, 30)
    k_plain = e._sched_key
    assert e.ad_gate_tab is None and k_plain[11] is None and k_plain.adapter is None
    e.adapter = _FakeAdapter()
    with pytest.raises(L.ImhError, match="set_adapter_image"):
        e.set_schedule(sch, 30)
    e.ad = dict(image=torch.zeros(1, 3, 64, 64), scale=0.75, feats=[None] * 4)
    e.set_schedule(sch, 30, adapter_conditioning_factor=0.5)
    k_half = e._sched_key
    assert e.ad_gate_tab.tolist() == [1.0] * 15 + [0.0] * 15 and e.ad_gate_tab.dtype == torch.float32
    e.set_schedule(sch, 30)
    k_full = e._sched_key
    assert e.ad_gate_tab.tolist() == [1.0] * 30
    e.ad["scale"] = 0.5
    e.set_schedule(sch, 30)
    k_scale = e._sched_key
    assert len({k_plain, k_half, k_full, k_scale}) == 4                   # with / without, the factor and the scale are all in the key
    assert k_full[:11] == k_plain[:11] and k_full[12:] == k_plain[12:]    # ... and nothing else moved
    assert k_full == k_plain._replace(adapter=k_full.adapter) and k_full.adapter[1] == 0.75 and k_scale.adapter == (k_full.adapter[0], 0.5)
    # denoising_end cuts the list first: the factor counts the steps that run (upstream truncates num_inference_steps before its loop)
    e.set_schedule(sch, 30, denoising_end=0.5, adapter_conditioning_factor=0.5)
    n = e.steps
    assert 0 < n < 30 and e.ad_gate_tab.tolist() == [1.0] * int(n * 0.5) + [0.0] * (n - int(n * 0.5))
    for kw in (dict(t_start=3), dict(inpaint=True)):
        with pytest.raises(NotImplementedError, match="text-to-image"):
            e.set_schedule(sch, 30, **kw)


# ---------------------------------------------------------------------------------------------------- refusals, all before a Ctx exists
@pytest.fixture
def no_ctx(monkeypatch):
    from imagharmony_amd import ctx as ctx_mod

    def boom(*a, **k):
        raise AssertionError("a Ctx was created before the refusal")
    monkeypatch.setattr(ctx_mod.Ctx, "__init__", boom)


def test_model_refusals(no_ctx):
    from imagharmony_amd import T2IAdapter
    for kind in ("full_adapter", "light_adapter"):
        with pytest.raises(NotImplementedError, match=kind):
            T2IAdapter(adapter_type=kind)
    with pytest.raises(ValueError):
        T2IAdapter(adapter_type="something_else")
    m = T2IAdapter(channels=TINY)
    for shape in ((1, 3, 250, 256), (1, 3, 256, 48), (1, 3, 16, 16), (1, 4, 256, 256), (3, 256, 256)):
        with pytest.raises(ValueError):
            m.forward(torch.zeros(shape))
    with pytest.raises(ValueError, match="does not match"):
        m.prepare_features(None, torch.zeros(1, 3, 256, 256), 16, 16)     # the call is 128 x 128
    m.check_image(torch.zeros(2, 3, 64, 96), 64, 96)


def test_unet_forward_refusals(no_ctx):
    from imagharmony_amd.unet import UNet2DConditionModel, UNetConfig
    cfg = UNetConfig(block_out_channels=(64, 128, 256), transformer_layers_per_block=(1, 1, 1), attention_head_dim=(1, 2, 4), cross_attention_dim=64,
                     addition_time_embed_dim=8, projection_class_embeddings_input_dim=16 + 48)
    unet = UNet2DConditionModel(cfg)
    x, f = torch.zeros(1, 4, 32, 32), [torch.zeros(1, 64, 16, 16)] * 4
    added = {"text_embeds": torch.zeros(1, 16), "time_ids": torch.zeros(1, 6)}
    with pytest.raises(NotImplementedError, match="ControlNet"):
        unet.forward(x, 1.0, torch.zeros(1, 8, 64), added_cond_kwargs=added, down_intrablock_additional_residuals=f,
                     down_block_additional_residuals=[x], mid_block_additional_residual=x)
    for bad in (f[:3], f + f[:1], f[0]):
        with pytest.raises(NotImplementedError, match="four"):
            unet.forward(x, 1.0, torch.zeros(1, 8, 64), added_cond_kwargs=added, down_intrablock_additional_residuals=bad)
    from imagharmony_amd.t2i_adapter import AdapterResiduals
    with pytest.raises(NotImplementedError):
        AdapterResiduals(f[:2])
    with pytest.raises(NotImplementedError, match="ControlNet"):
        unet.emit_forward(None, None, 1, 32, 32, control=object(), adapter=AdapterResiduals(f))


def test_engine_and_pipeline_refusals(no_ctx):
    from imagharmony_amd import T2IAdapter
    from imagharmony_amd.denoise import DenoiseEngine
    from imagharmony_amd.pipeline import StableDiffusionXLAdapterCustomPipeline, _AdapterCall, check_adapter_args
    a = T2IAdapter(channels=TINY)

    class Multi:
        adapters = [a, a]

    class CN:
        controlnet_down_blocks, prepare_hint = (), None
    e = _cpu_engine()
    for bad in ([a, a], (a,), Multi()):
        with pytest.raises(NotImplementedError, match="MultiAdapter"):
            e.set_adapter(bad)
        with pytest.raises(NotImplementedError, match="MultiAdapter"):
            StableDiffusionXLAdapterCustomPipeline(None, bad)
    with pytest.raises(TypeError):
        e.set_adapter(object())
    e.controlnet = CN()
    with pytest.raises(NotImplementedError, match="ControlNet"):
        e.set_adapter(a)
    e.controlnet = None
    e.set_adapter(a)
    assert e.adapter is a
    with pytest.raises(NotImplementedError, match="T2I-Adapter"):
        e.set_controlnet(CN())
    with pytest.raises(NotImplementedError, match="cfg_role"):
        e.set_conditioning(None, None, None, None, 256, 256, cfg_role=1)
    e.set_adapter(None)
    e.cfg_role = 0
    with pytest.raises(NotImplementedError, match="cfg_role"):
        e.set_adapter(a)
    e.cfg_role = None
    e.set_adapter(a)
    with pytest.raises(ValueError, match="multiples of 32"):
        e.set_adapter_image(torch.zeros(1, 3, 250, 256))
    # the call's own checks
    with pytest.raises(ValueError, match="needs `image`"):
        check_adapter_args(None, 1.0, 1.0)
    with pytest.raises(NotImplementedError, match="MultiAdapter"):
        check_adapter_args(torch.zeros(1, 3, 64, 64), [1.0, 1.0], 1.0)
    with pytest.raises(ValueError, match="factor"):
        check_adapter_args(torch.zeros(1, 3, 64, 64), 1.0, 1.5)

    class P:
        adapter, default_sample_size, vae_scale_factor = a, 32, 8
    for image, h, w in ((torch.zeros(1, 3, 256, 256), 128, 128), (torch.zeros(1, 3, 200, 256), None, None)):
        c = _AdapterCall(dict(image=image, height=h, width=w))
        with pytest.raises(ValueError):
            c.begin(P())
    c = _AdapterCall(dict(image=torch.zeros(3, 64, 96), height=None, width=None))
    c.begin(P())
    assert (c.height, c.width) == (64, 96) and tuple(c.cond.shape) == (1, 3, 64, 96)
    c.adapter_conditioning_factor = 0.5
    with pytest.raises(ValueError, match="one image, or one per sample"):
        _AdapterCall(dict(image=torch.zeros(3, 3, 64, 96), height=None, width=None, cond=torch.zeros(3, 3, 64, 96))).schedule_kw(P(), 2)


def test_pil_image_is_scaled_not_normalised_nor_resized():
    import numpy as np
    from PIL import Image
    from imagharmony_amd.pipeline import prepare_adapter_image
    arr = (np.arange(64 * 96 * 3) % 256).astype(np.uint8).reshape(64, 96, 3)
    t = prepare_adapter_image(Image.fromarray(arr))
    assert tuple(t.shape) == (1, 3, 64, 96) and t.dtype == torch.float32
    assert torch.equal(t[0], torch.from_numpy(arr.astype(np.float32) / 255.0).permute(2, 0, 1))
    assert tuple(prepare_adapter_image([Image.fromarray(arr)] * 2).shape) == (2, 3, 64, 96)


# ---------------------------------------------------------------------------------------------------- header / ABI
def _struct_names(hdr, cname):
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), hdr, re.S).group(1), flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            parts = decl.replace("*", " ").split(",")
            names.append(parts[0].split()[-1])
            names.extend(p.strip() for p in parts[1:])
    return names


def test_header_declares_and_binds_adapter_op_and_nothing_else_moved():
    """the entry is declared in include/imh_adapter.h, a companion of include/imh.h: tests/test_controlnet_edit_host.py pins the
    declarations of imh.h and the list lib.SYMBOLS to their hashes, so the additive entry has a header and a binding list of its own
    and both pins hold as they are"""
    from imagharmony_amd import lib as L
    l = L.load()
    hdr = open(os.path.join(ROOT, "include", "imh.h")).read()
    ahdr = open(os.path.join(ROOT, "include", "imh_adapter.h")).read()
    assert int(re.search(r"#define IMH_ABI_VERSION (\d+)", hdr).group(1)) == 13 == L.ABI_VERSION == l.imh_abi_version()
    assert "IMH_ABI_VERSION" not in re.sub(r"/\*.*?\*/", "", ahdr, flags=re.S) and '#include "imh.h"' in ahdr
    assert re.search(r"\bint imh_adapter_op\(const imh_adapter_args\* a, void\* stream\);", ahdr)
    # the companion header declares that one function, the companion list binds it, and the loaded library exports it
    assert set(re.findall(r"\b(imh_[a-z0-9_]+)\s*\(", ahdr)) == {"imh_adapter_op"} == {n for n, _, _ in L.ADAPTER_SYMBOLS}
    assert hasattr(l, "imh_adapter_op") and l.imh_adapter_op.restype is C.c_int
    assert _struct_names(ahdr, "imh_adapter_args") == [f[0] for f in L.AdapterArgs._fields_]
    modes = {m: int(v) for m, v in re.findall(r"#define IMH_ADAPTER_([A-Z0-9]+) (\d+)\b", ahdr)}
    assert modes == {"UNSHUFFLE": L.ADAPTER_UNSHUFFLE, "RELU": L.ADAPTER_RELU, "AVGPOOL2": L.ADAPTER_AVGPOOL2}
    assert "Memory:" in ahdr[:ahdr.index("int imh_adapter_op(")]
    # the two enums, as they were (and not restated in the companion)
    assert "enum" not in re.sub(r"/\*.*?\*/", "", ahdr, flags=re.S)
    kinds = re.search(r"enum imh_op_kind \{(.*?)\};", hdr, re.S).group(1)
    assert " ".join(kinds.split()) == ("IMH_OP_GEMM = 0, IMH_OP_ATTN = 1, IMH_OP_GROUPNORM = 2, IMH_OP_LAYERNORM = 3, IMH_OP_EW = 4, IMH_OP_ATTN_SMALL = 5, "
                                       "IMH_OP_GEMM_DUAL = 6, IMH_OP_XATTN = 7, IMH_OP_ATTN_ENC = 8, IMH_OP_ATTN_ENC_CAUSAL = 9, IMH_OP_STEP_SEEDED = 10, "
                                       "IMH_OP_RANDN_SEEDED = 11")
    flags = re.sub(r"/\*.*?\*/", "", re.search(r"enum imh_gemm_flags \{(.*?)\};", hdr, re.S).group(1), flags=re.S)
    assert re.findall(r"(IMH_GF_[A-Z0-9_]+) = (\d+)", flags) == [("IMH_GF_GEGLU", "1"), ("IMH_GF_ACT_GELU", "2"), ("IMH_GF_ACT_SILU", "4"), ("IMH_GF_VT_PERM", "8"),
                                                              ("IMH_GF_OUT_F32", "16"), ("IMH_GF_LN_ROW", "32"), ("IMH_GF_LN_COL", "64"), ("IMH_GF_ACT_QGELU", "128")]
    # every declaration of imh.h and every name of SYMBOLS is what it was: the hashes tests/test_controlnet_edit_host.py pins
    code = " ".join(re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)).split())
    assert hashlib.sha1(code.encode()).hexdigest() == "e6aa4af1b74e150873170422eca136a3e27f499b"
    names = [s[0] for s in L.SYMBOLS]
    assert len(names) == 40 and hashlib.sha1("\n".join(names).encode()).hexdigest() == "e116e35a79d4df2aae0ad48f44a0af4192c1a86c"
    # the entry is no plan kind: 16 is refused like 12 and 14
    p = l.imh_plan_create()
    a = L.AdapterArgs()
    for kind in (12, 14, 16):
        assert l.imh_plan_add(p, kind, C.byref(a), 0, 0) < 0
    l.imh_plan_destroy(p)


def test_adapter_op_argument_errors_are_status_codes():
    """null pointers, misalignment, overlap, bad extents and dtypes: refused on the host, before anything could launch (no device here)"""
    from imagharmony_amd import lib as L
    l = L.load()
    buf = (C.c_char * 8192)()
    base = (C.addressof(buf) + 15) & ~15

    def call(**kw):
        a = L.AdapterArgs()
        a.x, a.y, a.mode, a.N, a.C, a.H, a.W, a.f, a.Cp, a.n, a.dtype = base, base + 4096, L.ADAPTER_UNSHUFFLE, 1, 1, 4, 4, 2, 8, 0, 0
        for k, v in kw.items():
            setattr(a, k, v)
        return l.imh_adapter_op(C.byref(a), None)
    assert l.imh_adapter_op(None, None) == -1
    assert call(x=None) == -1 and call(y=None) == -1 and b"null" in l.imh_last_error()
    assert call(mode=3) == -1 and call(mode=-1) == -1
    assert call(y=base + 4096 + 8) == -1 and call(x=base + 2) == -1                       # alignment
    assert call(mode=L.ADAPTER_RELU, n=64, x=base + 8) == -1                               # relu / avgpool2 read 16-byte groups
    assert call(dtype=2) == -3 and call(dtype=-1) == -3
    assert call(H=5) == -2 and call(W=6, f=4) == -2 and call(f=0) == -2                    # H % f, W % f
    assert call(Cp=4) == -2 and call(Cp=12) == -2 and call(C=3, Cp=8) == -2                # Cp % 8, Cp < C f^2
    assert call(N=0) == -2 and call(C=0) == -2 and call(H=0) == -2 and call(W=-4) == -2
    assert call(N=1 << 20, H=1 << 10, W=1 << 10) == -2                                     # 2^31 elements or more
    assert call(mode=L.ADAPTER_RELU, n=0) == -2 and call(mode=L.ADAPTER_RELU, n=1 << 31) == -2
    assert call(mode=L.ADAPTER_AVGPOOL2, C=12) == -2
    assert call(y=base + 16) == -1 and b"overlap" in l.imh_last_error()                     # y inside x
    assert call(mode=L.ADAPTER_RELU, n=64, y=base + 16) == -1                              # relu: a partial overlap
    assert call(mode=L.ADAPTER_AVGPOOL2, C=8, y=base) == -1                                # avgpool2 has no in-place form
