"""Host-side (no GPU) tests of AutoencoderTiny: the model's key schema and parameter count, the strict state-dict round trip with the CPU
restatement (tests/tiny_vae_reference.py), the refusals (all raised before a Ctx exists), the opt-in wiring of preview_vae= and the
header / library checks of the one new entry, imh_tinyvae_conv."""
import ctypes as C
import hashlib
import os
import re
import types

import pytest
import torch

import tiny_vae_reference as tvr
from test_t2i_adapter_host import _struct_names

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def no_ctx(monkeypatch):
    """a refusal "before any GPU work" is one that is raised before a Ctx exists"""
    from imagharmony_amd import ctx as ctx_mod

    def boom(self, *a, **kw):
        raise AssertionError("a Ctx was built: the refusal came too late")
    monkeypatch.setattr(ctx_mod.Ctx, "__init__", boom)


def _expected_keys():
    keys = {"decoder.layers.0.weight", "decoder.layers.0.bias", "decoder.layers.18.weight", "decoder.layers.18.bias"}
    keys |= {f"decoder.layers.{i}.weight" for i in (6, 11, 16)}                  # the convs behind the upsamplers: no bias
    for i in (2, 3, 4, 7, 8, 9, 12, 13, 14, 17):
        keys |= {f"decoder.layers.{i}.conv.{j}.{p}" for j in (0, 2, 4) for p in ("weight", "bias")}
    return keys


def test_key_schema_and_parameter_count():
    from imagharmony_amd import AutoencoderTiny
    m = AutoencoderTiny()
    sd = m.state_dict()
    assert set(sd) == _expected_keys()
    assert sum(v.numel() for v in sd.values()) == tvr.N_PARAMS == 1_222_531
    assert sd["decoder.layers.0.weight"].shape == (64, 4, 3, 3) and sd["decoder.layers.18.weight"].shape == (3, 64, 3, 3)
    for i in (6, 11, 16):
        assert sd[f"decoder.layers.{i}.weight"].shape == (64, 64, 3, 3) and m.decoder.layers[i].bias is None
    for i in (5, 10, 15):
        assert isinstance(m.decoder.layers[i], torch.nn.Upsample)
    ref = tvr.RefAutoencoderTiny()
    assert {k: tuple(v.shape) for k, v in ref.state_dict().items()} == {k: tuple(v.shape) for k, v in sd.items()}
    c = m.config
    assert (c.scaling_factor, c.latent_channels, c.num_blocks, c.act_fn) == (1.0, 4, (3, 3, 3, 1), "relu")


def test_strict_round_trip_with_the_reference_and_encoder_keys_ignored():
    from imagharmony_amd import AutoencoderTiny
    ref = tvr.reference()
    m = AutoencoderTiny()
    m.load_state_dict(ref.state_dict(), strict=True)
    back = tvr.RefAutoencoderTiny()
    back.load_state_dict(m.state_dict(), strict=True)
    for k, v in ref.state_dict().items():
        assert torch.equal(back.state_dict()[k], v), k
    # a full diffusers checkpoint also carries the encoder: accepted and ignored, strictly
    sd = dict(ref.state_dict())
    sd["encoder.layers.0.weight"], sd["encoder.layers.0.bias"] = torch.zeros(64, 3, 3, 3), torch.zeros(64)
    m2 = AutoencoderTiny()
    m2.load_state_dict(sd, strict=True)
    assert all(torch.equal(m2.state_dict()[k], v) for k, v in ref.state_dict().items()) and not any(k.startswith("encoder") for k in m2.state_dict())
    with pytest.raises(RuntimeError):
        m2.load_state_dict({k: v for k, v in sd.items() if k != "decoder.layers.6.weight"}, strict=True)
    # init_random_ is seeded and fills everything; dtype follows the parameters
    a, b = AutoencoderTiny().init_random_(3), AutoencoderTiny().init_random_(3)
    assert all(torch.equal(p, q) and p.abs().sum() > 0 for p, q in zip(a.parameters(), b.parameters()))
    assert a.to(torch.float16).dtype == torch.float16


def test_reference_is_not_degenerate():
    """a dead random network must not pass for parity: on the shared inputs the image has spread and the last block's ReLU is neither
    always off nor always on"""
    for h, w in ((5, 7), (16, 16)):
        z, img = tvr.decoded(2, h, w)
        assert img.shape == (2, 3, 8 * h, 8 * w) and torch.isfinite(img).all()
        assert float(img.std()) > 0.5
        with torch.no_grad():
            act = tvr.reference().decoder(z, upto=17)
        share = float((act > 0).float().mean())
        assert act.shape == (2, 64, 8 * h, 8 * w) and 0.2 <= share <= 0.8, share


def test_model_refusals(no_ctx):
    from imagharmony_amd import AutoencoderTiny, TinyVAEConfig
    m = AutoencoderTiny()
    with pytest.raises(NotImplementedError, match="encoder"):
        m.encode(torch.zeros(1, 3, 64, 64))
    with pytest.raises(ValueError, match="fp32"):
        m.decode(torch.zeros(1, 4, 8, 8), precision="fp32")
    with pytest.raises(ValueError):
        m.decode(torch.zeros(1, 4, 8, 8), precision="bf16")
    with pytest.raises(ValueError):
        m.decode(torch.zeros(1, 3, 8, 8))
    for precision in (None, "auto", "native"):
        assert m.precision_for(precision) == "native"
    for bad in (dict(decoder_block_out_channels=(32, 32, 32, 32)), dict(decoder_block_out_channels=(64, 64, 64, 128)),
                dict(num_decoder_blocks=(3, 3, 3, 3)), dict(num_decoder_blocks=(1, 1, 1)), dict(act_fn="swish"), dict(latent_channels=16)):
        with pytest.raises(NotImplementedError):
            AutoencoderTiny(TinyVAEConfig(**bad))
    with pytest.raises(NotImplementedError):
        m.enable_tiling()


def test_edit_pipelines_refuse_a_tiny_vae(no_ctx):
    """image-to-image and inpainting encode the image: the tiny encoder's NotImplementedError, before any GPU work"""
    from imagharmony_amd import AutoencoderTiny
    from imagharmony_amd import schedulers as hs
    from imagharmony_amd.ip_adapter import IPAdapterXL
    from imagharmony_amd.pipeline import StableDiffusionXLImg2ImgCustomPipeline, StableDiffusionXLInpaintCustomPipeline, _EditCall
    tiny = AutoencoderTiny()

    class P:
        vae, default_sample_size, vae_scale_factor = tiny, 4, 8
    ns = dict(latents=None, image=torch.zeros(1, 3, 32, 32), mask_image=torch.ones(1, 1, 32, 32), strength=0.5, height=None, width=None)
    for edit in ("image-to-image", "inpainting"):
        with pytest.raises(NotImplementedError, match="tiny encoder"):
            _EditCall(ns, edit).begin(P())
    for cls in (StableDiffusionXLImg2ImgCustomPipeline, StableDiffusionXLInpaintCustomPipeline):
        ip = IPAdapterXL.__new__(IPAdapterXL)
        pipe = cls.__new__(cls)
        pipe.vae, pipe.vae_decode, pipe.scheduler = tiny, None, hs.DDIMScheduler()
        ip.pipe = pipe
        with pytest.raises(NotImplementedError, match="tiny encoder"):
            ip._pns_edit_inputs(torch.zeros(1, 3, 32, 32), torch.ones(1, 1, 32, 32) if "Inpaint" in cls.__name__ else None, 0.5, 2, 4,
                                "latent", "global")


def test_preview_vae_is_opt_in(monkeypatch):
    """preview_vae=None hands _default_scorer the pipe's own VAE, as before; preview_vae=tiny hands it the tiny one -- and only the judge
    sees it: the final image still goes through pipe.vae"""
    from test_clip_preprocess_host import _bare_adapter
    from imagharmony_amd import AutoencoderTiny, pns
    from imagharmony_amd import pipeline as pl
    from imagharmony_amd.ip_adapter import IPAdapterXL as IPAdapter
    import inspect
    assert inspect.signature(IPAdapter._default_scorer).parameters.keys() == {"self", "vae", "fused", "judge_preprocess"}
    ip, eng = _bare_adapter()
    tiny, kl = AutoencoderTiny(), object()
    ip.pipe.vae = kl
    seen, decoded = [], []
    monkeypatch.setattr(type(ip), "_default_scorer", lambda self, vae, fused, jp: (seen.append((vae, jp)), pns.default_scorer)[1])
    monkeypatch.setattr(pl, "decode_output", lambda vae, vd, lat, ot, **kw: (decoded.append(vae), lat)[1])
    kw = dict(clip_image_embeds=torch.randn(1, 8), prompt_embeds=(torch.randn(1, 3, 6), torch.randn(1, 3, 6), torch.randn(1, 5), torch.randn(1, 5)),
              preview_steps=2, num_inference_steps=3, output_type="pt")
    torch.manual_seed(0)
    a = ip.generate_pns([3, 9, 27], **kw)
    b = ip.generate_pns([3, 9, 27], preview_vae=None, **kw)
    c = ip.generate_pns([3, 9, 27], preview_vae=tiny, **kw)
    assert [s[0] for s in seen] == [kl, kl, tiny] and decoded == [kl, kl, kl]
    assert torch.equal(a["scores"], b["scores"]) and torch.equal(a["latents"], b["latents"]) and torch.equal(a["latents"], c["latents"])
    # a caller's scorer never sees the preview VAE
    n = len(seen)
    ip.generate_pns([3, 9], preview_vae=tiny, scorer=pns.default_scorer, **kw)
    assert len(seen) == n
    # the real _default_scorer on a tiny VAE builds the CLIP judge over tiny.decode
    monkeypatch.undo()
    ip.image_encoder = types.SimpleNamespace()
    j = IPAdapter._default_scorer(ip, tiny, torch.zeros(1, 8), "torch")
    assert isinstance(j, pns.ClipPreferenceJudge)
    assert IPAdapter._default_scorer(ip, None, torch.zeros(1, 8), "torch") is pns.default_scorer


# ---------------------------------------------------------------------------------------------------- header / ABI
def test_header_declares_and_binds_tinyvae_conv_and_nothing_else_moved():
    from imagharmony_amd import lib as L
    l = L.load()
    hdr = open(os.path.join(ROOT, "include", "imh.h")).read()
    thdr = open(os.path.join(ROOT, "include", "imh_tinyvae.h")).read()
    assert int(re.search(r"#define IMH_ABI_VERSION (\d+)", hdr).group(1)) == 13 == L.ABI_VERSION == l.imh_abi_version()
    code = re.sub(r"/\*.*?\*/", "", thdr, flags=re.S)
    assert "IMH_ABI_VERSION" not in code and '#include "imh.h"' in thdr and "enum" not in code
    assert re.search(r"\bint imh_tinyvae_conv\(const imh_tinyvae_args\* a, void\* stream\);", thdr)
    assert set(re.findall(r"\b(imh_[a-z0-9_]+)\s*\(", code)) == {"imh_tinyvae_conv"} == {n for n, _, _ in L.TINYVAE_SYMBOLS}
    assert hasattr(l, "imh_tinyvae_conv") and l.imh_tinyvae_conv.restype is C.c_int
    assert _struct_names(thdr, "imh_tinyvae_args") == [f[0] for f in L.TinyVaeArgs._fields_]
    flags = {m: int(v) for m, v in re.findall(r"#define IMH_TINYVAE_([A-Z0-9]+) (\d+)\b", thdr)}
    assert flags == {"RELU": L.TINYVAE_RELU, "UP2": L.TINYVAE_UP2, "HEAD": L.TINYVAE_HEAD, "TAIL": L.TINYVAE_TAIL}
    assert "Memory:" in thdr[:thdr.index("int imh_tinyvae_conv(")]
    # every declaration of imh.h and every name of SYMBOLS is what it was: the hashes tests/test_controlnet_edit_host.py pins
    code = " ".join(re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)).split())
    assert hashlib.sha1(code.encode()).hexdigest() == "e6aa4af1b74e150873170422eca136a3e27f499b"
    names = [s[0] for s in L.SYMBOLS]
    assert len(names) == 40 and hashlib.sha1("\n".join(names).encode()).hexdigest() == "e116e35a79d4df2aae0ad48f44a0af4192c1a86c"
    # the entry is no plan kind
    p = l.imh_plan_create()
    a = L.TinyVaeArgs()
    for kind in (12, 14, 16, 18):
        assert l.imh_plan_add(p, kind, C.byref(a), 0, 0) < 0
    l.imh_plan_destroy(p)


def test_tinyvae_conv_argument_errors_are_status_codes():
    """null pointers, misalignment, flag combinations, overlap, bad extents and dtypes: refused on the host, before anything could launch
    (no device here)"""
    from imagharmony_amd import lib as L
    l = L.load()
    buf = (C.c_char * (1 << 16))()
    base = (C.addressof(buf) + 15) & ~15
    X, W_, BIAS, RES, Y = base, base + 8192, base + 8192 + 4096, base + 16384, base + 32768

    def call(**kw):
        a = L.TinyVaeArgs()
        a.x, a.w, a.bias, a.residual, a.y, a.B, a.H, a.W, a.flags, a.dtype = X, W_, BIAS, None, Y, 1, 4, 4, L.TINYVAE_RELU, 0
        for k, v in kw.items():
            setattr(a, k, v)
        return l.imh_tinyvae_conv(C.byref(a), None)
    assert l.imh_tinyvae_conv(None, None) == -1
    assert call(x=None) == -1 and call(w=None) == -1 and call(y=None) == -1 and b"null" in l.imh_last_error()
    for k in ("x", "w", "bias", "y"):
        assert call(**{k: {"x": X, "w": W_, "bias": BIAS, "y": Y}[k] + 8}) == -1, k                # 16-byte alignment
    assert call(residual=RES + 2) == -1
    assert call(flags=16) == -1 and call(flags=-1) == -1 and b"flag" in l.imh_last_error()
    H_, T_, U_, R_ = L.TINYVAE_HEAD, L.TINYVAE_TAIL, L.TINYVAE_UP2, L.TINYVAE_RELU
    assert call(flags=H_ | T_) == -1 and call(flags=H_ | U_) == -1 and call(flags=T_ | U_) == -1
    assert call(flags=H_, residual=RES) == -1 and call(flags=T_, residual=RES) == -1 and call(flags=T_ | R_) == -1
    assert call(flags=H_, x=X + 2) == -1 and call(flags=T_, y=Y + 2) == -1                          # fp32 operands: 4 bytes
    assert call(dtype=2) == -3 and call(dtype=-1) == -3
    assert call(B=0) == -2 and call(H=0) == -2 and call(W=-4) == -2
    assert call(B=1 << 10, H=1 << 10, W=1 << 10) == -2 and b"2^31" in l.imh_last_error()            # 2^36 elements
    assert call(B=1, H=1 << 12, W=1 << 12, flags=U_) == -2                                         # x has 2^30, y 2^32
    assert call(B=1, H=1 << 14, W=1 << 13, flags=T_) == -2                                         # x has 2^33
    assert call(y=X) == -1 and b"overlap" in l.imh_last_error()                                    # in place
    assert call(y=X + 2048 - 16) == -1                                                             # y begins inside x ([1, 4, 4, 64] of 2 bytes)
    assert call(residual=Y) == -1 and call(residual=Y + 16) == -1                                   # y == residual is not allowed
    assert call(flags=U_, residual=RES, y=RES + 4096) == -1                                        # residual has the OUTPUT's extent
