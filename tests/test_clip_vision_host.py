"""Host side of imagharmony_amd.clip_vision.CLIPVisionEncoder (no GPU): state-dict compatibility with transformers'
CLIPVisionModelWithProjection, the derived (packed / padded) weights, from_pretrained, and the refusals."""
import pytest
import torch

VIT_H = dict(hidden_size=1280, intermediate_size=5120, num_attention_heads=16, projection_dim=1024)
VIT_BIGG = dict(hidden_size=1664, intermediate_size=8192, num_attention_heads=16, projection_dim=1280)
TINY = dict(hidden_size=64, intermediate_size=128, num_attention_heads=4, projection_dim=32, image_size=28)


def _hf(depth=2, hidden_act="gelu", seed=0, **kw):
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    torch.manual_seed(seed)
    return CLIPVisionModelWithProjection(CLIPVisionConfig(num_hidden_layers=depth, patch_size=14, hidden_act=hidden_act,
                                                          **{"image_size": 224, **kw})).eval()


@pytest.fixture(scope="module", params=[VIT_H, VIT_BIGG], ids=["vit_h", "vit_bigg"])
def pair(request):
    from imagharmony_amd.clip_vision import CLIPVisionEncoder, CLIPVisionEncoderConfig
    hf = _hf(**request.param)
    enc = CLIPVisionEncoder(CLIPVisionEncoderConfig(num_hidden_layers=2, **request.param))
    return hf, enc


def test_state_dict_keys_and_shapes_equal_transformers(pair):
    hf, enc = pair
    a = {k: tuple(v.shape) for k, v in hf.state_dict().items()}
    b = {k: tuple(v.shape) for k, v in enc.state_dict().items()}
    assert a == b
    assert "vision_model.pre_layrnorm.weight" in b


def test_strict_load_round_trips(pair):
    hf, enc = pair
    enc.load_state_dict(hf.state_dict(), strict=True)
    sd = enc.state_dict()
    for k, v in hf.state_dict().items():
        assert torch.equal(sd[k], v), k
    hf.load_state_dict(sd, strict=True)


def test_derived_weights_equal_their_sources_and_follow_a_reload(pair):
    hf, enc = pair
    enc.load_state_dict(hf.state_dict(), strict=True)
    d = enc.derived()
    hid = enc.config.hidden_size
    for i, ly in enumerate(hf.vision_model.encoder.layers):
        a = ly.self_attn
        assert d["wqkv"][i].shape == (3 * hid, hid) and d["bqkv"][i].shape == (3 * hid,)
        for j, lin in enumerate((a.q_proj, a.k_proj, a.v_proj)):
            assert torch.equal(d["wqkv"][i][j * hid:(j + 1) * hid], lin.weight)
            assert torch.equal(d["bqkv"][i][j * hid:(j + 1) * hid], lin.bias)
    pw = hf.vision_model.embeddings.patch_embedding.weight
    assert d["patch_k"] == 588 and d["patch_w"].shape == (hid, 640)
    assert torch.equal(d["patch_w"][:, :588], pw.reshape(hid, 588)) and not d["patch_w"][:, 588:].any()
    assert torch.equal(d["cls_pos"], hf.vision_model.embeddings.class_embedding + hf.vision_model.embeddings.position_embedding.weight[0])
    assert enc.derived() is d                       # cached while nothing changed
    sd = {k: v + 1 for k, v in hf.state_dict().items()}
    enc.load_state_dict(sd, strict=True)            # loading rebuilds the caches
    d2 = enc.derived()
    assert d2 is not d and torch.equal(d2["wqkv"][0][:hid], sd["vision_model.encoder.layers.0.self_attn.q_proj.weight"])
    assert torch.equal(d2["patch_w"][:, :588], sd["vision_model.embeddings.patch_embedding.weight"].reshape(hid, 588))


@pytest.mark.parametrize("fmt", ["safetensors", "bin"])
def test_from_pretrained_reads_a_saved_directory(tmp_path, fmt):
    import os
    from imagharmony_amd.clip_vision import CLIPVisionEncoder
    hf = _hf(depth=1, seed=3, **TINY)
    hf.save_pretrained(tmp_path)
    if fmt == "bin":
        os.remove(tmp_path / "model.safetensors")
        torch.save(hf.state_dict(), tmp_path / "pytorch_model.bin")
    enc = CLIPVisionEncoder.from_pretrained(str(tmp_path), device="cpu", dtype=torch.bfloat16)
    cfg = enc.config
    assert (cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers, cfg.num_attention_heads, cfg.image_size, cfg.patch_size,
            cfg.projection_dim, cfg.hidden_act) == (64, 128, 1, 4, 28, 14, 32, "gelu")
    assert cfg.layer_norm_eps == hf.config.layer_norm_eps
    assert enc.dtype == torch.bfloat16 and next(enc.parameters()).dtype == torch.bfloat16
    for k, v in hf.state_dict().items():
        assert torch.equal(enc.state_dict()[k], v.to(torch.bfloat16)), k


def test_from_hf_copies_config_and_weights():
    from imagharmony_amd.clip_vision import CLIPVisionEncoder
    hf = _hf(depth=1, seed=4, **TINY)
    enc = CLIPVisionEncoder.from_hf(hf)
    assert enc.config.projection_dim == 32 and enc.config.hidden_size == 64 and enc.config.image_size == 28
    for k, v in hf.state_dict().items():
        assert torch.equal(enc.state_dict()[k], v), k


def test_package_exports_the_class():
    import imagharmony_amd as pkg
    from imagharmony_amd.clip_vision import CLIPVisionEncoder
    assert pkg.CLIPVisionEncoder is CLIPVisionEncoder


@pytest.mark.parametrize("case", ["quick_gelu", "interpolate_pos_encoding", "output_attentions", "image_size"])
def test_refusals_raise_before_any_context_exists(case, monkeypatch):
    """every refusal is a NotImplementedError raised before a Ctx is built (on a machine without a GPU a Ctx would raise ImhError)"""
    from imagharmony_amd import clip_vision
    from imagharmony_amd.clip_vision import CLIPVisionEncoder, CLIPVisionEncoderConfig

    def no_ctx(*a, **k):
        raise AssertionError("a Ctx was built before the refusal")
    monkeypatch.setattr(clip_vision, "Ctx", no_ctx)
    enc = CLIPVisionEncoder(CLIPVisionEncoderConfig(num_hidden_layers=1, hidden_act="quick_gelu" if case == "quick_gelu" else "gelu", **TINY))
    px = torch.zeros(1, 3, 28, 28)
    kw = {}
    if case == "image_size":
        px = torch.zeros(1, 3, 42, 42)
    elif case != "quick_gelu":
        kw[case] = True
    with pytest.raises(NotImplementedError):
        enc(px, **kw)


def test_abi_13_and_the_encoder_attention_struct():
    import ctypes
    import os
    import re
    from imagharmony_amd import lib as L
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "imh.h")).read()
    assert L.ABI_VERSION == 13 and "#define IMH_ABI_VERSION 13" in hdr
    assert L.OP_ATTN_ENC == 8 and re.search(r"IMH_OP_ATTN_ENC = 8\b", hdr)
    body = re.search(r"typedef struct imh_enc_attn_args \{(.*?)\} imh_enc_attn_args;", hdr, re.S).group(1)
    names = []
    for decl in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";"):
        parts = decl.replace("*", " ").split(",")
        if decl.strip():
            names += [parts[0].split()[-1]] + [x.strip() for x in parts[1:]]
    fields = [f[0] for f in L.EncAttnArgs._fields_]
    assert names == fields
    assert ctypes.sizeof(L.EncAttnArgs) == 4 * 8 + 10 * 4
    assert any(s[0] == "imh_attention_enc" for s in L.SYMBOLS)
