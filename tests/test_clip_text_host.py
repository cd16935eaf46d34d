"""Host side of imagharmony_amd.clip_text.CLIPTextEncoder (no GPU): state-dict compatibility with transformers' CLIPTextModel /
CLIPTextModelWithProjection, the derived (packed) weights, from_pretrained over both key spellings, the EOS-row rule, the refusals,
the additive ABI pieces (causal encoder attention, quick-GELU flag, row gather) and SDXLPromptEncoder's backend switch."""
import ctypes
import os
import re

import pytest
import torch

CLIP_L = dict(hidden_size=768, intermediate_size=3072, num_attention_heads=12, projection_dim=768, hidden_act="quick_gelu")
BIGG = dict(hidden_size=1280, intermediate_size=5120, num_attention_heads=20, projection_dim=1280, hidden_act="gelu")
TINY = dict(vocab_size=100, hidden_size=128, intermediate_size=256, num_attention_heads=2, projection_dim=64, hidden_act="quick_gelu")


def _hf(proj, depth=2, seed=0, **kw):
    from transformers import CLIPTextConfig, CLIPTextModel, CLIPTextModelWithProjection
    torch.manual_seed(seed)
    cfg = CLIPTextConfig(**{**dict(vocab_size=1000, num_hidden_layers=depth, max_position_embeddings=77, bos_token_id=1, eos_token_id=2,
                                   pad_token_id=0), **kw})
    return (CLIPTextModelWithProjection if proj else CLIPTextModel)(cfg).eval()


def _preset(name, **kw):
    from imagharmony_amd.clip_text import CLIPTextEncoderConfig
    return (CLIPTextEncoderConfig.clip_l if name == "clip_l" else CLIPTextEncoderConfig.open_clip_bigg)(**kw)


@pytest.fixture(scope="module", params=[("clip_l", False), ("clip_l", True), ("bigg", False), ("bigg", True)],
                ids=["clip_l", "clip_l_proj", "bigg", "bigg_proj"])
def pair(request):
    from imagharmony_amd.clip_text import CLIPTextEncoder
    name, proj = request.param
    hf = _hf(proj, **(CLIP_L if name == "clip_l" else BIGG))
    enc = CLIPTextEncoder(_preset(name, num_hidden_layers=2, vocab_size=1000), with_projection=proj)
    return hf, enc, proj


def test_presets():
    l, g = _preset("clip_l"), _preset("bigg")
    assert (l.hidden_size, l.num_attention_heads, l.num_hidden_layers, l.intermediate_size, l.hidden_act) == (768, 12, 12, 3072, "quick_gelu")
    assert (g.hidden_size, g.num_attention_heads, g.num_hidden_layers, g.intermediate_size, g.hidden_act, g.projection_dim) == \
        (1280, 20, 32, 5120, "gelu", 1280)
    for c in (l, g):
        assert c.max_position_embeddings == 77 and c.vocab_size == 49408 and c.layer_norm_eps == 1e-5 and isinstance(c.eos_token_id, int)


def test_state_dict_keys_and_shapes_equal_transformers(pair):
    hf, enc, proj = pair
    a = {k: tuple(v.shape) for k, v in hf.state_dict().items()}
    b = {k: tuple(v.shape) for k, v in enc.state_dict().items()}
    assert a == b
    assert ("text_projection.weight" in b) == proj


def test_strict_load_round_trips(pair):
    hf, enc, _ = pair
    enc.load_state_dict(hf.state_dict(), strict=True)
    sd = enc.state_dict()
    for k, v in hf.state_dict().items():
        assert torch.equal(sd[k], v), k
    hf.load_state_dict(sd, strict=True)


def test_derived_weights_equal_their_sources_and_follow_a_reload(pair):
    hf, enc, proj = pair
    enc.load_state_dict(hf.state_dict(), strict=True)
    d = enc.derived()
    hid = enc.config.hidden_size
    layers = (hf.text_model if proj else hf).encoder.layers
    for i, ly in enumerate(layers):
        a = ly.self_attn
        assert d["wqkv"][i].shape == (3 * hid, hid) and d["bqkv"][i].shape == (3 * hid,)
        for j, lin in enumerate((a.q_proj, a.k_proj, a.v_proj)):
            assert torch.equal(d["wqkv"][i][j * hid:(j + 1) * hid], lin.weight)
            assert torch.equal(d["bqkv"][i][j * hid:(j + 1) * hid], lin.bias)
    assert enc.derived() is d                       # cached while nothing changed
    sd = {k: v + 1 for k, v in hf.state_dict().items()}
    enc.load_state_dict(sd, strict=True)            # loading rebuilds the caches
    d2 = enc.derived()
    pre = "text_model." if proj else ""
    assert d2 is not d and torch.equal(d2["wqkv"][0][:hid], sd[pre + "encoder.layers.0.self_attn.q_proj.weight"])
    assert torch.equal(d2["bqkv"][1][2 * hid:], sd[pre + "encoder.layers.1.self_attn.v_proj.bias"])


@pytest.mark.parametrize("position_ids", [False, True], ids=["", "stray_position_ids"])
@pytest.mark.parametrize("prefix", [True, False], ids=["text_model_prefix", "no_prefix"])
@pytest.mark.parametrize("proj", [False, True], ids=["CLIPTextModel", "CLIPTextModelWithProjection"])
@pytest.mark.parametrize("fmt", ["safetensors", "bin"])
def test_from_pretrained_reads_a_saved_directory(tmp_path, fmt, proj, prefix, position_ids):
    """both key spellings of both classes: transformers 4.x wrote ``text_model.`` everywhere (the published SDXL checkpoints), the
    installed version only under CLIPTextModelWithProjection; older checkpoints also persist the position_ids buffer"""
    from safetensors.torch import save_file
    from imagharmony_amd.clip_text import CLIPTextEncoder
    hf = _hf(proj, depth=1, seed=3, **TINY)
    hf.save_pretrained(tmp_path)                    # config.json (+ the weights in the installed spelling, replaced below)
    bare = {(k[len("text_model."):] if k.startswith("text_model.") else k): v.contiguous() for k, v in hf.state_dict().items()}
    sd = {(("text_model." + k) if prefix and not k.startswith("text_projection.") else k): v for k, v in bare.items()}
    if position_ids:
        sd[("text_model." if prefix else "") + "embeddings.position_ids"] = torch.arange(77).unsqueeze(0)
    os.remove(tmp_path / "model.safetensors")
    if fmt == "bin":
        torch.save(sd, tmp_path / "pytorch_model.bin")
    else:
        save_file(sd, str(tmp_path / "model.safetensors"))
    enc = CLIPTextEncoder.from_pretrained(str(tmp_path), device="cpu", dtype=torch.bfloat16)
    cfg = enc.config
    assert enc.with_projection == proj
    assert (cfg.vocab_size, cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers, cfg.num_attention_heads, cfg.max_position_embeddings,
            cfg.projection_dim, cfg.hidden_act, cfg.eos_token_id) == (100, 128, 256, 1, 2, 77, 64, "quick_gelu", 2)
    assert cfg.layer_norm_eps == hf.config.layer_norm_eps
    assert enc.dtype == torch.bfloat16 and next(enc.parameters()).dtype == torch.bfloat16
    got = enc.state_dict()
    assert set(got) == set(hf.state_dict())
    for k, v in hf.state_dict().items():
        assert torch.equal(got[k], v.to(torch.bfloat16)), k


def test_from_pretrained_without_projection_drops_a_checkpoints_projection(tmp_path):
    from imagharmony_amd.clip_text import CLIPTextEncoder
    hf = _hf(True, depth=1, seed=3, **TINY)
    hf.save_pretrained(tmp_path)
    enc = CLIPTextEncoder.from_pretrained(str(tmp_path), with_projection=False)
    assert not enc.with_projection and "text_projection.weight" not in enc.state_dict()
    assert torch.equal(enc.state_dict()["final_layer_norm.weight"], hf.state_dict()["text_model.final_layer_norm.weight"])


@pytest.mark.parametrize("proj", [False, True])
def test_from_hf_copies_config_and_weights(proj):
    from imagharmony_amd.clip_text import CLIPTextEncoder
    hf = _hf(proj, depth=1, seed=4, **{**TINY, "eos_token_id": 99})
    enc = CLIPTextEncoder.from_hf(hf)
    assert enc.with_projection == proj and enc.config.eos_token_id == 99 and enc.config.hidden_act == "quick_gelu"
    assert enc.config.projection_dim == 64 and enc.config.hidden_size == 128 and enc.config.vocab_size == 100
    for k, v in hf.state_dict().items():
        assert torch.equal(enc.state_dict()[k], v), k


def test_package_exports_the_class():
    import imagharmony_amd as pkg
    from imagharmony_amd.clip_text import CLIPTextEncoder, CLIPTextEncoderConfig
    assert pkg.CLIPTextEncoder is CLIPTextEncoder and pkg.CLIPTextEncoderConfig is CLIPTextEncoderConfig


# ---------------------------------------------------------------------------------------------- EOS rule
def _ids(eos, positions, L=77, vocab=49408, seed=0):
    """rows of ids with the token `eos` at the given positions (a list per row) and ordinary tokens below it elsewhere"""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, min(vocab, 40000), (len(positions), L), generator=g)
    for r, ps in enumerate(positions):
        for p in ps:
            ids[r, p] = eos
    return ids


@pytest.mark.parametrize("eos_cfg", [2, 49407])
def test_eos_rows_agree_with_transformers_pooler_output(eos_cfg):
    """the pooled row transformers picks (pooler_output == a row of last_hidden_state) is the row eos_positions names: EOS at
    positions 1, 10 and 76, and two EOS tokens in one row (the first one counts; the padding may be the EOS token)"""
    from imagharmony_amd.clip_text import eos_positions
    hf = _hf(False, depth=1, seed=5, **{**TINY, "vocab_size": 49408, "eos_token_id": eos_cfg})
    positions = [[1], [10], [76], [10, 40], [5, 6, 76]]
    ids = _ids(49407, positions)                    # the tokenizer's end-of-text id is 49407 under either config value
    with torch.no_grad():
        out = hf(ids)
    pos = eos_positions(ids, eos_cfg)
    assert pos.dtype == torch.int64 and pos.tolist() == [p[0] for p in positions]
    for r in range(len(positions)):
        assert torch.equal(out.pooler_output[r], out.last_hidden_state[r, pos[r]])
        others = [p for p in range(77) if p != int(pos[r])]
        assert not any(torch.equal(out.pooler_output[r], out.last_hidden_state[r, p]) for p in others)


def test_eos_rule_differs_between_the_two_config_values():
    from imagharmony_amd.clip_text import eos_positions
    ids = torch.tensor([[1, 7, 300, 9, 2, 0, 0], [1, 2, 2, 500, 4, 4, 4]])
    assert eos_positions(ids, 2).tolist() == [2, 3]         # argmax of the ids
    assert eos_positions(ids, 9).tolist() == [3, 0]         # first occurrence; none -> 0, as upstream's argmax over zeros
    assert eos_positions(ids.tolist(), 4).tolist() == [0, 4]


# ---------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("case", ["attention_mask", "position_ids", "output_attentions", "too_long", "hidden_act", "head_dim_not_8",
                                  "head_dim_over_128", "ids_negative", "ids_beyond_vocab"])
def test_refusals_raise_before_any_context_exists(case, monkeypatch):
    from imagharmony_amd import clip_text
    from imagharmony_amd.clip_text import CLIPTextEncoder, CLIPTextEncoderConfig

    def no_ctx(*a, **k):
        raise AssertionError("a Ctx was built before the refusal")
    monkeypatch.setattr(clip_text, "Ctx", no_ctx)
    kw = dict(TINY, num_hidden_layers=1)
    if case == "hidden_act":
        kw["hidden_act"] = "gelu_new"
    elif case == "head_dim_not_8":
        kw.update(hidden_size=192, num_attention_heads=16)          # head dim 12
    elif case == "head_dim_over_128":
        kw.update(hidden_size=256, num_attention_heads=1)
    enc = CLIPTextEncoder(CLIPTextEncoderConfig(**kw))
    ids = torch.randint(0, 100, (2, 77))
    call = {}
    if case == "attention_mask":
        call["attention_mask"] = torch.ones(2, 77, dtype=torch.long)
    elif case == "position_ids":
        call["position_ids"] = torch.arange(77).unsqueeze(0)
    elif case == "output_attentions":
        call["output_attentions"] = True
    elif case == "too_long":
        ids = torch.randint(0, 100, (2, 78))
    elif case == "ids_negative":
        ids[1, 3] = -1
    elif case == "ids_beyond_vocab":
        ids[0, 76] = 100
    with pytest.raises(ValueError if case.startswith("ids_") else NotImplementedError):
        enc(ids, **call)


def test_vision_tower_still_refuses_quick_gelu():
    from imagharmony_amd.clip_vision import CLIPVisionEncoder, CLIPVisionEncoderConfig
    enc = CLIPVisionEncoder(CLIPVisionEncoderConfig(num_hidden_layers=1, hidden_act="quick_gelu", hidden_size=64, intermediate_size=128,
                                                    num_attention_heads=4, projection_dim=32, image_size=28))
    with pytest.raises(NotImplementedError):
        enc(torch.zeros(1, 3, 28, 28))


def test_output_object_indexing():
    from imagharmony_amd.clip_text import CLIPTextEncoderOutput
    a, b, c, h = (torch.zeros(1) + i for i in range(4))
    o = CLIPTextEncoderOutput(last_hidden_state=a, pooler_output=b, hidden_states=(h, h))
    assert o[0] is a and o[1] is b and o[2] == (h, h) and o["pooler_output"] is b and o.text_embeds is None
    o = CLIPTextEncoderOutput(last_hidden_state=a, pooler_output=b, text_embeds=c)
    assert o[0] is c and o[1] is a and o.hidden_states is None and len(o.to_tuple()) == 2


# ---------------------------------------------------------------------------------------------- ABI
def _enum(hdr, name):
    """{enumerator: value} of ``enum name { ... }`` by C's rule: an explicit value, or the previous one plus one"""
    body = re.search(r"enum %s \{(.*?)\};" % name, hdr, re.S).group(1)
    vals, nxt = {}, 0
    for item in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(","):
        if item.strip():
            k, _, v = item.partition("=")
            nxt = int(v) if v.strip() else nxt
            vals[k.strip()] = nxt
            nxt += 1
    return vals


def test_abi_stays_13_and_the_additions_agree_between_header_and_binding():
    from imagharmony_amd import lib as L
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "imh.h")).read()
    assert L.ABI_VERSION == 13 and "#define IMH_ABI_VERSION 13" in hdr
    assert ctypes.sizeof(L.EncAttnArgs) == 72
    assert L.OP_ATTN_ENC_CAUSAL == 9 and re.search(r"IMH_OP_ATTN_ENC_CAUSAL = 9\b", hdr)
    assert L.GF_ACT_QGELU == 128 and re.search(r"IMH_GF_ACT_QGELU = 128\b", hdr)
    assert L.EW_GATHER_ROWS == 12 and _enum(hdr, "imh_ew_op")["IMH_EW_GATHER_ROWS"] == 12
    assert _enum(hdr, "imh_op_kind")["IMH_OP_ATTN_ENC_CAUSAL"] == 9 and _enum(hdr, "imh_gemm_flags")["IMH_GF_ACT_QGELU"] == 128
    assert re.search(r"int imh_attention_enc_causal\(const imh_enc_attn_args\* a, void\* stream\);", hdr)
    sym = [s for s in L.SYMBOLS if s[0] == "imh_attention_enc_causal"]
    assert len(sym) == 1 and sym[0][1] is ctypes.c_int and sym[0][2][0]._type_ is L.EncAttnArgs
    # the earlier values did not move
    assert (L.OP_GEMM, L.OP_ATTN_ENC, L.GF_GEGLU, L.GF_ACT_GELU, L.GF_ACT_SILU, L.GF_LN_COL, L.EW_TIMESTEP, L.EW_STEP_ROW) == (0, 8, 1, 2, 4, 64, 0, 11)


def test_causal_plan_accounting_is_half_the_bidirectional(monkeypatch):
    """a dry recording context (no GPU): the causal call records kind OP_ATTN_ENC_CAUSAL and half the FLOPs"""
    from imagharmony_amd import lib as L
    from imagharmony_amd.ctx import Ctx
    ctx = Ctx("cpu", torch.bfloat16, record=True, dry=True)
    qkv = torch.zeros(2 * 77, 3 * 128, dtype=torch.bfloat16)
    for causal in (False, True):
        ctx.attention_enc(qkv[:, :128], qkv[:, 128:256], qkv[:, 256:], 2, 2, 77, 64, causal=causal, out=torch.zeros(154, 128, dtype=torch.bfloat16))
    (_, k0, _, f0, *_), (_, k1, _, f1, *_) = ctx.tags
    assert (k0, k1) == (L.OP_ATTN_ENC, L.OP_ATTN_ENC_CAUSAL) and f1 == f0 / 2
    assert ctx.lib.imh_plan_get_kind(ctx.plan, 1) == 9


# ---------------------------------------------------------------------------------------------- SDXLPromptEncoder
def test_prompt_encoder_backend_validation():
    from imagharmony_amd.clip_text import CLIPTextEncoder
    from imagharmony_amd.text import SDXLPromptEncoder
    from test_text_encoder import _Tok
    e1, e2 = _hf(False, depth=1, **TINY), _hf(True, depth=1, seed=1, **TINY)
    with pytest.raises(ValueError):
        SDXLPromptEncoder(_Tok(), _Tok(), e1, e2, text_encoder_backend="triton")
    stock = SDXLPromptEncoder(_Tok(), _Tok(), e1, e2)
    assert stock.text_encoder_backend == "transformers" and stock.pairs[0][1] is e1 and stock.pairs[1][1] is e2
    hip = SDXLPromptEncoder(_Tok(), _Tok(), e1, e2, text_encoder_backend="hip")
    t1, t2 = hip.pairs[0][1], hip.pairs[1][1]
    assert isinstance(t1, CLIPTextEncoder) and isinstance(t2, CLIPTextEncoder) and not t1.with_projection and t2.with_projection
    assert torch.equal(t2.text_projection.weight, e2.text_projection.weight)
    own = SDXLPromptEncoder(_Tok(), _Tok(), t1, t2, text_encoder_backend="hip")     # instances pass through, under either backend
    assert own.pairs[0][1] is t1 and SDXLPromptEncoder(_Tok(), _Tok(), t1, t2).pairs[1][1] is t2
