"""Host side (no GPU) of the two shared pieces under everything that is recorded into a plan:

* imagharmony_amd.derived -- the one cache of packed / padded / folded / stacked weight copies.  Every accessor that goes through it is
  put through the same contract: the same object while nothing changes, a rebuild equal to a fresh build after an in-place change of
  each source on its own and for another target dtype, and no value handed across the keyed extras (pad_out, cpad, cin_pad).
* imagharmony_amd.clip_tower -- the encoder stack of both CLIP towers.  tests/golden/clip_tower_trace.json holds ``ctx.tags`` (tag, kind,
  descr, flops, bytes, shape, epilogue with ``cfg``) and the buffer aliasing of dry recordings of both towers, dumped at the commit before
  the towers were put on one stack; a dry recording through the shared path must equal it entry for entry.
"""
import copy
import ctypes as C
import importlib.util
import json
import os

import pytest
import torch

BF16, FP16 = torch.bfloat16, torch.float16


def _ctx(dtype=BF16):
    from imagharmony_amd.ctx import Ctx
    return Ctx("cpu", dtype, record=True, dry=True)


# ---------------------------------------------------------------------------------------------- the cache contract
def _randomise(mod, seed=0):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in mod.parameters():
            p.copy_(torch.randn(p.shape, generator=g))
    return mod


def _fresh(mod):
    """a deep copy that has never built a derived copy"""
    m = copy.deepcopy(mod)
    for sub in m.modules():
        for k in [k for k in vars(sub) if k.startswith("_imh_") or k == "_derived"]:
            delattr(sub, k)
    return m


def _tensors(v):
    if torch.is_tensor(v):
        return [v]
    if isinstance(v, dict):
        v = list(v.values())
    return [t for x in v for t in _tensors(x)] if isinstance(v, (list, tuple)) else [v]


def _equal(a, b):
    a, b = _tensors(a), _tensors(b)
    return len(a) == len(b) and all((torch.equal(x, y) and x.dtype == y.dtype) if torch.is_tensor(x) else x == y for x, y in zip(a, b))


def _contract(mods, get, sources, dtypes=True):
    """mods: the modules the accessor reads (deep-copied together for the fresh build); get(mods, dtype) -> the accessor's value;
    sources(mods) -> every tensor it is keyed by.  dtypes=False: the accessor has no target dtype (the fp32 copies)."""
    v = get(mods, BF16)
    assert get(mods, BF16) is v                                        # cached while nothing changes
    assert _equal(v, get(_fresh(mods), BF16))
    for i in range(len(sources(mods))):
        with torch.no_grad():
            sources(mods)[i].add_(0.75)                                # in place: the address stays, the version moves
        v1 = get(mods, BF16)
        assert v1 is not v, f"source {i}: not rebuilt"
        assert _equal(v1, get(_fresh(mods), BF16)), f"source {i}: the rebuilt copy is not what a fresh build gives"
        assert get(mods, BF16) is v1
        v = v1
    if dtypes:
        h = get(mods, FP16)
        assert h is not v and _equal(h, get(_fresh(mods), FP16)) and not _equal(h, v)
        assert any(torch.is_tensor(t) and t.dtype == FP16 for t in _tensors(h))
        b = get(mods, BF16)                                            # ... and back: never the other dtype's copy
        assert not _equal(b, h) and _equal(b, get(_fresh(mods), BF16))


def _params(*names):
    def sources(mods):
        out = []
        for n in names:
            t = mods
            for part in n.split("."):
                t = t[int(part)] if part.isdigit() else getattr(t, part)
            out.append(t)
        return out
    return sources


def _holder(**mods):
    return torch.nn.ModuleDict(mods)


def _folded_case(slot, groups):
    from imagharmony_amd.attention_processor import _folded
    from imagharmony_amd.unet import Attention, Norm
    srcs = [f"attn.{n}.weight" for g in groups for n in g] + ["norm.weight", "norm.bias"]
    return (lambda: _randomise(_holder(attn=Attention(64, 1), norm=Norm(64, 1e-5))),
            lambda m, dt: _folded(m["attn"], slot, groups, m["norm"], _ctx(dt)), _params(*srcs), True)


def _tiny_unet():
    from imagharmony_amd.unet import UNet2DConditionModel, UNetConfig
    cfg = UNetConfig(block_out_channels=(64, 64), layers_per_block=1, transformer_layers_per_block=(1, 1), attention_head_dim=(1, 1),
                     cross_attention_dim=64, addition_time_embed_dim=8, projection_class_embeddings_input_dim=16 + 6 * 8, sample_size=8)
    return UNet2DConditionModel(cfg)


def _temb_sources(u):
    return [t for r in u.resnets() for t in (r.time_emb_proj.weight, r.time_emb_proj.bias)]


def _text_tower():
    from imagharmony_amd.clip_text import CLIPTextEncoder
    return CLIPTextEncoder(vocab_size=50, hidden_size=64, intermediate_size=64, num_hidden_layers=2, num_attention_heads=1, projection_dim=32,
                           max_position_embeddings=8, with_projection=True)


def _vision_tower():
    from imagharmony_amd.clip_vision import CLIPVisionEncoder
    return CLIPVisionEncoder(hidden_size=64, intermediate_size=64, num_hidden_layers=2, num_attention_heads=1, projection_dim=32, image_size=28)


def _tower_value(enc, dtype):
    if enc.dtype != dtype:
        enc.to(dtype)                   # a tower's copies are in its own dtype: the other target dtype is a cast tower
    return enc.derived()


def _cases():
    from imagharmony_amd import vae as V
    from imagharmony_amd.attention_processor import _packed_qk
    from imagharmony_amd.tiny_vae import _Conv
    from imagharmony_amd.unet import GEGLU, Attention, Conv2d, Linear, Norm, UNetEncoderModel
    conv = lambda: _randomise(Conv2d(8, 16, 3))                                            # noqa: E731
    geglu = lambda: _randomise(_holder(ge=GEGLU(32, 64), norm=Norm(32, 1e-5)))             # noqa: E731
    f32 = lambda attr: ((lambda: _randomise(Norm(16, 1e-5))), lambda m, dt: V._f32_vec(m, attr), _params(attr), False)      # noqa: E731
    return {
        "Conv2d.packed": (conv, lambda m, dt: m.packed(_ctx(dt)), _params("weight"), True),
        "Conv2d.packed_padded": (conv, lambda m, dt: m.packed_padded(_ctx(dt)), _params("weight", "bias"), True),
        "Conv2d.packed_padded/pad_out=False": (conv, lambda m, dt: m.packed_padded(_ctx(dt), pad_out=False), _params("weight", "bias"), True),
        "Conv2d.packed_phase": (conv, lambda m, dt: m.packed_phase(_ctx(dt)), _params("weight"), True),
        "GEGLU.packed": (geglu, lambda m, dt: m["ge"].packed(_ctx(dt)), _params("ge.proj.weight", "ge.proj.bias"), True),
        "GEGLU.packed_ln": (geglu, lambda m, dt: m["ge"].packed_ln(_ctx(dt), m["norm"]),
                            _params("ge.proj.weight", "ge.proj.bias", "norm.weight", "norm.bias"), True),
        "_temb_stack": (lambda: _randomise(_tiny_unet()), lambda m, dt: UNetEncoderModel._temb_stack(m, _ctx(dt)), _temb_sources, True),
        "_packed_qk": (lambda: _randomise(Attention(64, 1)), lambda m, dt: _packed_qk(m, _ctx(dt)), _params("to_q.weight", "to_k.weight"), True),
        "folded/_imh_ln_qkv": _folded_case("_imh_ln_qkv", (("to_q", "to_k"), ("to_v",))),
        "folded/_imh_ln_qkv3": _folded_case("_imh_ln_qkv3", (("to_q", "to_k", "to_v"),)),
        "folded/_imh_ln_q": _folded_case("_imh_ln_q", (("to_q",),)),
        "vae._pad_1x1": (lambda: _randomise(Conv2d(8, 8, 1)), lambda m, dt: V._pad_1x1(m, 64, dt, torch.device("cpu")), _params("weight", "bias"), True),
        "vae._f32_w/conv": (conv, lambda m, dt: V._f32_w(m, 64), _params("weight"), False),
        "vae._f32_w/linear": (lambda: _randomise(Linear(8, 16)), lambda m, dt: V._f32_w(m), _params("weight"), False),
        "vae._f32_vec/weight": f32("weight"),
        "vae._f32_vec/bias": f32("bias"),
        "tiny_vae._Conv.packed": (lambda: _randomise(_Conv(8, 16)), lambda m, dt: m.packed(_ctx(dt)), _params("weight", "bias"), True),
        "tiny_vae._Conv.packed/no bias": (lambda: _randomise(_Conv(8, 16, bias=False)), lambda m, dt: m.packed(_ctx(dt)), _params("weight"), True),
        "CLIPTextEncoder.derived": (lambda: _randomise(_text_tower()).to(BF16), _tower_value, lambda m: list(m.parameters()), True),
        "CLIPVisionEncoder.derived": (lambda: _randomise(_vision_tower()).to(BF16), _tower_value, lambda m: list(m.parameters()), True),
    }


_NAMES = ["Conv2d.packed", "Conv2d.packed_padded", "Conv2d.packed_padded/pad_out=False", "Conv2d.packed_phase", "GEGLU.packed", "GEGLU.packed_ln",
          "_temb_stack", "_packed_qk", "folded/_imh_ln_qkv", "folded/_imh_ln_qkv3", "folded/_imh_ln_q", "vae._pad_1x1", "vae._f32_w/conv",
          "vae._f32_w/linear", "vae._f32_vec/weight", "vae._f32_vec/bias", "tiny_vae._Conv.packed", "tiny_vae._Conv.packed/no bias",
          "CLIPTextEncoder.derived", "CLIPVisionEncoder.derived"]


def test_every_accessor_is_listed():
    assert sorted(_cases()) == sorted(_NAMES)


@pytest.mark.parametrize("name", _NAMES)
def test_cache_contract(name):
    make, get, sources, dtypes = _cases()[name]
    _contract(make(), get, sources, dtypes=dtypes)


def test_keyed_extras_do_not_share_a_value():
    """pad_out, cpad and cin_pad are part of the key (or of the slot): alternating variants never see one another's copy"""
    from imagharmony_amd import vae as V
    from imagharmony_amd.unet import Conv2d
    ctx = _ctx()
    conv = _randomise(Conv2d(8, 16, 3))
    for _ in range(2):
        (w1, b1), (w0, b0) = conv.packed_padded(ctx, pad_out=True), conv.packed_padded(ctx, pad_out=False)
        assert w1.shape == (64, 9 * 64) and b1.shape == (64,) and w0.shape == (16, 9 * 64) and b0.shape == (16,)
        assert torch.equal(w1[:16], w0) and torch.equal(b1[:16], b0) and not w1[16:].any() and not b1[16:].any()
    one = _randomise(Conv2d(8, 8, 1))
    for _ in range(2):
        (wa, ba), (wb, bb) = V._pad_1x1(one, 64, BF16, torch.device("cpu")), V._pad_1x1(one, 128, BF16, torch.device("cpu"))
        assert wa.shape == (64, 64) and ba.shape == (64,) and wb.shape == (128, 128) and bb.shape == (128,)
        assert torch.equal(wb[:64, :64], wa) and torch.equal(wa[:8, :8], one.weight.view(8, 8).to(BF16))
    assert V._pad_1x1(one, 64, BF16, torch.device("cpu"))[0] is wa and V._pad_1x1(one, 128, BF16, torch.device("cpu"))[0] is wb      # a slot per cpad
    for _ in range(2):
        p, q = V._f32_w(conv, 64), V._f32_w(conv, 0)
        assert p.shape == (16, 9 * 64) and q.shape == (16, 9 * 8) and p.dtype == q.dtype == torch.float32
        assert torch.equal(p.view(16, 9, 64)[:, :, :8], q.view(16, 9, 8)) and not p.view(16, 9, 64)[:, :, 8:].any()


def test_a_missing_source_is_part_of_the_key():
    from imagharmony_amd.derived import derived, vkey
    t = torch.zeros(3)
    assert vkey(t, None) == ((t.data_ptr(), t._version), None) and vkey() == ()
    h, built = torch.nn.Module(), []
    get = lambda srcs, **kw: derived(h, "_imh_x", srcs, lambda: built.append(1) or len(built), **kw)      # noqa: E731
    assert get((t, None)) == 1 and get((t, None)) == 1
    assert get((t,)) == 2 and get((t, None)) == 3
    assert get((t, None), where=(BF16, "cpu")) == 4 and get((t, None), where=(FP16, "cpu")) == 5 and get((t, None), where=(FP16, "cuda:0")) == 6
    assert get((t, None), where=(FP16, "cuda:0"), extra=(64,)) == 7 and get((t, None), where=(FP16, "cuda:0"), extra=(64,)) == 7
    t.add_(1)
    assert get((t, None), where=(FP16, "cuda:0"), extra=(64,)) == 8
    assert get((t.clone(), None), where=(FP16, "cuda:0"), extra=(64,)) == 9                # another storage


@pytest.mark.parametrize("make", [_text_tower, _vision_tower], ids=["text", "vision"])
def test_a_tower_drops_its_plans_with_its_copies(make):
    enc = _randomise(make()).to(BF16)
    d = enc.derived()
    enc._plans[2] = "recorded with d"
    assert enc.derived() is d and enc._plans == {2: "recorded with d"}
    with torch.no_grad():
        next(iter(enc.parameters())).mul_(2.0)
    assert enc.derived() is not d and enc._plans == {}
    enc._plans[2] = "recorded again"
    enc.to(FP16)
    assert enc.derived()["wqkv"][0].dtype == FP16 and enc._plans == {}


# ---------------------------------------------------------------------------------------------- the towers' launch sequence
def _pointers(a):
    """every c_void_p field of an argument struct in _fields_ order (a nested struct's in place)"""
    out = []
    for name, typ in a._fields_:
        if typ is C.c_void_p:
            out.append(getattr(a, name))
        elif isinstance(typ, type) and issubclass(typ, C.Structure):
            out.extend(_pointers(getattr(a, name)))
    return out


def _describe(ctx):
    """ctx.tags as JSON gives them back, and per launch its pointer arguments, each address replaced by the index of its first appearance
    in the recording: which launch reads what which launch wrote, and which pool buffer is reused where (the free order)"""
    first, alias = {}, []
    for o in ctx._ops:
        structs = list(o[1]) if isinstance(o[1], C.Array) else [o[1]]
        alias.append([None if not p else first.setdefault(p, len(first)) for s in structs for p in _pointers(s)])
    return dict(tags=json.loads(json.dumps([list(t) for t in ctx.tags])), alias=alias, args=list(_forward_trace_tool().args_digest(ctx)))


def _forward_trace_tool():
    """tools/forward_trace.py, for its args_digest: the exact arguments of every recorded launch"""
    spec = importlib.util.spec_from_file_location("forward_trace", os.path.join(os.path.dirname(os.path.dirname(__file__)), "tools", "forward_trace.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TOWER = dict(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, projection_dim=64)


def _record_text(act, proj):
    from imagharmony_amd.clip_text import CLIPTextEncoder
    enc = CLIPTextEncoder(hidden_act=act, with_projection=proj, **TOWER).to(BF16)
    return enc._record(2, 77, ctx=_ctx())


def _record_vision(B):
    from imagharmony_amd.clip_vision import CLIPVisionEncoder
    enc = CLIPVisionEncoder(image_size=28, patch_size=14, **TOWER).to(BF16)
    return enc._record(B, ctx=_ctx())


_RECORDINGS = {f"text/{act}/{'proj' if proj else 'noproj'}/B2_L77": (lambda act=act, proj=proj: _record_text(act, proj))
               for act in ("quick_gelu", "gelu") for proj in (True, False)}
_RECORDINGS.update({f"vision/B{B}": (lambda B=B: _record_vision(B)) for B in (1, 3)})


@pytest.fixture(scope="module")
def tower_trace():
    with open(os.path.join(os.path.dirname(__file__), "golden", "clip_tower_trace.json")) as f:
        return json.load(f)


def test_the_fixture_holds_exactly_these_recordings(tower_trace):
    assert sorted(tower_trace) == sorted(_RECORDINGS)
    assert {k: len(v["tags"]) for k, v in tower_trace.items()} == {
        "text/quick_gelu/proj/B2_L77": 18, "text/quick_gelu/noproj/B2_L77": 17, "text/gelu/proj/B2_L77": 18, "text/gelu/noproj/B2_L77": 17,
        "vision/B1": 18, "vision/B3": 20}


@pytest.mark.parametrize("name", sorted(_RECORDINGS))
def test_towers_record_what_they_recorded_before_they_shared_a_stack(tower_trace, name):
    plan = _RECORDINGS[name]()
    ctx = plan["ctx"]
    assert ctx.dry and not ctx.captured
    got, want = _describe(ctx), tower_trace[name]
    assert len(got["tags"]) == len(want["tags"])
    for i, (g, w) in enumerate(zip(got["tags"], want["tags"])):
        assert g == w, f"launch {i}: {g} != {w}"
    for i, (g, w) in enumerate(zip(got["alias"], want["alias"])):
        assert g == w, f"launch {i} ({want['tags'][i][2]}): buffers {g} != {w}"
    assert got["args"] == want["args"], "the same launches over the same buffers, but a scalar argument, a byte offset or a prefetch differs"
    # the records still answer what the GPU tests and the timing tools read
    keys = ("ctx", "ids", "eos", "hidden", "last", "pooled", "embeds") if name.startswith("text") else ("ctx", "patches", "hidden", "embeds")
    assert all(k in plan for k in keys) and len(plan["hidden"]) == 3
    assert len({h.data_ptr() for h in plan["hidden"]}) == 3            # every layer's output stays live


def test_text_tower_imports_nothing_from_the_vision_tower():
    import imagharmony_amd.clip_text as T
    src = open(T.__file__).read()
    assert "clip_vision" not in src.split('"""', 2)[2]
