"""imh_attention_enc and imagharmony_amd.clip_vision.CLIPVisionEncoder on the GPU, against fp32 CPU references:
torch's scaled_dot_product_attention for the kernel, transformers' CLIPVisionModelWithProjection (seeded random weights)
for the module.  Bounds: the per-module ones of SURVEY.md 8(c), rel-RMS <= 1.5e-2 (bf16) / 2e-3 (fp16) -- about 2.5x the
transformers module's own dtype noise against its fp32 self at depth 2 (bf16 6.1e-3 / 4.8e-3, fp16 7.6e-4 / 6.0e-4 for
image_embeds / hidden_states[-2]).  At full depth the error compounds, so there the bound is measured in the test: 3x the
rel-RMS the transformers module in the run dtype shows against its own fp32 (different accumulation order and exp / erf
approximations; the same ratio the processor tests carry over the reference's bf16 noise)."""
import copy
import ctypes as C
import json
import os

import pytest
import torch

from conftest import ROOT, record_parity, rel_rms

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BOUND = {torch.bfloat16: 1.5e-2, torch.float16: 2e-3}
DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
VIT_H = dict(hidden_size=1280, intermediate_size=5120, num_attention_heads=16, projection_dim=1024)
VIT_BIGG = dict(hidden_size=1664, intermediate_size=8192, num_attention_heads=16, projection_dim=1280)
SHAPES = [(16, 80, 257, 2), (16, 104, 257, 1), (16, 80, 577, 1), (20, 64, 77, 2), (4, 80, 50, 1), (2, 128, 1, 1)]


# ---------------------------------------------------------------------------------------------- kernel
_QKV = {}


def _qkv(shape, dtype):
    """inputs rounded to the run dtype (CPU) and their fp32 SDPA reference, computed once per (shape, dtype)"""
    key = (shape, dtype)
    if key not in _QKV:
        H, d, L_, B = shape
        g = torch.Generator().manual_seed(1000 * d + L_ + H)
        qkv = (torch.randn(B * L_, 3 * H * d, generator=g) * 1.5).to(dtype)
        q, k, v = (t.float().view(B, L_, H, d).transpose(1, 2) for t in qkv.split(H * d, dim=1))
        ref = torch.nn.functional.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B * L_, H * d)
        _QKV[key] = (qkv, ref)
    return _QKV[key]


@pytest.mark.parametrize("packed", [False, True], ids=["three_tensors", "packed"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "H%d_d%d_L%d_B%d" % s)
def test_attention_enc_matches_fp32_sdpa(shape, dtype, packed):
    from imagharmony_amd.ctx import Ctx
    H, d, L_, B = shape
    qkv, ref = _qkv(shape, dtype)
    ctx = Ctx(DEV, dtype)
    dq = qkv.to(DEV)
    if packed:
        q, k, v = dq[:, :H * d], dq[:, H * d:2 * H * d], dq[:, 2 * H * d:]
    else:
        q, k, v = (t.contiguous() for t in dq.split(H * d, dim=1))
    o = ctx.attention_enc(q, k, v, B, H, L_, d)
    torch.cuda.synchronize()
    r = rel_rms(o.float().cpu(), ref)
    print(f"attention_enc {shape} {dtype} packed={packed}: rel-rms {r:.3e}")
    assert o.shape == (B * L_, H * d) and torch.isfinite(o.float()).all()
    assert r <= BOUND[dtype], f"rel-rms {r:.3e}"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [(16, 80, 257, 2), (16, 104, 257, 1), (4, 80, 50, 1), (2, 128, 1, 1)], ids=lambda s: "H%d_d%d_L%d_B%d" % s)
def test_attention_enc_reads_and_writes_only_its_rows(shape, dtype):
    """operands as views into larger NaN-filled tensors: a masked-but-loaded row beyond the last key / query tile would put NaN into
    the result (NaN * 0 = NaN); the rows of O around [0, B*L) must keep their NaN"""
    from imagharmony_amd.ctx import Ctx
    H, d, L_, B = shape
    qkv, _ = _qkv(shape, dtype)
    ctx = Ctx(DEV, dtype)
    dq = qkv.to(DEV)
    plain = ctx.attention_enc(dq[:, :H * d], dq[:, H * d:2 * H * d], dq[:, 2 * H * d:], B, H, L_, d).clone()
    pad, M = 72, B * L_                      # more than one key tile of rows on either side
    big = torch.full((M + 2 * pad, 3 * H * d), float("nan"), dtype=dtype, device=DEV)
    big[pad:pad + M] = dq
    obig = torch.full((M + 2 * pad, H * d), float("nan"), dtype=dtype, device=DEV)
    w = big[pad:pad + M]
    ctx.attention_enc(w[:, :H * d], w[:, H * d:2 * H * d], w[:, 2 * H * d:], B, H, L_, d, out=obig[pad:pad + M])
    torch.cuda.synchronize()
    assert torch.isfinite(obig[pad:pad + M].float()).all()
    assert torch.equal(obig[pad:pad + M], plain)
    assert torch.isnan(obig[:pad]).all() and torch.isnan(obig[pad + M:]).all()


def test_attention_enc_error_codes():
    from imagharmony_amd import lib as L
    lib = L.load()
    t = torch.zeros(64, 3 * 2 * 136, dtype=torch.bfloat16, device=DEV)
    o = torch.zeros(64, 2 * 136, dtype=torch.bfloat16, device=DEV)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(d, q=t.data_ptr()):
        a = L.EncAttnArgs()
        a.Q, a.K, a.V, a.O = q, t.data_ptr(), t.data_ptr(), o.data_ptr()
        a.B, a.H, a.L, a.d = 1, 2, 64, d
        a.ldq = a.ldk = a.ldv = t.stride(0)
        a.ldo, a.scale, a.dtype = o.stride(0), 0.1, L.IMH_DT_BF16
        return lib.imh_attention_enc(C.byref(a), s)
    assert call(80) == 0
    assert call(12) == -2 and b"multiple of 8" in lib.imh_last_error()         # IMH_ERR_SHAPE
    assert call(136) == -2                                                       # d > 128
    assert call(80, q=None) == -1 and b"null" in lib.imh_last_error()           # IMH_ERR_ARG
    torch.cuda.synchronize()


def test_attention_enc_records_and_replays_in_a_plan():
    from imagharmony_amd import lib as L
    from imagharmony_amd.ctx import Ctx
    shape, dtype = (4, 80, 50, 1), torch.bfloat16
    H, d, L_, B = shape
    qkv, ref = _qkv(shape, dtype)
    dq = qkv.to(DEV)
    rec = Ctx(DEV, dtype, record=True)
    o = rec.attention_enc(dq[:, :H * d], dq[:, H * d:2 * H * d], dq[:, 2 * H * d:], B, H, L_, d)
    assert rec.lib.imh_plan_get_kind(rec.plan, 0) == L.OP_ATTN_ENC
    rec.capture()
    o.zero_()
    rec.replay()
    torch.cuda.synchronize()
    assert rel_rms(o.float().cpu(), ref) <= BOUND[dtype]


# ---------------------------------------------------------------------------------------------- module
def _hf(depth, seed=0, **kw):
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    torch.manual_seed(seed)
    return CLIPVisionModelWithProjection(CLIPVisionConfig(num_hidden_layers=depth, patch_size=14, image_size=224, hidden_act="gelu", **kw)).eval()


def _pixels(B, seed=5):
    return torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(seed))


_D2 = {}


def _depth2(name):
    """(transformers module fp32 on the CPU, pixel batch, its fp32 outputs per dtype-rounded input), built once per width"""
    if name not in _D2:
        hf = _hf(2, **(VIT_H if name == "vit_h" else VIT_BIGG))
        _D2[name] = dict(hf=hf, px=_pixels(2 if name == "vit_h" else 1), ref={})
    return _D2[name]


def _ref(e, dtype):
    if dtype not in e["ref"]:
        with torch.no_grad():
            e["ref"][dtype] = e["hf"](e["px"].to(dtype).float(), output_hidden_states=True)
    return e["ref"][dtype]


def _enc(hf, dtype):
    from imagharmony_amd.clip_vision import CLIPVisionEncoder
    return CLIPVisionEncoder.from_hf(hf).to(DEV, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ["vit_h", "vit_bigg"])
def test_module_depth2_full_width_matches_transformers_fp32(name, dtype):
    e = _depth2(name)
    ref = _ref(e, dtype)
    enc = _enc(e["hf"], dtype)
    out = enc(e["px"].to(DEV, dtype), output_hidden_states=True)
    assert len(out.hidden_states) == 3 and out.image_embeds.shape == ref.image_embeds.shape
    assert torch.equal(out.last_hidden_state, out.hidden_states[-1])
    pairs = dict(image_embeds=(out.image_embeds, ref.image_embeds), last_hidden_state=(out.last_hidden_state, ref.last_hidden_state),
                 hidden_m2=(out.hidden_states[-2], ref.hidden_states[-2]), hidden_0=(out.hidden_states[0], ref.hidden_states[0]))
    res = {k: rel_rms(a.float().cpu(), b) for k, (a, b) in pairs.items()}
    print(f"clip_vision depth 2 {name} {dtype}: {res}")
    for k, r in res.items():
        record_parity(f"clip_vision.depth2.{name}.{IDS[DTYPES.index(dtype)]}.{k}", r, BOUND[dtype])
    for k, r in res.items():
        assert r <= BOUND[dtype], f"{k}: rel-rms {r:.3e}"


_FULL = {}


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_module_full_depth_vit_h_within_3x_of_the_references_own_dtype_noise(dtype):
    if not _FULL:
        hf = _hf(32, seed=1, **VIT_H)
        px = _pixels(1, seed=6)
        _FULL.update(hf=hf, px=px)
    hf, px = _FULL["hf"], _FULL["px"]
    pxd = px.to(dtype)
    with torch.no_grad():
        r32 = hf(pxd.float(), output_hidden_states=True)
        enc = _enc(hf, dtype)
        lo = copy.deepcopy(hf).to(dtype)
        rlo = lo(pxd, output_hidden_states=True)
        del lo
    out = enc(pxd.to(DEV), output_hidden_states=True)
    res = {}
    for k, get in (("image_embeds", lambda o: o.image_embeds), ("hidden_m2", lambda o: o.hidden_states[-2])):
        noise = rel_rms(get(rlo).float(), get(r32))
        ours = rel_rms(get(out).float().cpu(), get(r32))
        res[k] = dict(reference_dtype_noise=noise, hip=ours, bound=3 * noise)
    print(f"clip_vision full depth vit_h {dtype}: {res}")
    path = os.path.join(ROOT, "profiles", "clip_vision_parity.json")
    try:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        try:
            with open(path) as f:
                rec = json.load(f)
        except (OSError, ValueError):
            rec = {}
        rec[IDS[DTYPES.index(dtype)]] = res
        with open(path, "w") as f:
            json.dump(rec, f, indent=1, sort_keys=True)
    except OSError:
        pass
    for k, v in res.items():
        assert v["hip"] <= v["bound"], f"{k}: {v}"


def test_module_behaviour_replay_batches_and_hidden_state_switch():
    dtype = torch.bfloat16
    e = _depth2("vit_h")
    enc = _enc(e["hf"], dtype)
    px8 = _pixels(8, seed=7).to(DEV, dtype)
    a = enc(px8[:2])
    plan = enc._plans[2]
    b = enc(px8[:2], output_hidden_states=True)
    assert enc._plans[2] is plan and plan["ctx"].captured                   # the second call replayed the recorded plan
    assert torch.equal(a.image_embeds, b.image_embeds) and torch.equal(a.last_hidden_state, b.last_hidden_state)
    assert a.hidden_states is None and len(b.hidden_states) == 3
    o8 = enc(px8)
    assert sorted(enc._plans) == [2, 8]
    for i in (0, 3, 7):
        o1 = enc(px8[i:i + 1])
        assert rel_rms(o8.image_embeds[i].float(), o1.image_embeds[0].float()) <= BOUND[dtype]
        assert rel_rms(o8.last_hidden_state[i].float(), o1.last_hidden_state[0].float()) <= BOUND[dtype]
    assert sorted(enc._plans) == [1, 2, 8]
    assert torch.equal(enc(px8[:2]).image_embeds, a.image_embeds)           # ... and the earlier plan still replays the same


# ---------------------------------------------------------------------------------------------- integration
class _Pipe:
    def __init__(self, unet):
        self.unet = unet

    def to(self, device):
        return self


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_adapters_and_judge_agree_with_the_transformers_module(dtype):
    import numpy as np
    from PIL import Image
    from oracle.detfill import det_fill
    from smoke_impl import build_pair
    from imagharmony_amd import pns
    from imagharmony_amd.ip_adapter import IPAdapterPlusXL, IPAdapterXL
    e = _depth2("vit_h")
    enc = _enc(e["hf"], dtype)
    hf = copy.deepcopy(e["hf"]).to(DEV, dtype)
    _, hu, _ = build_pair(DEV, dtype)
    img = Image.fromarray((np.random.RandomState(0).rand(260, 300, 3) * 255).astype("uint8"))
    for cls, kw in ((IPAdapterXL, dict(num_tokens=4)), (IPAdapterPlusXL, dict(num_tokens=16))):
        outs = []
        for tower in (enc, hf):
            ip = cls(_Pipe(hu), None, None, DEV, dtype=dtype, image_encoder=tower, **kw)
            assert ip.clip_embeddings_dim == 1024 and ip.clip_hidden_size == 1280
            det_fill(ip.image_proj_model, 5)
            outs.append(ip.get_image_embeds(pil_image=img))
        for a, b in zip(*outs):
            r = rel_rms(a.float(), b.float())
            print(f"{cls.__name__} {dtype}: rel-rms {r:.3e}")
            assert a.shape == b.shape and r <= BOUND[dtype]
    lat = torch.randn(4, 4, 32, 32, generator=torch.Generator().manual_seed(2)).to(DEV)
    decode = lambda z: torch.nn.functional.interpolate(torch.tanh(z[:, :3]), size=(256, 256), mode="bilinear")      # noqa: E731
    target = torch.randn(1, 1024, generator=torch.Generator().manual_seed(3))
    s_hip = pns.ClipPreferenceJudge(decode, enc, target)(lat)
    s_ref = pns.ClipPreferenceJudge(decode, hf, target)(lat)
    print(f"judge {dtype}: {s_hip.tolist()} vs {s_ref.tolist()}")
    assert s_hip.shape == (4,) and (s_hip - s_ref).abs().max().item() <= BOUND[dtype]      # cosine scores: scale 1


def test_ipadapter_hip_backend_constructs_from_a_saved_directory(tmp_path):
    from transformers import CLIPImageProcessor, CLIPVisionConfig, CLIPVisionModelWithProjection
    from smoke_impl import build_pair
    from imagharmony_amd.clip_vision import CLIPVisionEncoder
    from imagharmony_amd.ip_adapter import IPAdapterXL
    dtype = torch.bfloat16
    torch.manual_seed(0)
    hf = CLIPVisionModelWithProjection(CLIPVisionConfig(hidden_size=128, intermediate_size=256, num_hidden_layers=1, num_attention_heads=2,
                                                        image_size=28, patch_size=14, projection_dim=64, hidden_act="gelu")).eval()
    hf.save_pretrained(tmp_path)
    _, hu, _ = build_pair(DEV, dtype)
    proc = CLIPImageProcessor(size={"shortest_edge": 28}, crop_size={"height": 28, "width": 28})
    ip = IPAdapterXL(_Pipe(hu), str(tmp_path), None, DEV, dtype=dtype, image_encoder_backend="hip", clip_image_processor=proc)
    assert isinstance(ip.image_encoder, CLIPVisionEncoder) and ip.clip_embeddings_dim == 64 and ip.image_encoder.dtype == dtype
    px = torch.randn(2, 3, 28, 28, generator=torch.Generator().manual_seed(1)).to(dtype)
    with torch.no_grad():
        ref = hf(px.float()).image_embeds
    got = ip.image_encoder(px.to(DEV)).image_embeds
    assert rel_rms(got.float().cpu(), ref) <= BOUND[dtype]
    with pytest.raises(ValueError):
        IPAdapterXL(_Pipe(hu), str(tmp_path), None, DEV, dtype=dtype, image_encoder_backend="triton")
