"""imh_attention_enc_causal, the quick-GELU epilogue, the row gather and imagharmony_amd.clip_text.CLIPTextEncoder on the GPU, against
fp32 CPU references: torch's scaled_dot_product_attention(is_causal=True) for the kernel, plain torch for the epilogue and the gather
(bit-equal), transformers' CLIPTextModel / CLIPTextModelWithProjection (seeded random weights) for the module.

Bounds.  Kernel: the per-module ones of SURVEY.md 8(c) that test_attention_enc_matches_fp32_sdpa carries, rel-RMS <= 1.5e-2 (bf16) /
2e-3 (fp16).  Quick-GELU GEMM: test_gpu_ops.assert_close as the GF_ACT_GELU cases use it.  Module: measured in the test -- 3x the rel-RMS
that the transformers module cast to the run dtype shows against its own fp32 on the same ids (different accumulation order and
different exp / sigmoid / erf approximations; the ratio the full-depth vision test uses).  On the CPU that bf16 reference noise is
about 8.0e-3 (pooled) and 7.1e-3 (hidden_states[-2]) at depth 2."""
import copy
import ctypes as C
import json
import os

import pytest
import torch

from conftest import ROOT, record_parity, rel_rms
from guarded import run_dense_and_guarded
from test_gpu_ops import L, assert_close, rnd  # noqa: F401

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BOUND = {torch.bfloat16: 1.5e-2, torch.float16: 2e-3}
DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
# (H, d, L, B): one tile exactly, one key past a tile, three tiles (block 0 skips two), L = 1, padded head dims
SHAPES = [(12, 64, 77, 2), (20, 64, 77, 1), (4, 64, 64, 1), (4, 64, 65, 1), (2, 64, 1, 1), (4, 80, 130, 2), (2, 128, 200, 1)]
_sid = lambda s: "H%d_d%d_L%d_B%d" % s      # noqa: E731


# ---------------------------------------------------------------------------------------------- causal kernel
_QKV = {}


def _qkv(shape, dtype):
    """inputs rounded to the run dtype (CPU) and their fp32 causal SDPA reference, computed once per (shape, dtype)"""
    key = (shape, dtype)
    if key not in _QKV:
        H, d, L_, B = shape
        g = torch.Generator().manual_seed(1000 * d + L_ + H)
        qkv = (torch.randn(B * L_, 3 * H * d, generator=g) * 1.5).to(dtype)
        q, k, v = (t.float().view(B, L_, H, d).transpose(1, 2) for t in qkv.split(H * d, dim=1))
        ref = torch.nn.functional.scaled_dot_product_attention(q, k, v, is_causal=True).transpose(1, 2).reshape(B * L_, H * d)
        _QKV[key] = (qkv, ref)
    return _QKV[key]


def _split(dq, H, d):
    return dq[:, :H * d], dq[:, H * d:2 * H * d], dq[:, 2 * H * d:]


@pytest.mark.parametrize("packed", [False, True], ids=["three_tensors", "packed"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_attention_enc_causal_matches_fp32_sdpa(shape, dtype, packed):
    from imagharmony_amd.ctx import Ctx
    H, d, L_, B = shape
    qkv, ref = _qkv(shape, dtype)
    ctx = Ctx(DEV, dtype)
    dq = qkv.to(DEV)
    q, k, v = _split(dq, H, d) if packed else (t.contiguous() for t in dq.split(H * d, dim=1))
    o = ctx.attention_enc(q, k, v, B, H, L_, d, causal=True)
    torch.cuda.synchronize()
    r = rel_rms(o.float().cpu(), ref)
    print(f"attention_enc_causal {shape} {dtype} packed={packed}: rel-rms {r:.3e}")
    assert o.shape == (B * L_, H * d) and torch.isfinite(o.float()).all()
    assert r <= BOUND[dtype], f"rel-rms {r:.3e}"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [(12, 64, 77, 2), (4, 80, 130, 2)], ids=_sid)
def test_attention_enc_causal_is_independent_of_the_future(shape, dtype):
    """K and V rows >= j overwritten with large FINITE values (a masked key of the diagonal tile is still staged, and 0 * NaN would
    condemn a correct kernel): O rows < j keep their bits; the bidirectional call on the same data does not"""
    from imagharmony_amd.ctx import Ctx
    H, d, L_, B = shape
    qkv, _ = _qkv(shape, dtype)
    ctx = Ctx(DEV, dtype)
    dq = qkv.to(DEV)
    base = ctx.attention_enc(*_split(dq, H, d), B, H, L_, d, causal=True).clone().view(B, L_, H * d)
    base_bi = ctx.attention_enc(*_split(dq, H, d), B, H, L_, d).clone().view(B, L_, H * d)
    for j in (1, 63, 64, 65, L_ - 1):
        pert = dq.clone().view(B, L_, 3 * H * d)
        sign = torch.where(torch.arange(2 * H * d, device=DEV) % 2 == 0, 3e4, -3e4).to(dtype)
        pert[:, j:, H * d:] = sign
        pert = pert.view(B * L_, 3 * H * d)
        o = ctx.attention_enc(*_split(pert, H, d), B, H, L_, d, causal=True).clone().view(B, L_, H * d)
        o_bi = ctx.attention_enc(*_split(pert, H, d), B, H, L_, d).clone().view(B, L_, H * d)
        torch.cuda.synchronize()
        assert torch.isfinite(o.float()).all()
        assert torch.equal(o[:, :j], base[:, :j]), f"j={j}: a row before the perturbation changed"
        assert not torch.equal(o[:, j:], base[:, j:]), f"j={j}: the perturbed rows did not change (the test cannot fail)"
        assert not torch.equal(o_bi[:, :j], base_bi[:, :j]), f"j={j}: the bidirectional kernel ignored the future"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [(12, 64, 77, 2), (4, 64, 65, 1), (4, 80, 130, 2), (2, 64, 1, 1)], ids=_sid)
def test_attention_enc_causal_reads_and_writes_only_its_rows(shape, dtype):
    """operands as views into larger NaN-filled tensors with 72 rows on either side: a loaded row outside [0, B*L) would put NaN into the
    result; the rows of O around it must keep their NaN"""
    from imagharmony_amd.ctx import Ctx
    H, d, L_, B = shape
    qkv, _ = _qkv(shape, dtype)
    ctx = Ctx(DEV, dtype)
    dq = qkv.to(DEV)
    plain = ctx.attention_enc(*_split(dq, H, d), B, H, L_, d, causal=True).clone()
    pad, M = 72, B * L_
    big = torch.full((M + 2 * pad, 3 * H * d), float("nan"), dtype=dtype, device=DEV)
    big[pad:pad + M] = dq
    obig = torch.full((M + 2 * pad, H * d), float("nan"), dtype=dtype, device=DEV)
    ctx.attention_enc(*_split(big[pad:pad + M], H, d), B, H, L_, d, out=obig[pad:pad + M], causal=True)
    torch.cuda.synchronize()
    assert torch.isfinite(obig[pad:pad + M].float()).all()
    assert torch.equal(obig[pad:pad + M], plain)
    assert torch.isnan(obig[:pad]).all() and torch.isnan(obig[pad + M:]).all()


def _settle(dense, guarded, arena, what):
    arena.check()
    for i, (a, b) in enumerate(zip(dense, guarded)):
        assert a.shape == b.shape and a.dtype == b.dtype
        assert torch.equal(a, b), f"{what}: result {i}: {int((a != b).sum())} of {a.numel()} elements differ from the dense run"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_guarded_placement_of_the_three_new_launches(L, dtype):
    """tests/guarded.py: every operand a view into one NaN-sentinel arena with guard bands and a row pitch wider than the row -- same
    bits as the dense run, guards intact, outputs finite"""
    H, d, L_, B = 4, 80, 130, 2
    qkv = _qkv((H, d, L_, B), dtype)[0].to(DEV)

    def attn(ctx, put, out):
        p = put(qkv, ld=3 * H * d + 64)
        return ctx.attention_enc(*_split(p, H, d), B, H, L_, d, causal=True, out=out((B * L_, H * d), dtype, ld=H * d + 24))
    _settle(*run_dense_and_guarded(DEV, dtype, attn), "attention_enc_causal")

    Cc, P, rows = 72, 77, 50
    table, pos = rnd(rows, Cc, dtype=dtype, seed=1), rnd(P, Cc, dtype=dtype, seed=2)
    idx = torch.randint(0, rows, (2 * P,), generator=torch.Generator().manual_seed(3), dtype=torch.int32)
    idx[0], idx[-1] = rows - 1, 0
    idx = idx.to(DEV)

    def gather(ctx, put, out):
        return ctx.gather_rows(put(table, ld=Cc + 8), put(idx), add=put(pos, ld=Cc + 16), out=out((2 * P, Cc), dtype, ld=Cc + 24))
    dense, guarded, arena = run_dense_and_guarded(DEV, dtype, gather)
    _settle(dense, guarded, arena, "gather_rows")
    assert torch.equal(dense[0], (table[idx.long()].float() + pos[torch.arange(2 * P, device=DEV) % P].float()).to(dtype))

    M, N, K = 77, 200, 128
    x, w, b = rnd(M, K, dtype=dtype, seed=4), rnd(N, K, dtype=dtype, seed=5, scale=K ** -0.5), rnd(N, dtype=dtype, seed=6)

    def qgelu(ctx, put, out):
        return ctx.gemm(put(x, ld=K + 64), put(w, ld=K + 8), out=out((M, N), dtype, ld=N + 24), bias=put(b), flags=L.GF_ACT_QGELU)
    _settle(*run_dense_and_guarded(DEV, dtype, qgelu), "gemm + quick-GELU")


def test_attention_enc_causal_records_and_replays_in_a_plan(L):
    from imagharmony_amd.ctx import Ctx
    shape, dtype = (4, 64, 65, 1), torch.bfloat16
    H, d, L_, B = shape
    qkv, ref = _qkv(shape, dtype)
    dq = qkv.to(DEV)
    rec = Ctx(DEV, dtype, record=True)
    o = rec.attention_enc(*_split(dq, H, d), B, H, L_, d, causal=True)
    assert rec.lib.imh_plan_get_kind(rec.plan, 0) == L.OP_ATTN_ENC_CAUSAL == 9
    rec.run()
    first = o.clone()
    rec.capture()
    o.zero_()
    rec.replay()
    torch.cuda.synchronize()
    assert torch.equal(o, first) and rel_rms(o.float().cpu(), ref) <= BOUND[dtype]


def test_attention_enc_causal_error_codes(L):
    lib = L.load()
    t = torch.zeros(64, 3 * 2 * 136, dtype=torch.bfloat16, device=DEV)
    o = torch.zeros(64, 2 * 136, dtype=torch.bfloat16, device=DEV)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(d, q=t.data_ptr(), ldq=None, dt=L.IMH_DT_BF16):
        a = L.EncAttnArgs()
        a.Q, a.K, a.V, a.O = q, t.data_ptr(), t.data_ptr(), o.data_ptr()
        a.B, a.H, a.L, a.d = 1, 2, 64, d
        a.ldq = a.ldk = a.ldv = t.stride(0)
        if ldq is not None:
            a.ldq = ldq
        a.ldo, a.scale, a.dtype = o.stride(0), 0.1, dt
        return lib.imh_attention_enc_causal(C.byref(a), s)
    assert call(80) == 0
    assert call(12) == -2 and b"multiple of 8" in lib.imh_last_error()         # IMH_ERR_SHAPE
    assert call(136) == -2                                                       # d > 128
    assert call(80, ldq=100) == -2                                               # row stride below H*d
    assert call(80, q=None) == -1 and b"null" in lib.imh_last_error()           # IMH_ERR_ARG
    assert call(80, q=t.data_ptr() + 2) == -1                                    # alignment
    assert call(80, dt=7) == -3                                                  # IMH_ERR_DTYPE
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- quick-GELU epilogue
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape,cfg", [((2, 8, 64), (64, 64, 1)), ((77, 200, 128), (64, 64, 1)), ((77, 200, 128), (128, 128, 1)),
                                       ((154, 3072, 768), None)], ids=["2x8x64", "77x200x128_t64", "77x200x128_t128", "clip_l_fc1_heuristic"])
def test_gemm_quick_gelu_matches_fp32_torch(L, dtype, shape, cfg):
    from imagharmony_amd.ctx import Ctx
    M, N, K = shape
    ctx = Ctx(DEV, dtype)
    x, w, b = rnd(M, K, dtype=dtype, seed=1), rnd(N, K, dtype=dtype, seed=2, scale=2.0 * K ** -0.5), rnd(N, dtype=dtype, seed=3)
    pre = x.float() @ w.float().t() + b.float()
    y = ctx.gemm(x, w, bias=b, flags=L.GF_ACT_QGELU, cfg=cfg)
    torch.cuda.synchronize()
    assert_close(y, pre * torch.sigmoid(1.702 * pre), dtype, f"quick_gelu {shape} {cfg}")
    assert not torch.equal(y, ctx.gemm(x, w, bias=b, flags=L.GF_ACT_GELU, cfg=cfg))      # ... and it is not the erf GELU


def test_gemm_quick_gelu_is_exclusive_with_the_other_activations(L):
    from imagharmony_amd.ctx import Ctx
    ctx = Ctx(DEV, torch.bfloat16)
    x, w = rnd(16, 64, dtype=torch.bfloat16, seed=1), rnd(32, 64, dtype=torch.bfloat16, seed=2)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for other in (L.GF_ACT_GELU, L.GF_ACT_SILU, L.GF_GEGLU):
        a = ctx.gemm(x, w, flags=L.GF_ACT_QGELU | other, _args_only=True)[0]
        assert ctx.lib.imh_gemm(C.byref(a), s) == -1 and b"exclusive" in ctx.lib.imh_last_error()
        assert ctx.lib.imh_gemm_dual(C.byref(a), C.byref(a), s) == -1
    a = ctx.gemm(x, w, flags=L.GF_ACT_QGELU, _args_only=True)[0]
    assert ctx.lib.imh_gemm(C.byref(a), s) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- gather
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("Cc", [8, 768, 1280])
def test_gather_rows_is_bit_equal_to_torch(L, dtype, Cc):
    from imagharmony_amd.ctx import Ctx
    ctx = Ctx(DEV, dtype)
    rows, P, B = 300, 77, 2
    table, pos = rnd(rows, Cc, dtype=dtype, seed=1), rnd(P, Cc, dtype=dtype, seed=2)
    idx = torch.randint(0, rows, (B * P,), generator=torch.Generator().manual_seed(3), dtype=torch.int32)
    idx[0], idx[1], idx[-1] = 0, rows - 1, rows - 1
    idx = idx.to(DEV)
    r = torch.arange(B * P, device=DEV)
    y = ctx.gather_rows(table, idx, add=pos)
    assert torch.equal(y, (table[idx.long()].float() + pos[r % P].float()).to(dtype))
    assert torch.equal(ctx.gather_rows(table, idx), table[idx.long()])
    # the EOS pooling form: one row per sample out of [B * P, C] rows
    eos = torch.tensor([5, P + 76], dtype=torch.int32, device=DEV)
    assert torch.equal(ctx.gather_rows(y, eos), y[eos.long()])
    a = L.EwArgs()
    a.a, a.b, a.y, a.n, a.i0, a.i1, a.i2, a.i5, a.dtype = table.data_ptr(), idx.data_ptr(), y.data_ptr(), B * P, Cc + 4, Cc + 4, Cc + 4, rows, ctx.dt
    assert ctx.lib.imh_elementwise(L.EW_GATHER_ROWS, C.byref(a), ctx.stream()) == -2         # C not a multiple of 8
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- module
CLIP_L = dict(hidden_size=768, intermediate_size=3072, num_attention_heads=12, projection_dim=768, hidden_act="quick_gelu")
BIGG = dict(hidden_size=1280, intermediate_size=5120, num_attention_heads=20, projection_dim=1280, hidden_act="gelu")
VOCAB, EOT = 49408, 49407


def _hf(name, depth, eos, seed=0):
    """CLIP-L as CLIPTextModel, bigG as CLIPTextModelWithProjection: the two classes of an SDXL checkpoint"""
    from transformers import CLIPTextConfig, CLIPTextModel, CLIPTextModelWithProjection
    torch.manual_seed(seed)
    cfg = CLIPTextConfig(vocab_size=VOCAB, num_hidden_layers=depth, max_position_embeddings=77, bos_token_id=49406, eos_token_id=eos,
                         pad_token_id=1, **(CLIP_L if name == "clip_l" else BIGG))
    return (CLIPTextModel if name == "clip_l" else CLIPTextModelWithProjection)(cfg).eval()


def _ids(B=2, seed=11):
    """row 0: end-of-text at position 5 and as the padding behind it (CLIP-L's tokenizer pads with it), row 1: at position 76; further rows
    at 5 + 9 r.  Ordinary tokens stay below the end-of-text id, so argmax (eos_token_id == 2) and first-occurrence name the same rows."""
    ids = torch.randint(3, 40000, (B, 77), generator=torch.Generator().manual_seed(seed))
    ids[:, 0] = 49406
    for r in range(B):
        p = 76 if r == 1 else 5 + 9 * (r // 2)
        ids[r, p:] = EOT
    return ids


_CASES = {}


def _case(name, depth, eos):
    key = (name, depth, eos)
    if key not in _CASES:
        _CASES[key] = dict(hf=_hf(name, depth, eos), ids=_ids(), out={})
    return _CASES[key]


def _pooled(o):
    return o.text_embeds if getattr(o, "text_embeds", None) is not None else o.pooler_output


def _fields(o):
    return dict(hidden_0=o.hidden_states[0], hidden_m2=o.hidden_states[-2], last_hidden_state=o.last_hidden_state, pooled=_pooled(o))


def _measure(e, dtype, ids=None):
    """{field: dict(reference_dtype_noise, hip, bound = 3 x noise)} of one case: fp32 transformers module on the CPU = the reference, the
    same module cast to the run dtype (CPU) = the noise, CLIPTextEncoder on the GPU = ours"""
    from imagharmony_amd.clip_text import CLIPTextEncoder
    ids = e["ids"] if ids is None else ids
    with torch.no_grad():
        if "fp32" not in e["out"]:
            e["out"]["fp32"] = _fields(e["hf"](ids, output_hidden_states=True))
        lo = copy.deepcopy(e["hf"]).to(dtype)
        rlo = _fields(lo(ids, output_hidden_states=True))
        del lo
    enc = CLIPTextEncoder.from_hf(e["hf"]).to(DEV, dtype)
    out = enc(ids.to(DEV), output_hidden_states=True)
    ours = _fields(out)
    r32 = e["out"]["fp32"]
    res = {}
    for k in r32:
        noise = rel_rms(rlo[k].float(), r32[k])
        res[k] = dict(reference_dtype_noise=noise, hip=rel_rms(ours[k].float().cpu(), r32[k]), bound=3 * noise)
    return res, enc, out


def _record(tag, dtype, res):
    path = os.path.join(ROOT, "profiles", "clip_text_parity.json")
    try:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        try:
            with open(path) as f:
                rec = json.load(f)
        except (OSError, ValueError):
            rec = {}
        rec.setdefault(tag, {})[IDS[DTYPES.index(dtype)]] = res
        with open(path, "w") as f:
            json.dump(rec, f, indent=1, sort_keys=True)
    except OSError:
        pass
    for k, v in res.items():
        record_parity(f"clip_text.{tag}.{IDS[DTYPES.index(dtype)]}.{k}", v["hip"], v["bound"], reference_dtype_noise=v["reference_dtype_noise"])


@pytest.mark.parametrize("eos", [2, EOT], ids=["eos2", "eos49407"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ["clip_l", "bigg"])
def test_module_depth2_full_width_matches_transformers_fp32(name, dtype, eos):
    e = _case(name, 2, eos)
    res, enc, out = _measure(e, dtype)
    print(f"clip_text depth 2 {name} {dtype} eos_token_id={eos}: {res}")
    _record(f"depth2.{name}.eos{eos}", dtype, res)
    cfg = enc.config
    assert cfg.eos_token_id == eos and enc.with_projection == (name == "bigg")
    assert len(out.hidden_states) == 3 and out.last_hidden_state.shape == (2, 77, cfg.hidden_size)
    assert out.pooler_output.shape == (2, cfg.hidden_size)
    assert torch.equal(out.pooler_output[0], out.last_hidden_state[0, 5]) and torch.equal(out.pooler_output[1], out.last_hidden_state[1, 76])
    if name == "bigg":
        assert out.text_embeds.shape == (2, 1280) and out[0] is out.text_embeds
    else:
        assert out.text_embeds is None and out[0] is out.last_hidden_state
    for k, v in res.items():
        assert v["hip"] <= v["bound"], f"{k}: {v}"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_module_full_depth_clip_l_within_3x_of_the_references_own_dtype_noise(dtype):
    e = _case("clip_l", 12, 2)
    res, _, out = _measure(e, dtype)
    print(f"clip_text full depth clip_l {dtype}: {res}")
    _record("full_depth.clip_l", dtype, res)
    assert len(out.hidden_states) == 13
    for k, v in res.items():
        assert v["hip"] <= v["bound"], f"{k}: {v}"


def test_module_behaviour_replay_batches_and_causality_through_the_stack():
    dtype = torch.bfloat16
    e = _case("clip_l", 2, 2)
    res, enc, a = _measure(e, dtype)
    bound = {k: v["bound"] for k, v in res.items()}
    ids4 = _ids(4, seed=12).to(DEV)
    plan = enc._plans[2]
    b = enc(e["ids"].to(DEV))
    assert enc._plans[2] is plan and plan["ctx"].captured                   # the second call replayed the recorded plan
    assert torch.equal(a.last_hidden_state, b.last_hidden_state) and torch.equal(a.pooler_output, b.pooler_output)
    assert b.hidden_states is None and len(a.hidden_states) == 3
    o4 = enc(ids4, output_hidden_states=True)
    assert sorted(enc._plans) == [2, 4]
    for i in (0, 1, 3):
        o1 = enc(ids4[i:i + 1], output_hidden_states=True)
        assert rel_rms(o4.hidden_states[-2][i].float(), o1.hidden_states[-2][0].float()) <= bound["hidden_m2"]
        assert rel_rms(o4.pooler_output[i].float(), o1.pooler_output[0].float()) <= bound["pooled"]
    assert sorted(enc._plans) == [1, 2, 4]
    assert torch.equal(enc(e["ids"].to(DEV)).pooler_output, a.pooler_output)           # ... and the earlier plan still replays the same
    # two id batches that differ only after position p: the rows up to p keep their bits through gather, LayerNorms, GEMMs and attention
    for p in (0, 30, 63, 75):
        other = ids4.clone()
        other[:, p + 1:] = torch.randint(3, 40000, (4, 76 - p), generator=torch.Generator().manual_seed(p)).to(DEV)
        ho = enc(other, output_hidden_states=True).hidden_states[-2]
        assert torch.equal(ho[:, :p + 1], o4.hidden_states[-2][:, :p + 1]), f"p={p}"
        assert not torch.equal(ho[:, p + 1:], o4.hidden_states[-2][:, p + 1:])
    with pytest.raises(ValueError):
        enc(torch.full((1, 77), VOCAB, device=DEV))


# ---------------------------------------------------------------------------------------------- integration
def _small_pair(dtype):
    """stock encoders of small widths with head dim 64 and stub tokenizers (no vocabulary files offline)"""
    from transformers import CLIPTextConfig, CLIPTextModel, CLIPTextModelWithProjection
    from test_text_encoder import _Tok

    class Tok77(_Tok):
        model_max_length = 77
    torch.manual_seed(0)
    kw = dict(vocab_size=100, num_hidden_layers=2, max_position_embeddings=77, bos_token_id=1, eos_token_id=2, pad_token_id=0)
    e1 = CLIPTextModel(CLIPTextConfig(hidden_size=128, intermediate_size=256, num_attention_heads=2, projection_dim=128,
                                      hidden_act="quick_gelu", **kw)).eval()
    e2 = CLIPTextModelWithProjection(CLIPTextConfig(hidden_size=256, intermediate_size=512, num_attention_heads=4, projection_dim=64,
                                                    hidden_act="gelu", **kw)).eval()
    return Tok77, e1, e2


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_prompt_encoder_hip_backend_agrees_with_the_stock_modules(dtype):
    from imagharmony_amd.clip_text import CLIPTextEncoder
    from imagharmony_amd.pipeline import StableDiffusionXLCustomPipeline
    from imagharmony_amd.text import SDXLPromptEncoder
    Tok77, e1, e2 = _small_pair(dtype)
    g1, g2 = copy.deepcopy(e1).to(DEV, dtype), copy.deepcopy(e2).to(DEV, dtype)
    ref = SDXLPromptEncoder(Tok77(), Tok77(), e1, e2)                                 # fp32 on the CPU: the reference
    stock = SDXLPromptEncoder(Tok77(), Tok77(), g1, g2)                               # the run dtype on the GPU: the noise
    hip = SDXLPromptEncoder(Tok77(), Tok77(), g1, g2, text_encoder_backend="hip")
    assert all(isinstance(e, CLIPTextEncoder) and e.dtype == dtype for _, e in hip.pairs)
    call = dict(prompt=["a photo of three cats", "two dogs"], negative_prompt="blurry", num_images_per_prompt=2)
    r, s, h = ref(**call), stock(**call), hip(**call)
    for name, tr, ts, th in zip(("prompt_embeds", "negative_prompt_embeds", "pooled", "negative_pooled"), r, s, h):
        noise, ours = rel_rms(ts.float().cpu(), tr), rel_rms(th.float().cpu(), tr)
        print(f"SDXLPromptEncoder {dtype} {name}: reference dtype noise {noise:.3e}, hip {ours:.3e}")
        assert th.shape == ts.shape == tr.shape and th.dtype == dtype and th.is_cuda
        assert ours <= 3 * noise, f"{name}: hip {ours:.3e}, reference dtype noise {noise:.3e}"
    assert h[0].shape == (4, 77, 384) and h[2].shape == (4, 64)
    assert torch.equal(h[0][0], h[0][1]) and torch.equal(h[0][2], h[0][3]) and not torch.equal(h[0][0], h[0][2])      # tiling per prompt
    assert torch.equal(h[2][0], h[2][1]) and torch.equal(h[1][0], h[1][3])
    z, zs = hip("x", negative_prompt=None), stock("x", negative_prompt=None)
    assert torch.count_nonzero(z[1]) == 0 and torch.count_nonzero(z[3]) == 0 and z[1].shape == zs[1].shape       # force_zeros_for_empty_prompt
    pipe = StableDiffusionXLCustomPipeline.__new__(StableDiffusionXLCustomPipeline)
    pipe.text_encoder = hip
    out = pipe.encode_prompt("a photo of three cats", num_images_per_prompt=1, do_classifier_free_guidance=True, negative_prompt="blurry")
    assert len(out) == 4 and out[0].shape == (1, 77, 384) and torch.equal(out[0][0], h[0][0])
