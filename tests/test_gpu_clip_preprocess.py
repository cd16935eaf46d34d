"""imh_clip_preprocess on the GPU against its float64 restatement (imagharmony_amd/imageops.py), CLIPVisionEncoder.embed_decoded against
forward, and the "hip" judge against the "torch" judge.  Shapes, inputs and bounds: tests/clip_pre_cases.py."""
import ctypes as C

import pytest
import torch

import clip_pre_cases as cases
from conftest import rel_rms

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS = ["fp32", "bf16", "fp16"]
SENT = -77.0            # exactly representable in every T


def _ctx(dtype=torch.bfloat16):
    from imagharmony_amd.ctx import Ctx
    return Ctx(DEV, dtype)


def _run(x, size, patch, dtype, ldp, ctx=None):
    """rows [S g g, ldp] prefilled with SENT; the op writes columns [0, 3 p p)"""
    from imagharmony_amd.imageops import CLIP_MEAN, CLIP_STD
    S, g = x.shape[0], size // patch
    buf = torch.full((S * g * g, ldp), SENT, dtype=dtype, device=DEV)
    (ctx or _ctx()).clip_preprocess(x.to(DEV), buf, size, patch, CLIP_MEAN, CLIP_STD)
    torch.cuda.synchronize()
    return buf


def _hold(buf, ref, dtype, what):
    k = ref.shape[1]
    y = buf[:, :k].double().cpu()
    err = (y - ref).abs()
    lim = cases.bound_for(ref, dtype)
    worst = float((err / lim).max())
    print(f"clip_preprocess {what} {dtype}: max |y - ref| {float(err.max()):.3e}, worst err / bound {worst:.3f}")
    assert torch.isfinite(y).all()
    assert bool((err <= lim).all()), f"{what}: max |y - ref| {float(err.max()):.3e}, worst err / bound {worst:.3f}"
    assert bool((buf[:, k:] == SENT).all()), f"{what}: padding columns were written"


# ---------------------------------------------------------------------------------------------- 1. kernel vs restatement
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("hw", cases.SHAPES, ids=lambda s: "%dx%d" % s)
def test_kernel_matches_restatement(hw, dtype):
    c = cases.case(*hw)
    k = 3 * cases.PATCH ** 2
    for ldp in (k, 640, cases.padded_k(cases.PATCH) + 8):          # dense; ViT's 640 for K = 588; the padded K inside a wider row
        _hold(_run(c["x"], cases.SIZE, cases.PATCH, dtype, ldp), c["ref"], dtype, f"{hw} ldp={ldp}")


def test_kernel_clamps_bite_in_the_inputs():
    """the inputs do exercise both clamps: values outside [-1, 1] go in, and the reference holds outputs at both clamp levels that an
    unclamped resize would have pushed past them"""
    from imagharmony_amd import imageops as io
    c = cases.case(40, 56)
    x = c["x"].double().numpy()
    assert (abs(x[1]) > 1).mean() > 0.2
    nh, nw, top, left = io.clip_geometry(40, 56, cases.SIZE)
    import numpy as np
    u = np.clip(x[0, 0] / 2 + 0.5, 0, 1)
    v = io.aa_matrix(40, nh) @ u @ io.aa_matrix(56, nw).T
    assert v.max() > 1.01 and v.min() < -0.01


# ---------------------------------------------------------------------------------------------- 2. full size
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_kernel_full_size(dtype):
    H, W, size, patch = cases.FULL
    c = cases.case(H, W, size, patch, S=1)
    _hold(_run(c["x"], size, patch, dtype, 640), c["ref"], dtype, "1024x1024 -> 224")


# ---------------------------------------------------------------------------------------------- 3. guarded placement
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_guarded_placement(dtype):
    from guarded import run_dense_and_guarded
    from imagharmony_amd.imageops import CLIP_MEAN, CLIP_STD
    c = cases.case(31, 50)
    x = c["x"].to(DEV)
    S, g, k = x.shape[0], cases.SIZE // cases.PATCH, 3 * cases.PATCH ** 2

    def body(ctx, put, out):
        y = out((S * g * g, k), dtype, ld=640)
        ctx.clip_preprocess(put(x), y, cases.SIZE, cases.PATCH, CLIP_MEAN, CLIP_STD)
        return y
    dense, guarded, arena = run_dense_and_guarded(DEV, torch.bfloat16, body)
    arena.check()                                  # guards and the row gaps [k, 640) keep the sentinel; every written value is finite
    assert guarded[0].stride(0) == 640 and torch.equal(dense[0], guarded[0])
    _hold(torch.cat([guarded[0], torch.full((S * g * g, 1), SENT, dtype=dtype, device=DEV)], 1), c["ref"], dtype, "guarded")


# ---------------------------------------------------------------------------------------------- 4. eager == plan == graph; refusals
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_eager_plan_and_graph_agree_bit_for_bit(dtype):
    from imagharmony_amd import lib as L
    from imagharmony_amd.ctx import Ctx
    from imagharmony_amd.imageops import CLIP_MEAN, CLIP_STD
    c = cases.case(72, 40)
    eager = _run(c["x"], cases.SIZE, cases.PATCH, dtype, 640)
    x = c["x"].to(DEV)
    rec = Ctx(DEV, torch.bfloat16, record=True)
    buf = torch.full_like(eager, SENT)
    rec.clip_preprocess(x, buf, cases.SIZE, cases.PATCH, CLIP_MEAN, CLIP_STD)
    assert rec.lib.imh_plan_get_kind(rec.plan, 0) == L.OP_CLIP_PREPROCESS == 13
    assert bool((buf == SENT).all())               # recording launches nothing
    rec.run()
    torch.cuda.synchronize()
    assert torch.equal(buf, eager)
    rec.capture()
    buf.fill_(SENT)
    rec.replay()
    rec.replay()
    torch.cuda.synchronize()
    assert torch.equal(buf, eager)


def test_refusals_return_a_status_without_launching():
    from imagharmony_amd import lib as L
    from imagharmony_amd.imageops import CLIP_MEAN, CLIP_STD, clip_geometry
    lib = L.load()
    x = torch.zeros(1, 3, 40, 56, device=DEV)
    y = torch.full((4, 640), SENT, dtype=torch.bfloat16, device=DEV)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    nh, nw, top, left = clip_geometry(40, 56, 28)

    def call(**kw):
        a = L.ClipPreprocessArgs()
        a.x, a.y, a.S, a.H, a.W = x.data_ptr(), y.data_ptr(), 1, 40, 56
        a.nh, a.nw, a.top, a.left, a.size, a.patch, a.ldp = nh, nw, top, left, 28, 14, 640
        a.mean0, a.mean1, a.mean2 = CLIP_MEAN
        a.std0, a.std1, a.std2 = CLIP_STD
        a.dtype = L.IMH_DT_BF16
        for k, v in kw.items():
            setattr(a, k, v)
        rc = lib.imh_clip_preprocess(C.byref(a), s)
        return rc, lib.imh_last_error() or b""

    for kw, word in ((dict(size=27), b"multiple"), (dict(nh=27), b"smaller"), (dict(nw=20), b"smaller"), (dict(top=1), b"outside"),
                     (dict(left=nw - 27), b"outside"), (dict(left=-1), b"outside"), (dict(ldp=587), b"ldp"), (dict(x=None), b"null"),
                     (dict(y=None), b"null"), (dict(dtype=3), b"dtype"), (dict(dtype=-1), b"dtype"), (dict(S=0), b"positive"),
                     (dict(std1=0.0), b"std")):
        rc, msg = call(**kw)
        assert rc in (-1, -2) and b"imh_clip_preprocess" in msg and word in msg, (kw, rc, msg)
    assert lib.imh_clip_preprocess(None, s) == -1
    torch.cuda.synchronize()
    assert bool((y == SENT).all())                  # none of them launched
    assert call()[0] == 0
    torch.cuda.synchronize()
    assert bool((y[:, :588] != SENT).all()) and bool((y[:, 588:] == SENT).all())
    # the host layer refuses before the library is asked
    ctx = _ctx()
    with pytest.raises(L.ImhError):
        ctx.clip_preprocess(x, y, 27, 14, CLIP_MEAN, CLIP_STD)
    with pytest.raises(L.ImhError):
        ctx.clip_preprocess(x, y[:, :500], 28, 14, CLIP_MEAN, CLIP_STD)
    with pytest.raises(L.ImhError):
        ctx.clip_preprocess(x.half(), y, 28, 14, CLIP_MEAN, CLIP_STD)


# ---------------------------------------------------------------------------------------------- 5. embed_decoded vs forward
CLIP_TINY = dict(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, image_size=28, patch_size=14,
                 projection_dim=128, hidden_act="gelu")
_TOWER = {}


def _tower(dtype):
    """(CLIPVisionEncoder in dtype on the GPU, its transformers twin in fp32 on the CPU): seeded random weights, built once per dtype"""
    if dtype not in _TOWER:
        from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
        from imagharmony_amd.clip_vision import CLIPVisionEncoder
        if "hf" not in _TOWER:
            torch.manual_seed(11)
            _TOWER["hf"] = CLIPVisionModelWithProjection(CLIPVisionConfig(**CLIP_TINY)).eval()
        _TOWER[dtype] = CLIPVisionEncoder.from_hf(_TOWER["hf"]).to(DEV, dtype)
    return _TOWER[dtype], _TOWER["hf"]


def _decoded(n, H=72, W=56, seed=3):
    """n "decoded" images [n, 3, H, W] fp32: smooth random fields a little beyond [-1, 1]"""
    g = torch.Generator().manual_seed(seed)
    low = torch.randn(n, 3, 6, 5, generator=g)
    x = torch.nn.functional.interpolate(low, size=(H, W), mode="bilinear") * 0.9 + 0.1 * torch.randn(n, 3, H, W, generator=g)
    return x.contiguous()


def _noise_of_the_encoder(dtype, images):
    """(embed_decoded's and forward's image_embeds, rel-RMS of forward's run-dtype embeds against the fp32 transformers twin on the same pixels)"""
    from imagharmony_amd.pns import ClipPreferenceJudge
    enc, hf = _tower(dtype)
    judge = ClipPreferenceJudge(lambda z: z, enc, torch.zeros(1, CLIP_TINY["projection_dim"]))
    px = judge.preprocess(images.to(DEV)).to(dtype)
    fwd = enc(px).image_embeds
    with torch.no_grad():
        twin = hf(px.float().cpu()).image_embeds
    enc(torch.zeros_like(px))                        # other pixels through the plan's patch buffer: embed_decoded must write all of it
    new = enc.embed_decoded(images.to(DEV)).image_embeds
    rows = enc._plans[images.shape[0]]["patches"][:, :3 * CLIP_TINY["patch_size"] ** 2]
    g = CLIP_TINY["image_size"] // CLIP_TINY["patch_size"]
    want = px.reshape(-1, 3, g, 14, g, 14).permute(0, 2, 4, 1, 3, 5).reshape(rows.shape)
    print(f"patch rows {dtype}: {int((rows != want).sum())} of {rows.numel()} differ between the two pixel paths")
    return new, fwd, rel_rms(fwd.float().cpu(), twin)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_embed_decoded_matches_forward_within_the_encoders_own_noise(dtype):
    # 75 x 61 -> 34 x 28: a scale that is no power of two, so that torch's fp32 tap positions and the kernel's exact ones give weights
    # that differ in their last bits (at 72 x 56 both are exact and the two paths round to the very same rows); image 0 is the +-1
    # checkerboard, whose edge pixels then round differently in the run dtype here and there
    images = _decoded(3, H=75, W=61)
    images[0] = cases.images(75, 61, cases.SIZE, S=1)[0]
    new, fwd, noise = _noise_of_the_encoder(dtype, images)
    diff = rel_rms(new.float(), fwd.float())
    print(f"embed_decoded vs forward {dtype}: rel-rms {diff:.3e}; the encoder's own dtype noise vs fp32 twin {noise:.3e}")
    assert new.shape == fwd.shape and new.dtype == dtype and torch.isfinite(new.float()).all()
    assert diff <= noise, f"rel-rms {diff:.3e} > {noise:.3e}"
    enc, _ = _tower(dtype)
    plan = enc._plans[3]
    again = enc.embed_decoded(images.to(DEV))
    assert enc._plans[3] is plan and torch.equal(again.image_embeds, new)           # replayed; a pure function of the images
    out = enc.embed_decoded(images.to(DEV), output_hidden_states=True)
    assert len(out.hidden_states) == CLIP_TINY["num_hidden_layers"] + 1 and torch.equal(out.last_hidden_state, out.hidden_states[-1])
    with pytest.raises(Exception):
        enc.embed_decoded(images)                                                    # CPU tensor
    with pytest.raises(Exception):
        enc.embed_decoded(images.to(DEV).half())


# ---------------------------------------------------------------------------------------------- 6. judge ranking
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_hip_judge_ranks_like_the_torch_judge(dtype):
    from imagharmony_amd.pns import ClipPreferenceJudge
    enc, hf = _tower(dtype)
    images = _decoded(8, seed=17).to(DEV)
    _, _, noise = _noise_of_the_encoder(dtype, images.cpu())
    # two unit vectors whose un-normalised difference is `noise` in rel-RMS differ by at most ~noise in norm; their cosines with a
    # third unit vector by at most 2 * noise (the difference, then the renormalisation)
    spread = 2 * noise
    # the target: what sets the second image's embedding apart from the eight's mean (a random tower's embeddings are nearly collinear:
    # against one of them every score is 0.94 .. 0.998), so that one score leads the rest by a clear margin
    t = torch.nn.functional.normalize(enc.embed_decoded(images).image_embeds.float(), dim=-1)
    target = (t[1] - t.mean(0)).unsqueeze(0)
    dec = lambda z: z                                                                # noqa: E731  (the "latents" are the decoded images)
    s_t = ClipPreferenceJudge(dec, enc, target)(images)
    s_h = ClipPreferenceJudge(dec, enc, target, preprocess_backend="hip")(images)
    top = torch.sort(s_t, descending=True).values
    gap = float(top[0] - top[1])
    print(f"judge {dtype}: torch {s_t.tolist()} hip {s_h.tolist()} spread bound {spread:.3e} top-two gap {gap:.3e}")
    assert gap > 10 * spread, f"top-two gap {gap:.3e} is not > 10 x {spread:.3e}: the images do not separate"
    assert s_h.shape == (8,) and float((s_h - s_t).abs().max()) <= spread
    assert int(torch.argmax(s_h)) == int(torch.argmax(s_t))
    with pytest.raises(ValueError):
        ClipPreferenceJudge(dec, hf, target, preprocess_backend="hip")
    with pytest.raises(ValueError):
        ClipPreferenceJudge(dec, enc, target, preprocess_backend="triton")
