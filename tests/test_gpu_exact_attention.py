"""Every attention kernel behind the C ABI on operands for which softmax is a SELECTION (tests/attention_needles.py): the output has one
right value -- V of the needle key, the mean of an equal group, the weighted sum over two key sets -- and the comparison is
torch.equal.  A key dropped, counted twice, taken from the neighbouring 16-group, left unmasked in the padding or visible past the
diagonal changes whole rows by far more than a unit in the last place, whichever rows it touches; the assert_close tests of
test_gpu_ops.py / test_gpu_guarded_ops.py / test_gpu_clip_*.py stay as the net for rounding and overflow.

Every case calls assert_premise on the operands it launches (the statement and the premise are computed once per problem, in float64 on
the device), launches twice and compares the two outputs (race screen), and goes through Ctx like test_gpu_ops.py.

Exceptions to bit equality: none -- every kernel reproduces the statement's bits in both dtypes."""
import pytest
import torch
import torch.nn.functional as F

import attention_needles as an
from conftest import experimental, ref_row_stats
from test_gpu_ops import make_vt

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
_CTX = {}


@pytest.fixture(scope="module")
def L():
    from imagharmony_amd import lib
    lib.load()
    return lib


def ctx_for(dtype):
    from imagharmony_amd.ctx import Ctx
    if dtype not in _CTX:
        _CTX[dtype] = Ctx(DEV, dtype)
    return _CTX[dtype]


def make_k(kk):
    """[B, n_pad, C] -> every 16-group of head dims stored as [0-3, 8-11, 4-7, 12-15] (the fused kernels' K caches, GF_VT_PERM)"""
    B, n_pad, C_ = kk.shape
    return kk.view(B, n_pad, C_ // 16, 4, 4)[:, :, :, [0, 2, 1, 3], :].reshape(B, n_pad, C_).contiguous()


def flat(t):
    """[B, n, H, d] -> [B, n, H * d]"""
    return t.reshape(t.shape[0], t.shape[1], -1)


def problem(p):
    """the problem on the device, its premise asserted"""
    p = p.to(DEV)
    an.assert_premise(p)
    return p


def twice(launch, p, what):
    """launch() -> out; the second launch's bits are the first's, and both are the statement's"""
    first = launch().clone()
    again = launch()
    torch.cuda.synchronize()
    an.assert_selected(first, p, what)
    assert torch.equal(again, first), f"{what} [{p.what}]: not bitwise repeatable"
    return first


def with_mode(L, key, mode, fn):
    assert L.load().imh_debug_set(key, mode) == 0
    try:
        return fn()
    finally:
        L.load().imh_debug_set(key, 0)


# ------------------------------------------------------------------------------------ ctx.attention, self
def self_modes():
    """imh_debug_set key 4 (test_gpu_ops.test_attention_self): 0 what the forward runs, 1 in-order, 2 / 3 pipelined with the textbook / the
    deferred maximum, 7 whole items only (no key-quarter workgroups), 5 / 6 the key-split kernel of an experimental build"""
    return [0, 1, 2, 3, 7] + ([5, 6] if experimental() else [])


def _self_launch(ctx, p):
    B, Lq, H, _ = p.q.shape
    s = p.sets[0]
    assert s.Lp == Lq
    C_ = H * 64
    qk = torch.cat([flat(p.q), flat(s.k)], -1).reshape(B * Lq, 2 * C_).contiguous()
    vt = make_vt(flat(s.v), s.Lp)
    out = ctx.new(B * Lq, C_)

    def launch():
        out.zero_()
        return ctx.attention(qk[:, :C_], qk[:, C_:], vt, out, B, H, Lq, s.Lk, s.Lp, 2 * C_, 2 * C_, B * s.Lp, C_, p.scale)
    return launch


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,H,Lq", an.SELF_SHAPES)
def test_self_attention_selects(L, dtype, B, H, Lq):
    """every tail of the unrolled tile loop (1 .. 8, 16, 64 tiles) and the key-quarter workgroups of (2, 20, 1024), in every mode: single
    needles over every key, groups of 2 .. 128 across 16-key groups, tiles, ring wraps, key quarters and halves"""
    p = problem(an.single_set(B, H, Lq, Lq, Lq, dtype, seed=Lq // 64))
    launch = _self_launch(ctx_for(dtype), p)
    for mode in self_modes():
        with_mode(L, 4, mode, lambda: twice(launch, p, f"self attention, mode {mode}"))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,H,Lk,Lk_pad", an.SELF_MASKED)
def test_self_attention_masked_keys_select(L, dtype, B, H, Lk, Lk_pad):
    """keys of [Lk, Lk_pad) repeat real needles' codes (the first of them the last real key's) with V = -100: one unmasked pad key
    halves a row towards -100"""
    p = problem(an.single_set(B, H, Lk_pad, Lk, Lk_pad, dtype, seed=Lk))
    launch = _self_launch(ctx_for(dtype), p)
    for mode in self_modes():
        with_mode(L, 4, mode, lambda: twice(launch, p, f"self attention with masked keys, mode {mode}"))


@pytest.mark.parametrize("dtype", DTYPES)
def test_wrong_launches_are_refused(L, dtype):
    """the check bites on real launches: the pad keys declared real, V^T handed over without its 16-group permutation, the bidirectional
    encoder kernel on the causal problem -- each is a launch whose result the equality check must refuse, naming a row"""
    ctx = ctx_for(dtype)
    p = problem(an.single_set(1, 2, 128, 100, 128, dtype, seed=100))
    s = p.sets[0]
    qk = torch.cat([flat(p.q), flat(s.k)], -1).reshape(128, 256).contiguous()
    vt, vt_plain = make_vt(flat(s.v), 128), flat(s.v).permute(2, 0, 1).reshape(128, 128).contiguous()
    run = lambda lk, v: ctx.attention(qk[:, :128], qk[:, 128:], v, ctx.new(128, 128), 1, 2, 128, lk, 128, 256, 256, 128, 128, p.scale)
    an.assert_selected(run(100, vt), p, "the right launch")
    with pytest.raises(AssertionError, match="unseen key"):
        an.assert_selected(run(128, vt), p, "pad keys declared real")
    with pytest.raises(AssertionError, match="needle key"):
        an.assert_selected(run(100, vt_plain), p, "V^T without its permutation")
    c = problem(an.causal_set(1, 2, 77, 64, dtype, seed=77))
    q, k, v = (flat(t).reshape(77, 128).contiguous() for t in (c.q, c.sets[0].k, c.sets[0].v))
    an.assert_selected(ctx.attention_enc(q, k, v, 1, 2, 77, 64, causal=True), c, "the right launch")
    with pytest.raises(AssertionError, match="unseen key"):
        an.assert_selected(ctx.attention_enc(q, k, v, 1, 2, 77, 64, causal=False), c, "the bidirectional kernel")


# ------------------------------------------------------------------------------------ ctx.attention, two key sets
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,H,Lq,nt,nip", an.SELF_K2)
def test_attention_two_key_sets_select(L, dtype, B, H, Lq, nt, nip):
    """text + scale2 * image prompt (scale2 = 0.5) with plain K rows: both sets ragged, padded with poison"""
    ctx = ctx_for(dtype)
    p = problem(an.two_sets(B, H, Lq, nt, nip, dtype, seed=nip))
    s1, s2 = p.sets
    C_ = H * 64
    q = flat(p.q).reshape(B * Lq, C_).contiguous()
    k1, vt1, k2, vt2 = flat(s1.k).contiguous(), make_vt(flat(s1.v), s1.Lp), flat(s2.k).contiguous(), make_vt(flat(s2.v), s2.Lp)
    out = ctx.new(B * Lq, C_)

    def launch():
        out.zero_()
        return ctx.attention(q, k1, vt1, out, B, H, Lq, s1.Lk, s1.Lp, C_, C_, B * s1.Lp, C_, p.scale, k2=k2, vt2=vt2, Lk2=s2.Lk, Lk2_pad=s2.Lp,
                             ldk2=C_, ldvt2=B * s2.Lp, scale2=s2.w)
    twice(launch, p, "attention with two key sets")


# ------------------------------------------------------------------------------------ ctx.cross_attention
def _to_q(ctx, p, ln):
    """x, wq and the ln argument of a fused launch whose to_q gives p.q: Wq = A I, the token rows are the codes themselves.  ln = 1 .. 3
    (no statistics from the caller / handed over in 32-wide slots / from the row-statistics kernel): identity affine; the rows are
    balanced codes (mean 0, variance 1 per head chunk), LN(x) A differs from A x by eps / 2 = 5e-6 relative and rounds to it in T --
    asserted here on q_ref before any case relies on it"""
    from imagharmony_amd.attention_processor import fold_ln
    B, Lq, H, _ = p.q.shape
    C_ = H * 64
    x = (flat(p.q) / p.A).reshape(B * Lq, C_).contiguous()
    wq = (p.A * torch.eye(C_)).float()
    if not ln:
        wg = wq.to(DEV, p.dtype)
        assert torch.equal((x.float() @ wg.float().t()).to(p.dtype), flat(p.q).reshape(B * Lq, C_))
        return x, wg, None
    assert bool((x.float().view(B * Lq, H, 64).mean(-1) == 0).all()), "ln: every head chunk of a token row has mean 0"
    norm = torch.nn.LayerNorm(C_, eps=1e-5)
    wg, s_, c_ = fold_ln(wq, norm, ctx)
    q_ref = (F.layer_norm(x.float(), (C_,), norm.weight.to(DEV), norm.bias.to(DEV), 1e-5) @ wq.to(DEV).t()).to(p.dtype)
    assert torch.equal(q_ref, flat(p.q).reshape(B * Lq, C_)), "q_ref == A x"
    st = None if ln == 1 else ((ref_row_stats(x.float(), C_ // 32).to(DEV), C_ // 32) if ln == 2 else ctx.row_stats(x))
    return x, wg, (s_, c_, 1e-5, st)


def _cross_problem(B, H, Lq, nt, nip, dtype):
    if nip:
        return an.two_sets(B, H, Lq, nt, nip, dtype, seed=nt + nip)
    return an.single_set(B, H, Lq, nt, an.pad64(nt), dtype, seed=nt, balanced=True, gmax=4)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,H,Lq,nt,nip,ln", an.CROSS)
def test_fused_cross_attention_selects(L, dtype, B, H, Lq, nt, nip, ln):
    """csrc/xattn.hip, imh_debug_set key 3: 0 what the forward runs, 1 one head per workgroup (with half items where an XCD has 33 .. 63
    items: the last case), 9 the same without half items, 10 the wide form (where it fits: Lq % 128 == 0 and H % 5 == 0), 2 .. 4 the
    two-head kernel of an experimental build.  The wide form's bits are the one-head form's."""
    ctx = ctx_for(dtype)
    p = problem(_cross_problem(B, H, Lq, nt, nip, dtype))
    x, wg, lnq = _to_q(ctx, p, ln)
    s1 = p.sets[0]
    C_ = H * 64
    kw = {}
    if nip:
        s2 = p.sets[1]
        kw = dict(k2=make_k(flat(s2.k)), vt2=make_vt(flat(s2.v), s2.Lp), Lk2=s2.Lk, Lk2_pad=s2.Lp, ldk2=C_, ldvt2=B * s2.Lp, scale2=s2.w)
    k1, vt1 = make_k(flat(s1.k)), make_vt(flat(s1.v), s1.Lp)
    out = ctx.new(B * Lq, C_)

    def launch():
        out.zero_()
        return ctx.cross_attention(x, wg, k1, vt1, out, B, H, Lq, s1.Lk, s1.Lp, C_, B * s1.Lp, p.scale, ln=lnq, **kw)
    modes = [0, 1, 9] + ([10] if Lq % 128 == 0 and H % 5 == 0 else []) + ([2, 3, 4] if experimental() else [])
    outs = {m: with_mode(L, 3, m, lambda: twice(launch, p, f"fused cross attention ln={ln}, mode {m}")) for m in modes}
    if 10 in outs:
        assert torch.equal(outs[10], outs[1]), "the wide form is not bit-identical to the one-head form"


# ------------------------------------------------------------------------------------ ctx.cross_attention_regions
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("given", [False, True])
@pytest.mark.parametrize("B,H,Lq,nt,T,N", an.REGIONS)
def test_cross_attention_regions_select(L, dtype, given, B, H, Lq, nt, T, N):
    """csrc/xattn_regions.hip: N images per sample, masks of {0, 1, 0.5} with every fifth row 0 in all images, weights NULL or powers of
    two.  The rows whose masks are all 0 carry the bits of the text-only launch."""
    ctx = ctx_for(dtype)
    masks = an.region_masks(N, Lq, seed=N)
    weights = an.region_weights(N) if given else None
    p = problem(an.two_sets(B, H, Lq, nt, T, dtype, seed=T + N, scale2=1.0, n_img=N, masks=masks, weights=weights))
    x, wg, _ = _to_q(ctx, p, 0)
    s1, imgs = p.sets[0], p.sets[1:]
    C_, lp2 = H * 64, imgs[0].Lp
    k1, vt1 = make_k(flat(s1.k)).view(-1, C_), make_vt(flat(s1.v), s1.Lp)
    k2 = make_k(torch.stack([flat(s.k) for s in imgs], 1).reshape(B * N, lp2, C_)).view(-1, C_)         # image i of batch b at key (b N + i) lp2
    vt2 = make_vt(torch.stack([flat(s.v) for s in imgs], 1).reshape(B * N, lp2, C_), lp2)
    m, w = masks.to(DEV).contiguous(), None if weights is None else weights.to(DEV)
    out = ctx.new(B * Lq, C_)

    def launch():
        out.zero_()
        return ctx.cross_attention_regions(x, wg, k1, vt1, out, B, H, Lq, s1.Lk, s1.Lp, C_, B * s1.Lp, p.scale, k2, vt2, T, lp2, C_, B * N * lp2,
                                           N, m, weights=w, scale2=1.0)
    y = twice(launch, p, f"cross attention regions, weights {'given' if given else 'NULL'}").view(B, Lq, C_)
    text = torch.zeros(B * Lq, C_, dtype=dtype, device=DEV)
    ctx.cross_attention(x, wg, k1, vt1, text, B, H, Lq, s1.Lk, s1.Lp, C_, B * s1.Lp, p.scale)
    dark = (masks == 0).all(0).to(DEV)
    assert int(dark.sum()) >= Lq // 5
    assert torch.equal(y[:, dark], text.view(B, Lq, C_)[:, dark]), "rows whose masks are all 0 differ from the text-only launch"


# ------------------------------------------------------------------------------------ ctx.attention_small
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,H,Lq,Lk,dq,dv,which", an.SMALL)
def test_attention_small_selects(L, dtype, B, H, Lq, Lk, dq, dv, which):
    """both kernels of imh_attention_small: the LDS-resident one at key counts on both sides of its 64-key rounds, the fallback taken by
    a K row pitch that is no multiple of 8, by dq = 36, and above 150 KB of LDS; dv != dq, codes on the largest two-part split below dq"""
    ctx = ctx_for(dtype)
    p = problem(an.single_set(B, H, Lq, Lk, Lk, dtype, seed=Lk + dq, d=dq, dv=dv, scale=0.125))
    s = p.sets[0]
    q, v = flat(p.q).reshape(B * Lq, H * dq).contiguous(), flat(s.v).reshape(B * Lk, H * dv).contiguous()
    k = flat(s.k).reshape(B * Lk, H * dq).contiguous()
    if which == "pitch":
        wide = torch.zeros(B * Lk, H * dq + 4, dtype=dtype, device=DEV)
        wide[:, :H * dq] = k
        k = wide[:, :H * dq]
    lds = not (dq % 8 or dv % 8 or k.stride(0) % 8) and an.small_lds_bytes(Lk, dq, dv) <= 150 * 1024
    assert lds == (which == "lds"), f"{which}: the launch would take the {'LDS-resident' if lds else 'fallback'} kernel"
    twice(lambda: ctx.attention_small(q, k, v, B, H, Lq, Lk, dq, dv, p.scale), p, f"attention_small ({which})")


# ------------------------------------------------------------------------------------ ctx.attention_enc
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("packed", [True, False])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("B,H,L_,d", an.ENC)
def test_attention_enc_selects(L, dtype, packed, causal, B, H, L_, d):
    """imh_attention_enc / imh_attention_enc_causal at the entry's own scale d^-0.5, Q / K / V as three column ranges of one packed buffer
    or three tensors: the bidirectional form with groups across its 64-key tiles, the causal form with every fourth row's needle code
    repeated two keys later (past the diagonal for that row, inside the diagonal tile or in the tile after it)"""
    ctx = ctx_for(dtype)
    p = problem(an.causal_set(B, H, L_, d, dtype, seed=L_) if causal else an.single_set(B, H, L_, L_, L_, dtype, seed=L_, d=d, dv=d, scale=d ** -0.5))
    s = p.sets[0]
    w = H * d
    if packed:
        qkv = torch.cat([flat(p.q), flat(s.k), flat(s.v)], -1).reshape(B * L_, 3 * w).contiguous()
        q, k, v = qkv[:, :w], qkv[:, w:2 * w], qkv[:, 2 * w:]
    else:
        q, k, v = (flat(t).reshape(B * L_, w).contiguous() for t in (p.q, s.k, s.v))
    twice(lambda: ctx.attention_enc(q, k, v, B, H, L_, d, causal=causal), p, f"attention_enc causal={causal} packed={packed}")
