"""GPU tests of perturbed-attention guidance: the identity-attention form of IMH_EW_CONCAT (csrc/elementwise.hip identity_rows_kernel)
against the torch index expression, bit for bit; the three-term forms of the step and rescale launches against the float64 statement
of the formula, at the bounds their two-term forms are held to; the self-attention processor's split; the UNet forward and the
denoise loop against the oracle wrapped by tests/pag_reference.py; the pipeline switch."""
import functools
import itertools
import json
import os

import pytest
import torch

from conftest import PARITY_JSON, rel_rms
from oracle.detfill import det_randn

import pag_reference as PR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float16, torch.bfloat16]
U = 2.0 ** -24
PARITY = {}


def _name(dtype):
    return str(dtype).replace("torch.", "")


def _bits(t):
    return t.contiguous().view(torch.int16)


def _write_parity():
    try:
        out_dir = os.path.dirname(PARITY_JSON)          # beside the suite's measured-parity record; the committed copy is profiles/pag_parity.json
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "pag_parity.json"), "w") as f:
            json.dump(PARITY, f, indent=1, sort_keys=True)
    except OSError:
        pass


# ---------------------------------------------------------------------------------------------------- the copy
# (n, C, col0, ldvt, ld_out): one tile; a partial channel tile; the minimum; an offset, several tiles and slack columns on both sides of
# V^T; output rows wider than C
COPY_SHAPES = [(64, 64, 0, 64, 64), (64, 72, 0, 64, 72), (16, 8, 16, 48, 8), (192, 256, 128, 320, 256), (128, 64, 64, 192, 96)]


def _perm16(r):
    q = (r >> 2) & 3
    return (torch.where(q == 1, 2, torch.where(q == 2, 1, q)) << 2) | (r & 3)


@functools.lru_cache(maxsize=None)
def _copy_case(shape, dtype):
    """V^T with NaN in every column the launch must not read, and the torch index expression of the result: once per (shape, dtype)"""
    n, C, col0, ldvt, _ = shape
    vt = torch.full((C, ldvt), float("nan"), dtype=dtype)
    vt[:, col0:col0 + n] = det_randn((C, n), 51).to(dtype)
    r = torch.arange(n)
    ref = vt[:, col0 + 16 * (r // 16) + _perm16(r % 16)].t().contiguous()
    assert torch.isfinite(ref.float()).all()
    return vt, ref


def _copy_launch(ctx, vt, out, shape):
    n, C, col0, _, _ = shape
    return ctx.identity_rows(vt, out, n, col0, descr="self.pag_rows")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", COPY_SHAPES)
def test_identity_rows_equal_the_index_expression_bit_for_bit(dtype, shape):
    """y[r, c] = Vt[c, col0 + 16 (r / 16) + perm16(r % 16)]; the slack of y's rows (ld_out > C) keeps what it held; eager, recorded and
    replayed launches give the same bits; under guarded placement nothing outside the operands is touched and no NaN column is read"""
    from guarded import run_dense_and_guarded
    from imagharmony_amd import lib as L
    from imagharmony_amd.ctx import Ctx
    n, C, col0, ldvt, ldo = shape
    vt, ref = _copy_case(shape, dtype)
    vd = vt.to(DEV)
    ctx = Ctx(DEV, dtype)
    buf = torch.full((n, ldo), 7.0, dtype=dtype, device=DEV)
    _copy_launch(ctx, vd, buf[:, :C], shape)
    torch.cuda.synchronize()
    assert torch.equal(_bits(buf[:, :C].cpu()), _bits(ref)), "eager"
    assert bool((buf[:, C:] == 7.0).all()), "the slack columns of the output rows were written"
    rec = Ctx(DEV, dtype, record=True)
    out = torch.zeros(n, ldo, dtype=dtype, device=DEV)
    _copy_launch(rec, vd, out[:, :C], shape)
    assert [t[1] for t in rec.tags] == [L.OP_EW]
    rec.run()
    torch.cuda.synchronize()
    assert torch.equal(_bits(out[:, :C].cpu()), _bits(ref)), "recorded"
    out.zero_()
    rec.capture()
    rec.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(out[:, :C].cpu()), _bits(ref)) and bool((out[:, C:] == 0).all()), "replayed"

    def body(c, put, carve):
        y = carve((n, C), dtype, ld=ldo)
        _copy_launch(c, put(vd), y, shape)
        return y
    dense, guarded, arena = run_dense_and_guarded(DEV, dtype, body)
    arena.check()
    assert torch.equal(_bits(guarded[0].cpu()), _bits(ref)) and torch.equal(_bits(dense[0].cpu()), _bits(ref))


# ---------------------------------------------------------------------------------------------------- the step launches
S_, HW_, G_, PS_ = 2, 35, 4.0, 2.0          # HW % 4 != 0: seeded quads straddle channels; power-of-two scales: their products are exact
SEEDS, LANES, ROW = [42, 2 ** 63 + 5], [0, 3], 1


def _pred(dtype, cfg, seed):
    """[blocks * S, HW, 4] with exact zeros, u == c (the CFG term cancels), c == p (the PAG term cancels) and c - u == -(c - p) s / g
    patterns among random values"""
    g = torch.Generator().manual_seed(seed)
    nb = 3 if cfg else 2
    n = torch.randn(nb, S_, HW_, 4, generator=g).to(dtype)
    c, p = (1, 2) if cfg else (0, 1)
    n[:, :, 0] = 0                                   # exact zeros in every block
    n[p, :, 1] = n[c, :, 1]                          # perturbed == conditional
    n[c, :, 2, :2] = 0                               # zero conditional, non-zero perturbed
    if cfg:
        n[0, :, 3] = n[1, :, 3]                      # uncond == cond
        n[2, :, 4] = (n[1, :, 4].float() + (G_ / PS_) * (n[1, :, 4].float() - n[0, :, 4].float())).to(dtype)    # the two guidance terms (nearly) cancel
    return n.reshape(nb * S_, HW_, 4)


def _eps64(npred, cfg, g=G_, s=PS_):
    n = npred.double().view(-1, S_, HW_, 4).permute(0, 1, 3, 2)          # [blocks, S, 4, HW]
    if cfg:
        u, c, p = n[0], n[1], n[2]
        return (u + g * (c - u)) + s * (c - p), [u, g * c, g * u, s * c, s * p]
    c, p = n[0], n[1]
    return c + s * (c - p), [c, s * c, s * p]


def _step_case(dtype, op, cfg, blend, use_w, seed):
    """one three-term step launch -> (x', h' or None), their float64 references and per-element magnitudes (sum of |term|)"""
    from imagharmony_amd import lib as L
    from imagharmony_amd import noise
    from imagharmony_amd.ctx import Ctx
    ctx = Ctx(DEV, dtype)
    g = torch.Generator().manual_seed(1000 + seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    lat, h0, z, nz = rn(S_, 4, HW_), rn(S_, 4, HW_), rn(S_, 4, HW_), rn(S_, 4, HW_)
    lat[:, :, :3] = 0                                # exact zeros in the latents too
    npred = _pred(dtype, cfg, seed)
    wf = torch.tensor([0.8, 1.1])
    mask = (torch.rand(max(blend, 1), HW_, generator=g) > 0.5).float()
    btab = torch.full((4, 2), float("nan"))
    btab[ROW] = torch.tensor([0.6, 0.8])
    step = torch.full((1,), ROW, dtype=torch.int32, device=DEV)
    kw = dict(x2=z.to(DEV), noise=nz.to(DEV), mask=mask.to(DEV), blend_tab=btab.to(DEV)) if blend else {}
    common = dict(a=npred.to(DEV), w=wf.to(DEV) if use_w else None, step=step, i=(S_, HW_, 1, int(cfg), blend, 0), f=(0.0, 0.0, G_, PS_))
    y = lat.clone().to(DEV)
    eps, leaves = _eps64(npred, cfg)
    if use_w:
        eps, leaves = eps * wf.double()[:, None, None], [t * wf.double()[:, None, None] for t in leaves]
    hist = None
    if op == "step":
        tab = torch.full((4, 2), float("nan"))
        tab[ROW] = torch.tensor([0.9371, -0.3127])
        ctx.ew(L.EW_CFG_STEP, y, tab=tab.to(DEV), **common, **kw)
        c = tab[ROW].double()
        terms = [c[0] * lat.double()] + [c[1] * t for t in leaves]
        ref = c[0] * lat.double() + c[1] * eps
        href = hmag = None
    else:
        tab = torch.full((4, 6), float("nan"))
        tab[ROW] = torch.tensor([0.9, -0.3, 0.45, 0.7, 1.6, -1.2]) + 0.1 * rn(6)
        hist = h0.clone().to(DEV)
        if op == "bank":
            bank = torch.full((4, S_, 4, HW_), float("nan"))
            bank[ROW] = rn(S_, 4, HW_)
            zz = bank[ROW]
            ctx.ew(L.EW_CFG_MSTEP, y, tab=tab.to(DEV), hist=hist, bank=bank.to(DEV), **common, **kw)
        else:
            rows = torch.from_numpy(noise.seed_rows(SEEDS, LANES).view("int32")).to(DEV)
            zz = ctx.randn_seeded(rows, HW_, row=ROW, out=torch.empty(S_, 4, HW_, device=DEV)).cpu()
            ctx.ew(L.EW_CFG_MSTEP, y, tab=tab.to(DEV), hist=hist, seeds=rows, **common, **kw)
        c = tab[ROW].double()
        terms = [c[0] * lat.double()] + [c[1] * t for t in leaves] + [c[2] * h0.double(), c[3] * zz.double()]
        ref = c[0] * lat.double() + c[1] * eps + c[2] * h0.double() + c[3] * zz.double()
        href = c[4] * lat.double() + c[5] * eps
        hmag = (c[4] * lat.double()).abs() + sum((c[5] * t).abs() for t in leaves)
    mag = sum(t.abs() for t in terms)
    if blend:
        m = mask[torch.arange(S_) % blend][:, None, :].double().expand(S_, 4, HW_)
        bt = [btab[ROW, 0].double() * z.double(), btab[ROW, 1].double() * nz.double()]
        ref, mag = torch.where(m == 1, ref, sum(bt)), torch.where(m == 1, mag, sum(t.abs() for t in bt))
    torch.cuda.synchronize()
    return (y.cpu(), ref, mag), (None if hist is None else (hist.cpu(), href, hmag)), (lat, common, kw, tab, npred)


@pytest.mark.parametrize("op", ["step", "bank", "seeded"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_three_term_step_matches_the_float64_formula(dtype, op):
    """IMH_EW_CFG_STEP, IMH_EW_CFG_MSTEP with a bank and the seeded step with i2 = 1: with and without CFG (i3), blend and the w factor,
    S = 2, HW = 35.  eps = (u + g (c - u)) + s (c - p), or c + s (c - p), stated in float64 on the launch's own (rounded) inputs.  Per
    element |y - ref| <= 8 * 2^-24 * sum |term| over the terms of that element -- tests/test_gpu_multistep.py's bound of the two-term
    launch, with eps counted by its own terms since the reference no longer forms it in fp32 -- for x' and for h'."""
    worst = 0.0
    for k, (cfg, blend, use_w) in enumerate(itertools.product((1, 0), (0, 2), (False, True))):
        xs, hs, _ = _step_case(dtype, op, cfg, blend, use_w, seed=10 * k)
        for name, got in (("x'", xs), ("h'", hs)):
            if got is None:
                continue
            y, ref, mag = got
            what = f"{op} {_name(dtype)} cfg={cfg} blend={blend} w={use_w}: {name}"
            assert torch.isfinite(y).all(), what
            ratio = ((y.double() - ref).abs() / (8 * U * mag).clamp_min(1e-300)).max().item()
            worst = max(worst, ratio)
            assert ratio <= 1.0, f"{what}: error / bound = {ratio:.3f}"
    print(f"three-term {op} {_name(dtype)}: worst error / bound {worst:.3f}")
    PARITY[f"step_{op}_{_name(dtype)}"] = dict(worst_error_over_bound=worst)
    _write_parity()


@pytest.mark.parametrize("op", ["step", "bank", "seeded"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_perturbed_equal_to_conditional_gives_the_bits_of_the_two_block_launch(dtype, op):
    """p == c: s * (c - p) is an exact zero added to the two-term eps -- x' and h' of the launch without the third block, bit for bit;
    and the third block matters: another p changes the result"""
    from imagharmony_amd import lib as L
    from imagharmony_amd import noise
    from imagharmony_amd.ctx import Ctx
    ctx = Ctx(DEV, dtype)
    g = torch.Generator().manual_seed(77)
    for blend, use_w in itertools.product((0, 2), (False, True)):
        lat, h0, z, nz = (torch.randn(S_, 4, HW_, generator=g).to(DEV) for _ in range(4))
        two = torch.randn(2 * S_, HW_, 4, generator=g).to(dtype)
        three = torch.cat([two, two[S_:]], 0).to(DEV)
        other = torch.cat([two, torch.randn(S_, HW_, 4, generator=g).to(dtype)], 0).to(DEV)
        two = two.to(DEV)
        wf = torch.tensor([0.8, 1.1], device=DEV)
        mask = (torch.rand(max(blend, 1), HW_, generator=g) > 0.5).float().to(DEV)
        btab = torch.tensor([[0.3, 0.4], [0.6, 0.2]], device=DEV)
        step = torch.ones(1, dtype=torch.int32, device=DEV)
        kw = dict(x2=z, noise=nz, mask=mask, blend_tab=btab) if blend else {}
        rows = torch.from_numpy(noise.seed_rows(SEEDS, LANES).view("int32")).to(DEV)
        if op == "step":
            more = lambda: dict(tab=torch.tensor([[0.5, 0.1], [0.9371, -0.3127]], device=DEV))
            o = L.EW_CFG_STEP
        else:
            tab6 = torch.tensor([[0.0] * 6, [0.9, -0.3, 0.45, 0.7, 1.6, -1.2]], device=DEV)
            bank = torch.randn(2, S_, 4, HW_, generator=g).to(DEV)
            more = (lambda: dict(tab=tab6, hist=h0.clone(), bank=bank)) if op == "bank" else (lambda: dict(tab=tab6, hist=h0.clone(), seeds=rows))
            o = L.EW_CFG_MSTEP
        res = []
        for a, i2, f3 in ((two, 0, 0.0), (three, 1, 3.0), (other, 1, 3.0)):
            y, m = lat.clone(), more()
            ctx.ew(o, y, a=a, w=wf if use_w else None, step=step, i=(S_, HW_, i2, 1, blend, 0), f=(0.0, 0.0, 5.0, f3), **m, **kw)
            res.append((y, m.get("hist")))
        torch.cuda.synchronize()
        what = f"{op} {_name(dtype)} blend={blend} w={use_w}"
        assert torch.equal(res[0][0], res[1][0]) and not torch.equal(res[0][0], lat), what
        assert not torch.equal(res[2][0], res[0][0]), what + ": the third block is not read"
        if res[0][1] is not None:
            assert torch.equal(res[0][1], res[1][1]) and not torch.equal(res[2][1], res[0][1]), what + ": h'"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("HW", [1, 60, 1024])
def test_three_term_rescale_matches_std_in_float64(dtype, HW):
    """IMH_EW_CFG_RESCALE with the third block: phi * std(c) / std(eps) + 1 - phi with eps the three-term combination, torch.std in
    float64; relative 1e-5, the bound of the two-term launch (tests/test_gpu_guarded_ops.py test_ew_cfg_rescale)"""
    from imagharmony_amd import lib as L
    from test_gpu_guarded_ops import run
    S, gs_, ps, gr = 3, 5.0, 3.0, 0.7
    npred = det_randn((3 * S, HW, 4), 5).to(dtype).to(DEV)

    def body(ctx, put, out):
        return ctx.ew(L.EW_CFG_RESCALE, out((S,), torch.float32), a=put(npred), i=(S, HW, 1, 0, 0, 0), f=(ps, 0, gs_, gr))
    y = run(dtype, body, f"cfg_rescale three-term HW={HW}")[0]
    n = npred.double().cpu().view(3, S, HW * 4)
    eps = (n[0] + gs_ * (n[1] - n[0])) + ps * (n[1] - n[2])
    factor = gr * n[1].std(dim=1) / eps.std(dim=1) + (1 - gr)
    two = gr * n[1].std(dim=1) / (n[0] + gs_ * (n[1] - n[0])).std(dim=1) + (1 - gr)
    rel = ((y.double().cpu() - factor).abs() / factor.abs()).max().item()
    print(f"cfg_rescale three-term {_name(dtype)} HW={HW}: relative error {rel:.3e}")
    assert rel <= 1e-5, rel
    assert ((two - factor).abs() / factor.abs()).min().item() > 1e-3          # the two-term factor would not pass


# ---------------------------------------------------------------------------------------------------- the processor
PROC_TOL = {torch.float16: 1.5e-3, torch.bfloat16: 1.2e-2}          # tests/test_gpu_processors.py TOL


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L_", [64, 63], ids=["folded64", "ragged63"])
def test_processor_splits_the_batch(dtype, L_):
    """AttnProcessor2_0.emit at C = 256, 4 heads, B = 3, k = 1: L = 64 with the LayerNorm folded into the projections, L = 63 on the
    ragged path (x layer-normed beforehand).  The perturbed sample's rows are to_out(to_v(LN x)) + residual, the others softmax
    attention, each against its fp32 statement at tests/test_gpu_processors.py's bound; and the perturbed rows lie at least 3 x that bound
    from softmax attention on the same input, so a processor that ignores the split cannot pass."""
    import torch.nn.functional as F
    from imagharmony_amd.attention_processor import AttnProcessor2_0
    from imagharmony_amd.ctx import Ctx
    from imagharmony_amd.unet import Attention, Norm
    C, H, B, k = 256, 4, 3, 1
    attn, norm = Attention(C, H), Norm(C, 1e-5)
    with torch.no_grad():
        for i, lin in enumerate((attn.to_q, attn.to_k, attn.to_v, attn.to_out[0])):
            lin.weight.copy_(det_randn(tuple(lin.weight.shape), 60 + i) * (2.0 if i < 2 else 1.0) * C ** -0.5)
        attn.to_out[0].bias.copy_(det_randn((C,), 65) * 0.1)
        norm.weight.copy_(1 + 0.2 * det_randn((C,), 66))
        norm.bias.copy_(0.1 * det_randn((C,), 67))
    attn, norm = attn.to(DEV, dtype), norm.to(DEV, dtype)
    x = (det_randn((B * L_, C), 68) * 1.5 + 0.3).to(dtype)
    f = lambda t: t.detach().float().cpu()
    ln = F.layer_norm(x.float(), (C,), f(norm.weight), f(norm.bias), norm.eps)
    folded = L_ % 64 == 0
    xin = x if folded else ln.to(dtype)                      # the ragged path takes layer-normed rows
    lnf = ln if folded else xin.float()
    q, kk, v = (lnf @ f(w.weight).t() for w in (attn.to_q, attn.to_k, attn.to_v))
    heads = lambda t: t.view(B, L_, H, 64).transpose(1, 2)
    sm = F.scaled_dot_product_attention(heads(q), heads(kk), heads(v)).transpose(1, 2).reshape(B * L_, C)
    out_of = lambda ao: ao @ f(attn.to_out[0].weight).t() + f(attn.to_out[0].bias) + x.float()
    ref_sm, ref_id = out_of(sm), out_of(v)
    ctx = Ctx(DEV, dtype)
    xd = x.to(DEV)
    kw = dict(ln=norm) if folded else {}
    y = AttnProcessor2_0().emit(ctx, attn, xin.to(DEV), B, L_, residual=xd, pag=k, **kw)
    y = (y[0] if isinstance(y, tuple) else y).float().cpu()
    plain = AttnProcessor2_0().emit(ctx, attn, xin.to(DEV), B, L_, residual=xd, **kw)
    plain = (plain[0] if isinstance(plain, tuple) else plain).float().cpu()
    n = (B - k) * L_
    r_sm, r_id, gap = rel_rms(y[:n], ref_sm[:n]), rel_rms(y[n:], ref_id[n:]), rel_rms(ref_id[n:], ref_sm[n:])
    print(f"processor L={L_} {_name(dtype)}: softmax rows {r_sm:.3e}, identity rows {r_id:.3e} (bound {PROC_TOL[dtype]:g}); identity vs softmax {gap:.3e}")
    PARITY[f"processor_L{L_}_{_name(dtype)}"] = dict(softmax_rows=r_sm, identity_rows=r_id, bound=PROC_TOL[dtype], identity_vs_softmax=gap)
    _write_parity()
    assert gap >= 3 * PROC_TOL[dtype], gap
    assert torch.isfinite(y).all() and r_sm < PROC_TOL[dtype] and r_id < PROC_TOL[dtype], (r_sm, r_id)
    assert rel_rms(y[n:], ref_sm[n:]) >= 3 * PROC_TOL[dtype]                            # ... and so do the launch's rows
    assert torch.equal(y[:n], plain[:n])                                                 # the other samples: the plain launch's bits


# ---------------------------------------------------------------------------------------------------- the UNet
T_STEP = 500.0
UNET_SIZES = [(32, 32), (36, 28)]            # the mid block at 64 tokens (folded path) and at 63 (ragged path)


def _unet_inputs(ocfg, Hl, Wl):
    """batch [cond, perturbed]: the same sample twice, as the pipeline runs it"""
    x = det_randn((1, 4, Hl, Wl), 3).repeat(2, 1, 1, 1)
    ehs = det_randn((1, 81, ocfg.cross_attention_dim), 4).repeat(2, 1, 1)
    te = det_randn((1, ocfg.pooled_dim), 6).repeat(2, 1)
    ids = torch.tensor([[Hl * 8, Wl * 8, 0, 0, Hl * 8, Wl * 8]], dtype=torch.float32).repeat(2, 1)
    return x, ehs, te, ids


@functools.lru_cache(maxsize=None)
def _oracle_forward(Hl, Wl, layers):
    """(oracle with the identity processors on `layers`, plain oracle) on test_gpu_unet's tiny pair, CPU fp32, once"""
    from test_gpu_unet import build_pair
    ou, _, ocfg = build_pair(torch.bfloat16)                       # (the oracle half does not depend on the dtype)
    x, ehs, te, ids = _unet_inputs(ocfg, Hl, Wl)
    added = {"text_embeds": te, "time_ids": ids}
    with torch.no_grad():
        plain = ou(x, torch.tensor(T_STEP), ehs, added_cond_kwargs=added)[0]
        with PR.oracle_pag(ou, layers, 1):
            pag = ou(x, torch.tensor(T_STEP), ehs, added_cond_kwargs=added)[0]
        assert torch.equal(plain, ou(x, torch.tensor(T_STEP), ehs, added_cond_kwargs=added)[0])      # the wrapper left the oracle as it was
    assert torch.equal(pag[:1], plain[:1])                         # the unperturbed sample of the batch is the plain oracle's, bit for bit
    return pag, plain


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layers", ["mid", "."])
@pytest.mark.parametrize("Hl,Wl", UNET_SIZES)
def test_unet_forward_with_perturbed_sample_matches_the_wrapped_oracle(dtype, layers, Hl, Wl):
    """tiny UNet, batch [cond, perturbed], test_gpu_unet.py's bounds (rel-RMS 6e-3 in fp16, 3e-2 in bf16).  The test can fail: in the
    oracle, identity attention moves the perturbed sample's prediction by 0.157 / 0.168 rel-RMS ("mid", 32 x 32 / 36 x 28) and 0.70 /
    0.74 (".") -- at least 5 x the bf16 bound, asserted.  The recorded plan gives the eager forward's bits."""
    from imagharmony_amd.ctx import Ctx
    from test_gpu_unet import TOL, build_pair
    ref, ref_plain = _oracle_forward(Hl, Wl, layers)
    vis = rel_rms(ref[1:], ref_plain[1:])
    assert vis >= 5 * TOL[torch.bfloat16], f"identity attention in {layers!r} moves the oracle's prediction by {vis:.3e} only"
    _, hu, ocfg = build_pair(dtype)
    x, ehs, te, ids = _unet_inputs(ocfg, Hl, Wl)
    added = {"text_embeds": te.to(DEV, dtype), "time_ids": ids.to(DEV)}
    try:
        hu.set_pag_applied_layers(layers)
        y = hu(x.to(DEV), torch.tensor(T_STEP), ehs.to(DEV, dtype), added_cond_kwargs=added, pag=1)[0]
        y_off = hu(x.to(DEV), torch.tensor(T_STEP), ehs.to(DEV, dtype), added_cond_kwargs=added)[0]
        pre = Ctx(DEV, dtype)
        st = hu.prepare_conditioning(pre, ehs.to(DEV, dtype), te.to(DEV, dtype), ids.to(DEV))
        st.t_value = torch.full((2,), T_STEP, device=DEV)
        st.latents = x.to(DEV).float().contiguous()
        rec = Ctx(DEV, dtype, record=True)
        out = hu.emit_forward(rec, st, 2, Hl, Wl, cfg_dup=False, pag=1, batch=2)
        rec.run()
        torch.cuda.synchronize()
        y_plan = out.view(2, Hl, Wl, 4).permute(0, 3, 1, 2).clone()
        out.zero_()
        rec.capture()
        rec.replay()
        torch.cuda.synchronize()
        y_replay = out.view(2, Hl, Wl, 4).permute(0, 3, 1, 2)
        assert torch.equal(y_plan, y) and torch.equal(y_replay, y)
    finally:
        hu.set_pag_applied_layers(None)
    yf = y.float().cpu()
    r_all, r_pert, r_off = rel_rms(yf, ref), rel_rms(yf[1:], ref[1:]), rel_rms(y_off.float().cpu(), ref_plain)
    print(f"unet tiny {Hl}x{Wl} {layers!r} {_name(dtype)}: rel-rms {r_all:.3e} (perturbed sample {r_pert:.3e}, PAG off {r_off:.3e}; bound {TOL[dtype]:.0e}); "
          f"identity attention moves the oracle by {vis:.3e}")
    PARITY[f"unet_tiny_{Hl}x{Wl}_{'all' if layers == '.' else layers}_{_name(dtype)}"] = dict(rel_rms=r_all, perturbed_sample=r_pert, pag_off=r_off,
                                                                                             bound=TOL[dtype], visibility=vis)
    _write_parity()
    assert torch.isfinite(yf).all() and r_all < TOL[dtype] and r_pert < TOL[dtype], (r_all, r_pert)
    assert r_off < TOL[dtype]
    assert torch.equal(y[:1], y_off[:1])                           # the unperturbed sample is the plain forward's, bit for bit


# ---------------------------------------------------------------------------------------------------- the loop
LOOP_BOUND = 4e-2            # tests/test_gpu_pipeline.py: the 3-step bf16 trajectory without PAG
STEPS = 3


def _loop_inputs(ocfg):
    cd = ocfg.cross_attention_dim
    return (det_randn((1, 4, 32, 32), 3), det_randn((1, 81, cd), 4), det_randn((1, 81, cd), 5), det_randn((1, ocfg.pooled_dim), 6),
            det_randn((1, ocfg.pooled_dim), 7))


def _oracle_scheduler(sched):
    if sched == "ddim":
        from oracle.schedulers import DDIMScheduler
        return DDIMScheduler()
    from multistep_reference import RefDPMSolverMultistep
    return RefDPMSolverMultistep()


@functools.lru_cache(maxsize=None)
def _oracle_loop(sched, guidance, pag_scale):
    """the fp32 reference trajectory, once: the helper's PAG loop, or oracle.pipeline.denoise with PAG off"""
    from oracle.pipeline import denoise as oracle_denoise
    ou, _, ocfg = _loop_pair()
    lat, pe, ne, po, no = _loop_inputs(ocfg)
    with torch.no_grad():
        if pag_scale:
            return PR.denoise_pag(ou, _oracle_scheduler(sched), lat, pe, ne, po, no, 256, 256, num_inference_steps=STEPS, guidance_scale=guidance,
                                  pag_scale=pag_scale, layers="mid")
        return oracle_denoise(ou, _oracle_scheduler(sched), lat, pe, ne, po, no, 256, 256, num_inference_steps=STEPS, guidance_scale=guidance)


@functools.lru_cache(maxsize=None)
def _loop_pair():
    from smoke_impl import build_pair
    return build_pair(DEV, torch.bfloat16)


def _product_loop(sched, guidance, pag_scale, graph):
    from imagharmony_amd import schedulers as hs
    from imagharmony_amd.pipeline import StableDiffusionXLCustomPipeline
    _, hu, ocfg = _loop_pair()
    lat, pe, ne, po, no = _loop_inputs(ocfg)
    pipe = StableDiffusionXLCustomPipeline(hu, scheduler=hs.DDIMScheduler() if sched == "ddim" else hs.DPMSolverMultistepScheduler(), device=DEV,
                                           dtype=torch.bfloat16, use_graph=graph)
    try:
        pipe.set_pag_applied_layers("mid")
        out = pipe(prompt_embeds=pe, negative_prompt_embeds=ne, pooled_prompt_embeds=po, negative_pooled_prompt_embeds=no, height=256, width=256,
                   num_inference_steps=STEPS, guidance_scale=guidance, latents=lat, output_type="latent", pag_scale=pag_scale).images.float().cpu()
    finally:
        pipe.set_pag_applied_layers(None)
    return out, pipe


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("sched,guidance", [("ddim", 5.0), ("dpmpp2m", 5.0), ("ddim", 1.0)], ids=["ddim-cfg5", "dpmpp2m-cfg5", "ddim-nocfg"])
def test_denoise_loop_with_pag_matches_the_restated_loop(sched, guidance, graph):
    """3 steps, bf16, PAG 3 in the mid block: DDIM (IMH_EW_CFG_STEP), DPM-Solver++ 2M (the general step) and the no-CFG form, with the
    graph and without, against tests/pag_reference.denoise_pag at the bound of the same loop without PAG (4e-2).  The test can fail:
    the reference with PAG lies further than that bound from the reference without, asserted first, and so does the result from the
    PAG-off run."""
    ref, ref_off = _oracle_loop(sched, guidance, 3.0), _oracle_loop(sched, guidance, 0.0)
    vis = rel_rms(ref, ref_off)
    assert vis > LOOP_BOUND, f"PAG moves the reference trajectory by {vis:.3e} only"
    out, pipe = _product_loop(sched, guidance, 3.0, graph)
    eng = pipe.engine
    descr = [t[2] for t in eng.plan.tags]
    cfg = guidance > 1.0
    assert eng.pag and eng.noise_pred.shape[0] == (3 if cfg else 2) and descr.count("self.pag_rows") == 2
    assert descr[-2:] == ["cfg+step+pag" if sched == "ddim" else "cfg+mstep+pag", "step++"]
    off, _ = _product_loop(sched, guidance, 0.0, graph)
    r, r_off, moved = rel_rms(out, ref), rel_rms(off, ref_off), rel_rms(out, off)
    name = f"loop_{sched}_{'cfg5' if cfg else 'nocfg'}_{'graph' if graph else 'eager'}"
    print(f"{name}: rel-rms {r:.3e} (PAG off {r_off:.3e}; bound {LOOP_BOUND:g}); PAG moves the reference by {vis:.3e}, the result by {moved:.3e}")
    PARITY[name] = dict(rel_rms=r, pag_off=r_off, bound=LOOP_BOUND, visibility_reference=vis, visibility_result=moved)
    _write_parity()
    assert torch.isfinite(out).all() and r < LOOP_BOUND, r
    assert r_off < LOOP_BOUND and moved > LOOP_BOUND


def test_denoise_loop_with_pag_and_guidance_rescale():
    """guidance_rescale under PAG: the rescale launch and the step both read the third block (rescale_noise_cfg of the three-term sum)"""
    from imagharmony_amd import schedulers as hs
    from imagharmony_amd.pipeline import StableDiffusionXLCustomPipeline
    ou, hu, ocfg = _loop_pair()
    lat, pe, ne, po, no = _loop_inputs(ocfg)
    with torch.no_grad():
        from oracle.schedulers import DDIMScheduler
        ref = PR.denoise_pag(ou, DDIMScheduler(), lat, pe, ne, po, no, 256, 256, num_inference_steps=STEPS, guidance_scale=7.0, pag_scale=3.0,
                             layers="mid", guidance_rescale=0.7)
    pipe = StableDiffusionXLCustomPipeline(hu, scheduler=hs.DDIMScheduler(), device=DEV, dtype=torch.bfloat16)
    try:
        pipe.set_pag_applied_layers("mid")
        out = pipe(prompt_embeds=pe, negative_prompt_embeds=ne, pooled_prompt_embeds=po, negative_pooled_prompt_embeds=no, height=256, width=256,
                   num_inference_steps=STEPS, guidance_scale=7.0, guidance_rescale=0.7, latents=lat, output_type="latent",
                   pag_scale=3.0).images.float().cpu()
    finally:
        pipe.set_pag_applied_layers(None)
    descr = [t[2] for t in pipe.engine.plan.tags]
    r = rel_rms(out, ref)
    print(f"loop ddim cfg7 rescale 0.7 PAG 3: rel-rms {r:.3e} (bound {LOOP_BOUND:g})")
    PARITY["loop_ddim_cfg7_rescale"] = dict(rel_rms=r, bound=LOOP_BOUND)
    _write_parity()
    assert descr[-3:] == ["cfg.rescale", "cfg+step+pag", "step++"]
    assert torch.isfinite(out).all() and r < LOOP_BOUND, r


# ---------------------------------------------------------------------------------------------------- the pipelines
def test_pipeline_switch_records_one_plan_and_switching_back_none():
    from imagharmony_amd.pipeline import StableDiffusionXLCustomPipeline
    _, hu, ocfg = _loop_pair()
    lat, pe, ne, po, no = _loop_inputs(ocfg)
    pipe = StableDiffusionXLCustomPipeline(hu, device=DEV, dtype=torch.bfloat16)
    eng = pipe.engine
    count = [0]
    record = eng._record

    def counted():
        count[0] += 1
        return record()
    eng._record = counted
    kw = dict(prompt_embeds=pe.to(DEV), negative_prompt_embeds=ne.to(DEV), pooled_prompt_embeds=po.to(DEV), negative_pooled_prompt_embeds=no.to(DEV),
              height=256, width=256, num_inference_steps=STEPS, output_type="latent", return_dict=False)
    try:
        plain = pipe(latents=lat.clone(), **kw)[0].clone()
        assert count[0] == 1 and len(eng._plans) == 1
        pipe.set_pag_applied_layers("mid")
        zero = pipe(latents=lat.clone(), pag_scale=0.0, **kw)[0].clone()              # layers set, scale 0: the call it was, bit for bit
        assert torch.equal(zero, plain) and not eng.pag and eng._sched_key.pag is None and len(eng._sched_key) == 13 and len(eng._plans) == 1
        n0 = count[0]
        on = pipe(latents=lat.clone(), pag_scale=3.0, **kw)[0].clone()
        assert count[0] == n0 + 1 and eng.pag and eng._sched_key.pag is not None and len(eng._plans) == 1
        assert sum(t[2] == "self.pag_rows" for t in eng.plan.tags) == 2
        back = pipe(latents=lat.clone(), **kw)[0].clone()                              # PAG off again: the earlier conditioning and plan
        assert count[0] == n0 + 1 and not eng.pag and not any(t[2] == "self.pag_rows" for t in eng.plan.tags)
        again = pipe(latents=lat.clone(), pag_scale=3.0, **kw)[0].clone()
        assert count[0] == n0 + 1 and eng.pag
        pipe.set_pag_applied_layers(None)
        none = pipe(latents=lat.clone(), pag_scale=3.0, **kw)[0].clone()               # a scale without layers: the call it was
    finally:
        pipe.set_pag_applied_layers(None)
    assert torch.isfinite(on).all() and not torch.equal(on, plain)
    assert torch.equal(back, plain) and torch.equal(again, on) and torch.equal(none, plain)


@pytest.mark.parametrize("mode", ["img2img", "inpaint"])
def test_edit_pipelines_run_with_pag(mode):
    """image-to-image, and inpainting through the 4-channel blend, with PAG: finite latents that differ from the PAG-off result; the
    blend invariant holds for the three-block step too (outside the mask: the image latents themselves)"""
    from imagharmony_amd import schedulers as hs
    from imagharmony_amd.pipeline import StableDiffusionXLImg2ImgCustomPipeline, StableDiffusionXLInpaintCustomPipeline
    from test_gpu_inpaint import IMG, build_pair, build_vae_pair, centred_mask, embeds
    dtype = torch.bfloat16
    _, hu, ocfg = build_pair(dtype, 4)
    _, hv = build_vae_pair()
    emb = embeds(ocfg, 1)
    cls = StableDiffusionXLImg2ImgCustomPipeline if mode == "img2img" else StableDiffusionXLInpaintCustomPipeline
    pipe = cls(hu, scheduler=hs.DDIMScheduler(), device=DEV, dtype=dtype, vae=hv)
    kw = dict(image=IMG(), strength=0.75, num_inference_steps=4, guidance_scale=5.0, output_type="latent", **emb)
    if mode == "inpaint":
        kw["mask_image"] = centred_mask(256, 256)
    gen = lambda: torch.Generator().manual_seed(11)
    try:
        off = pipe(generator=gen(), **kw).images.float().cpu()
        pipe.set_pag_applied_layers("mid")
        on = pipe(generator=gen(), pag_scale=3.0, **kw).images.float().cpu()
        descr = [t[2] for t in pipe.engine.plan.tags]
    finally:
        pipe.set_pag_applied_layers(None)
    assert descr[-2:] == ["cfg+step+pag" + ("+blend" if mode == "inpaint" else ""), "step++"] and descr.count("self.pag_rows") == 2
    assert torch.isfinite(on).all() and on.shape == off.shape and rel_rms(on, off) > 1e-2
    if mode == "inpaint":
        m = torch.nn.functional.interpolate(centred_mask(256, 256), size=(32, 32)).expand_as(on)
        assert torch.equal(on[m == 0], off[m == 0])             # outside the mask both end on the image latents
