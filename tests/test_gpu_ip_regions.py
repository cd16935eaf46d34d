"""GPU: the kernel of regional image prompts (csrc/xattn_regions.hip, include/imh_regions.h) called directly through Ctx, with K / V caches
from project_kv.  C = 128, H = 2, both dtypes.  Properties that need no measured number come first (the bits of today's launch, zero
masks, disjoint masks row by row, the image-to-batch mapping), then parity against the fp32 restatement (tests/ip_regions_reference.py)
at the processor's bound, guarded placement, the dispatch contract and the refusals."""
import ctypes as C
import json
import os

import pytest
import torch

import ip_regions_cases as rc
from conftest import PARITY_JSON, rel_rms
from guarded import run_dense_and_guarded
from ip_regions_cases import C_, CD, H, SCALE, TOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float16, torch.bfloat16]
PARITY = {}


def _bits(t):
    return t.contiguous().view(torch.int16)


class Prep:
    """the operands of one problem on the device: token rows, to_q, the text caches and the image caches (image i of batch b at key
    (b * N + i) * lk2_pad: the image tokens projected as a batch of B * N)"""

    def __init__(self, inp, dtype, ctx=None):
        from imagharmony_amd.attention_processor import project_kv
        from imagharmony_amd.ctx import Ctx
        self.ctx = ctx or Ctx(DEV, dtype)
        d = lambda t: t.to(DEV, dtype).contiguous()
        self.B, self.Lq, self.T, self.N, self.dtype = inp["B"], inp["Lq"], inp["T"], inp["N"], dtype
        self.x, self.wq = d(inp["x"]), d(inp["wq"])
        k, self.vt, self.lk, self.lkp = project_kv(self.ctx, d(inp["text"]), d(inp["wk"]), d(inp["wv"]))
        self.k = k.view(-1, C_)
        ip = d(inp["ip"]).reshape(self.B * self.N, self.T, CD)
        k2, self.vt2, self.lk2, self.lk2p = project_kv(self.ctx, ip, d(inp["wk_ip"]), d(inp["wv_ip"]))
        self.k2 = k2.view(-1, C_)

    def image(self, i):
        """the caches of image i alone, as a batch of B: what today's launch takes"""
        B, N, P = self.B, self.N, self.lk2p
        return (self.k2.view(B, N, P, C_)[:, i].reshape(B * P, C_).contiguous(), self.vt2.view(C_, B, N, P)[:, :, i].reshape(C_, B * P).contiguous())

    def regions(self, rows, weights=None, ctx=None, ln=None, wq=None, **kw):
        ctx = ctx or self.ctx
        out = torch.zeros(self.B * self.Lq, C_, dtype=self.dtype, device=DEV)
        w = None if weights is None else torch.tensor(list(weights), dtype=torch.float32, device=DEV)
        ctx.cross_attention_regions(self.x, self.wq if wq is None else wq, self.k, self.vt, out, self.B, H, self.Lq, self.lk, self.lkp, C_,
                                    self.B * self.lkp, 0.125, self.k2, self.vt2, self.lk2, self.lk2p, C_, self.B * self.N * self.lk2p, self.N,
                                    rows.to(DEV).contiguous(), weights=w, ln=ln, **{"scale2": SCALE, **kw})
        return out

    def plain(self, i=None, ln=None, wq=None, **kw):
        """today's launch (csrc/xattn.hip): the text keys and, i given, image i"""
        out = torch.zeros(self.B * self.Lq, C_, dtype=self.dtype, device=DEV)
        if i is not None:
            k2, vt2 = self.image(i)
            kw = dict(k2=k2, vt2=vt2, Lk2=self.lk2, Lk2_pad=self.lk2p, ldk2=C_, ldvt2=self.B * self.lk2p, **{"scale2": SCALE, **kw})
        self.ctx.cross_attention(self.x, self.wq if wq is None else wq, self.k, self.vt, out, self.B, H, self.Lq, self.lk, self.lkp, C_,
                                 self.B * self.lkp, 0.125, ln=ln, **kw)
        return out


def _ones(N, Lq):
    return torch.ones(N, Lq)


# ---------------------------------------------------------------------------------------------------- the bits of today's launch
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,Lq,T", [(2, 60, 4), (2, 144, 16), (2, 128, 33)])
def test_one_image_all_ones_is_todays_launch_bit_for_bit(B, Lq, T, dtype):
    """N = 1, mask ones, weight 1 (given, or NULL): the bits of imh_cross_attention with K2 -- the arithmetic order is pinned.  T = 33 is
    the first size at which both 32-key sub-tiles of an image tile are live.  With and without the folded LayerNorm."""
    from imagharmony_amd.attention_processor import fold_ln
    p = Prep(rc.inputs(B, Lq, T, 1, seed=3), dtype)
    want = p.plain(0)
    assert torch.isfinite(want).all() and want.abs().max() > 0
    for weights in (None, (1.0,)):
        assert torch.equal(_bits(p.regions(_ones(1, Lq), weights)), _bits(want))
    assert not torch.equal(_bits(p.regions(_ones(1, Lq), (0.5,))), _bits(want))
    norm = torch.nn.LayerNorm(C_, eps=1e-5)
    with torch.no_grad():
        norm.weight.copy_(1 + 0.2 * torch.randn(C_, generator=torch.Generator().manual_seed(3)))
        norm.bias.copy_(0.3 * torch.randn(C_, generator=torch.Generator().manual_seed(4)))
    wg, s_, c_ = fold_ln(rc.inputs(B, Lq, T, 1, seed=3)["wq"], norm, p.ctx)
    want_ln = p.plain(0, ln=(s_, c_, 1e-5, None), wq=wg)
    assert torch.equal(_bits(p.regions(_ones(1, Lq), ln=(s_, c_, 1e-5, None), wq=wg)), _bits(want_ln)) and not torch.equal(_bits(want_ln), _bits(want))
    # the per-step gate: row *step of the table in place of scale2
    tab, step = torch.tensor([0.3, SCALE, 0.5], device=DEV), torch.tensor([1], dtype=torch.int32, device=DEV)
    assert torch.equal(_bits(p.regions(_ones(1, Lq), scale2=0.0, scale2_tab=tab, step=step)), _bits(want))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [1, 3])
def test_zero_mask_or_zero_gate_row_is_the_text_only_launch(N, dtype):
    Lq = 144
    p = Prep(rc.inputs(2, Lq, 4, N, seed=5), dtype)
    text_only = p.plain()
    assert torch.equal(_bits(p.regions(torch.zeros(N, Lq))), _bits(text_only))
    tab, step = torch.tensor([1.0, 0.0, 0.5], device=DEV), torch.tensor([1], dtype=torch.int32, device=DEV)
    assert torch.equal(_bits(p.regions(_ones(N, Lq), scale2_tab=tab, step=step)), _bits(text_only))
    step.fill_(2)
    assert not torch.equal(_bits(p.regions(_ones(N, Lq), scale2_tab=tab, step=step)), _bits(text_only))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,Lq,N", [(2, 60, 2), (2, 144, 2), (2, 9216, 2), (2, 60, 3)])
def test_disjoint_masks_select_one_image_per_row(B, Lq, N, dtype):
    """complementary 0 / 1 masks drawn per token: every output row has the bits of the N = 1 run of the image whose mask is 1 there.
    Lq 144 = a block plus a 16-row tail; B 2, H 2, Lq 9216 = 288 items, 36 per XCD, hence four half items with qoff = 64: a wrong
    row-to-lane or q0 mapping of the mask read shows as a row taken from the wrong image."""
    p = Prep(rc.inputs(B, Lq, 4, N, seed=7), dtype)
    pick = torch.randint(0, N, (Lq,), generator=torch.Generator().manual_seed(11))
    rows = torch.stack([(pick == i).float() for i in range(N)])
    y = p.regions(rows).view(B, Lq, C_)
    singles = [p.plain(i).view(B, Lq, C_) for i in range(N)]
    assert not torch.equal(_bits(singles[0]), _bits(singles[1]))
    for i in range(N):
        sel = (pick == i).to(DEV)
        assert int(sel.sum()) > 0
        bad = (_bits(y[:, sel]) != _bits(singles[i][:, sel])).any(-1)
        assert not bool(bad.any()), f"image {i}: {int(bad.sum())} of {bad.numel()} rows differ from its own N = 1 run"


@pytest.mark.parametrize("dtype", DTYPES)
def test_image_to_batch_mapping(dtype):
    """B = 4, N = 2: swapping the two images' tokens under the same masks is visible; swapping tokens and masks together matches the
    reference of the swapped problem"""
    B, grid, T, N = 4, (6, 10), 4, 2
    Lq = grid[0] * grid[1]
    inp = rc.inputs(B, Lq, T, N, seed=9)
    rows, weights = rc.soft_rows(N, grid), (1.0, 0.5)
    sw = dict(inp, ip=torch.cat([inp["ip"][:, T:], inp["ip"][:, :T]], 1))
    y = Prep(inp, dtype).regions(rows, weights).float().cpu()
    y_sw = Prep(sw, dtype).regions(rows, weights).float().cpu()
    y_both = Prep(sw, dtype).regions(rows.flip(0), weights[::-1]).float().cpu()
    with torch.no_grad():
        ref, ref_sw, ref_both = rc.reference(inp, rows, weights), rc.reference(sw, rows, weights), rc.reference(sw, rows.flip(0), weights[::-1])
    assert rel_rms(y, ref) < TOL[dtype] and rel_rms(y_sw, ref_sw) < TOL[dtype] and rel_rms(y_both, ref_both) < TOL[dtype]
    assert rel_rms(y_sw, ref) > TOL[dtype] and rel_rms(y_sw, y) > TOL[dtype]
    assert rel_rms(y_both, y) < 2 * TOL[dtype]          # the swapped problem is the same picture


# ---------------------------------------------------------------------------------------------------- parity
def _write_parity():
    try:
        out_dir = os.path.dirname(PARITY_JSON)          # beside the suite's measured-parity record; the kept copy is profiles/ip_regions_parity.json
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "ip_regions_parity.json"), "w") as f:
            json.dump(PARITY, f, indent=1, sort_keys=True)
    except OSError:
        pass


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(rc.PARITY))
def test_parity_against_the_restatement(name, dtype):
    """soft (bicubic) masks, weights (1.0, 0.5, ...), N in {1, 2, 4}: rel-RMS under the processor's bound; the masks move the reference by
    at least 5 x that bound against the unmasked sum, so a kernel that ignores them cannot pass"""
    inp, rows, weights = rc.parity_case(name)
    with torch.no_grad():
        ref, unmasked = rc.reference(inp, rows, weights), rc.reference(inp, torch.ones_like(rows), weights)
    vis = rel_rms(ref, unmasked)
    assert vis >= 5 * TOL[dtype], f"the masks move the reference by {vis:.3e} only"
    y = Prep(inp, dtype).regions(rows, weights).float().cpu()
    r = rel_rms(y, ref)
    print(f"{name} {dtype}: rel-rms {r:.3e} (bound {TOL[dtype]:.1e}); the masks move the reference by {vis:.3e}")
    PARITY[f"{name}.{str(dtype).replace('torch.', '')}"] = dict(value=r, bound=TOL[dtype], mask_visibility=vis)
    _write_parity()
    assert torch.isfinite(y).all() and r < TOL[dtype], r


# ---------------------------------------------------------------------------------------------------- guarded placement
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,grid,T,N,ldm_extra", [(2, (6, 10), 4, 2, 0), (2, (6, 10), 4, 2, 20), (1, (12, 12), 33, 3, 7)])
def test_guarded_placement(B, grid, T, N, ldm_extra, dtype):
    """every operand between guard bands, every leading dimension wider than the row, the mask rows with ldm == Lq and with ldm > Lq:
    the same bits as the dense run, nothing outside the contract touched, nothing outside an operand read into a result"""
    Lq = grid[0] * grid[1]
    inp = rc.inputs(B, Lq, T, N, seed=13)
    rows, weights = rc.soft_rows(N, grid), tuple(1.0 - 0.25 * i for i in range(N))
    src = Prep(inp, dtype)
    wts = torch.tensor(weights, dtype=torch.float32, device=DEV)

    def body(ctx, put, out):
        k, vt = put(src.k, ld=C_ + 64), put(src.vt, ld=src.vt.shape[1] + 16)
        k2, vt2 = put(src.k2, ld=C_ + 64), put(src.vt2, ld=src.vt2.shape[1] + 16)
        o = out((B * Lq, C_), dtype, ld=C_ + 64)
        ctx.cross_attention_regions(put(src.x, ld=C_ + 64), put(src.wq, ld=C_ + 8), k, vt, o, B, H, Lq, src.lk, src.lkp, k.stride(0), vt.stride(0), 0.125,
                                    k2, vt2, src.lk2, src.lk2p, k2.stride(0), vt2.stride(0), N, put(rows.to(DEV), ld=Lq + ldm_extra), weights=put(wts),
                                    scale2=SCALE)
        return o
    dense, guarded, arena = run_dense_and_guarded(DEV, dtype, body)
    arena.check()
    assert torch.equal(_bits(dense[0]), _bits(guarded[0]))
    with torch.no_grad():
        assert rel_rms(dense[0].float().cpu(), rc.reference(inp, rows, weights)) < TOL[dtype]


# ---------------------------------------------------------------------------------------------------- dispatch contract, refusals
def _args(src, out, rows, wts, N):
    """a filled imh_xattn_regions_args over real tensors: what the recorder builds for a good call"""
    from imagharmony_amd import lib as L
    a = L.XAttnRegionsArgs()
    a.X, a.Wq, a.K, a.Vt, a.K2, a.Vt2, a.O = (t.data_ptr() for t in (src.x, src.wq, src.k, src.vt, src.k2, src.vt2, out))
    a.B, a.H, a.Lq, a.C, a.Lk, a.Lk_pad, a.Lk2, a.Lk2_pad = src.B, H, src.Lq, C_, src.lk, src.lkp, src.lk2, src.lk2p
    a.ldx = a.ldw = a.ldk = a.ldk2 = a.ldo = C_
    a.ldvt, a.ldvt2 = src.vt.stride(0), src.vt2.stride(0)
    a.scale, a.scale2, a.dtype = 0.125, SCALE, L.IMH_DT_BF16 if src.dtype == torch.bfloat16 else L.IMH_DT_F16
    a.n_img, a.mask, a.ldm, a.weights = N, rows.data_ptr(), rows.stride(0), wts.data_ptr()
    return a


# (field changes, the status the header promises); None: a good call
MATRIX = [({}, 0), (dict(weights=None), 0), (dict(n_img=1), 0), (dict(mask=None), -1), (dict(K2=None), -1), (dict(Vt2=None), -1), (dict(O=None), -1),
          (dict(mask="+2"), -1), (dict(weights="+1"), -1), (dict(scale2_tab="tab"), -1), (dict(step="step"), -1), (dict(scale2_tab="tab", step="step"), 0),
          (dict(ln_s="tab"), -1), (dict(n_img=0), -2), (dict(n_img=9), -2), (dict(ldm=59), -2), (dict(Lk2=0), -2), (dict(Lk2_pad=96), -2),
          (dict(Lk2=65), -2), (dict(C=192), -2), (dict(Lk_pad=100), -2), (dict(Lk=0), -2), (dict(ldo=C_ + 4), -2), (dict(B=0), -2), (dict(dtype=7), -3)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_dispatch_contract_and_refusals(dtype):
    """over good and bad argument sets: Ctx.regions_refusal approves exactly what the library accepts, every refusal returns the status
    of include/imh_regions.h and launches nothing (the output keeps its sentinel), and a refused recording leaves the plan empty"""
    from imagharmony_amd import lib as L
    from imagharmony_amd.ctx import Ctx
    B, Lq, T, N = 2, 60, 4, 2
    # the caches hold room for nine images, so that no argument set of the matrix could reach past an operand if it were launched
    src = Prep(rc.inputs(B, Lq, T, 9, seed=17), dtype)
    rows = torch.rand(9, Lq + 8, device=DEV)
    wts = torch.ones(9, device=DEV)
    tab, step = torch.tensor([1.0, 0.5], device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    lib = L.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for change, status in MATRIX:
        out = torch.full((B * Lq, C_), 7.0, dtype=dtype, device=DEV)
        a = _args(src, out, rows, wts, N)
        for k, v in change.items():          # "tab" / "step": that tensor's address; "+n": the pointer moved by n bytes
            if v in ("tab", "step"):
                v = (tab if v == "tab" else step).data_ptr()
            elif isinstance(v, str):
                v = getattr(a, k) + int(v)
            setattr(a, k, v)
        why = Ctx.regions_refusal(a)
        rc_ = lib.imh_cross_attention_regions(C.byref(a), stream)
        torch.cuda.synchronize()
        assert rc_ == status, f"{change}: status {rc_}, the header says {status} ({lib.imh_last_error().decode()})"
        assert (why is None) == (rc_ == 0), f"{change}: Ctx says {why!r}, the library returned {rc_}"
        if status:
            assert bool((out == 7.0).all()), f"{change}: refused, but the output was written"
        else:
            assert torch.isfinite(out).all() and not bool((out == 7.0).all())
    # the recorder itself: eager and recording, a refusal raises at the call, writes nothing and records nothing
    good = Prep(rc.inputs(B, Lq, T, N, seed=17), dtype)
    for record in (False, True):
        ctx = Ctx(DEV, dtype, record=record)
        for bad in (dict(rows=torch.ones(N, Lq - 1)), dict(rows=torch.ones(N + 1, Lq)), dict(weights=(1.0,)), dict(rows=torch.ones(N, Lq), scale2_tab=tab)):
            with pytest.raises(L.ImhError):
                good.regions(bad.pop("rows", torch.ones(N, Lq)), bad.pop("weights", None), ctx=ctx, **bad)
        with pytest.raises(L.ImhError):
            ctx.cross_attention_regions(good.x, good.wq, good.k, good.vt, torch.zeros(B * Lq, C_, dtype=dtype, device=DEV), B, H, Lq, good.lk, good.lkp, C_,
                                        B * good.lkp, 0.125, good.k2, good.vt2, good.lk2, good.lk2p, C_, B * N * good.lk2p, N + 1,
                                        torch.ones(N + 1, Lq, device=DEV))          # caches of N images, n_img = N + 1
        assert not ctx.tags
        y = good.regions(torch.ones(N, Lq), ctx=ctx)
        if record:
            assert [t[1] for t in ctx.tags] == [L.OP_XATTN_REGIONS] and not bool(y.any())
            ctx.run()
            eager = good.regions(torch.ones(N, Lq))
            assert torch.equal(_bits(y), _bits(eager))
            y.zero_()
            ctx.capture()
            ctx.replay()
            torch.cuda.synchronize()
            assert torch.equal(_bits(y), _bits(eager))
