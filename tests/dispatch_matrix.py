"""Cells of the dispatch contract (tests/test_gpu_dispatch_contract.py): one GEMM or conv3x3 request -- a feature of Ctx.gemm /
Ctx.conv3x3, a shape, a dtype -- built once with its float64 statement, then asked of a Ctx either without cfg= (the tuning table holds
the variant under test) or with cfg= forced.  Every operand, output and side output lives in a guard arena (tests/guarded.py), so a
refusal can be shown to have touched nothing and a stray store of a ragged edge tile has a location.

A plain helper module; no fixtures, no pytest settings."""
import torch
import torch.nn.functional as F

import exact_operands as exo
from guarded import Arena
from imagharmony_amd import lib as L
from imagharmony_amd.ctx import Ctx, GnSpec, GnStats
from test_gpu_gnstats import pack_conv
from test_gpu_ops import DEV, rnd

G = 32
ARENA_BYTES = 160 << 20

# ------------------------------------------------------------------------------------------------ variants
PLAIN = [(bm, bn, sp) for bm in (64, 128) for bn in (64, 128) for sp in (1, 2, 4)]
WS_SET = [(1464, 160, 1), (2464, 160, 1), (24128, 160, 1), (23256, 160, 1), (23256, 128, 1), (22128, 160, 1)]
HALO_CODES = [(7128, 320, 1), (7128, 160, 1), (7128, 80, 1), (7256, 160, 1), (7356, 160, 1), (7328, 160, 1), (7428, 160, 1), (7564, 160, 1),
              (7564, 320, 1), (7256, 80, 1)]
YT_OK = {(23256, 160): 256, (24128, 160): 128, (22128, 160): 128, (2464, 160): 64, (1464, 160): 64, (23256, 128): 256}   # gemm_launch: tile rows of the Yt variants


def uniq(cases):
    seen, out = set(), []
    for c in cases:
        if c not in seen:
            seen.add(c)
            out.append(c)
    return out


def gemm_variants(big):
    """every GEMM variant of the default library: the plain tiles at splits 1 / 2 / 4, the big-tile list of test_gpu_ops (already filtered
    by built()), the wave-specialised set and the sixteen-wave tile"""
    return uniq(PLAIN + list(big) + [v for v in WS_SET if L.variant_built(v)] + [(26256, 320, 1)])


def conv_variants(conv_list):
    return uniq(list(conv_list) + [v for v in HALO_CODES if L.variant_built(v)])


# ------------------------------------------------------------------------------------------------ arena context
class ArenaCtx(Ctx):
    """guarded.GuardCtx that can also record; the split-K workspace is carved as 4 KB rows (a one-row carve would ask for a guard of 320
    times its own size)"""

    def __init__(self, arena, dtype, record=False):
        super().__init__(arena.device, dtype, record=record)
        self.arena = arena
        self.role = "out"

    def new(self, *shape, dtype=None):
        return self.arena.carve(shape, dtype or self.dtype, role=self.role)

    def workspace(self, nbytes):
        return self.arena.carve(((int(nbytes) + 4095) // 4096, 4096), torch.uint8, role="scratch")

    def free(self, t):
        pass

    def row_stats(self, x, descr="row_stats"):
        self.role = "in"          # the statistics are an operand of the launch that follows, not one of its outputs (outputs_untouched)
        try:
            return super().row_stats(x, descr=descr)
        finally:
            self.role = "out"


_ARENA = None


def fresh_arena():
    """ONE arena for the whole module, wiped between cells (sentinel everywhere, no carves)"""
    global _ARENA
    if _ARENA is None:
        _ARENA = Arena(DEV, ARENA_BYTES)
    _ARENA.reset()
    return _ARENA


def outputs_untouched(arena):
    """every carve the call could have written (outputs, side outputs, workspaces) still holds the sentinel bit for bit"""
    name = arena.written()
    return (False, name) if name else (not arena.damage(), "guards")


def is_library_refusal(e):
    """L.check's wording: the launch reached the library and came back with a status"""
    return "failed (status" in str(e)


# ------------------------------------------------------------------------------------------------ GEMM cells
GEMM_FEATURES = ["none", "bias", "residual", "residual_inplace", "rowadd", "silu", "gelu", "qgelu", "geglu", "out_f32", "vt_perm",
                 "ln_row_stats", "ln_row", "ln_geglu", "ln_col", "x2", "yt", "stats_out", "gn_out",
                 "bias_residual", "ln_stats_out", "silu_gn_out"]
WHOLE, RAGGED = (512, 640, 128), (300, 200, 192)
# what the feature's own rule leaves of the ragged shape: GEGLU pairs 16 columns, the V^T layout 16 keys (N = 208); yt and gn_out are
# whole-tile features by their definition (Ctx.gemm), so the ragged yt cell is the one request no variant can serve
RAGGED_N = {"geglu": 208, "ln_geglu": 208, "vt_perm": 208}
LN_FEATS = ("ln_row_stats", "ln_row", "ln_geglu", "ln_col", "yt", "ln_stats_out")


def gemm_shapes(feat):
    if feat in ("gn_out", "silu_gn_out"):
        return [WHOLE]
    M, N, K = RAGGED
    return [WHOLE, (M, RAGGED_N.get(feat, N), K)]


def _ln_norm(K):
    norm = torch.nn.LayerNorm(K, eps=1e-5)
    with torch.no_grad():
        norm.weight.copy_(1 + 0.2 * torch.randn(K, generator=torch.Generator().manual_seed(3)))
        norm.bias.copy_(0.3 * torch.randn(K, generator=torch.Generator().manual_seed(4)))
    return norm


class GemmCell:
    """inputs and the float64 statement of one (feature, shape, dtype); call(ctx, cfg) places everything in ctx.arena and issues the request.
    exact=True (the features of exact_operands.GEMM_FEATURES): the operands come from the binary grids of tests/exact_operands.py, the statement
    and the placement stay as they are, and check() asks for the statement's one correctly rounded value, element for element"""

    def __init__(self, feat, shape, dtype, exact=False):
        from conftest import ref_row_stats
        from test_gpu_ops import geglu_ref
        self.feat, self.shape, self.dtype = feat, shape, dtype
        M, N, K = shape
        self.k = 4.0
        f = feat
        self.flags = 0
        self.x = rnd(M, K, dtype=dtype, seed=1)
        self.w = rnd(N, K, dtype=dtype, seed=2, scale=K ** -0.5)
        self.bias = rnd(N, dtype=dtype, seed=3) if f in ("bias", "bias_residual", "silu", "stats_out", "gn_out", "silu_gn_out") else None
        n_out = N // 2 if f in ("geglu", "ln_geglu") else N
        self.res = (rnd(M, n_out, dtype=dtype, seed=4) * 1.5 + 0.5).contiguous() if f in ("residual", "residual_inplace", "bias_residual", "stats_out") else None
        self.rpb = (M + 2) // 3 if f == "rowadd" else 0
        self.rowadd = rnd(3, N + 64, dtype=dtype, seed=5) if f == "rowadd" else None
        self.exact = exact
        if exact:
            assert f in exo.GEMM_FEATURES, f"{f} has no exact form"
            o = exo.gemm_operands(f, shape, dtype)
            assert all((getattr(self, n) is None) == (o[n] is None) for n in ("bias", "rowadd")) and (self.res is None) == (o["residual"] is None)
            self.x, self.w, self.bias, self.res, self.rowadd = (None if t is None else t.to(DEV) for t in (o["x"], o["w"], o["bias"], o["residual"], o["rowadd"]))
            self.assert_premise()
        self.hw = 256 if f in ("gn_out", "silu_gn_out") else 0
        self.ln = None
        if f in LN_FEATS:
            from imagharmony_amd.attention_processor import fold_ln
            toks = N if f == "ln_col" else M
            outs = M if f == "ln_col" else N
            tok = (rnd(toks, K, dtype=dtype, seed=1) * 1.5 + 2.0).contiguous()
            wf = rnd(outs, K, dtype=torch.float32, seed=2, scale=K ** -0.5)
            norm = _ln_norm(K)
            wg, s, c = fold_ln(wf, norm, Ctx(DEV, dtype))
            full = F.layer_norm(tok.double(), (K,), norm.weight.double().to(DEV), norm.bias.double().to(DEV), 1e-5) @ wf.double().t()
            self.ln = (s, c)
            self.st = ref_row_stats(tok.float(), 1).to(DEV) if f != "ln_row_stats" else None
            self.k = 8.0 if f == "ln_geglu" else 6.0
            if f == "ln_col":
                self.x, self.w, self.flags, ref = wg, tok, L.GF_LN_COL, full.t()
            else:
                self.x, self.w, self.flags, ref = tok, wg, L.GF_LN_ROW, full
            if f == "ln_geglu":
                self.flags |= L.GF_GEGLU
                ref = geglu_ref(ref)
        else:
            acc = self.x.double() @ self.w.double().t()
            if self.bias is not None:
                acc = acc + self.bias.double()
            if self.rowadd is not None:
                acc = acc + self.rowadd[:, 32:32 + N].double()[torch.arange(M, device=DEV) // self.rpb]
            if f in ("silu", "silu_gn_out"):
                self.flags, acc = L.GF_ACT_SILU, F.silu(acc)
            if f == "gelu":
                self.flags, acc = L.GF_ACT_GELU, F.gelu(acc)
            if f == "qgelu":
                self.flags, acc = L.GF_ACT_QGELU, acc * torch.sigmoid(1.702 * acc)
            if f == "geglu":
                self.flags, acc = L.GF_GEGLU, geglu_ref(acc)
            if f == "out_f32":
                self.flags = L.GF_OUT_F32
            if f == "vt_perm":
                self.flags = L.GF_VT_PERM
            if self.res is not None:
                acc = acc + self.res.double()
            ref = acc
        if f == "x2":
            self.k1 = K - 64
        self.col0 = N // 2 if f == "yt" else 0          # 320 of 640: a multiple of 160
        self.ref = ref
        self.n_out = self.col0 or n_out

    def assert_premise(self):
        """exact cells: the launch's partial sums are exact in fp32 (again after a test replaced an operand)"""
        ra = None if self.rowadd is None else self.rowadd[:, 32:32 + self.shape[1]]
        exo.assert_exact_in_fp32(self.shape[2], self.x, self.w, self.bias, ra, self.res)

    def extras(self):
        return self.bias is not None or self.res is not None or self.rowadd is not None or self.feat in ("x2", "yt")

    def variant_ok(self, cfg):
        """Ctx's own gate for this request (what _config asks before it takes a table entry)"""
        M, N, K = self.shape
        if self.feat == "x2" and not (cfg[0] <= 128 or cfg[0] in Ctx._WS):           # (gemm(): the two-source gate)
            return False
        if self.feat == "yt" and not (tuple(cfg[:2]) in YT_OK and cfg[2] == 1 and M % YT_OK[tuple(cfg[:2])] == 0 and N % cfg[1] == 0 and self.col0 % cfg[1] == 0):
            return False                                                              # (Ctx._yt_config)
        return Ctx._variant_ok(cfg[0], cfg[2], self.flags, 0, 1, self.ln is not None, M, N, self.extras())      # (ln_pre: Ctx.gemm supplies the statistics where the caller has none)

    def call(self, ctx, cfg=None):
        a = ctx.arena
        M, N, K = self.shape
        f = self.feat
        kw = dict(flags=self.flags, cfg=cfg)
        if f == "x2":
            x, kw["x2"] = a.place(self.x[:, :self.k1].contiguous(), ld=self.k1 + 64), a.place(self.x[:, self.k1:].contiguous())
        else:
            x = a.place(self.x, ld=K + 64)
        w = a.place(self.w, ld=K + 8)
        if self.bias is not None:
            kw["bias"] = a.place(self.bias)
        odt = torch.float32 if f == "out_f32" else self.dtype
        if f == "residual_inplace":
            out = a.carve((M, self.n_out), odt, ld=self.n_out + 16, role="in")
            out.copy_(self.res)
            kw["residual"] = out
        else:
            out = a.carve((M, self.n_out), odt, ld=self.n_out + 24)
            if self.res is not None:
                kw["residual"] = a.place(self.res, ld=self.n_out + 16)
        if self.rowadd is not None:
            kw.update(rowadd=a.place(self.rowadd)[:, 32:32 + N], rows_per_batch=self.rpb, ldra=N + 64)
        if self.ln is not None:
            s, c = a.place(self.ln[0]), a.place(self.ln[1])
            kw["ln"] = (s, c, 1e-5) if self.st is None else (s, c, 1e-5, (a.place(self.st), 1))
        yt = None
        if f == "yt":
            yt = a.carve((N - self.col0, M), self.dtype, ld=M + 64)
            kw["yt"] = (yt, self.col0)
        if f in ("stats_out", "ln_stats_out"):
            kw["stats_out"] = True
        if self.hw:
            kw["gn_out"] = self.hw
        r = ctx.gemm(x, w, out=out, **kw)
        side = r[1] if isinstance(r, tuple) else None
        return out, side, yt

    def check(self, out, side, yt, what):
        from test_gpu_gnstats import _check_partials, _ref_partials
        from test_gpu_lnstats import _check_stats
        from test_gpu_ops import assert_close, vt_unpermute
        f = self.feat
        ref = self.ref
        if self.exact:
            odt = torch.float32 if f == "out_f32" else self.dtype
            assert out.dtype == odt
            exo.assert_equal(vt_unpermute(out.contiguous()) if f == "vt_perm" else out, exo.expected(ref, odt), what)
            return
        if f == "yt":
            assert_close(out, ref[:, :self.col0], self.dtype, what + " [Q|K]", k=self.k)
            assert_close(vt_unpermute(yt.contiguous()), ref[:, self.col0:].t(), self.dtype, what + " V^T", k=self.k)
            return
        y = vt_unpermute(out.contiguous()) if f == "vt_perm" else out
        if f == "out_f32":
            assert out.dtype == torch.float32
        assert_close(y, ref, self.dtype, what, k=self.k)
        if f in ("stats_out", "ln_stats_out"):
            st, slots = side
            _check_stats(st, slots, out.contiguous(), what + " row statistics")
        if self.hw and side is not None:       # (None: the variant has no GroupNorm epilogue; the consumer runs gn_stats -- Ctx.gemm)
            assert isinstance(side, GnStats)
            B = self.shape[0] // self.hw
            yc = out.contiguous()
            _check_partials(side, _ref_partials(yc, B, self.hw, side.nblk, 10), yc, what + " GroupNorm partials")


# ------------------------------------------------------------------------------------------------ conv cells
CONV_FEATURES = ["s1", "s2", "pad1", "up1", "up2", "residual", "rowadd", "gn_groups", "gn_table", "gn_spec", "x2"]
CONV_SHAPES = [(2, 16, 16, 64, 160), (1, 12, 20, 128, 200), (1, 16, 32, 64, 160)]


def conv_ref64(x, w4, bias, stride=1, up=0, pad=0):
    """NHWC x as stored -> float64 conv as im2col + matmul (no vendor conv library): [B, Ho, Wo, Cout]"""
    from test_gpu_parity_fullsize import _conv3x3_ref
    xin = x.double().permute(0, 3, 1, 2)
    if up:
        xin = xin.repeat_interleave(2, 2).repeat_interleave(2, 3)
    w = w4.double()
    if pad:
        B, Cin, H, W = xin.shape
        cols = F.unfold(F.pad(xin, (0, 1, 0, 1)), 3, padding=0, stride=2)
        y = (w.reshape(w.shape[0], -1) @ cols).view(B, w.shape[0], (H - 2) // 2 + 1, (W - 2) // 2 + 1)
    else:
        y = _conv3x3_ref(xin, w, stride)
    return (y + bias.double()[None, :, None, None]).permute(0, 2, 3, 1)


def gn_ref64(x, gamma, beta, silu, dtype):
    """GroupNorm (+ SiLU) of NHWC x in float64, rounded to the storage dtype like the kernel's staged halo"""
    n = F.group_norm(x.double().permute(0, 3, 1, 2), G, gamma.double(), beta.double(), 1e-5)
    if silu:
        n = F.silu(n)
    return n.permute(0, 2, 3, 1).to(dtype)


def ref_gn_partials(arena, x, sub):
    """GnStats of NHWC x in the hand-over format, one pixel block per sample, (sum, M2) of every run of `sub` channels in float64"""
    B, H, W, C_ = x.shape
    v = x.double().view(B, H * W, C_ // sub, sub)
    s = v.sum(dim=(1, 3))
    m2 = (v - v.mean(dim=(1, 3), keepdim=True)).pow(2).sum(dim=(1, 3))
    t = arena.place(torch.stack([s, m2], -1).float().view(B, 1, C_ // sub, 2).contiguous())
    return GnStats(t, 1, sub, H * W * sub, C_)


def ref_gn_table(x, gamma, beta):
    """the (scale, shift) table [B, C, 2] fp32 of GroupNorm(32) over NHWC x, in float64"""
    B, H, W, C_ = x.shape
    xg = x.double().view(B, H * W, G, C_ // G)
    mean, var = xg.mean(dim=(1, 3)), xg.var(dim=(1, 3), unbiased=False)
    sc = gamma.double()[None] * (var + 1e-5).rsqrt().repeat_interleave(C_ // G, 1)
    sh = beta.double()[None] - mean.repeat_interleave(C_ // G, 1) * sc
    return torch.stack([sc, sh], -1).float().contiguous()


class ConvCell:
    """exact=True (the features of exact_operands.CONV_FEATURES): grid operands, the same statement and placement, equality in check().
    gn_affine (exact only): conv3x3(gn=(table, False)) with a hand-made [B, Cin, 2] table whose fma(x, scale, shift) is exact in T"""

    def __init__(self, feat, shape, dtype, two_source=None, exact=False):
        if feat == "x2" and shape[3] < 128:          # the feature's own rule: two sources of at least 64 channels each
            shape = shape[:3] + (128,) + shape[4:]
        self.feat, self.shape, self.dtype = feat, shape, dtype
        B, H, W, Cin, Cout = shape
        f = feat
        self.stride = 2 if f in ("s2", "pad1") else 1
        self.pad = 1 if f == "pad1" else 0
        self.up = 1 if f == "up1" else (2 if f == "up2" else 0)
        self.gn = f in ("gn_table", "gn_spec")
        self.exact, self.table = exact, None
        assert exact or f != "gn_affine"
        self.c1 = (Cin - 64 if two_source is None else two_source) if f == "x2" or two_source else Cin
        self.x = (rnd(B, H, W, Cin, dtype=dtype, seed=1) * (1.3 if self.gn else 1.0) + (0.4 if self.gn else 0.0)).contiguous()
        self.w4 = rnd(Cout, Cin, 3, 3, dtype=dtype, seed=2, scale=(9 * Cin) ** -0.5)
        self.bias = rnd(Cout, dtype=dtype, seed=3)
        self.k = 6.0 if self.gn else 4.0
        xin = self.x
        if self.gn:
            self.gamma, self.beta = rnd(Cin, dtype=dtype, seed=11) * 0.2 + 1.0, rnd(Cin, dtype=dtype, seed=12) * 0.3
            xin = gn_ref64(self.x, self.gamma, self.beta, True, dtype)
        ref = conv_ref64(xin, self.w4, self.bias, self.stride, 1 if self.up else 0, self.pad)
        self.res = self.rowadd = None
        if f == "residual":
            self.res = rnd(*ref.shape, dtype=dtype, seed=5)
            ref = ref + self.res.double()
        if f == "rowadd":
            self.rowadd = rnd(B, Cout + 64, dtype=dtype, seed=4)
            ref = ref + self.rowadd[:, 32:32 + Cout].double()[:, None, None, :]
        if exact:          # the same statement over the grid operands; xin: what the MFMAs read (x, or the staged halo of gn_affine)
            assert f in exo.CONV_FEATURES and two_source is None, f"{f} has no exact form"
            o = exo.conv_operands(f, shape, dtype)
            self.x, self.w4, self.bias = o["x"].to(DEV), o["w4"].to(DEV), o["bias"].to(DEV)
            self.res, self.rowadd = (None if o[n] is None else o[n].to(DEV) for n in ("residual", "rowadd"))
            self.xin = self.x
            if f == "gn_affine":
                self.table = o["table"].to(DEV)
                self.xin = exo.affine(self.x, self.table, dtype)
            ref = conv_ref64(self.xin, self.w4, self.bias, self.stride, 1 if self.up else 0, self.pad)
            if self.res is not None:
                ref = ref + self.res.double()
            if self.rowadd is not None:
                ref = ref + self.rowadd[:, 32:32 + Cout].double()[:, None, None, :]
        self.ref = ref
        self.K = 9 * Cin
        self.M = ref.shape[0] * ref.shape[1] * ref.shape[2]
        if exact:
            self.assert_premise()

    def assert_premise(self):
        """exact cells: the launch's partial sums are exact in fp32 (again after a test replaced an operand, and xin with it)"""
        ra = None if self.rowadd is None else self.rowadd[:, 32:32 + self.shape[4]]
        exo.assert_exact_in_fp32(self.K, self.xin, self.w4, self.bias, ra, self.res)

    def variant_ok(self, cfg):
        if self.up == 2:
            return (cfg[0], cfg[1]) in Ctx._PHASE and self.shape[4] % cfg[1] == 0 and cfg[2] == 1
        if (self.gn or self.table is not None or self.c1 != self.shape[3]) and cfg[0] not in Ctx._HALO:      # (conv_fuses_gn: the front end lives in the LDS-halo kernels)
            return False
        return Ctx._variant_ok(cfg[0], cfg[2], 0, 1, self.stride, False, self.M, self.shape[4], pad=self.pad)

    def call(self, ctx, cfg=None, fused=True):
        """fused=False (the product's protocol when conv_fuses_gn says no, unet.py): GroupNorm / concat as passes, then the plain conv"""
        a = ctx.arena
        B, H, W, Cin, Cout = self.shape
        kw = dict(stride=self.stride, up=self.up, pad=self.pad, cfg=cfg, bias=a.place(self.bias))
        two = self.c1 != Cin
        xa = a.place(self.x[..., :self.c1].contiguous())
        xb = a.place(self.x[..., self.c1:].contiguous()) if two else None
        # (placed as [9 Cout, Cin] rows: the guard of a carve is 320 of its rows, and one packed row of the widest cell is 200 KB)
        w = a.place(pack_conv(self.w4).view(9 * Cout, Cin)).view(Cout, 9 * Cin)
        if self.res is not None:
            kw["residual"] = a.place(self.res).view(-1, Cout)
        if self.rowadd is not None:
            kw.update(rowadd=a.place(self.rowadd)[:, 32:32 + Cout], ldra=Cout + 64)
        if self.feat == "gn_groups":
            kw["gn_groups"] = G
        wide = Cin > 4096        # beyond the statistics pass and the table launch (norm.hip: C / 8 threads): partials / table stated in float64
        if self.gn:
            stats = (lambda t: ref_gn_partials(a, t, 2)) if wide else (lambda t: ctx.gn_stats(t.view(B, H * W, t.shape[-1]), sub=2))
            parts = [stats(xa)] + ([stats(xb)] if two else [])
            gamma, beta = a.place(self.gamma), a.place(self.beta)
        # (a.seal(): what the passes before the conv wrote are its operands; outputs_untouched looks at the conv's own outputs)
        if not fused:
            xc = a.place(self.x) if two else xa
            if self.gn:
                tab = ctx.gn_table(parts if two else parts[0], gamma, beta, G, 1e-5, H * W)
                xc = ctx.gn_apply(xc.view(B, H * W, Cin), tab, True).view(B, H, W, Cin)
            a.seal()
            r = ctx.conv3x3(xc, w, **kw)
        else:
            if self.gn:
                if self.feat == "gn_spec":
                    kw["gn"] = (GnSpec(parts if two else parts[0], gamma, beta, G, 1e-5), True)
                elif wide:
                    kw["gn"] = (a.place(ref_gn_table(self.x, self.gamma, self.beta)), True)
                else:
                    kw["gn"] = (ctx.gn_table(parts if two else parts[0], gamma, beta, G, 1e-5, H * W), True)
            if self.table is not None:
                kw["gn"] = (a.place(self.table), False)
            a.seal()
            r = ctx.conv3x3(xa, w, x2=xb, **kw)
        return (r[0], r[1]) if isinstance(r, tuple) else (r, None)

    def check(self, out, side, what, cfg_used=None):
        from test_gpu_gnstats import _check_partials, _ref_partials
        from test_gpu_ops import assert_close
        assert tuple(out.shape) == tuple(self.ref.shape), (out.shape, self.ref.shape)
        if self.exact:
            exo.assert_equal(out, exo.expected(self.ref, self.dtype), what)
            return
        assert_close(out, self.ref, self.dtype, what, k=self.k)
        if self.feat == "gn_groups" and side is not None:
            B, Ho, Wo, Cout = self.ref.shape
            y2 = out.reshape(B * Ho * Wo, Cout)
            bm = cfg_used[0]
            tile = (Ho, Wo, side.npart // 10 // 4, 16, 4) if bm in Ctx._HALO else None      # (a wave's rows of the patch are one block)
            _check_partials(side, _ref_partials(y2, B, Ho * Wo, side.nblk, 10, tile=tile), y2, what + " GroupNorm partials")
