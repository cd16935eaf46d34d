"""SDXL ``UNet2DConditionModel`` forward on the gfx950 kernels.

What the reference calls at ip_adapter/custom_pipelines.py:338-345 / train.py:310 is diffusers' UNet
(third-party; architecture per SURVEY.md Appendix A).  This module keeps its contract -- the SDXL
state-dict key schema, ``.config``, ``.attn_processors``, ``.set_attn_processor(dict)``, and
``forward(sample, timestep, encoder_hidden_states, added_cond_kwargs=..., return_dict=False)[0]`` --
but the arithmetic is emitted as calls into libimh_hip.so:

  * activations live token-major / NHWC ([B, H*W, C]) for the whole network, so the
    NCHW<->token permutes of Transformer2DModel disappear and every 3x3 conv is an implicit GEMM
    with a contiguous K axis; NCHW exists only at conv_in's input and after conv_out;
  * GEGLU, bias, residual adds, time-embedding adds and nearest-upsampling are epilogue / gather
    options of the GEMM kernel, not separate passes;
  * the 17 ``time_emb_proj`` Linears are stacked into ONE GEMM per step;
  * text / image-prompt K,V of the 70 cross-attention layers come from a per-image cache.

torch is used for parameter storage and device memory only.  ``emit_forward`` records the whole
forward into a ``Ctx`` (plan / hipGraph); ``forward`` is the eager drop-in signature.
"""
import math
import os
from dataclasses import dataclass
from typing import Dict, Tuple

import torch
import torch.nn as nn

from . import lib as L
from .attention_processor import AttnProcessor2_0, CNAttnProcessor2_0, IPAttnProcessor2_0, _b, _w, fold_ln
from .ctx import Ctx, GnSpec
from .derived import derived
from .lora import LoRAMixin


# BasicTransformerBlock.norm1/2/3 folded into the consumer GEMMs (exact algebra, tested): the consumer takes the
# un-normalised residual stream and normalises in its epilogue, y = rstd * (acc - mean * s) + c -- 210 LayerNorm launches and
# 0.84 GB of HBM traffic per forward disappear.  False = the stand-alone LayerNorm kernel in front of every consumer (A/B and
# debugging).
FOLD_LAYERNORM = True
# The rows' (mean, rstd) travel with the residual stream: the GEMM that WRITES a LayerNorm input (proj_in, to_out + residual,
# ff.out + residual) leaves (sum, M2) slot partials behind from its epilogue (csrc/imh_lnstats.h) and every consumer -- the
# [Q|K] + V^T pair (norm1), the fused cross-attention's to_q (norm2), ff.net.0 (norm3) -- merges them in its prologue:
# Welford / Chan all the way, like torch.nn.LayerNorm (which the reference runs ahead of attn.to_q,
# ip_adapter/attention_processor.py:396).  The in-loop E[x^2] - mean^2 form of rounds 2-3 no longer exists in the library; rows no
# epilogue covers get their statistics from a stand-alone row-statistics launch (Ctx.gemm / Ctx.gemm_dual supply it).
# GroupNorm statistics the same way: the conv / GEMM that writes a GroupNorm input (conv1 -> norm2, conv2 / proj_out / the
# stride-2 downsampler -> the next block's norm1 / Transformer2DModel.norm / conv_norm_out, ALSO through the up path's channel
# concats: the two producers' partials are merged) leaves (sum, M2) partials per 10-channel sub-run behind from its epilogue
# (imh_gemm_args.gn_out), from which the per-sample (scale, shift) table of the GroupNorm is built (below).  Tensors no epilogue
# covers (conv_in, split-K / ring variants) get theirs from one statistics pass.  False = every tensor takes the pass (A/B;
# IMH_GN_STATS=0).
GN_STATS_HANDOVER = os.environ.get("IMH_GN_STATS", "1") != "0"
# ... and the GroupNorm itself -- diffusers ResnetBlock2D: norm -> SiLU -> conv -- is applied INSIDE the consuming
# conv3x3's halo staging wherever that conv runs on the LDS-halo kernel (the 128 x 128 and 64 x 64 levels): no normalised tensor in
# memory, and the up path's torch.cat([hidden, skip], 1) is read from its two producers by the same kernel (and by conv_shortcut's
# GEMM): no concat pass either.  False = apply pass + materialised concat everywhere (A/B; IMH_GN_FUSE=0).
GN_FUSE = os.environ.get("IMH_GN_FUSE", "1") != "0"
# The table step has no launch of its own in either form: the consumer -- the fused conv, or the apply pass in front of a Linear --
# builds its sample's (scale, shift) table in its prologue from the producers' partials (imh_gemm_args.gn_part, IMH_GN_TABLE_APPLY;
# csrc/imh_gntable.h: the same routine as Ctx.gn_table's launch, bit-identical).


# a ControlNet carries ONE CNAttnProcessor2_0 object on all its layers (ip_adapter/ip_adapter.py:126-133): on attn1 it is plain
# self-attention, which this processor records (no parameters, no state); on attn2 it is IPAttnProcessor2_0(skip=True) by its own emit
_SELF_ATTN = AttnProcessor2_0()


def gn_sub(C_, groups):
    """channels per sub-run of the GroupNorm partials of a C-channel tensor no conv / GEMM epilogue covers: sub-runs of
    gcd(C / groups, 10) channels tile the groups of every reader, alone or through a concat with a tensor of a multiple of C channels
    (SDXL: 10, like the producers' epilogues)"""
    return math.gcd(C_ // groups, 10)


class Feat:
    """an activation travelling through the UNet with the GroupNorm partials its writing launch left behind (or None)"""
    __slots__ = ("t", "gs")

    def __init__(self, t, gs=None):
        self.t, self.gs = t, gs

    @classmethod
    def of(cls, r):
        """what Ctx.conv3x3(gn_groups=), Ctx.gemm(gn_out=) and Ctx.control_add(gn_sub=) return -- (tensor, GnStats or None) where the
        partials were asked for, else the tensor alone -- as a Feat"""
        return cls(*r) if isinstance(r, tuple) else cls(r)

    def stats(self, ctx, groups):
        """the tensor's GroupNorm partials: the producer's, else one statistics pass (kept: skip tensors are normalised twice)"""
        if self.gs is None:
            B, C_ = self.t.shape[0], self.t.shape[-1]
            self.gs = ctx.gn_stats(self.t.view(B, -1, C_), sub=gn_sub(C_, groups))
        return self.gs

    def free(self, ctx):
        ctx.free(self.t)
        if self.gs is not None:
            ctx.free(self.gs.t)
            self.gs = None


@dataclass
class UNetConfig:
    in_channels: int = 4
    out_channels: int = 4
    sample_size: int = 128
    block_out_channels: Tuple[int, ...] = (320, 640, 1280)
    layers_per_block: int = 2
    transformer_layers_per_block: Tuple[int, ...] = (1, 2, 10)
    attention_head_dim: Tuple[int, ...] = (5, 10, 20)
    cross_attention_dim: int = 2048
    addition_time_embed_dim: int = 256
    projection_class_embeddings_input_dim: int = 2816
    norm_num_groups: int = 32
    norm_eps: float = 1e-5

    @property
    def time_embed_dim(self):
        return self.block_out_channels[0] * 4

    @property
    def pooled_dim(self):
        return self.projection_class_embeddings_input_dim - 6 * self.addition_time_embed_dim

    def get(self, k, d=None):
        return getattr(self, k, d)


# ------------------------------------------------------------------ parameter holders
class Linear(nn.Module):
    def __init__(self, cin, cout, bias=True):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(cout, cin), requires_grad=False)
        self.bias = nn.Parameter(torch.empty(cout), requires_grad=False) if bias else None


class Conv2d(nn.Module):
    def __init__(self, cin, cout, k):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(cout, cin, k, k), requires_grad=False)
        self.bias = nn.Parameter(torch.empty(cout), requires_grad=False)

    def packed(self, ctx):
        """[Cout, Cin, k, k] -> [Cout, k*k*Cin] (K index = (ky*k+kx)*Cin + c), cached."""
        def build():
            w = self.weight.detach().permute(0, 2, 3, 1).reshape(self.weight.shape[0], -1)
            return w.to(device=ctx.device, dtype=ctx.dtype).contiguous()
        return derived(self, "_imh_packed", (self.weight,), build, where=(ctx.dtype, str(ctx.device)))

    def packed_padded(self, ctx, pad_out=True):
        """-> (packed [Cout', k*k * Cin'], bias [Cout']) with Cin' (and Cout' unless pad_out is False) zero-padded to a multiple of 64, so
        a conv over a few channels runs on the implicit-GEMM kernel: the padded output channels are exact zeros, silu(0) = 0, so a chain
        of such convs stays what the unpadded convs give.  Cached."""
        def build():
            w = self.weight.detach()
            co, ci = w.shape[:2]
            cop, cip = ((co + 63) // 64 * 64 if pad_out else co), (ci + 63) // 64 * 64
            wp = torch.zeros(cop, cip, *w.shape[2:], dtype=w.dtype, device=w.device)
            wp[:co, :ci] = w
            bp = torch.zeros(cop, dtype=w.dtype, device=w.device)
            bp[:co] = self.bias.detach()
            return wp.permute(0, 2, 3, 1).reshape(cop, -1).to(device=ctx.device, dtype=ctx.dtype).contiguous(), bp.to(device=ctx.device, dtype=ctx.dtype)
        return derived(self, "_imh_padded", (self.weight, self.bias), build, where=(ctx.dtype, str(ctx.device)), extra=(pad_out,))

    def packed_phase(self, ctx):
        """the 3 x 3 weight of an upsampler conv in the phase form of Ctx.conv3x3(up=2): [4 * Cout, 4 * Cin], pre-summed in fp32 from
        the stored weight and rounded once to the model dtype (ctx.phase_pack), cached."""
        from .ctx import phase_pack
        return derived(self, "_imh_packed_phase", (self.weight,), lambda: phase_pack(self.weight).to(device=ctx.device, dtype=ctx.dtype).contiguous(),
                       where=(ctx.dtype, str(ctx.device)))


class Norm(nn.Module):
    def __init__(self, c, eps):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(c), requires_grad=False)
        self.bias = nn.Parameter(torch.empty(c), requires_grad=False)
        self.eps = eps


class Dropout(nn.Module):
    pass


class Attention(nn.Module):
    """Parameter holder with the attribute surface the processors touch."""

    def __init__(self, query_dim, heads, dim_head=64, cross_attention_dim=None):
        super().__init__()
        inner = heads * dim_head
        self.heads = heads
        self.scale = dim_head ** -0.5
        self.spatial_norm = None
        self.group_norm = None
        self.norm_cross = None
        self.residual_connection = False
        self.rescale_output_factor = 1.0
        kv = cross_attention_dim if cross_attention_dim is not None else query_dim
        self.to_q = Linear(query_dim, inner, bias=False)
        self.to_k = Linear(kv, inner, bias=False)
        self.to_v = Linear(kv, inner, bias=False)
        self.to_out = nn.ModuleList([Linear(inner, query_dim), Dropout()])
        self.processor = AttnProcessor2_0()

    def get_processor(self):
        return self.processor

    def set_processor(self, p):
        if "processor" in self._modules and not isinstance(p, nn.Module):
            self._modules.pop("processor")
        self.processor = p

    def forward(self, hidden_states, encoder_hidden_states=None, attention_mask=None, **kw):
        return self.processor(self, hidden_states, encoder_hidden_states=encoder_hidden_states,
                              attention_mask=attention_mask)


def geglu_interleave(t):
    """[2 * inner, ...] = [values; gates] (diffusers GEGLU.proj: hidden, gate = proj(x).chunk(2)) -> rows in quads (value_2k,
    value_2k+1, gate_2k, gate_2k+1): one output tile holds both halves and the two gates of a quad land in one even-aligned
    accumulator register pair of the MFMA tile (IMH_GF_GEGLU: packed-fp32 GELU on both at once)"""
    inner = t.shape[0] // 2
    v, g = t[:inner].reshape((inner // 2, 2) + tuple(t.shape[1:])), t[inner:].reshape((inner // 2, 2) + tuple(t.shape[1:]))
    return torch.cat([v, g], 1).reshape((2 * inner,) + tuple(t.shape[1:])).contiguous()


class GEGLU(nn.Module):
    def __init__(self, dim, inner):
        super().__init__()
        self.proj = Linear(dim, inner * 2)

    def packed(self, ctx):
        """rows interleaved in (value, value, gate, gate) quads (geglu_interleave; GF_GEGLU epilogue)."""
        def build():
            w, b = self.proj.weight.detach(), self.proj.bias.detach()
            wi, bi = geglu_interleave(w), geglu_interleave(b)
            return wi.to(device=ctx.device, dtype=ctx.dtype).contiguous(), bi.to(device=ctx.device, dtype=ctx.dtype).contiguous()
        return derived(self, "_imh_packed", (self.proj.weight, self.proj.bias), build, where=(ctx.dtype, str(ctx.device)))

    def packed_ln(self, ctx, norm):
        """GEGLU projection with LayerNorm folded in (see attention_processor.fold_ln), rows interleaved in quads (geglu_interleave)."""
        def build():
            wg, s, cc = fold_ln(self.proj.weight, norm, ctx)
            il = geglu_interleave
            # the Linear's bias rides in the fold's constant term, c = W beta + b (fp32): one epilogue operand (and twenty live
            # registers per lane of the 256 x 160 kernel's epilogue) less than a separate bias vector
            b = self.proj.bias.detach().to(device=ctx.device, dtype=torch.float32)
            return il(wg), None, il(s), il(cc + b)
        return derived(self, "_imh_packed_ln", (self.proj.weight, self.proj.bias, norm.weight, norm.bias), build, where=(ctx.dtype, str(ctx.device)))


class FeedForward(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.net = nn.ModuleList([GEGLU(dim, dim * 4), Dropout(), Linear(dim * 4, dim)])

    def emit(self, ctx, x, residual, ln=None, ln_stats=None, want_stats=False):
        """-> (out, the row statistics of out where want_stats, else None)"""
        if ln is None:
            w1, b1 = self.net[0].packed(ctx)
            g = ctx.gemm(x, w1, bias=b1, flags=L.GF_GEGLU, descr="ff.geglu")
        else:       # x un-normalised, LayerNorm `ln` folded into the (interleaved) GEGLU projection
            w1, b1, s1, c1 = self.net[0].packed_ln(ctx, ln)
            g = ctx.gemm(x, w1, bias=b1, flags=L.GF_GEGLU | L.GF_LN_ROW, ln=(s1, c1, ln.eps, ln_stats), descr="ff.geglu")
        out = _with_stats(ctx.gemm(g, _w(self.net[2], ctx), bias=_b(self.net[2], ctx), residual=residual, descr="ff.out", stats_out=want_stats))
        ctx.free(g)
        return out


def _with_stats(r):
    """what Ctx.gemm(stats_out=) and a processor's emit(want_stats=) return -- (rows, their LayerNorm statistics) where those were asked
    for, else the rows alone -- as (rows, statistics or None)"""
    return r if isinstance(r, tuple) else (r, None)


def _free_rows(ctx, h, stats):
    ctx.free(h)
    if stats is not None:
        ctx.free(stats[0])


def _ln(ctx, norm, x, descr):
    return ctx.layernorm(x, _w(norm, ctx), _b(norm, ctx), norm.eps, descr=descr)


# ------------------------------------------------------------------ the GroupNorm front end
def _gn_spec(ctx, norm, groups, *srcs):
    """GroupNorm `norm` over the Feat srcs[0], or over the channel concat of two, as its consumer takes it: the consumer builds its
    sample's (scale, shift) table itself from the producers' partials (Feat.stats: one statistics pass where a producer left none)"""
    return GnSpec([f.stats(ctx, groups) for f in srcs], _w(norm, ctx), _b(norm, ctx), groups, norm.eps)


def _gn_pass(ctx, spec, x, silu, descr):
    """the GroupNorm (+ SiLU) of NHWC x as a pass, for the consumers that cannot take it themselves: the Linears, the convs that do not run
    on the LDS-halo kernel"""
    return ctx.gn_table_apply(x.view(x.shape[0], -1, x.shape[-1]), spec, silu, descr=descr).view(x.shape)


def _gn_conv(ctx, spec, conv, x, x2, descr, norm_descr, **epi):
    """conv(silu(GroupNorm(cat[x, x2]))), diffusers ResnetBlock2D's norm -> nonlinearity -> conv, x2 = None: of x alone.  Where the conv
    runs on the LDS-halo kernel (GN_FUSE, Ctx.conv_fuses_gn) the norm and the concat happen inside its halo staging, else as passes
    in front of it.  epi: the conv's epilogue arguments.  -> (Feat of the output, the concat where it was materialised, else None)"""
    M, (Cout, Cin) = x.numel() // x.shape[-1], conv.weight.shape[:2]
    kw = dict(bias=_b(conv, ctx), descr=descr, **epi)
    if GN_FUSE and ctx.conv_fuses_gn(M, Cout, 9 * Cin):
        return Feat.of(ctx.conv3x3(x, conv.packed(ctx), gn=(spec, True), x2=x2, **kw)), None
    xc = ctx.concat(x, x2, descr="skip.concat") if x2 is not None else None
    n = _gn_pass(ctx, spec, x if xc is None else xc, True, norm_descr)
    out = Feat.of(ctx.conv3x3(n, conv.packed(ctx), **kw))
    ctx.free(n)
    return out, xc


class BasicTransformerBlock(nn.Module):
    def __init__(self, dim, heads, cross_attention_dim):
        super().__init__()
        self.norm1 = Norm(dim, 1e-5)
        self.attn1 = Attention(dim, heads)
        self.norm2 = Norm(dim, 1e-5)
        self.attn2 = Attention(dim, heads, cross_attention_dim=cross_attention_dim)
        self.norm3 = Norm(dim, 1e-5)
        self.ff = FeedForward(dim)

    def fused(self, L_):
        """the folded-LayerNorm form applies (both processors are the HIP ones -- a ControlNet's CNAttnProcessor2_0 on both layers
        included --, 64-aligned token count)"""
        return FOLD_LAYERNORM and isinstance(self.attn1.processor, (AttnProcessor2_0, CNAttnProcessor2_0)) \
            and isinstance(self.attn2.processor, (IPAttnProcessor2_0, CNAttnProcessor2_0)) and L_ % 64 == 0

    def emit(self, ctx, h, B, L_, kv, st, stats=None, want_stats=False, grid=None):
        """h: the residual stream [B*L, C]; stats: the row statistics of h from the GEMM that wrote it, or None (both consumed)
        -> (h3, the statistics of h3 for the next block's norm1 where want_stats and this block runs folded, else None).
        grid = (h, w) of the L tokens: handed to a cross-attention processor that carries regional image prompts (regions.py)."""
        p1, p2 = self.attn1.processor, self.attn2.processor
        if isinstance(p1, CNAttnProcessor2_0):
            p1 = _SELF_ATTN
        if not hasattr(p1, "emit") or not hasattr(p2, "emit"):
            raise L.ImhError("a non-HIP attention processor is installed; the fused forward needs "
                             "imagharmony_amd.attention_processor processors")
        ip2 = isinstance(p2, IPAttnProcessor2_0)
        rk = dict(grid=grid) if ip2 and getattr(p2, "regions", None) is not None else {}      # (without regions: the call as it always was)
        # perturbed-attention guidance: in a chosen layer (set_pag_applied_layers) the last st.pag samples' self-attention map is the identity
        pk = dict(pag=st.pag) if getattr(st, "pag", 0) and getattr(self.attn1, "pag_identity", False) else {}
        if pk and not isinstance(p1, AttnProcessor2_0):
            raise L.ImhError(f"perturbed-attention guidance needs the HIP self-attention processor on attn1, not {type(p1).__name__}")
        if self.fused(L_):
            # LayerNorm never materialises: every consumer GEMM reads the residual stream itself, and takes the rows' statistics
            # from the epilogue of the GEMM that wrote it
            h1, s1 = p1.emit(ctx, self.attn1, h, B, L_, residual=h, ln=self.norm1, ln_stats=stats, want_stats=True, **pk)
            _free_rows(ctx, h, stats)
            h2, s2 = p2.emit(ctx, self.attn2, h1, B, L_, residual=h1, kv=kv, step=st.step, scale_tab=st.ip_scale_tab, ln=self.norm2,
                             ln_stats=s1, want_stats=True, **rk)
            _free_rows(ctx, h1, s1)
            h3, s3 = self.ff.emit(ctx, h2, residual=h2, ln=self.norm3, ln_stats=s2, want_stats=want_stats)
            _free_rows(ctx, h2, s2)
            return h3, s3
        if stats is not None:
            ctx.free(stats[0])
        n = _ln(ctx, self.norm1, h, "norm1")
        h1 = p1.emit(ctx, self.attn1, n, B, L_, residual=h, **pk)
        ctx.free(n); ctx.free(h)
        n = _ln(ctx, self.norm2, h1, "norm2")
        h2 = p2.emit(ctx, self.attn2, n, B, L_, residual=h1, kv=kv, step=st.step, scale_tab=st.ip_scale_tab, **rk) \
            if ip2 else p2.emit(ctx, self.attn2, n, B, L_, residual=h1, kv=kv)
        ctx.free(n); ctx.free(h1)
        n = _ln(ctx, self.norm3, h2, "norm3")
        h3, _ = self.ff.emit(ctx, n, residual=h2)
        ctx.free(n); ctx.free(h2)
        return h3, None


class Transformer2DModel(nn.Module):
    def __init__(self, channels, heads, n_layers, cross_attention_dim, groups):
        super().__init__()
        self.norm = Norm(channels, 1e-6)
        self.groups = groups
        self.proj_in = Linear(channels, channels)
        self.transformer_blocks = nn.ModuleList(
            [BasicTransformerBlock(channels, heads, cross_attention_dim) for _ in range(n_layers)])
        self.proj_out = Linear(channels, channels)

    def emit(self, ctx, f, kvs, st):
        """f: Feat of NHWC [B, H, W, C] (consumed) -> Feat of the same shape, with the GroupNorm partials of the output left by
        proj_out's epilogue (None if its variant has none)."""
        x = f.t
        B, Hh, Ww, C_ = x.shape
        L_ = Hh * Ww
        x2 = x.view(B * L_, C_)
        n = _gn_pass(ctx, _gn_spec(ctx, self.norm, self.groups, f), x, False, "t2d.norm")
        blocks = list(self.transformer_blocks)
        # the rows' LayerNorm statistics go from each writing GEMM to the next folded block's norm1
        ho = bool(blocks) and blocks[0].fused(L_)
        h, stats = _with_stats(ctx.gemm(n.view(B * L_, C_), _w(self.proj_in, ctx), bias=_b(self.proj_in, ctx), descr="t2d.proj_in", stats_out=ho))
        ctx.free(n)
        for i, (blk, kv) in enumerate(zip(blocks, kvs)):
            more = ho and i + 1 < len(blocks) and blocks[i + 1].fused(L_)
            h, stats = blk.emit(ctx, h, B, L_, kv, st, stats=stats, want_stats=more, grid=(Hh, Ww))
        out = Feat.of(ctx.gemm(h, _w(self.proj_out, ctx), bias=_b(self.proj_out, ctx), residual=x2, descr="t2d.proj_out",
                               gn_out=L_ if GN_STATS_HANDOVER else None))
        ctx.free(h)
        f.free(ctx)
        out.t = out.t.view(B, Hh, Ww, C_)
        return out


class ResnetBlock2D(nn.Module):
    def __init__(self, cin, cout, temb_dim, groups, eps):
        super().__init__()
        self.groups = groups
        self.norm1 = Norm(cin, eps)
        self.conv1 = Conv2d(cin, cout, 3)
        self.time_emb_proj = Linear(temb_dim, cout)
        self.norm2 = Norm(cout, eps)
        self.conv2 = Conv2d(cout, cout, 3)
        self.conv_shortcut = Conv2d(cin, cout, 1) if cin != cout else None
        self.temb_offset = 0    # column of this block inside the stacked time_emb_proj output

    def emit(self, ctx, f, st, skip=None, keep_input=False):
        """f: Feat of NHWC [B, H, W, C1]; skip: Feat of the skip connection (the block's input is torch.cat([f, skip], channels),
        diffusers UpBlock2D / CrossAttnUpBlock2D) or None -> Feat [B, H, W, Cout].  Both inputs are consumed unless keep_input.
        GroupNorm statistics travel with the tensors (Feat.gs); where the convs run on the LDS-halo kernel, norm1 / norm2 (+ SiLU)
        and the concat happen inside them (GN_FUSE), else as passes."""
        x = f.t
        B, Hh, Ww, C1 = x.shape
        HW = Hh * Ww
        M = B * HW
        sk = skip.t if skip is not None else None
        Cin = C1 + (sk.shape[-1] if sk is not None else 0)
        Cout = self.conv1.weight.shape[0]
        want = int(GN_STATS_HANDOVER)   # the convs leave the partials of their output behind for the next norm
        spec1 = _gn_spec(ctx, self.norm1, self.groups, f, *([skip] if skip is not None else []))
        ra = st.temb_all[:, self.temb_offset:self.temb_offset + Cout]
        # xc: the materialised concat, where something still needs it
        hf, xc = _gn_conv(ctx, spec1, self.conv1, x, sk, "res.conv1", "res.norm1", rowadd=ra, ldra=st.temb_all.stride(0), gn_groups=want)
        spec2 = _gn_spec(ctx, self.norm2, self.groups, hf)
        if self.conv_shortcut is not None:
            wsc, bsc = self.conv_shortcut.packed(ctx), _b(self.conv_shortcut, ctx)
            if sk is not None and xc is None:
                sc = ctx.gemm(x.view(M, C1), wsc, bias=bsc, x2=sk.view(M, Cin - C1), descr="res.shortcut")
            else:
                sc = ctx.gemm((xc if xc is not None else x).view(M, Cin), wsc, bias=bsc, descr="res.shortcut")
        else:
            # identity shortcut: the residual is the block's INPUT -- with a skip connection that is the concatenated tensor (no SDXL up
            # block gets here: Cin = C1 + Cskip != Cout always has a conv_shortcut)
            if sk is not None and xc is None:
                xc = ctx.concat(x, sk, descr="skip.concat")
            sc = (xc if xc is not None else x).view(M, Cin)
        out, _ = _gn_conv(ctx, spec2, self.conv2, hf.t, None, "res.conv2", "res.norm2", residual=sc, gn_groups=want)
        hf.free(ctx)
        if self.conv_shortcut is not None:
            ctx.free(sc)
        if xc is not None:
            ctx.free(xc)
        if not keep_input:
            f.free(ctx)
            if skip is not None:
                skip.free(ctx)
        return out


class Downsample2D(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.conv = Conv2d(c, c, 3)


class Upsample2D(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.conv = Conv2d(c, c, 3)


class DownBlock(nn.Module):
    def __init__(self, cin, cout, n_res, n_tf, heads, cfg, add_down):
        super().__init__()
        if n_tf:
            self.attentions = nn.ModuleList(
                [Transformer2DModel(cout, heads, n_tf, cfg.cross_attention_dim, cfg.norm_num_groups)
                 for _ in range(n_res)])
        self.resnets = nn.ModuleList(
            [ResnetBlock2D(cin if i == 0 else cout, cout, cfg.time_embed_dim, cfg.norm_num_groups, cfg.norm_eps)
             for i in range(n_res)])
        self.downsamplers = nn.ModuleList([Downsample2D(cout)]) if add_down else None
        self.has_attn = bool(n_tf)


class MidBlock(nn.Module):
    def __init__(self, c, n_tf, heads, cfg):
        super().__init__()
        self.attentions = nn.ModuleList([Transformer2DModel(c, heads, n_tf, cfg.cross_attention_dim,
                                                            cfg.norm_num_groups)])
        self.resnets = nn.ModuleList([ResnetBlock2D(c, c, cfg.time_embed_dim, cfg.norm_num_groups, cfg.norm_eps)
                                      for _ in range(2)])


class UpBlock(nn.Module):
    def __init__(self, cin, cout, cprev, n_res, n_tf, heads, cfg, add_up):
        super().__init__()
        if n_tf:
            self.attentions = nn.ModuleList(
                [Transformer2DModel(cout, heads, n_tf, cfg.cross_attention_dim, cfg.norm_num_groups)
                 for _ in range(n_res)])
        res = []
        for i in range(n_res):
            skip = cin if i == n_res - 1 else cout
            rin = cprev if i == 0 else cout
            res.append(ResnetBlock2D(rin + skip, cout, cfg.time_embed_dim, cfg.norm_num_groups, cfg.norm_eps))
        self.resnets = nn.ModuleList(res)
        self.upsamplers = nn.ModuleList([Upsample2D(cout)]) if add_up else None
        self.has_attn = bool(n_tf)


class TimestepEmbedding(nn.Module):
    def __init__(self, in_dim, dim):
        super().__init__()
        self.linear_1 = Linear(in_dim, dim)
        self.linear_2 = Linear(dim, dim)


class StepState:
    """Device-resident per-image / per-step state the recorded forward reads."""
    pag = 0        # trailing samples of the forward's batch whose chosen self-attention layers run the identity map: set by emit_forward(pag=)

    def __init__(self):
        self.latents = None        # fp32 [S, 4, H, W] (NCHW) -- scheduler state
        self.conv_in_extra = None  # fp32 [S, 5, H, W] (NCHW): [mask | masked-image latents], channels 4-8 of a 9-channel conv_in (inpainting UNet)
        self.blend_tab = None      # fp32 [steps, 2] add_noise pair of the inpainting blend per step (4-channel UNet), or None
        self.inp_z = self.inp_noise = self.inp_mask = None   # fp32 [S, 4 | 4 | 1, H, W]: image latents, add-noise noise, latent mask of that blend
        self.coef6_tab = None      # fp32 [steps, 6] (cx, ce, ch, cn, hx, he) of the general step (multistep / ancestral schedulers), or None
        self.hist = None           # fp32 [S, 4, H, W] its history slot: the previous step's data prediction, or None
        self.noise_bank = None     # fp32 [steps, S, 4, H, W] its per-step noise (stochastic schedulers), or None
        self.seed_rows = None      # int32 bits of uint32 [S, 4] (seed low, seed high, lane, 0): a seeded schedule's step noise comes from these, or None
        self.t_table = None        # fp32 [steps] timesteps
        self.step = None           # int32 [1] device step counter
        self.in_scale_tab = None   # fp32 [steps] scale_model_input factor (Euler) or None
        self.ip_scale_tab = None   # fp32 [steps] IP scale per step (control_guidance gating) or None
        self.aug_emb = None        # [B, time_embed_dim]  add_embedding(text_embeds ++ time_ids) (step-invariant)
        self.kv = None             # {attn2 processor name: KVCache}
        self.temb_all = None       # [B, sum Cout] stacked time_emb_proj output (per step)
        self.temb_table = None     # [steps, B * sum Cout] the same for EVERY step of the schedule (precompute_temb), or None
        self.t_value = None        # fp32 [B] explicit timestep values (eager forward)


class UNetEncoderModel(nn.Module):
    """What UNet2DConditionModel and controlnet.ControlNetModel have in common: a subclass creates conv_in, time_embedding,
    add_embedding, down_blocks and mid_block under their diffusers names (the order of creation is the order of the state dict and of
    attn_processors) and numbers its ResNets (_number_time_emb_proj); this class holds the processor protocol, the packed / stacked
    weights, the checkpoint loader, the step-invariant conditioning, the time-embedding chain, conv_in's launch, the walk over the
    down path and the mid block, and the set-up of the eager forwards."""

    def resnets(self):
        for blk in list(self.down_blocks) + [self.mid_block]:
            for r in blk.resnets:
                yield r

    def _number_time_emb_proj(self):
        """the column of every ResNet inside the stacked time_emb_proj output"""
        off = 0
        for r in self.resnets():
            r.temb_offset = off
            off += r.time_emb_proj.weight.shape[0]
        self.temb_total = off

    # ---- processor protocol (ip_adapter/ip_adapter.py:102,125) ----
    def _attentions(self):
        """[(module name, Attention)] in module order (a list: set_processor changes the tree under the walk)"""
        return [(name, mod) for name, mod in self.named_modules() if hasattr(mod, "set_processor")]

    @property
    def attn_processors(self) -> Dict[str, object]:
        return {f"{name}.processor": mod.get_processor() for name, mod in self._attentions()}

    def set_attn_processor(self, processor):
        attns = self._attentions()
        if isinstance(processor, dict) and len(processor) != len(attns):
            raise ValueError(f"A dict of processors was passed, but the number of processors {len(processor)} "
                             f"does not match the number of attention layers: {len(attns)}.")
        for name, mod in attns:
            mod.set_processor(processor[f"{name}.processor"] if isinstance(processor, dict) else processor)

    def attn2_modules(self):
        """[(processor name, Attention)] for the cross-attention layers, in attn_processors order."""
        return [(f"{name}.processor", mod) for name, mod in self._attentions() if name.endswith("attn2")]

    def _pname(self, attn2):
        names = getattr(self, "_imh_pnames", None)
        if names is None or id(attn2) not in names:      # (a deepcopy carries stale ids)
            names = self._imh_pnames = {id(mod): name for name, mod in self.attn2_modules()}
        return names[id(attn2)]

    def _kv_of(self, st, t2d):
        """the K / V caches of a Transformer2DModel's cross-attention layers, in block order"""
        return [st.kv[self._pname(blk.attn2)] for blk in t2d.transformer_blocks]

    # ---- random init directly on the device (synthetic-weight benchmarks) ----
    @torch.no_grad()
    def init_random_(self, seed=1234):
        g = torch.Generator(device=self.conv_in.weight.device).manual_seed(seed)
        for name, p in self.named_parameters():
            if p.ndim >= 2:
                fan_in = p[0].numel()
                p.copy_(torch.randn(p.shape, generator=g, device=p.device, dtype=torch.float32).mul_(fan_in ** -0.5))
            elif name.endswith("bias"):
                p.copy_(torch.randn(p.shape, generator=g, device=p.device, dtype=torch.float32).mul_(0.02))
            else:
                p.fill_(1.0)
        return self

    # ---- checkpoints (the on-disk format either side of the path) ----
    @classmethod
    def from_safetensors(cls, path, cfg: "UNetConfig" = None, device="cpu", dtype=None):
        """Load a diffusers-format SDXL UNet checkpoint (``diffusion_pytorch_model.safetensors``): the key schema is
        the one this module keeps, so this is a strict ``load_state_dict``."""
        from safetensors.torch import load_file
        sd = load_file(path, device="cpu")
        m = cls(cfg)
        own = m.state_dict()
        extra = [k for k in sd if k not in own]
        missing = [k for k in own if k not in sd and ".processor." not in k]
        if extra or missing:
            raise KeyError(f"checkpoint / model key mismatch: {len(missing)} missing (e.g. {missing[:3]}), "
                           f"{len(extra)} unexpected (e.g. {extra[:3]})")
        m.load_state_dict(sd, strict=False)
        m = m.to(device)
        return m.to(dtype) if dtype is not None else m

    # ---- packed / stacked weights ----
    def _temb_stack(self, ctx):
        lins = [r.time_emb_proj for r in self.resnets()]

        def build():
            w, b = torch.cat([p.weight.detach() for p in lins], 0), torch.cat([p.bias.detach() for p in lins], 0)
            return w.to(device=ctx.device, dtype=ctx.dtype).contiguous(), b.to(device=ctx.device, dtype=ctx.dtype)
        return derived(self, "_imh_temb", [t for p in lins for t in (p.weight, p.bias)], build, where=(ctx.dtype, str(ctx.device)))

    def _temb_chain(self, ctx, tsin, aug):
        """time_embedding(t) + aug_emb -> SiLU -> the 17 stacked time_emb_proj Linears: [rows, 320] -> [rows, sum Cout]"""
        te = self.time_embedding
        h = ctx.gemm(tsin, _w(te.linear_1, ctx), bias=_b(te.linear_1, ctx), flags=L.GF_ACT_SILU, descr="time_emb.1")
        # emb = time_embedding(t) + aug_emb, then SiLU (every ResnetBlock2D applies it before time_emb_proj)
        emb = ctx.gemm(h, _w(te.linear_2, ctx), bias=_b(te.linear_2, ctx), residual=aug, descr="time_emb.2")
        semb = ctx.silu(emb, descr="silu(emb)")
        wt, bt = self._temb_stack(ctx)
        out = ctx.gemm(semb, wt, bias=bt, descr="time_emb_proj(all)")
        ctx.free(h); ctx.free(emb); ctx.free(semb)
        return out

    @torch.no_grad()
    def precompute_temb(self, ctx, st, timesteps):
        """st.temb_table = the stacked time-embedding projections of EVERY step of a schedule ([steps, B * sum Cout]; row i = what
        the per-step chain yields at timestep i): they depend on the step and on the conditioning (aug_emb), not on the latent,
        so a denoise loop computes them once per (schedule, conditioning) instead of five launches per step (r03 DESIGN 9.4)."""
        B = st.aug_emb.shape[0]
        ts = timesteps.to(device=ctx.device, dtype=torch.float32).reshape(-1)
        n = ts.numel()
        tv = ts.repeat_interleave(B).contiguous()                      # row i * B + b -> timestep i
        tsin = ctx.new(n * B, self.config.block_out_channels[0])
        ctx.ew(L.EW_TIMESTEP, tsin, a=tv, n=n * B, i=(self.config.block_out_channels[0], 0, 0, 0, 0, 0), descr="time_proj(all steps)")
        aug = st.aug_emb.repeat(n, 1).contiguous()                     # plumbing: the residual rows of every step
        tab = self._temb_chain(ctx, tsin, aug)
        ctx.free(tsin)
        st.temb_table = tab.view(n, B * self.temb_total)
        if ctx.record:
            ctx.keep.extend([tv, aug])
        return st.temb_table

    # ---- step-invariant conditioning ----
    @torch.no_grad()
    def prepare_conditioning(self, ctx, encoder_hidden_states, text_embeds, time_ids, st=None):
        """aug_emb = add_embedding(cat[text_embeds, Timesteps(256)(time_ids)]) and the K/V cache of every
        cross-attention layer (all independent of the denoise step)."""
        st = st or StepState()
        cfg = self.config
        B = encoder_hidden_states.shape[0]
        ids = time_ids.to(device=ctx.device, dtype=torch.float32).reshape(-1).contiguous()
        te = ctx.new(ids.numel(), cfg.addition_time_embed_dim)
        ctx.ew(L.EW_TIMESTEP, te, a=ids, n=ids.numel(), i=(cfg.addition_time_embed_dim, 0, 0, 0, 0, 0),
               descr="add_time_proj")
        add_in = torch.cat([text_embeds.to(device=ctx.device, dtype=ctx.dtype), te.view(B, -1)], dim=-1).contiguous()
        ae = self.add_embedding
        h = ctx.gemm(add_in, _w(ae.linear_1, ctx), bias=_b(ae.linear_1, ctx), flags=L.GF_ACT_SILU, descr="add_emb.1")
        st.aug_emb = ctx.gemm(h, _w(ae.linear_2, ctx), bias=_b(ae.linear_2, ctx), descr="add_emb.2")
        ehs = encoder_hidden_states.to(device=ctx.device, dtype=ctx.dtype)
        st.kv = {}
        for name, attn in self.attn2_modules():
            proc = attn.processor
            if not hasattr(proc, "prepare_kv"):
                raise L.ImhError(f"{name}: processor {type(proc).__name__} has no HIP K/V path")
            st.kv[name] = proc.prepare_kv(ctx, attn, ehs)
        if ctx.record:
            ctx.keep.extend([ids, add_in, ehs])
        return st

    def _emit_time_embedding(self, ctx, st, B):
        """st.temb_all = the stacked time_emb_proj rows of this step (shared with ControlNetModel, whose encoder has the same chain)"""
        boc = self.config.block_out_channels
        if st.temb_table is not None and st.t_table is not None and st.temb_table.shape[1] == B * self.temb_total:
            # the chain below depends on the step and the conditioning only, not on the latent: all steps' rows were computed once
            # per schedule (precompute_temb); the step's row is copied in (one launch instead of five)
            st.temb_all = ctx.new(B, self.temb_total)
            ctx.ew(L.EW_STEP_ROW, st.temb_all, a=st.temb_table, step=st.step, n=B * self.temb_total, descr="temb_row(step)",
                   nbytes=2.0 * B * self.temb_total * st.temb_all.element_size())
        else:
            tsin = ctx.new(B, boc[0])
            if st.t_table is not None:
                ctx.ew(L.EW_TIMESTEP, tsin, a=st.t_table, step=st.step, n=B, i=(boc[0], 0, 0, 0, 0, 0), descr="time_proj")
            else:
                ctx.ew(L.EW_TIMESTEP, tsin, a=st.t_value, n=B, i=(boc[0], 0, 0, 0, 0, 0), descr="time_proj")
            st.temb_all = self._temb_chain(ctx, tsin, st.aug_emb)
            ctx.free(tsin)

    def _latent_batch(self, S, Hl, Wl, cfg_dup):
        """the batch of a forward over S latents of Hl x Wl (2S when cfg_dup: the CFG halves share the latent, custom_pipelines.py:332);
        refuses sides the down path cannot halve"""
        div = 1 << (len(self.config.block_out_channels) - 1)
        if Hl % div or Wl % div:
            # diffusers interpolates the up path to the skip's size in that case (forward_upsample_size); the
            # fused nearest-x2 upsampling here does not, so refuse instead of producing misaligned skips
            raise L.ImhError(f"latent {Hl}x{Wl}: sides must be multiples of {div} (image sides multiples of {8 * div})")
        return 2 * S if cfg_dup else S

    def _emit_conv_in(self, ctx, st, S, B, Hl, Wl, descr, extra=None):
        """conv_in (+ CFG duplication + scale_model_input) over st.latents, fp32 NCHW [S, 4, Hl, Wl] -> NHWC [B, Hl, Wl, C0] in the compute
        dtype.  extra: fp32 [S, 5, Hl, Wl], channels 4-8 of a 9-channel conv_in"""
        c0 = self.config.block_out_channels[0]
        x = ctx.new(B, Hl, Wl, c0)
        ctx.ew(L.EW_CONV_IN, x, a=st.latents, w=_w(self.conv_in, ctx), bias=_b(self.conv_in, ctx),
               tab=st.in_scale_tab, step=st.step if st.in_scale_tab is not None else None,
               i=(S, Hl, Wl, c0, B, 9 if extra is not None else 0), f=(1.0, 0, 0, 0), descr=descr, x2=extra,
               nbytes=2.0 * B * Hl * Wl * c0)
        return x

    # ---- the encoder (down path + mid block) ----
    def _emit_encoder(self, ctx, st, h, tags, tag_step=0, prefix="", adapter=None):
        """h: the Feat after conv_in -> (the mid block's output, [h and every down-path output in skip order]).
        tags = (down ResNets / downsamplers, down transformers, mid ResNets, mid transformer); the first two advance by tag_step per
        down block; prefix goes in front of the downsamplers' descr.
        adapter: a t2i_adapter.AdapterResiduals (diffusers UNet2DConditionModel.forward with down_intrablock_additional_residuals on the
        SDXL layout; restated from its published source): feature 0 is added to the output of down block 0's downsampler, features 1 and
        2 to the output of the last attention of down blocks 1 and 2 (before block 1's downsampler), feature 3 to the mid block's output
        when the shapes match.  The sum REPLACES the tensor for every later reader, the skip connection included: upstream adds features
        1 and 2 before it appends the skip, and writes ``sample += r`` for 0 and 3 into the tensor it has already appended.  Each
        injection is one Ctx.control_add into a fresh buffer whose partials stand in for the superseded tensor's.  None: the launch
        list is what it is without the argument (the ControlNet's walk never passes one)."""
        t_res, t_attn, t_mid_res, t_mid_attn = tags
        feats = [h]
        nb = len(self.down_blocks)
        if adapter is not None and (nb != 3 or self.down_blocks[0].has_attn or not (self.down_blocks[1].has_attn and self.down_blocks[2].has_attn)):
            raise NotImplementedError("the adapter's injection points are those of the SDXL layout: DownBlock2D, CrossAttnDownBlock2D x 2, mid block")

        def inject(f, k):
            r = adapter.feats[k]
            if r.dim() != 4 or tuple(r.shape[1:]) != tuple(f.t.shape[1:]) or f.t.shape[0] % r.shape[0] or not r.is_contiguous():
                raise L.ImhError(f"adapter feature {k} {tuple(r.shape)} does not serve {tuple(f.t.shape)} (same pixels and channels, a batch that divides)")
            tag, ctx.tag = ctx.tag, 33
            # the partials of the sum stand in for the ones the superseded tensor's writer left (the ControlNet injections' gn_sub rule);
            # a tensor that had none keeps getting them from its readers' statistics pass: the step grows by these four launches exactly
            sub = gn_sub(f.t.shape[-1], self.config.norm_num_groups) if f.gs is not None else None
            y = Feat.of(ctx.control_add(f.t, r, scale=adapter.scale, tab=adapter.tab, step=adapter.step, gn_sub=sub, descr=f"adapter.{k}"))
            f.free(ctx)
            ctx.tag = tag
            return y

        for bi, blk in enumerate(self.down_blocks):
            for i, r in enumerate(blk.resnets):
                ctx.tag = t_res + bi * tag_step
                h = r.emit(ctx, h, st, keep_input=True)       # inputs are skip tensors: keep
                if blk.has_attn:
                    ctx.tag = t_attn + bi * tag_step
                    h = blk.attentions[i].emit(ctx, h, self._kv_of(st, blk.attentions[i]), st)
                    if adapter is not None and i == len(blk.resnets) - 1:
                        h = inject(h, bi)
                feats.append(h)
            if blk.downsamplers is not None:
                ctx.tag = t_res + bi * tag_step
                d = blk.downsamplers[0].conv
                h = Feat.of(ctx.conv3x3(h.t, d.packed(ctx), bias=_b(d, ctx), stride=2, descr=prefix + "downsample", gn_groups=int(GN_STATS_HANDOVER)))
                if adapter is not None and bi == 0:
                    h = inject(h, 0)
                feats.append(h)
        ctx.tag = t_mid_res
        mb = self.mid_block
        h = mb.resnets[0].emit(ctx, h, st, keep_input=True)
        ctx.tag = t_mid_attn
        h = mb.attentions[0].emit(ctx, h, self._kv_of(st, mb.attentions[0]), st)
        ctx.tag = t_mid_res
        h = mb.resnets[1].emit(ctx, h, st)
        if adapter is not None and tuple(adapter.feats[3].shape[1:]) == tuple(h.t.shape[1:]):
            h = inject(h, 3)
        return h, feats

    # ---- what the eager forwards (the diffusers signatures) start from ----
    def _eager_state(self, sample, timestep, encoder_hidden_states, added_cond_kwargs):
        """-> (an eager Ctx in the weights' 16-bit dtype, else the sample's, else bf16; the StepState of this one call: conditioning
        prepared, the timestep as explicit values, the first four channels of sample as the latents)"""
        dtype = next((d for d in (self.conv_in.weight.dtype, sample.dtype) if d in (torch.bfloat16, torch.float16)), torch.bfloat16)
        ctx = Ctx(sample.device, dtype)
        st = self.prepare_conditioning(ctx, encoder_hidden_states, added_cond_kwargs["text_embeds"], added_cond_kwargs["time_ids"])
        t = timestep if torch.is_tensor(timestep) else torch.tensor([float(timestep)])
        st.t_value = t.to(device=sample.device, dtype=torch.float32).reshape(-1).expand(sample.shape[0]).contiguous()
        st.latents = sample[:, :4].to(torch.float32).contiguous()
        return ctx, st


class UNet2DConditionModel(LoRAMixin, UNetEncoderModel):
    """(LoRAMixin: load_lora_weights / set_adapters / ... merge adapters into the weights, lora.py; a UNet without one is what it was)"""

    def __init__(self, cfg: UNetConfig = None):
        super().__init__()
        cfg = cfg or UNetConfig()
        self.config = cfg
        boc = cfg.block_out_channels
        nb = len(boc)
        if cfg.in_channels not in (4, 9):
            raise ValueError(f"in_channels must be 4 (SDXL base) or 9 (SDXL inpainting: latents, mask, masked-image latents), got {cfg.in_channels}")
        self.conv_in = Conv2d(cfg.in_channels, boc[0], 3)
        self.time_embedding = TimestepEmbedding(boc[0], cfg.time_embed_dim)
        self.add_embedding = TimestepEmbedding(cfg.projection_class_embeddings_input_dim, cfg.time_embed_dim)
        self.down_blocks = nn.ModuleList([])
        self.up_blocks = nn.ModuleList([])     # created before mid_block: fixes the attn_processors order
        out = boc[0]
        for i in range(nb):
            cin, out = out, boc[i]
            n_tf = 0 if i == 0 else cfg.transformer_layers_per_block[i]
            self.down_blocks.append(DownBlock(cin, out, cfg.layers_per_block, n_tf, cfg.attention_head_dim[i], cfg,
                                              add_down=(i != nb - 1)))
        self.mid_block = MidBlock(boc[-1], cfg.transformer_layers_per_block[-1], cfg.attention_head_dim[-1], cfg)
        rev, rev_tf = list(reversed(boc)), list(reversed(cfg.transformer_layers_per_block))
        rev_heads = list(reversed(cfg.attention_head_dim))
        out = rev[0]
        for i in range(nb):
            prev, out = out, rev[i]
            cin = rev[min(i + 1, nb - 1)]
            n_tf = 0 if i == nb - 1 else rev_tf[i]
            self.up_blocks.append(UpBlock(cin, out, prev, cfg.layers_per_block + 1, n_tf, rev_heads[i], cfg,
                                          add_up=(i != nb - 1)))
        self.conv_norm_out = Norm(boc[0], cfg.norm_eps)
        self.conv_out = Conv2d(boc[0], cfg.out_channels, 3)
        self._number_time_emb_proj()

    def resnets(self):
        yield from super().resnets()
        for blk in self.up_blocks:
            yield from blk.resnets

    # ---- FreeU (diffusers enable_freeu / disable_freeu; freeu.py states the arithmetic) ----
    freeu = None             # (s1, s2, b1, b2) or None: part of what a recorded plan is (denoise.PlanKey)

    def enable_freeu(self, s1, s2, b1, b2):
        """diffusers' UNet2DConditionModel.enable_freeu: in every ResNet of up block 0 the first half of the hidden channels is scaled
        by b1 and the skip tensor goes through fourier_filter(threshold = 1, scale = s1) before torch.cat([hidden, skip], 1); up block
        1 the same with (b2, s2); later up blocks are untouched.  SDXL's published values: s1 = 0.6, s2 = 0.4, b1 = 1.1, b2 = 1.2.
        Takes effect at the next recording (DenoiseEngine.set_schedule sees the change) and in the eager forward."""
        self.freeu = tuple(float(v) for v in (s1, s2, b1, b2))

    def disable_freeu(self):
        self.freeu = None

    def _freeu_of(self, bi):
        """(b, s) of up block bi under the current setting, or None (diffusers apply_freeu: resolution_idx 0 and 1 only)"""
        from .freeu import unet_settings
        return unet_settings(self.freeu, bi)

    # ---- perturbed-attention guidance (diffusers PAGMixin.set_pag_applied_layers; the guidance itself is the engine's: denoise.py) ----
    pag_layers = None        # the patterns as given (a tuple), or None: part of what a recorded plan is (denoise.PlanKey)

    def set_pag_applied_layers(self, layers):
        """layers: a regular expression or a list of them, each re.search-ed in the dotted names of the attn1 (self-attention) modules as
        diffusers >= 0.30 does -- "mid" (the mid block's ten layers at SDXL), "down_blocks.2", "up_blocks.0.attentions.1", "." (all) --;
        the layers any of them matches replace the attention map of the perturbed samples by the identity (out = to_out(to_v(x))).  An
        entry that matches no attn1 raises ValueError and changes nothing.  None (the default state): off.  Takes effect at the next
        recording (DenoiseEngine sees the change) and in the eager forward(..., pag=k)."""
        import re
        attn1 = [(name, mod) for name, mod in self._attentions() if name.endswith("attn1")]
        if layers is None:
            pats = ()
        else:
            pats = (layers,) if isinstance(layers, str) else tuple(layers)
            if not pats or not all(isinstance(p, str) for p in pats):
                raise ValueError(f"pag_applied_layers takes a regular expression or a non-empty list of them, got {layers!r}")
        hit = set()
        for pat in pats:
            m = {name for name, _ in attn1 if re.search(pat, name) is not None}
            if not m:
                raise ValueError(f"pag_applied_layers: {pat!r} matches no self-attention layer (attn1) of this UNet")
            hit |= m
        for name, mod in attn1:
            mod.pag_identity = name in hit
        self.pag_layers = pats or None

    def pag_layer_names(self):
        """the dotted names of the attn1 modules the current setting chooses, in module order"""
        return [name for name, mod in self._attentions() if name.endswith("attn1") and getattr(mod, "pag_identity", False)]

    # ---- the forward, as emitted ops ----
    def emit_forward(self, ctx, st, S, Hl, Wl, cfg_dup=True, control=None, adapter=None, pag=0, batch=None):
        """Records one UNet forward.  Reads st.latents (fp32 NCHW [S,4,Hl,Wl]); batch B = 2S when
        cfg_dup (CFG halves share the latent, custom_pipelines.py:332).  Returns the noise prediction
        as NHWC [B, Hl*Wl, 4] in the compute dtype.
        control: a controlnet.ControlResiduals (diffusers down_block_additional_residuals / mid_block_additional_residual): after the
        mid block and before the up path every skip and the mid output are replaced by x + g * r (Ctx.control_add, whose partials
        take the place of the superseded tensor's); the down path and the mid block have read the unmodified tensors, as upstream.
        The residuals are consumed.  None: the launch list is what it is without the argument.
        adapter: a t2i_adapter.AdapterResiduals (diffusers down_intrablock_additional_residuals): four gated adds inside the down path and
        behind the mid block (_emit_encoder); the features are per-image state and are not consumed.  Not together with control.
        pag = k > 0 (perturbed-attention guidance): k further samples BEHIND the (CFG-duplicated) batch, B = 2S + k | S + k -- batch member
        b reads latent b % S, so k = S gives [uncond | cond | perturbed] -- conditioned by the rows of st the caller put there; in the
        layers set_pag_applied_layers chose, their self-attention map is the identity.  Without chosen layers, or with a ControlNet or a
        T2I-Adapter (their branches would need the further batch member), refused.  batch: the whole batch where it is not the sum above
        (the eager forward: the last k of the samples it was given)."""
        if adapter is not None and control is not None:
            raise NotImplementedError("a T2I-Adapter together with a ControlNet is not built")
        cfg = self.config
        B = self._latent_batch(S, Hl, Wl, cfg_dup) + int(pag)
        if batch is not None:
            B = int(batch)
        if pag:
            if control is not None or adapter is not None:
                raise NotImplementedError("perturbed-attention guidance under a ControlNet or a T2I-Adapter is not built")
            if not self.pag_layers:
                raise L.ImhError("perturbed samples without chosen layers: set_pag_applied_layers first")
            if not 0 < int(pag) < B:
                raise L.ImhError(f"{pag} perturbed samples of a batch of {B}")
        if pag or getattr(st, "pag", 0):
            st.pag = int(pag)
        # -- time embedding --
        ctx.tag = 1
        self._emit_time_embedding(ctx, st, B)
        # -- conv_in (+ CFG duplication + scale_model_input) --
        ctx.tag = 2
        cin, extra = cfg.in_channels, None
        if cin == 9:
            # diffusers StableDiffusionXLInpaintPipeline (num_channels_unet == 9): cat([scale_model_input(latents), mask, masked_image_latents], 1)
            extra = getattr(st, "conv_in_extra", None)
            if extra is None or tuple(extra.shape) != (S, 5, Hl, Wl):
                raise L.ImhError(f"a UNet with in_channels = 9 reads [mask | masked-image latents] from StepState.conv_in_extra, fp32 "
                                 f"[{S}, 5, {Hl}, {Wl}]; got {None if extra is None else tuple(extra.shape)}")
        elif cin != 4:
            raise L.ImhError(f"conv_in runs 4 or 9 input channels, not {cin}")
        # (conv_in has no statistics epilogue: Feat.stats() takes one pass, shared by both readers)
        h = Feat(self._emit_conv_in(ctx, st, S, B, Hl, Wl, "conv_in", extra))
        h, skips = self._emit_encoder(ctx, st, h, (10, 20, 30, 31), 1, **({"adapter": adapter} if adapter is not None else {}))
        if control is not None:
            ctx.tag = 32
            if len(control.down) != len(skips):
                raise L.ImhError(f"{len(control.down)} ControlNet residuals for {len(skips)} skip connections")
            inject = lambda f, r, descr: Feat.of(ctx.control_add(f.t, r.view(r.shape[0], *f.t.shape[1:]), scale=control.scale, tab=control.tab, step=control.step,
                                                                 gn_sub=gn_sub(f.t.shape[-1], cfg.norm_num_groups), descr=descr))
            for i, r in enumerate(control.down):
                f = skips[i]
                skips[i] = inject(f, r, "control.skip")
                f.free(ctx); ctx.free(r)
            f = h
            h = inject(f, control.mid, "control.mid")
            f.free(ctx); ctx.free(control.mid)
        # -- up --
        for bi, blk in enumerate(self.up_blocks):
            for i, r in enumerate(blk.resnets):
                ctx.tag = 40 + bi
                fu = self._freeu_of(bi)
                if fu is not None:
                    # FreeU acts at the concat, so here it is an op of its own: one launch scales half of the hidden channels, filters
                    # the skip and writes the concatenated tensor, which the ResNet then takes as a single input (its norm1 statistics
                    # from one statistics pass; conv1 and the shortcut read the materialised tensor)
                    sk = skips.pop()
                    cat = Feat(ctx.concat(h.t, sk.t, descr="freeu.concat", freeu=(h.t.shape[-1] // 2, fu[0], fu[1])))
                    h.free(ctx); sk.free(ctx)
                    h = r.emit(ctx, cat, st)
                else:
                    h = r.emit(ctx, h, st, skip=skips.pop())      # torch.cat([hidden, skip], 1) is read from its two producers
                if blk.has_attn:
                    ctx.tag = 50 + bi
                    h = blk.attentions[i].emit(ctx, h, self._kv_of(st, blk.attentions[i]), st)
            if blk.upsamplers is not None:
                ctx.tag = 40 + bi
                u = blk.upsamplers[0].conv
                Bu, Hu, Wu, Cu = h.t.shape
                kw = dict(bias=_b(u, ctx), descr="upsample", gn_groups=int(GN_STATS_HANDOVER))
                if ctx.conv_up_phase_cfg(Bu, Hu, Wu, Cu, u.weight.shape[0]) is not None:
                    # four 2 x 2-tap phase convs on the low-res input: 4/9 of the multiply-adds of the conv over the upsampled image
                    up = Feat.of(ctx.conv3x3(h.t, None, up=2, w_phase=u.packed_phase(ctx), **kw))
                else:
                    up = Feat.of(ctx.conv3x3(h.t, u.packed(ctx), up=1, **kw))
                h.free(ctx)
                h = up
        # -- out --
        ctx.tag = 60
        Bh, Hh, Ww, C0 = h.t.shape
        n = _gn_pass(ctx, _gn_spec(ctx, self.conv_norm_out, cfg.norm_num_groups, h), h.t, True, "conv_norm_out")
        h.free(ctx)
        out = ctx.conv3x3(n, self.conv_out.packed(ctx), bias=_b(self.conv_out, ctx), descr="conv_out")
        ctx.free(n)
        ctx.tag = 0
        return out.view(B, Hh * Ww, cfg.out_channels)

    # ---- eager drop-in signature (diffusers UNet2DConditionModel.forward) ----
    @torch.no_grad()
    def forward(self, sample, timestep, encoder_hidden_states, added_cond_kwargs=None, cross_attention_kwargs=None,
                return_dict=False, **kw):
        """pag = k (keyword; default 0): the last k samples of the batch are perturbed ones -- in the layers set_pag_applied_layers chose
        their self-attention map is the identity (what diffusers' PAG processors do to the trailing chunk of the batch)"""
        pag = int(kw.pop("pag", 0))
        intra = kw.pop("down_intrablock_additional_residuals", None)
        if intra is not None:                    # a T2I-Adapter's features: four NCHW tensors, already scaled (diffusers T2IAdapter.forward's outputs)
            if kw.get("down_block_additional_residuals") is not None or kw.get("mid_block_additional_residual") is not None:
                raise NotImplementedError("down_intrablock_additional_residuals together with the ControlNet pair is not built")
            if not isinstance(intra, (list, tuple)) or len(intra) != 4:
                raise NotImplementedError("down_intrablock_additional_residuals is the list of the XL adapter's four features")
        ctx, st = self._eager_state(sample, timestep, encoder_hidden_states, added_cond_kwargs)
        B, _, Hl, Wl = sample.shape
        nhwc = lambda t: t.to(device=ctx.device, dtype=ctx.dtype).permute(0, 2, 3, 1).contiguous()
        adapter = None
        if intra is not None:
            from .t2i_adapter import AdapterResiduals
            adapter = AdapterResiduals([nhwc(t) for t in intra])
        if sample.shape[1] == 9:                 # the inpainting UNet's [latents | mask | masked-image latents]
            st.conv_in_extra = sample[:, 4:].to(torch.float32).contiguous()
        control = None
        down_res, mid_res = kw.pop("down_block_additional_residuals", None), kw.pop("mid_block_additional_residual", None)
        if (down_res is None) != (mid_res is None):
            raise NotImplementedError("ControlNet residuals come as the pair down_block_additional_residuals + mid_block_additional_residual")
        if down_res is not None:                 # NCHW, already scaled (diffusers ControlNetModel.forward's outputs)
            from .controlnet import ControlResiduals
            control = ControlResiduals([nhwc(t) for t in down_res], nhwc(mid_res))
        out = self.emit_forward(ctx, st, B, Hl, Wl, cfg_dup=False, control=control, **({"adapter": adapter} if adapter is not None else {}),
                                **({"pag": pag, "batch": B} if pag else {}))
        y = out.view(B, Hl, Wl, -1).permute(0, 3, 1, 2).to(sample.dtype)
        return (y,)
