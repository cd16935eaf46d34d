"""SDXL VAE decode on the HIP path -- the row right after the denoise loop:
``image = vae.decode(latents / scaling_factor)`` (ip_adapter/custom_pipelines.py:365-379, run in fp32 upstream
because the SDXL VAE overflows in fp16; test.py:73 turns tiling on) and ``image_processor.postprocess`` (:386).

Same parameter names as diffusers' ``AutoencoderKL`` (``decoder.*``, ``post_quant_conv.*``; encoder keys are accepted
and ignored -- or, with ``with_encoder=True``, held and loaded strictly), so a real SDXL VAE state dict drops in.  The encoder
(``encode``, image-to-image) runs the same two compute modes on the same kernels; its downsamplers are the stride-2 conv3x3 with
right / bottom padding (imh_gemm_args.pad = 1, diffusers ``Downsample2D(padding=0)``).  Two compute modes, chosen like the reference chooses
(``needs_upcasting = vae.dtype == float16 and vae.config.force_upcast`` -> ``upcast_vae()``, custom_pipelines.py:366-372):

* **fp32** (round 6; a float16 module with ``force_upcast``, or a float32 module): fp32 activations, fp32 weights (the stored
  weights upcast exactly, as ``vae.to(float32)`` does) and fp32 arithmetic on the fp32 kernels of csrc/f32.hip
  (``v_mfma_f32_32x32x2_f32`` implicit-GEMM conv3x3 / GEMM, GroupNorm statistics merged in double, row softmax) -- the
  reference's precision, no fp16 overflow; ~0.1 s per 1024^2 image (the fp32 matrix rate is 1/16 of bf16's).
* **native** (a bfloat16 module -- which the reference does not upcast either -- or ``precision="native"``): NHWC activations
  in the module's 16-bit dtype on the UNet's own kernels -- GroupNorm(+SiLU), implicit-GEMM conv3x3 (fused nearest-x2
  upsampling), GEMM -- 18 ms per image, 1e-2 rel-RMS from the fp32 result in bf16.

Both run a materialised single-head attention for the mid block (scores GEMM -> fp32 row softmax -> PV GEMM: one head of
width 512 does not fit the head_dim-64 flash kernel, and it runs once per image).  Tiled decoding follows diffusers'
``tiled_decode`` (overlapping 64x64-latent tiles, linear blends).  Host-side torch is plumbing only: channel padding
of the 4-channel latent, the tile blends / concatenation, and the final NHWC->image conversion.

The graph is written once: ``_decode_walk`` / ``_encode_walk`` (and the ResNet block, attention and mid block under them) run against a
back-end object, ``_Native`` or ``_F32``, that owns what differs between the modes; the modules below only hold parameters.
"""
from dataclasses import dataclass
from typing import Tuple

import torch
import torch.nn as nn

from . import lib as L
from .attention_processor import _b, _w
from .ctx import Ctx
from .derived import derived
from .unet import Conv2d, Linear, Norm


@dataclass
class VAEConfig:
    in_channels: int = 3
    out_channels: int = 3
    latent_channels: int = 4
    block_out_channels: Tuple[int, ...] = (128, 256, 512, 512)
    layers_per_block: int = 2
    norm_num_groups: int = 32
    sample_size: int = 1024
    scaling_factor: float = 0.13025
    force_upcast: bool = True
    tile_overlap_factor: float = 0.25


class ResnetBlock2D(nn.Module):
    def __init__(self, cin, cout, groups):
        super().__init__()
        self.groups = groups
        self.norm1 = Norm(cin, 1e-6)
        self.conv1 = Conv2d(cin, cout, 3)
        self.norm2 = Norm(cout, 1e-6)
        self.conv2 = Conv2d(cout, cout, 3)
        self.conv_shortcut = Conv2d(cin, cout, 1) if cin != cout else None


class VAEAttention(nn.Module):
    """mid-block attention: heads = 1, GroupNorm over the tokens, projections with bias, residual"""

    def __init__(self, channels, groups):
        super().__init__()
        self.groups = groups
        self.group_norm = Norm(channels, 1e-6)
        self.to_q = Linear(channels, channels)
        self.to_k = Linear(channels, channels)
        self.to_v = Linear(channels, channels)
        self.to_out = nn.ModuleList([Linear(channels, channels), nn.Identity()])


class Upsample2D(nn.Module):
    def __init__(self, ch):
        super().__init__()
        self.conv = Conv2d(ch, ch, 3)


class UpDecoderBlock2D(nn.Module):
    def __init__(self, cin, cout, n, groups, up):
        super().__init__()
        self.resnets = nn.ModuleList([ResnetBlock2D(cin if i == 0 else cout, cout, groups) for i in range(n)])
        if up:
            self.upsamplers = nn.ModuleList([Upsample2D(cout)])


class Downsample2D(nn.Module):
    """diffusers Downsample2D(padding=0): conv3x3(F.pad(x, (0, 1, 0, 1)), stride 2) -- the pad is the conv's padding mode 1"""

    def __init__(self, ch):
        super().__init__()
        self.conv = Conv2d(ch, ch, 3)


class DownEncoderBlock2D(nn.Module):
    def __init__(self, cin, cout, n, groups, down):
        super().__init__()
        self.resnets = nn.ModuleList([ResnetBlock2D(cin if i == 0 else cout, cout, groups) for i in range(n)])
        if down:
            self.downsamplers = nn.ModuleList([Downsample2D(cout)])


class MidBlock(nn.Module):
    def __init__(self, ch, groups):
        super().__init__()
        self.attentions = nn.ModuleList([VAEAttention(ch, groups)])
        self.resnets = nn.ModuleList([ResnetBlock2D(ch, ch, groups), ResnetBlock2D(ch, ch, groups)])


class Decoder(nn.Module):
    def __init__(self, cfg: VAEConfig):
        super().__init__()
        ch = tuple(reversed(cfg.block_out_channels))
        g = cfg.norm_num_groups
        self.groups = g
        self.conv_in = Conv2d(cfg.latent_channels, ch[0], 3)
        self.mid_block = MidBlock(ch[0], g)
        self.up_blocks = nn.ModuleList()
        c = ch[0]
        for i, co in enumerate(ch):
            self.up_blocks.append(UpDecoderBlock2D(c, co, cfg.layers_per_block + 1, g, up=i < len(ch) - 1))
            c = co
        self.conv_norm_out = Norm(ch[-1], 1e-6)
        self.conv_out = Conv2d(ch[-1], cfg.out_channels, 3)


class Encoder(nn.Module):
    """diffusers Encoder (down blocks, mid block, GroupNorm + SiLU, conv_out to the 2 x latent_channels moments), double_z"""

    def __init__(self, cfg: VAEConfig):
        super().__init__()
        ch = cfg.block_out_channels
        g = cfg.norm_num_groups
        self.groups = g
        self.conv_in = Conv2d(cfg.in_channels, ch[0], 3)
        self.down_blocks = nn.ModuleList()
        c = ch[0]
        for i, co in enumerate(ch):
            self.down_blocks.append(DownEncoderBlock2D(c, co, cfg.layers_per_block, g, down=i < len(ch) - 1))
            c = co
        self.mid_block = MidBlock(ch[-1], g)
        self.conv_norm_out = Norm(ch[-1], 1e-6)
        self.conv_out = Conv2d(ch[-1], 2 * cfg.latent_channels, 3)


class DiagonalGaussianDistribution:
    """diffusers DiagonalGaussianDistribution over the moments [B, 2 C, h, w] (fp32): logvar clamped to [-30, 20]"""

    def __init__(self, parameters):
        self.parameters = parameters
        self.mean, self.logvar = torch.chunk(parameters, 2, dim=1)
        self.logvar = torch.clamp(self.logvar, -30.0, 20.0)
        self.std = torch.exp(0.5 * self.logvar)
        self.var = torch.exp(self.logvar)

    def sample(self, generator=None):
        """diffusers: mean + std * randn_tensor(mean.shape, generator, dtype=fp32) -- drawn on the generator's device"""
        from .pipeline import randn_latents
        return self.mean + self.std * randn_latents(self.mean.shape, generator).to(self.parameters.device)

    def mode(self):
        return self.mean


@dataclass
class AutoencoderKLOutput:
    latent_dist: DiagonalGaussianDistribution


def _pad_1x1(conv, cpad, dtype, device):
    """a 1 x 1 conv as a [cpad, cpad] matrix and a [cpad] bias, zero-padded, cached per cpad"""
    def build():
        w = conv.weight.detach().view(conv.weight.shape[0], -1)
        wp = torch.zeros(cpad, cpad, dtype=w.dtype, device=w.device)
        wp[:w.shape[0], :w.shape[1]] = w
        bp = torch.zeros(cpad, dtype=w.dtype, device=w.device)
        bp[:w.shape[0]] = conv.bias.detach()
        return wp.to(device=device, dtype=dtype).contiguous(), bp.to(device=device, dtype=dtype)
    return derived(conv, f"_imh_padded{cpad}", (conv.weight, conv.bias), build, where=(dtype, str(device)), extra=(cpad,))


def _f32_w(mod, cin_pad=0):
    """a Linear's [N, K], or a conv's [Cout, Cin, k, k] -> packed [Cout, k*k * Cin'] (K index = (ky*k+kx)*Cin' + c) with Cin zero-padded
    to cin_pad, in fp32 where the weight lives; cached"""
    def build():
        w = mod.weight.detach().float()
        if w.dim() == 4:
            if cin_pad > w.shape[1]:
                wp = torch.zeros(w.shape[0], cin_pad, *w.shape[2:], dtype=torch.float32, device=w.device)
                wp[:, :w.shape[1]] = w
                w = wp
            w = w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)
        return w.contiguous()
    return derived(mod, "_imh_f32_w", (mod.weight,), build, where=(str(mod.weight.device),), extra=(cin_pad,))


def _f32_vec(mod, attr="bias"):
    """``mod.<attr>`` in fp32 where it lives; cached"""
    t = getattr(mod, attr)
    return derived(mod, "_imh_f32_" + attr, (t,), lambda: t.detach().float().contiguous(), where=(str(t.device),))


# ---- the two back ends: everything that differs between the compute modes; the walks below are written once against them ----
class _Native:
    """16-bit: NHWC activations in the module's dtype on the UNet's own kernels"""
    pre = "vae."        # descr prefix
    kstep = 64          # the K step of the GEMM / implicit-GEMM kernels: the few-channel inputs and the attention's keys are padded to it

    def __init__(self, device, dtype):
        if dtype not in (torch.bfloat16, torch.float16):
            raise L.ImhError("the native HIP VAE path computes in bf16 or fp16 (precision='fp32' runs any module in fp32)")
        self.ctx = ctx = Ctx(device, dtype)
        self.dtype = dtype
        self.conv3x3, self.gemm = ctx.conv3x3, ctx.gemm

    def w(self, mod, cin_pad=False):
        if cin_pad:     # conv_in reads a 3- / 4-channel input: Cin zero-padded to 64 so it runs on the implicit-GEMM kernel (K = 9*64)
            return mod.packed_padded(self.ctx, pad_out=False)[0]
        return mod.packed(self.ctx) if mod.weight.dim() == 4 else _w(mod, self.ctx)

    def b(self, mod):
        return _b(mod, self.ctx)

    def groupnorm(self, norm, x, groups, silu, descr):
        return self.ctx.groupnorm(x, _w(norm, self.ctx), _b(norm, self.ctx), groups, norm.eps, silu=silu, descr=descr)

    def probs_scratch(self, Lq, Lp):
        """fp32 scores and the probabilities in the compute dtype.  The softmax runs over Ls >= Lq columns (a multiple of 4) whose tail
        holds -inf scores (weight 0); the scores GEMM writes the Lq real ones"""
        ctx, Ls = self.ctx, (Lq + 3) // 4 * 4
        if Ls == Lq:
            sc = ctx.new(Lq, Lp, dtype=torch.float32)
        else:
            sc = ctx.zeros(Lq, Lp, dtype=torch.float32)
            sc[:, Lq:Ls] = float("-inf")                                                    # plumbing: the softmax's padded columns
        return sc, (ctx.new(Lq, Lp) if Lp == Lq else ctx.zeros(Lq, Lp))

    def probs(self, q, k, scratch, scale):
        sc, pr = scratch
        (Lq, Lp), Ls = pr.shape, (pr.shape[0] + 3) // 4 * 4
        self.ctx.gemm(q, k, out=sc[:, :Lq], flags=L.GF_OUT_F32, descr="vae.attn.scores")   # [L, L] fp32
        self.ctx.ew(L.EW_SOFTMAX, pr, a=sc, i=(Lq, Ls, Lp, Lp, 0, 0), f=(scale, 0.0, 0.0, 0.0), descr="vae.attn.softmax", nbytes=6.0 * Lq * Ls)
        return pr

    def post_quant(self, conv, zp):
        wq, bq = _pad_1x1(conv, self.kstep, self.dtype, self.ctx.device)
        return self.ctx.gemm(zp, wq, bias=bq, descr="vae.post_quant")

    def quant(self, conv, yp, c2):
        wq, bq = _pad_1x1(conv, self.kstep, self.dtype, self.ctx.device)
        m = torch.empty(yp.shape[0], self.kstep, dtype=torch.float32, device=yp.device)
        self.ctx.gemm(yp, wq, bias=bq, out=m, flags=L.GF_OUT_F32, descr="vae.enc.quant_conv")                 # fp32 moments
        return m[:, :c2]

    def image(self, y):
        return y.permute(0, 3, 1, 2).float()


class _F32:
    """fp32 (reference precision): fp32 activations, the stored weights upcast exactly, every product in fp32 on csrc/f32.hip"""
    pre = "vae32."
    kstep = 16
    dtype = torch.float32

    def __init__(self, device):
        self.ctx = ctx = Ctx(device, torch.bfloat16)                            # (pool / stream only: every tensor is fp32)
        self.conv3x3, self.gemm = ctx.f32_conv3x3, ctx.f32_gemm

    def w(self, mod, cin_pad=False):
        return _f32_w(mod, self.kstep if cin_pad else 0)

    def b(self, mod):
        return _f32_vec(mod)

    def groupnorm(self, norm, x, groups, silu, descr):
        return self.ctx.f32_groupnorm(x, _f32_vec(norm, "weight"), _f32_vec(norm, "bias"), groups, norm.eps, silu=silu, descr=descr)

    def probs_scratch(self, Lq, Lp):
        ctx = self.ctx
        return (ctx.new(Lq, Lq, dtype=torch.float32) if Lp == Lq else ctx.zeros(Lq, Lp, dtype=torch.float32),)

    def probs(self, q, k, scratch, scale):
        sc, Lq = scratch[0], q.shape[0]
        self.ctx.f32_gemm(q, k, out=sc[:, :Lq], descr="vae32.attn.scores")
        self.ctx.f32_softmax(sc[:, :Lq], sc[:, :Lq], scale, descr="vae32.attn.softmax")     # in place (a row is read before it is written)
        return sc

    def post_quant(self, conv, zp):
        wq, bq = _pad_1x1(conv, self.kstep, torch.float32, self.ctx.device)
        return self.ctx.f32_gemm(zp, wq, bias=bq, descr="vae32.post_quant")

    def quant(self, conv, yp, c2):
        return self.ctx.f32_gemm(yp, _f32_w(conv, self.kstep), bias=_f32_vec(conv), descr="vae32.enc.quant_conv").clone()

    def image(self, y):
        return y.permute(0, 3, 1, 2).contiguous()


def _gn(be, norm, x, groups, silu, descr):
    B, H, W, C_ = x.shape
    return be.groupnorm(norm, x.view(B, H * W, C_), groups, silu, be.pre + descr).view(B, H, W, C_)


def _conv(be, conv, x, descr, **kw):
    """x NHWC (consumed) -> conv3x3(x)"""
    out = be.conv3x3(x, be.w(conv), bias=be.b(conv), descr=be.pre + descr, **kw)
    be.ctx.free(x)
    return out


def _resnet(be, r, x):
    """x NHWC [B, H, W, Cin] (consumed) -> [B, H, W, Cout]"""
    ctx = be.ctx
    B, H, W, Cin = x.shape
    h = _conv(be, r.conv1, _gn(be, r.norm1, x, r.groups, True, "res.norm1"), "res.conv1")
    n = _gn(be, r.norm2, h, r.groups, True, "res.norm2")
    ctx.free(h)
    sc = x.view(B * H * W, Cin)
    if r.conv_shortcut is not None:
        sc = be.gemm(sc, be.w(r.conv_shortcut), bias=be.b(r.conv_shortcut), descr=be.pre + "res.shortcut")
    out = _conv(be, r.conv2, n, "res.conv2", residual=sc)
    if r.conv_shortcut is not None:
        ctx.free(sc)
    ctx.free(x)
    return out


def _attention(be, at, x):
    ctx = be.ctx
    B, H, W, C_ = x.shape
    Lq = H * W
    # a token count that is not a multiple of the PV GEMM's K step (a 100 x 100 latent): that GEMM runs over Lp keys from a probability
    # matrix and a V^T whose padded keys are zero-filled and never written, so they contribute exact zeros; the scores GEMM runs over
    # the Lq real keys
    Lp = (Lq + be.kstep - 1) // be.kstep * be.kstep
    n = _gn(be, at.group_norm, x, at.groups, False, "attn.norm").view(B * Lq, C_)
    q = be.gemm(n, be.w(at.to_q), bias=be.b(at.to_q), descr=be.pre + "attn.to_q")
    k = be.gemm(n, be.w(at.to_k), bias=be.b(at.to_k), descr=be.pre + "attn.to_k")
    # V^T = Wv n^T (swapped operands) feeds the PV GEMM as its [N, K] operand; softmax rows sum to 1, so the
    # to_v bias is added once after PV instead of to every value row
    if Lp == Lq:
        vt = be.gemm(be.w(at.to_v), n, descr=be.pre + "attn.to_v^T")                        # [C, B*L]
    else:
        vt = ctx.zeros(C_, B * Lp, dtype=be.dtype)                                          # [C, B*Lp], batch b's keys at b*Lp
        for b in range(B):
            be.gemm(be.w(at.to_v), n[b * Lq:(b + 1) * Lq], out=vt[:, b * Lp:b * Lp + Lq], descr=be.pre + "attn.to_v^T")
    ctx.free(n)
    o = ctx.new(B * Lq, C_, dtype=be.dtype)
    scratch = be.probs_scratch(Lq, Lp)
    for b in range(B):
        pr = be.probs(q[b * Lq:(b + 1) * Lq], k[b * Lq:(b + 1) * Lq], scratch, C_ ** -0.5)  # [Lq, Lp]
        be.gemm(pr, vt[:, b * Lp:(b + 1) * Lp], out=o[b * Lq:(b + 1) * Lq], bias=be.b(at.to_v), N=C_, K=Lp, ldw=B * Lp,
                descr=be.pre + "attn.pv")
    for t in (*scratch, q, k, vt):
        ctx.free(t)
    out = be.gemm(o, be.w(at.to_out[0]), bias=be.b(at.to_out[0]), residual=x.view(B * Lq, C_), descr=be.pre + "attn.to_out")
    ctx.free(o); ctx.free(x)
    return out.view(B, H, W, C_)


def _mid(be, mb, x):
    return _resnet(be, mb.resnets[1], _attention(be, mb.attentions[0], _resnet(be, mb.resnets[0], x)))


def _padded_input(be, x):
    """NCHW fp32 -> NHWC in the back end's dtype, the channels zero-padded to its K step (plumbing)"""
    B, c, H, W = x.shape
    xp = torch.zeros(B, H, W, be.kstep, dtype=be.dtype, device=x.device)
    xp[..., :c] = x.permute(0, 2, 3, 1).to(be.dtype)
    return xp


def _head(be, net, x, pre):
    """conv_out(silu(conv_norm_out(x))), x consumed"""
    n = _gn(be, net.conv_norm_out, x, net.groups, True, pre + "conv_norm_out")
    be.ctx.free(x)
    return _conv(be, net.conv_out, n, pre + "conv_out")


def _decode_walk(be, vae, z):
    """z: [B, 4, h, w] fp32 on the device -> [B, 3, 8h, 8w] fp32"""
    d = vae.decoder
    zp = _padded_input(be, z)
    B, h, w, kp = zp.shape
    t = be.post_quant(vae.post_quant_conv, zp.view(B * h * w, kp)).view(B, h, w, kp)
    x = be.conv3x3(t, be.w(d.conv_in, cin_pad=True), bias=be.b(d.conv_in), descr=be.pre + "conv_in")
    be.ctx.free(t)
    x = _mid(be, d.mid_block, x)
    for blk in d.up_blocks:
        for r in blk.resnets:
            x = _resnet(be, r, x)
        for u in getattr(blk, "upsamplers", []):
            x = _conv(be, u.conv, x, "upsample", up=1)                                      # nearest x2 fused
    return be.image(_head(be, d, x, ""))                                                    # [B, 8h, 8w, 3] -> NCHW


def _encode_walk(be, vae, x):
    """x: [B, 3, H, W] fp32 on the device -> the moments quant_conv(encoder(x)) as NHWC [B, h, w, 2 C] fp32"""
    e = vae._encoder()
    h = be.conv3x3(_padded_input(be, x), be.w(e.conv_in, cin_pad=True), bias=be.b(e.conv_in), descr=be.pre + "enc.conv_in")
    for blk in e.down_blocks:
        for r in blk.resnets:
            h = _resnet(be, r, h)
        for d in getattr(blk, "downsamplers", []):
            h = _conv(be, d.conv, h, "enc.downsample", stride=2, pad=1)
    y = _head(be, e, _mid(be, e.mid_block, h), "enc.")                                      # [B, h, w, 2C]
    B, hh, ww, c2 = y.shape
    yp = torch.zeros(B * hh * ww, be.kstep, dtype=be.dtype, device=x.device)                # plumbing: K padded to the K step
    yp[:, :c2] = y.view(-1, c2)
    be.ctx.free(y)
    return be.quant(vae.quant_conv, yp, c2).reshape(B, hh, ww, c2)


class AutoencoderKL(nn.Module):
    """AutoencoderKL.  ``decode(z)`` returns the image tensor [B, 3, 8h, 8w] (fp32, roughly [-1, 1]); with ``with_encoder=True``
    ``encode(x)`` returns diffusers' ``AutoencoderKLOutput`` (``.latent_dist``) of an image tensor [B, 3, H, W] in [-1, 1]."""

    def __init__(self, config: VAEConfig = None, with_encoder=False):
        super().__init__()
        self.config = config or VAEConfig()
        c = self.config
        # decoder first: init_random_(s) draws the decoder's weights identically with or without the encoder
        self.decoder = Decoder(c)
        self.post_quant_conv = Conv2d(c.latent_channels, c.latent_channels, 1)
        self.with_encoder = bool(with_encoder)
        if self.with_encoder:
            self.encoder = Encoder(c)
            self.quant_conv = Conv2d(2 * c.latent_channels, 2 * c.latent_channels, 1)
        self.use_tiling = False
        self.tile_sample_min_size = c.sample_size if c.sample_size < 512 else 512
        self.tile_latent_min_size = int(self.tile_sample_min_size / (2 ** (len(c.block_out_channels) - 1)))
        self.tile_overlap_factor = c.tile_overlap_factor

    # -- loading --
    def load_state_dict(self, sd, strict=True, **kw):
        if not self.with_encoder:
            sd = {k: v for k, v in sd.items() if not (k.startswith("encoder.") or k.startswith("quant_conv."))}
        return super().load_state_dict(sd, strict=strict, **kw)

    @classmethod
    def from_safetensors(cls, path, config: VAEConfig = None, device="cuda:0", dtype=torch.bfloat16, with_encoder=False):
        from safetensors.torch import load_file
        m = cls(config, with_encoder=with_encoder)
        m.load_state_dict(load_file(path), strict=True)
        return m.to(device, dtype)

    def init_random_(self, seed=0):
        g = torch.Generator().manual_seed(seed)
        for n, p in self.named_parameters():
            if p.dim() > 1:
                fan = p[0].numel()
                p.data.copy_((torch.randn(p.shape, generator=g) * fan ** -0.5).to(p.dtype))
            else:
                p.data.fill_(1.0 if n.endswith("weight") else 0.0)
        return self

    def enable_tiling(self, on=True):                 # pipe.enable_vae_tiling(), test.py:73
        self.use_tiling = on

    @property
    def dtype(self):
        return self.decoder.conv_in.weight.dtype

    # -- compute --
    def precision_for(self, precision=None):
        """'fp32' | 'native': the reference's rule (custom_pipelines.py:366-372) unless the caller names one"""
        precision = precision or getattr(self, "precision", "auto")
        if precision == "auto":
            dt = self.dtype
            precision = "fp32" if dt == torch.float32 or (dt == torch.float16 and self.config.force_upcast) else "native"
        if precision not in ("fp32", "native"):
            raise ValueError(f"precision {precision!r} (expected 'auto', 'fp32' or 'native')")
        return precision

    def _backend(self, device, precision):
        return _F32(device) if precision == "fp32" else _Native(device, self.dtype)

    def _decode_tile(self, z, precision="native"):
        """z: [B, 4, h, w] fp32 on the device -> [B, 3, 8h, 8w] fp32"""
        return _decode_walk(self._backend(z.device, precision), self, z)

    @staticmethod
    def _blend(a, b, extent, dim):
        """diffusers blend_v (dim 2) / blend_h (dim 3): linear cross-fade of b's first `extent` rows with a's last"""
        extent = min(a.shape[dim], b.shape[dim], extent)
        wgt = (torch.arange(extent, device=b.device, dtype=b.dtype) / extent).view([-1 if i == dim else 1 for i in range(4)])
        head = a.narrow(dim, a.shape[dim] - extent, extent) * (1 - wgt) + b.narrow(dim, 0, extent) * wgt
        return torch.cat([head, b.narrow(dim, extent, b.shape[dim] - extent)], dim)

    def _stitch(self, x, tile, stride, extent, limit, fn):
        """diffusers tiled_decode / tiled_encode: overlapping tiles of `tile` at `stride`, fn per tile (NCHW -> NCHW), in-place blend_v /
        blend_h over `extent` rows / columns, crop to `limit`, concatenate"""
        # every operation of the decoder / encoder is per sample, so the tiles of one shape run as ONE batch (round 6: 3 x 3 tiles of a 128 x 128
        # latent = 4 launches' worth of work instead of 9 under-filled ones; in the fp32 path the same bits per tile as one tile at a time, in the
        # 16-bit path the same to rounding -- there the GEMM variant depends on M)
        ii, jj = list(range(0, x.shape[2], stride)), list(range(0, x.shape[3], stride))
        tiles = {(i, j): x[:, :, i:i + tile, j:j + tile] for i in ii for j in jj}
        groups = {}
        for key, t in tiles.items():
            groups.setdefault(tuple(t.shape[2:]), []).append(key)
        done = {}
        for keys in groups.values():
            out = fn(torch.cat([tiles[k] for k in keys], 0).contiguous())
            for k, o in zip(keys, out.split(x.shape[0], 0)):
                done[k] = o
        rows = [[done[(i, j)] for j in jj] for i in ii]
        out_rows = []
        for i, row in enumerate(rows):
            out = []
            for j, t in enumerate(row):
                if i > 0:
                    t = self._blend(rows[i - 1][j], t, extent, 2)
                if j > 0:
                    t = self._blend(row[j - 1], t, extent, 3)
                row[j] = t               # diffusers blends in place: later tiles see the blended neighbour
                out.append(t[:, :, :limit, :limit])
            out_rows.append(torch.cat(out, dim=3))
        return torch.cat(out_rows, dim=2)

    def tiled_decode(self, z, precision="native"):
        lat, px, f = self.tile_latent_min_size, self.tile_sample_min_size, self.tile_overlap_factor
        return self._stitch(z, lat, int(lat * (1 - f)), int(px * f), px - int(px * f), lambda t: self._decode_tile(t, precision))

    @torch.no_grad()
    def decode(self, z, precision=None):
        """precision: None / 'auto' = the reference's rule (fp32 for a float16 module with force_upcast or a float32 module, the module's
        16-bit dtype for bfloat16); 'fp32' / 'native' force a mode"""
        precision = self.precision_for(precision)
        z = z.to(self.decoder.conv_in.weight.device, torch.float32)
        if self.use_tiling and (z.shape[-1] > self.tile_latent_min_size or z.shape[-2] > self.tile_latent_min_size):
            return self.tiled_decode(z, precision)
        return self._decode_tile(z, precision)

    # -- encode (image-to-image) --
    def _encoder(self):
        if not self.with_encoder:
            raise NotImplementedError("this AutoencoderKL holds no encoder: construct it with with_encoder=True (image-to-image)")
        return self.encoder

    def _encode_tile(self, x, precision="native"):
        """x: [B, 3, H, W] fp32 on the device -> moments NHWC [B, h, w, 2 C] fp32"""
        return _encode_walk(self._backend(x.device, precision), self, x)

    def tiled_encode(self, x, precision="native"):
        """diffusers 0.30 tiled_encode: tiles of tile_sample_min_size px at stride (1 - overlap) of that, encoder + quant_conv per tile,
        blends over int(tile_latent_min_size * overlap) latent rows, crop to tile_latent_min_size - blend_extent.
        Returns NCHW moments [B, 2 C, h, w]."""
        lat, px, f = self.tile_latent_min_size, self.tile_sample_min_size, self.tile_overlap_factor
        return self._stitch(x, px, int(px * (1 - f)), int(lat * f), lat - int(lat * f),
                            lambda t: self._encode_tile(t, precision).permute(0, 3, 1, 2))

    @torch.no_grad()
    def encode_moments(self, x, precision=None):
        """x: [B, 3, H, W] in [-1, 1], H and W multiples of 8 -> the moments quant_conv(encoder(x)) as NHWC [B, H/8, W/8, 2 C] fp32
        (the layout the img2img initial-latents op reads).  Tiled like diffusers when use_tiling and a side exceeds tile_sample_min_size."""
        precision = self.precision_for(precision)
        self._encoder()
        if x.dim() != 4 or x.shape[1] != self.config.in_channels or x.shape[2] % 8 or x.shape[3] % 8:
            raise ValueError(f"encode: expected an image [B, {self.config.in_channels}, H, W] with H and W multiples of 8, got {tuple(x.shape)}")
        x = x.to(self.decoder.conv_in.weight.device, torch.float32)
        if self.use_tiling and (x.shape[-1] > self.tile_sample_min_size or x.shape[-2] > self.tile_sample_min_size):
            return self.tiled_encode(x, precision).permute(0, 2, 3, 1).contiguous()
        return self._encode_tile(x, precision).contiguous()

    @torch.no_grad()
    def encode(self, x, precision=None):
        """diffusers AutoencoderKL.encode: -> AutoencoderKLOutput(latent_dist=DiagonalGaussianDistribution(moments [B, 2 C, h, w] fp32)).
        precision: as decode (the reference upcasts an fp16 VAE with force_upcast for encode too)"""
        return AutoencoderKLOutput(DiagonalGaussianDistribution(self.encode_moments(x, precision).permute(0, 3, 1, 2).contiguous()))


def preprocess(image):
    """VaeImageProcessor.preprocess (do_resize, do_normalize, vae_scale_factor 8, resample 'lanczos') for the img2img input:
    a PIL image, a list of them, or a float tensor [B, 3, H, W] / [3, H, W] -> fp32 [B, 3, H, W] in [-1, 1].  Sides that are not
    multiples of 8 are resized DOWN to the next multiple (PIL: Lanczos; tensor: nearest, F.interpolate's default); PIL pixels /255;
    then 2 x - 1 -- except for a tensor with min() < 0, which is taken as already in [-1, 1]."""
    import numpy as np
    try:
        from PIL import Image
    except ImportError:                                    # pragma: no cover - PIL ships with torchvision / diffusers installs
        Image = None
    if Image is not None and isinstance(image, Image.Image):
        image = [image]
    if isinstance(image, (list, tuple)):
        if not image or Image is None or not all(isinstance(i, Image.Image) for i in image):
            raise ValueError("preprocess: expected a PIL image, a list of PIL images or a tensor [B, 3, H, W]")
        w, h = image[0].size
        w, h = w - w % 8, h - h % 8
        arrs = []
        for im in image:
            if im.mode != "RGB":
                im = im.convert("RGB")
            if im.size != (w, h):
                im = im.resize((w, h), resample=Image.LANCZOS)
            arrs.append(np.asarray(im).astype(np.float32) / 255.0)
        x = torch.from_numpy(np.stack(arrs, 0)).permute(0, 3, 1, 2).contiguous()
        return 2.0 * x - 1.0
    if not torch.is_tensor(image):
        raise ValueError(f"preprocess: unsupported image type {type(image).__name__}")
    x = image.unsqueeze(0) if image.dim() == 3 else image
    if x.dim() != 4:
        raise ValueError(f"preprocess: expected [B, C, H, W], got {tuple(image.shape)}")
    x = x.float()
    h, w = x.shape[2] - x.shape[2] % 8, x.shape[3] - x.shape[3] % 8
    if (h, w) != tuple(x.shape[2:]):
        x = torch.nn.functional.interpolate(x, size=(h, w))
    if x.min() < 0:
        return x
    return 2.0 * x - 1.0


def preprocess_mask(mask_image, height, width):
    """diffusers StableDiffusionXLInpaintPipeline.mask_processor.preprocess(mask_image, height, width): a VaeImageProcessor with
    do_normalize=False, do_binarize=True, do_convert_grayscale=True.  A PIL image, a list of them, or a float tensor in [0, 1] of shape
    [H, W], [B, H, W] (a channel axis is inserted at 1, as upstream) or [B, 1, H, W] -> fp32 [B, 1, height, width] of zeros and ones
    (1 = repaint).  Resized to the image's size by preprocess's rules (PIL: Lanczos, then mode "L", pixels / 255; tensor: nearest),
    then binarised at 0.5: < 0.5 -> 0, else 1.  A mask that cannot be brought to one channel raises ValueError."""
    import numpy as np
    try:
        from PIL import Image
    except ImportError:                                    # pragma: no cover
        Image = None
    if Image is not None and isinstance(mask_image, Image.Image):
        mask_image = [mask_image]
    if isinstance(mask_image, (list, tuple)):
        if not mask_image or Image is None or not all(isinstance(i, Image.Image) for i in mask_image):
            raise ValueError("preprocess_mask: expected a PIL image, a list of PIL images or a tensor")
        arrs = []
        for im in mask_image:
            if im.size != (width, height):
                im = im.resize((width, height), resample=Image.LANCZOS)
            arrs.append(np.asarray(im.convert("L")).astype(np.float32) / 255.0)
        m = torch.from_numpy(np.stack(arrs, 0)).unsqueeze(1)
    elif torch.is_tensor(mask_image):
        m = mask_image.float()
        if m.dim() == 2:
            m = m[None, None]
        elif m.dim() == 3:
            m = m.unsqueeze(1)
        if m.dim() != 4 or m.shape[1] != 1:
            raise ValueError(f"preprocess_mask: a tensor mask is [H, W], [B, H, W] or [B, 1, H, W], got {tuple(mask_image.shape)}")
        if tuple(m.shape[2:]) != (height, width):
            m = torch.nn.functional.interpolate(m, size=(height, width))
    else:
        raise ValueError(f"preprocess_mask: unsupported mask type {type(mask_image).__name__}")
    return (m >= 0.5).to(torch.float32).contiguous()


def latent_mask(mask, h, w):
    """prepare_mask_latents: F.interpolate(mask, size=(h, w)) -- nearest, source index floor(i * H / h) -- of a binary [B, 1, H, W] mask"""
    return torch.nn.functional.interpolate(mask, size=(h, w)).contiguous()


def decode_latents(vae: AutoencoderKL, latents, precision=None):
    """custom_pipelines.py:365-379"""
    return vae.decode(latents.float() / vae.config.scaling_factor, precision=precision)


def postprocess(image, output_type="pil"):
    """VaeImageProcessor.postprocess (do_normalize=True), custom_pipelines.py:386: 'pt' | 'np' | 'pil'"""
    x = (image / 2 + 0.5).clamp(0, 1)
    if output_type == "pt":
        return x
    arr = x.cpu().permute(0, 2, 3, 1).float().numpy()
    if output_type == "np":
        return arr
    if output_type != "pil":
        raise ValueError(f"output_type {output_type!r} (expected 'latent', 'pt', 'np' or 'pil')")
    from PIL import Image
    return [Image.fromarray((a * 255).round().astype("uint8")) for a in arr]
