"""diffusers' ``AutoencoderTiny`` decoder (TAESD; ``madebyollin/taesdxl`` for SDXL) on csrc/tinyvae.hip: a 1.2 M-parameter stand-in for
the VAE decoder made of 64-channel 3 x 3 convs and ReLUs -- no GroupNorm, no attention -- for previews (``IPAdapter.generate_pns(...,
preview_vae=)``), where the full ``AutoencoderKL`` decode costs more than it tells the judge.

The state dict is diffusers' (restated here, unpinned: DESIGN.md section 5).  ``decoder.layers`` is an ``nn.Sequential``:

    0  Conv 4 -> 64 + bias     1  ReLU      2-4  Block x 3      5  Upsample x2 (nearest)      6  Conv 64 -> 64, no bias
    7-9  Block x 3            10  Upsample  11  Conv, no bias  12-14  Block x 3  15  Upsample  16  Conv, no bias
    17  Block                 18  Conv 64 -> 3 + bias

with Block(x) = relu(conv(x) + x), conv = Sequential(Conv + bias, ReLU, Conv + bias, ReLU, Conv + bias) (keys
``decoder.layers.N.conv.{0,2,4}.{weight,bias}``), every conv 3 x 3 with padding 1, and forward = layers(3 tanh(z / 3)) * 2 - 1.

``decode`` is 35 launches of ``imh_tinyvae_conv`` (head, 33 body convs, tail) and nothing else: the ReLUs, the skips, the three
upsamplings, the tanh clamp and the NCHW fp32 image all live in the launches' prologues and epilogues.  The encoder is not built."""
import torch
import torch.nn as nn

from . import lib as L
from .derived import derived


class TinyVAEConfig:
    """diffusers AutoencoderTiny's config, the fields the decoder reads (taesdxl's values)"""

    def __init__(self, latent_channels=4, out_channels=3, decoder_block_out_channels=(64, 64, 64, 64), num_decoder_blocks=(3, 3, 3, 1),
                 act_fn="relu", scaling_factor=1.0, upsampling_scaling_factor=2, force_upcast=False):
        self.latent_channels, self.out_channels = int(latent_channels), int(out_channels)
        self.decoder_block_out_channels = tuple(int(c) for c in decoder_block_out_channels)
        self.num_decoder_blocks = tuple(int(n) for n in num_decoder_blocks)
        self.num_blocks = self.num_decoder_blocks
        self.act_fn, self.scaling_factor = act_fn, float(scaling_factor)
        self.upsampling_scaling_factor, self.force_upcast = int(upsampling_scaling_factor), bool(force_upcast)


class _Conv(nn.Conv2d):
    """a parameter holder with diffusers' keys (nn.Conv2d: weight [Cout, Cin, 3, 3], bias [Cout] or none) and the packed weight the
    kernel reads, cached per weight version like unet.Conv2d's"""

    def __init__(self, cin, cout, bias=True):
        super().__init__(cin, cout, 3, padding=1, bias=bias)
        for p in self.parameters():
            p.requires_grad_(False)

    def packed(self, ctx):
        """-> ([Cout, 9 Cin] with K index = (ky * 3 + kx) * Cin + c, bias [Cout] or None) in the context's dtype"""
        def build():
            w = self.weight.detach().permute(0, 2, 3, 1).reshape(self.weight.shape[0], -1)
            b = None if self.bias is None else self.bias.detach().to(device=ctx.device, dtype=ctx.dtype).contiguous()
            return w.to(device=ctx.device, dtype=ctx.dtype).contiguous(), b
        return derived(self, "_imh_packed", (self.weight, self.bias), build, where=(ctx.dtype, str(ctx.device)))


class _Block(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.conv = nn.Sequential(_Conv(c, c), nn.ReLU(), _Conv(c, c), nn.ReLU(), _Conv(c, c))
        self.skip = nn.Identity()
        self.fuse = nn.ReLU()


class _Decoder(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        c = cfg.decoder_block_out_channels[0]
        layers = [_Conv(cfg.latent_channels, c), nn.ReLU()]
        for i, n in enumerate(cfg.num_decoder_blocks):
            layers += [_Block(c) for _ in range(n)]
            if i + 1 < len(cfg.num_decoder_blocks):
                layers += [nn.Upsample(scale_factor=cfg.upsampling_scaling_factor), _Conv(c, c, bias=False)]
        layers.append(_Conv(c, cfg.out_channels))
        self.layers = nn.Sequential(*layers)


# elements per operand the kernel accepts (imh_tinyvae_conv refuses 2^31 and more): the largest is the full-resolution activation,
# 64 channels x 64 pixels per latent pixel
_LIMIT = (1 << 31) - 1


class AutoencoderTiny(nn.Module):
    """``decode(z)`` returns the image tensor [B, 3, 8h, 8w] (fp32, roughly [-1, 1]) of latents [B, 4, h, w], like ``AutoencoderKL.decode``;
    ``vae.decode_latents`` and ``pipeline.decode_output`` take it unchanged (``config.scaling_factor`` is 1.0: TAESD reads the UNet's
    latents as they are)."""
    tiny = True

    def __init__(self, config: TinyVAEConfig = None):
        super().__init__()
        self.config = c = config or TinyVAEConfig()
        if (c.latent_channels, c.out_channels, c.upsampling_scaling_factor) != (4, 3, 2) or set(c.decoder_block_out_channels) != {64} \
                or c.num_decoder_blocks != (3, 3, 3, 1) or len(c.decoder_block_out_channels) != 4:
            raise NotImplementedError(f"AutoencoderTiny: the HIP decoder is built for taesdxl's shape (4 latent channels, width 64, "
                                      f"num_blocks (3, 3, 3, 1), x2 upsampling); got width {c.decoder_block_out_channels}, "
                                      f"num_blocks {c.num_decoder_blocks}")
        if c.act_fn != "relu":
            raise NotImplementedError(f"AutoencoderTiny: act_fn {c.act_fn!r} (the kernel's epilogue is a ReLU)")
        self.decoder = _Decoder(c)
        self.launches = 0           # imh_tinyvae_conv launches decode has issued so far (35 per batch chunk)

    # -- loading --
    def load_state_dict(self, sd, strict=True, **kw):
        return super().load_state_dict({k: v for k, v in sd.items() if not k.startswith("encoder.")}, strict=strict, **kw)

    @classmethod
    def from_safetensors(cls, path, config: TinyVAEConfig = None, device="cuda:0", dtype=torch.bfloat16):
        from safetensors.torch import load_file
        m = cls(config)
        m.load_state_dict(load_file(path), strict=True)
        return m.to(device, dtype)

    @torch.no_grad()
    def init_random_(self, seed=0):
        """fan-in scaled normal weights, small biases: a synthetic-weight stand-in for benchmarks and examples"""
        g = torch.Generator().manual_seed(seed)
        for n, p in self.named_parameters():
            if p.dim() > 1:
                p.copy_((torch.randn(p.shape, generator=g) * p[0].numel() ** -0.5).to(p.dtype))
            else:
                p.copy_((torch.randn(p.shape, generator=g) * 0.02).to(p.dtype))
        return self

    @property
    def dtype(self):
        return self.decoder.layers[0].weight.dtype

    def enable_tiling(self, on=True):
        if on:
            raise NotImplementedError("AutoencoderTiny: tiled decoding is not built")

    # -- compute --
    def encode(self, x=None, *a, **kw):
        raise NotImplementedError("AutoencoderTiny: the tiny encoder is not built (decode only); image-to-image and inpainting need "
                                  "vae=AutoencoderKL(config, with_encoder=True)")

    def precision_for(self, precision=None):
        precision = precision or "auto"
        if precision == "fp32":
            raise ValueError("AutoencoderTiny decodes in its 16-bit dtype on the HIP kernel: precision='fp32' is not built")
        if precision not in ("auto", "native"):
            raise ValueError(f"precision {precision!r} (expected None, 'auto' or 'native')")
        return "native"

    def _decode_chunk(self, ctx, z):
        L_ = self.decoder.layers
        n0 = 0
        w, b = L_[0].packed(ctx)
        x = ctx.tinyvae_conv(z, w, bias=b, head=True, relu=True, descr="tiny_vae.layers.0")
        n0 += 1
        up = False
        for i in range(2, 18):
            m = L_[i]
            if isinstance(m, nn.Upsample):
                up = True                      # folded into the next conv's patch staging
            elif isinstance(m, _Block):
                w0, b0 = m.conv[0].packed(ctx)
                w2, b2 = m.conv[2].packed(ctx)
                w4, b4 = m.conv[4].packed(ctx)
                t = ctx.tinyvae_conv(x, w0, bias=b0, relu=True, descr=f"tiny_vae.layers.{i}.conv.0")
                u = ctx.tinyvae_conv(t, w2, bias=b2, relu=True, descr=f"tiny_vae.layers.{i}.conv.2")
                ctx.free(t)
                y = ctx.tinyvae_conv(u, w4, bias=b4, residual=x, relu=True, descr=f"tiny_vae.layers.{i}.conv.4")
                ctx.free(u); ctx.free(x)
                x = y
                n0 += 3
            else:
                w, b = m.packed(ctx)
                y = ctx.tinyvae_conv(x, w, bias=b, up2=up, descr=f"tiny_vae.layers.{i}")
                ctx.free(x)
                x, up = y, False
                n0 += 1
        w, b = L_[18].packed(ctx)
        img = ctx.tinyvae_conv(x, w, bias=b, tail=True, descr="tiny_vae.layers.18")
        ctx.free(x)
        self.launches += n0 + 1
        return img

    @torch.no_grad()
    def decode(self, z, precision=None):
        """z: latents [B, 4, h, w] (any float dtype, any h, w >= 1) on the module's device -> fp32 [B, 3, 8h, 8w].  precision: None /
        'auto' / 'native' (the module's bf16 / fp16 on the HIP kernel); 'fp32' is refused.  The batch is split so that no operand of a
        launch reaches 2^31 elements."""
        self.precision_for(precision)
        if not torch.is_tensor(z) or z.dim() != 4 or z.shape[1] != 4 or z.numel() == 0:
            raise ValueError(f"AutoencoderTiny.decode: latents {tuple(z.shape) if torch.is_tensor(z) else type(z).__name__}: expected [B, 4, h, w]")
        p0 = self.decoder.layers[0].weight
        if p0.dtype not in (torch.bfloat16, torch.float16):
            raise L.ImhError(f"AutoencoderTiny: the HIP decoder computes in bf16 or fp16, the module is {p0.dtype} (there is no fp32 path)")
        from .ctx import Ctx
        dev = p0.device if p0.device.type == "cuda" else z.device
        ctx = Ctx(dev, p0.dtype)
        z = z.to(device=dev, dtype=torch.float32).contiguous()
        B, _, h, w = (int(v) for v in z.shape)
        per = 64 * 64 * h * w                       # the largest operand of one sample: [8h, 8w, 64]
        if per > _LIMIT:
            raise NotImplementedError(f"AutoencoderTiny.decode: a {8 * h} x {8 * w} image alone exceeds 2^31 activation elements (tiling is not built)")
        nb = max(1, min(B, _LIMIT // per))
        outs = [self._decode_chunk(ctx, z[i:i + nb]) for i in range(0, B, nb)]
        return outs[0] if len(outs) == 1 else torch.cat(outs, 0)
