"""SDXL ``T2IAdapter`` (diffusers 0.30, ``adapter_type="full_adapter_xl"``; restated from its published source -- ``FullAdapterXL``,
``AdapterBlock``, ``AdapterResnetBlock`` --, diffusers is not installed) on the gfx950 kernels.

The net is a 79 M-parameter stack of convs without a normalisation: PixelUnshuffle(16) -> conv_in -> four blocks, each an optional
AvgPool2d(2, 2, ceil_mode=True), an optional 1 x 1 ``in_conv`` and ``num_res_blocks`` times ``x = block2(relu(block1(x))) + x``.  It
reads the control image alone, so it runs ONCE per control image (``prepare_features``: eager ``Ctx.conv3x3`` / ``Ctx.gemm`` launches and
the three passes of csrc/adapter.hip); its four feature maps are added to the UNet's down path at every step
(``UNet2DConditionModel.emit_forward(adapter=AdapterResiduals(...))``: four ``Ctx.control_add`` launches, nothing else moves).

Not built: ``adapter_type`` "full_adapter" / "light_adapter" (the SD-1.x nets), ``MultiAdapter`` / a list of adapters (NotImplementedError).
"""
import torch
import torch.nn as nn

from . import lib as L
from .attention_processor import _b
from .unet import Conv2d


class AdapterResiduals:
    """what the adapter hands the UNet forward: its four NHWC features [1 | S, h, w, C] in injection order and the gate --
    g = scale * (tab[*step] if tab is given else 1) -- every injection multiplies them by (diffusers down_intrablock_additional_residuals)"""
    __slots__ = ("feats", "scale", "tab", "step")

    def __init__(self, feats, scale=1.0, tab=None, step=None):
        self.feats, self.scale, self.tab, self.step = list(feats), float(scale), tab, step
        if len(self.feats) != 4:
            raise NotImplementedError(f"{len(self.feats)} adapter features: the SDXL layout takes four (down blocks 0, 1, 2 and the mid block)")


class AdapterResnetBlock(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.block1 = Conv2d(c, c, 3)
        self.block2 = Conv2d(c, c, 1)


class AdapterBlock(nn.Module):
    def __init__(self, cin, cout, num_res_blocks, down=False):
        super().__init__()
        self.down = bool(down)                   # AvgPool2d(2, 2, ceil_mode=True) in front (no parameters)
        if cin != cout:
            self.in_conv = Conv2d(cin, cout, 1)
        self.resnets = nn.ModuleList([AdapterResnetBlock(cout) for _ in range(num_res_blocks)])


class FullAdapterXL(nn.Module):
    def __init__(self, in_channels, channels, num_res_blocks, downscale_factor):
        super().__init__()
        c = tuple(channels)
        self.conv_in = Conv2d(in_channels * downscale_factor ** 2, c[0], 3)
        # the XL wiring: only block 2 halves the resolution, blocks 1 and 2 change the width
        self.body = nn.ModuleList([AdapterBlock(c[0], c[0], num_res_blocks), AdapterBlock(c[0], c[1], num_res_blocks),
                                   AdapterBlock(c[1], c[2], num_res_blocks, down=True), AdapterBlock(c[3], c[3], num_res_blocks)])


class T2IAdapter(nn.Module):
    def __init__(self, in_channels=3, channels=(320, 640, 1280, 1280), num_res_blocks=2, downscale_factor=16, adapter_type="full_adapter_xl"):
        super().__init__()
        if adapter_type in ("full_adapter", "light_adapter"):
            raise NotImplementedError(f'adapter_type "{adapter_type}" (the SD-1.x adapters) is not built: "full_adapter_xl" only')
        if adapter_type != "full_adapter_xl":
            raise ValueError(f"unknown adapter_type {adapter_type!r}")
        channels = tuple(int(c) for c in channels)
        if len(channels) != 4 or channels[2] != channels[3]:
            raise ValueError(f"the XL adapter has four blocks, the last two of one width; got channels = {channels}")
        if int(num_res_blocks) < 1 or int(downscale_factor) < 1 or int(in_channels) < 1:
            raise ValueError("in_channels, num_res_blocks and downscale_factor must be positive")
        self.in_channels, self.channels = int(in_channels), channels
        self.num_res_blocks, self.downscale_factor, self.adapter_type = int(num_res_blocks), int(downscale_factor), adapter_type
        self.adapter = FullAdapterXL(self.in_channels, channels, self.num_res_blocks, self.downscale_factor)
        self.launches = 0           # launches prepare_features has issued so far (a cached control image issues none)

    @property
    def total_downscale_factor(self):
        return 2 * self.downscale_factor

    # ---- construction ----
    @classmethod
    def from_unet(cls, unet, seed=1234, **kw):
        """a fresh adapter for this UNet: channels (c0, c1, c2, c2) of its block_out_channels, on its device and in its dtype, with
        init_random_(seed) weights (upstream has no such constructor: a published adapter comes from from_safetensors)"""
        boc = tuple(unet.config.block_out_channels)
        if len(boc) != 3:
            raise ValueError(f"the XL adapter serves the three-level SDXL layout, not block_out_channels = {boc}")
        p0 = unet.conv_in.weight
        with torch.device(p0.device):
            m = cls(channels=(boc[0], boc[1], boc[2], boc[2]), **kw)
        return m.init_random_(seed).to(p0.dtype)

    @torch.no_grad()
    def init_random_(self, seed=1234):
        """fan-in scaled normal weights, small biases; the 1 x 1 block2 convs at a third of that, so that the eight residual additions
        keep the features' scale (a synthetic-weight stand-in for benchmarks and examples)"""
        p0 = self.adapter.conv_in.weight
        g = torch.Generator(device=p0.device).manual_seed(seed)
        for name, p in self.named_parameters():
            if p.ndim >= 2:
                s = p[0].numel() ** -0.5 * (1.0 / 3.0 if ".block2." in name else 1.0)
                p.copy_(torch.randn(p.shape, generator=g, device=p.device, dtype=torch.float32).mul_(s))
            else:
                p.copy_(torch.randn(p.shape, generator=g, device=p.device, dtype=torch.float32).mul_(0.02))
        return self

    @classmethod
    def from_safetensors(cls, path, device="cpu", dtype=None, **kw):
        """Load a diffusers-format T2I-Adapter checkpoint (``diffusion_pytorch_model.safetensors``): the key schema is the one this
        module keeps, so this is a strict ``load_state_dict``; kw: the config (in_channels, channels, num_res_blocks, downscale_factor)"""
        from safetensors.torch import load_file
        sd = load_file(path, device="cpu")
        m = cls(**kw)
        m.load_state_dict(sd, strict=True)
        m = m.to(device)
        return m.to(dtype) if dtype is not None else m

    # ---- the control image ----
    def check_image(self, image, height=None, width=None):
        """ValueError unless image is [n, in_channels, H, W] with sides that are multiples of 2 f (and equal height / width when given);
        no GPU work"""
        if not torch.is_tensor(image) or image.dim() != 4 or image.shape[1] != self.in_channels:
            raise ValueError(f"adapter image {tuple(image.shape) if torch.is_tensor(image) else type(image).__name__}: expected a float "
                             f"tensor [n, {self.in_channels}, H, W] in [0, 1]")
        H, W = int(image.shape[2]), int(image.shape[3])
        d = self.total_downscale_factor
        if H < d or W < d or H % d or W % d:
            raise ValueError(f"adapter image {H} x {W}: sides must be multiples of {d} (2 x downscale_factor)")
        if (height is not None and int(height) != H) or (width is not None and int(width) != W):
            raise ValueError(f"adapter image {H} x {W} does not match the call's {height} x {width}: resize the control image first")

    # ---- once per control image ----
    @torch.no_grad()
    def prepare_features(self, ctx, image, Hl, Wl):
        """the four features as NHWC tensors in the compute dtype: [n, Hl / 2, Wl / 2, c0], [.., c1] at the same size, [n, Hl / 4, Wl / 4,
        c2] twice.  image: float [n, in_channels, 8 Hl, 8 Wl] in [0, 1] (not normalised: upstream's _preprocess_adapter_image).  Eager: the
        features are step-invariant; they are never freed into ctx's pool, so a fresh context keeps them alive."""
        self.check_image(image, 8 * Hl, 8 * Wl)
        if ctx.record:
            raise L.ImhError("the adapter's features are step-invariant: they are computed eagerly, outside the recorded step")
        net, f = self.adapter, self.downscale_factor
        n0 = [0]

        def conv1x1(x, conv, residual=None, descr=""):
            B, H, W, Cc = x.shape
            n0[0] += 1
            return ctx.gemm(x.view(B * H * W, Cc), conv.packed(ctx), bias=_b(conv, ctx), residual=residual, descr=descr).view(B, H, W, -1)

        img = image.to(device=ctx.device, dtype=torch.float32).contiguous()
        cin = self.in_channels * f * f
        x = ctx.pixel_unshuffle(img, f, Cp=(cin + 63) // 64 * 64, descr="t2i.unshuffle")        # channels padded to the implicit GEMM's 64
        w, b = net.conv_in.packed_padded(ctx, pad_out=False)
        h = ctx.conv3x3(x, w, bias=b, descr="t2i.conv_in")
        ctx.free(x)
        n0[0] += 2
        feats = []
        for i, blk in enumerate(net.body):
            own = bool(feats) and h is feats[-1]          # h is the previous block's feature: read, never freed
            if blk.down:
                p = ctx.avgpool2(h, descr=f"t2i.body.{i}.downsample")
                n0[0] += 1
                if not own:
                    ctx.free(h)
                h, own = p, False
            if hasattr(blk, "in_conv"):
                p = conv1x1(h, blk.in_conv, descr=f"t2i.body.{i}.in_conv")
                if not own:
                    ctx.free(h)
                h, own = p, False
            for j, r in enumerate(blk.resnets):
                t = ctx.conv3x3(h, r.block1.packed(ctx), bias=_b(r.block1, ctx), descr=f"t2i.body.{i}.resnets.{j}.block1")
                ctx.relu(t, out=t, descr=f"t2i.body.{i}.resnets.{j}.act")
                B, H, W, Cc = h.shape
                p = conv1x1(t, r.block2, residual=h.view(B * H * W, Cc), descr=f"t2i.body.{i}.resnets.{j}.block2")
                n0[0] += 2
                ctx.free(t)
                if not own:
                    ctx.free(h)
                h, own = p, False
            feats.append(h)
        self.launches += n0[0]
        want = [(Hl // 2, Wl // 2, self.channels[0]), (Hl // 2, Wl // 2, self.channels[1]), (Hl // 4, Wl // 4, self.channels[2]),
                (Hl // 4, Wl // 4, self.channels[3])]
        for t, s in zip(feats, want):
            if tuple(t.shape[1:]) != s:
                raise L.ImhError(f"adapter feature {tuple(t.shape)} does not fit the latents {Hl} x {Wl}: expected [n, {s[0]}, {s[1]}, {s[2]}]")
        return feats

    # ---- eager drop-in signature (diffusers T2IAdapter.forward) ----
    @torch.no_grad()
    def forward(self, image):
        """-> four NCHW tensors, unscaled, in the image's dtype (fp32 images: the model dtype), as upstream's list of features"""
        from .ctx import Ctx
        p0 = self.adapter.conv_in.weight
        dtype = p0.dtype if p0.dtype in (torch.bfloat16, torch.float16) else \
            (image.dtype if image.dtype in (torch.bfloat16, torch.float16) else torch.bfloat16)
        self.check_image(image)
        ctx = Ctx(p0.device if p0.device.type == "cuda" else image.device, dtype)
        feats = self.prepare_features(ctx, image.float(), image.shape[2] // 8, image.shape[3] // 8)
        out_dtype = image.dtype if image.dtype in (torch.bfloat16, torch.float16) else dtype
        return [t.permute(0, 3, 1, 2).to(out_dtype) for t in feats]
