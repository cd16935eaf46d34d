"""SDXL ``ControlNetModel`` (diffusers 0.30, restated from its published source; diffusers is not installed) on the gfx950 kernels.

What the reference expects on the pipe: ``ip_adapter/ip_adapter.py:126-133`` installs ``CNAttnProcessor`` on every attention layer of
``pipe.controlnet``.  The model is the UNet's encoder (conv_in, time / add embeddings, down blocks, mid block -- unet.py's modules, same
state-dict names) plus

  * ``controlnet_cond_embedding``: the control image -> a hint of conv_in's shape (3 -> 16 -> 16 -> 32 -> 32 -> 96 -> 96 -> 256 -> C0, 3 x 3
    convs, every second one stride 2, SiLU between them).  Step-invariant: computed once per control image (``prepare_hint``) from
    ``Ctx.conv3x3`` launches with the channels zero-padded to the implicit GEMM's 64 and ``Ctx.silu`` passes;
  * ``controlnet_down_blocks`` (nine 1 x 1 "zero convs", one per UNet skip) and ``controlnet_mid_block``: the residuals the UNet adds to
    its skips and to its mid-block output (``UNet2DConditionModel.emit_forward(control=...)``, imh_control_add).

``emit_forward`` records the branch into the SAME plan as the UNet forward that consumes it -- a text-to-image step, an image-to-image
one or either inpainting mode: the branch reads the 4-channel latents whatever the UNet's ``in_channels``.  Not built: ``guess_mode``,
``global_pool_conditions``, class embeddings, ``MultiControlNetModel`` (NotImplementedError).
"""
import torch
import torch.nn as nn

from . import lib as L
from .attention_processor import _b
from .unet import Conv2d, DownBlock, Feat, MidBlock, StepState, TimestepEmbedding, UNetConfig, UNetEncoderModel, gn_sub

COND_CHANNELS = (16, 32, 96, 256)       # diffusers conditioning_embedding_out_channels (every published SDXL ControlNet)


class ControlResiduals:
    """what the ControlNet branch hands the UNet forward: nine NHWC residuals in skip order, the mid residual, and the gate --
    g = scale * (tab[*step] if tab is given else 1) -- every injection multiplies them by"""
    __slots__ = ("down", "mid", "scale", "tab", "step")

    def __init__(self, down, mid, scale=1.0, tab=None, step=None):
        self.down, self.mid, self.scale, self.tab, self.step = list(down), mid, float(scale), tab, step


class ControlNetConditioningEmbedding(nn.Module):
    def __init__(self, c0, channels=COND_CHANNELS):
        super().__init__()
        self.conv_in = Conv2d(3, channels[0], 3)
        blocks = []
        for i in range(len(channels) - 1):
            blocks.append(Conv2d(channels[i], channels[i], 3))
            blocks.append(Conv2d(channels[i], channels[i + 1], 3))           # stride 2
        self.blocks = nn.ModuleList(blocks)
        self.conv_out = Conv2d(channels[-1], c0, 3)


class ControlNetModel(UNetEncoderModel):
    """the processor protocol, the packed / stacked weights, the step-invariant conditioning, the checkpoint loader and the encoder
    walk are the base class's: the ones the UNet runs"""

    def __init__(self, cfg: UNetConfig = None, conditioning_embedding_out_channels=COND_CHANNELS, global_pool_conditions=False,
                 class_embed_type=None, num_class_embeds=None):
        super().__init__()
        if global_pool_conditions:
            raise NotImplementedError("global_pool_conditions is not built (no published SDXL ControlNet sets it)")
        if class_embed_type is not None or num_class_embeds is not None:
            raise NotImplementedError("class embeddings are not built: SDXL conditions through add_embedding (text_time)")
        cfg = cfg or UNetConfig()
        if cfg.in_channels != 4:
            raise ValueError(f"a ControlNet reads the 4-channel latents, got in_channels = {cfg.in_channels}")
        self.config = cfg
        boc = cfg.block_out_channels
        nb = len(boc)
        self.conv_in = Conv2d(4, boc[0], 3)
        self.time_embedding = TimestepEmbedding(boc[0], cfg.time_embed_dim)
        self.add_embedding = TimestepEmbedding(cfg.projection_class_embeddings_input_dim, cfg.time_embed_dim)
        self.controlnet_cond_embedding = ControlNetConditioningEmbedding(boc[0], tuple(conditioning_embedding_out_channels))
        self.down_blocks = nn.ModuleList([])
        skip_ch = [boc[0]]
        out = boc[0]
        for i in range(nb):
            cin, out = out, boc[i]
            n_tf = 0 if i == 0 else cfg.transformer_layers_per_block[i]
            self.down_blocks.append(DownBlock(cin, out, cfg.layers_per_block, n_tf, cfg.attention_head_dim[i], cfg, add_down=(i != nb - 1)))
            skip_ch += [out] * (cfg.layers_per_block + (i != nb - 1))
        self.controlnet_down_blocks = nn.ModuleList([Conv2d(c, c, 1) for c in skip_ch])
        self.controlnet_mid_block = Conv2d(boc[-1], boc[-1], 1)
        self.mid_block = MidBlock(boc[-1], cfg.transformer_layers_per_block[-1], cfg.attention_head_dim[-1], cfg)
        self._number_time_emb_proj()

    def zero_convs(self):
        """the convs upstream creates with zero_module: a fresh ControlNet adds nothing to the UNet"""
        return list(self.controlnet_down_blocks) + [self.controlnet_mid_block, self.controlnet_cond_embedding.conv_out]

    @classmethod
    @torch.no_grad()
    def from_unet(cls, unet, seed=1234, **kw):
        """diffusers ControlNetModel.from_unet: the encoder's weights are the UNet's, the zero convs stay zero; the other convs of the
        conditioning embedding get a fan-in scaled normal draw (upstream: torch's default Conv2d init)"""
        cfg = unet.config
        p0 = unet.conv_in.weight
        with torch.device(p0.device):
            m = cls(UNetConfig(**{k: getattr(cfg, k) for k in UNetConfig.__dataclass_fields__}), **kw)
        m = m.to(p0.dtype)
        own = dict(m.named_parameters())
        for k, v in unet.state_dict().items():
            if k.split(".")[0] in ("conv_in", "time_embedding", "add_embedding", "down_blocks", "mid_block") and k in own:
                own[k].copy_(v)
        g = torch.Generator(device="cpu").manual_seed(seed)
        emb = m.controlnet_cond_embedding
        for conv in [emb.conv_in] + list(emb.blocks):
            fan_in = conv.weight[0].numel()
            conv.weight.copy_(torch.randn(conv.weight.shape, generator=g).mul_(fan_in ** -0.5))
            conv.bias.zero_()
        for conv in m.zero_convs():
            conv.weight.zero_()
            conv.bias.zero_()
        return m

    # ---- once per control image ----
    @torch.no_grad()
    def prepare_hint(self, ctx, image, Hl, Wl):
        """controlnet_cond_embedding(image) as NHWC [Sh, Hl, Wl, C0] in the model dtype.  image: float [Sh, 3, 8 Hl, 8 Wl] in [0, 1]
        (not normalised: upstream's VaeImageProcessor(do_normalize=False)).  Eight conv3x3 launches and seven SiLU passes, eagerly."""
        if ctx.record:
            raise L.ImhError("the hint is step-invariant: it is computed eagerly, outside the recorded step")
        if image.dim() != 4 or image.shape[1] != 3 or tuple(image.shape[2:]) != (8 * Hl, 8 * Wl):
            raise L.ImhError(f"control image {tuple(image.shape)}: expected [Sh, 3, {8 * Hl}, {8 * Wl}] for {Hl} x {Wl} latents")
        emb = self.controlnet_cond_embedding
        Sh = image.shape[0]
        x = torch.zeros(Sh, 8 * Hl, 8 * Wl, 64, dtype=ctx.dtype, device=ctx.device)                 # plumbing: NHWC, channels padded to 64
        x[..., :3] = image.to(device=ctx.device, dtype=ctx.dtype).permute(0, 2, 3, 1)
        w, b = emb.conv_in.packed_padded(ctx)
        h = ctx.conv3x3(x, w, bias=b, descr="cn.hint.conv_in")
        for i, blk in enumerate(emb.blocks):
            s = ctx.silu(h, descr="cn.hint.silu")
            ctx.free(h)
            w, b = blk.packed_padded(ctx)
            h = ctx.conv3x3(s, w, bias=b, stride=2 if i % 2 else 1, descr=f"cn.hint.blocks.{i}")
            ctx.free(s)
        s = ctx.silu(h, descr="cn.hint.silu")
        ctx.free(h)
        w, b = emb.conv_out.packed_padded(ctx, pad_out=False)
        hint = ctx.conv3x3(s, w, bias=b, descr="cn.hint.conv_out")
        ctx.free(s)
        if tuple(hint.shape) != (Sh, Hl, Wl, self.config.block_out_channels[0]):
            raise L.ImhError(f"hint {tuple(hint.shape)} does not fit the latents {Hl} x {Wl}")
        return hint

    # ---- the branch, as emitted ops ----
    def emit_forward(self, ctx, st, S, Hl, Wl, cfg_dup=True, hint=None, scale=1.0, tab=None, guess_mode=False):
        """Records the ControlNet forward.  st: a StepState with the UNet's latents / step / t_table / in_scale_tab and the ControlNet's
        OWN aug_emb, kv (prepare_conditioning on this model) and temb_table; hint: prepare_hint's result, [1 | S, Hl, Wl, C0].
        Returns ControlResiduals for UNet2DConditionModel.emit_forward(control=...): the residuals are unscaled; scale / tab / st.step
        travel with them and the injections apply the gate."""
        if guess_mode:
            raise NotImplementedError("guess_mode is not built")
        cfg = self.config
        B = self._latent_batch(S, Hl, Wl, cfg_dup)
        c0 = cfg.block_out_channels[0]
        if hint is None or hint.dim() != 4 or tuple(hint.shape[1:]) != (Hl, Wl, c0) or hint.shape[0] not in (1, S) or not hint.is_contiguous():
            raise L.ImhError(f"hint {None if hint is None else tuple(hint.shape)}: expected contiguous [1 | {S}, {Hl}, {Wl}, {c0}] (prepare_hint)")
        ctx.tag = 81
        self._emit_time_embedding(ctx, st, B)
        ctx.tag = 82
        x = self._emit_conv_in(ctx, st, S, B, Hl, Wl, "cn.conv_in")
        # sample = conv_in(sample) + controlnet_cond_embedding(cond): the hint add leaves the GroupNorm partials a conv_in output needs
        y = Feat.of(ctx.control_add(x, hint, gn_sub=gn_sub(c0, cfg.norm_num_groups), descr="cn.hint_add"))
        ctx.free(x)
        h, feats = self._emit_encoder(ctx, st, y, (83, 84, 85, 86), prefix="cn.")
        # the zero convs: 1 x 1 convs are Linears over the pixels
        ctx.tag = 87
        down = []
        for f, conv in zip(feats, self.controlnet_down_blocks):
            Bf, Hf, Wf, Cf = f.t.shape
            r_ = ctx.gemm(f.t.view(Bf * Hf * Wf, Cf), conv.packed(ctx), bias=_b(conv, ctx), descr="cn.zero_conv")
            down.append(r_.view(Bf, Hf, Wf, Cf))
            f.free(ctx)
        Bf, Hf, Wf, Cf = h.t.shape
        mid = ctx.gemm(h.t.view(Bf * Hf * Wf, Cf), self.controlnet_mid_block.packed(ctx), bias=_b(self.controlnet_mid_block, ctx),
                       descr="cn.zero_conv.mid").view(Bf, Hf, Wf, Cf)
        h.free(ctx)
        ctx.free(st.temb_all)
        ctx.tag = 0
        return ControlResiduals(down, mid, scale=scale, tab=tab, step=st.step if tab is not None else None)

    # ---- eager drop-in signature (diffusers ControlNetModel.forward) ----
    @torch.no_grad()
    def forward(self, sample, timestep, encoder_hidden_states, controlnet_cond, conditioning_scale=1.0, added_cond_kwargs=None,
                guess_mode=False, return_dict=False, **kw):
        """-> (down_block_res_samples: nine NCHW tensors, mid_block_res_sample), each times conditioning_scale, as upstream"""
        if guess_mode:
            raise NotImplementedError("guess_mode is not built")
        ctx, st = self._eager_state(sample, timestep, encoder_hidden_states, added_cond_kwargs)
        B, _, Hl, Wl = sample.shape
        hint = self.prepare_hint(ctx, controlnet_cond, Hl, Wl)
        res = self.emit_forward(ctx, st, B, Hl, Wl, cfg_dup=False, hint=hint)
        out = [(r.permute(0, 3, 1, 2).float() * float(conditioning_scale)).to(sample.dtype) for r in res.down + [res.mid]]
        return out[:-1], out[-1]


def control_state(unet_state, own=None):
    """the StepState the ControlNet branch records against: the UNet's latents, step counter and schedule tables, the ControlNet's own
    conditioning (aug_emb, K / V caches) and time-embedding rows"""
    st = StepState()
    for k in ("latents", "t_table", "step", "in_scale_tab", "t_value"):
        setattr(st, k, getattr(unet_state, k, None))
    if own is not None:
        st.aug_emb, st.kv = own.aug_emb, own.kv
    return st
