"""Test-local CPU fp32 restatement of diffusers 0.30 ``ControlNetModel`` (SDXL), of ``UNet2DConditionModel.forward`` with
``down_block_additional_residuals`` / ``mid_block_additional_residual``, and of the CFG loop of ``StableDiffusionXLControlNetPipeline``
with its ``controlnet_keep`` rule -- recalled from the published sources; diffusers itself is not installed, so like the rest of the
oracle's diffusers half this is UNPINNED against diffusers.

Built from the blocks of ``oracle.sdxl_unet``, the processors of ``oracle.modules`` and the schedulers of ``oracle.schedulers`` (or any
object with their surface, e.g. tests/multistep_reference.py); imports nothing from the product.  Parameter names follow diffusers'
state dict, so ``imagharmony_amd.controlnet.ControlNetModel.load_state_dict(RefControlNet.state_dict())`` is strict.

A plain helper module; no fixtures, no pytest settings."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import modules as om
from oracle.sdxl_unet import DownBlock, MidBlock, TimestepEmbedding, timestep_embedding

COND_CHANNELS = (16, 32, 96, 256)


class RefCNAttnProcessor:
    """the reference's CNAttnProcessor2_0 (ip_adapter/attention_processor.py:534-621): one object on every layer of the ControlNet;
    self-attention unchanged, cross-attention over the text tokens only (the last ``num_tokens`` are sliced off)"""

    def __init__(self, num_tokens=4):
        self.num_tokens = num_tokens
        self._plain = om.AttnProcessor2_0()

    def __call__(self, attn, hidden_states, encoder_hidden_states=None, attention_mask=None, temb=None, *a, **k):
        if encoder_hidden_states is not None:
            encoder_hidden_states = encoder_hidden_states[:, :encoder_hidden_states.shape[1] - self.num_tokens]
        return self._plain(attn, hidden_states, encoder_hidden_states=encoder_hidden_states)


class RefCondEmbedding(nn.Module):
    """ControlNetConditioningEmbedding: conv_in, (c -> c, c -> next stride 2) per level, conv_out; SiLU after every conv but the last"""

    def __init__(self, c0, channels=COND_CHANNELS):
        super().__init__()
        self.conv_in = nn.Conv2d(3, channels[0], 3, padding=1)
        blocks = []
        for i in range(len(channels) - 1):
            blocks.append(nn.Conv2d(channels[i], channels[i], 3, padding=1))
            blocks.append(nn.Conv2d(channels[i], channels[i + 1], 3, padding=1, stride=2))
        self.blocks = nn.ModuleList(blocks)
        self.conv_out = nn.Conv2d(channels[-1], c0, 3, padding=1)

    def forward(self, x):
        h = F.silu(self.conv_in(x))
        for b in self.blocks:
            h = F.silu(b(h))
        return self.conv_out(h)


class RefControlNet(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.config = cfg
        boc = cfg.block_out_channels
        nb = len(boc)
        self.conv_in = nn.Conv2d(4, boc[0], 3, padding=1)
        self.time_embedding = TimestepEmbedding(boc[0], cfg.time_embed_dim)
        self.add_embedding = TimestepEmbedding(cfg.projection_class_embeddings_input_dim, cfg.time_embed_dim)
        self.controlnet_cond_embedding = RefCondEmbedding(boc[0])
        self.down_blocks = nn.ModuleList([])
        ch = [boc[0]]
        out = boc[0]
        for i in range(nb):
            cin, out = out, boc[i]
            n_tf = 0 if i == 0 else cfg.transformer_layers_per_block[i]
            self.down_blocks.append(DownBlock(cin, out, cfg.layers_per_block, n_tf, cfg.attention_head_dim[i], cfg, add_down=(i != nb - 1)))
            ch += [out] * (cfg.layers_per_block + (i != nb - 1))
        self.controlnet_down_blocks = nn.ModuleList([nn.Conv2d(c, c, 1) for c in ch])
        self.controlnet_mid_block = nn.Conv2d(boc[-1], boc[-1], 1)
        self.mid_block = MidBlock(boc[-1], cfg.transformer_layers_per_block[-1], cfg.attention_head_dim[-1], cfg)

    def set_attn_processor(self, proc):
        for m in self.modules():
            if hasattr(m, "set_processor"):
                m.set_processor(proc)

    def zero_convs(self):
        return list(self.controlnet_down_blocks) + [self.controlnet_mid_block, self.controlnet_cond_embedding.conv_out]

    def forward(self, sample, timestep, encoder_hidden_states, controlnet_cond, conditioning_scale=1.0, added_cond_kwargs=None):
        """-> (nine down residuals, mid residual), NCHW, each times conditioning_scale"""
        cfg = self.config
        b = sample.shape[0]
        t = timestep if torch.is_tensor(timestep) else torch.tensor([timestep], dtype=torch.float32)
        t = t.reshape(-1).expand(b)
        emb = self.time_embedding(timestep_embedding(t, cfg.block_out_channels[0]).to(sample.dtype))
        te = timestep_embedding(added_cond_kwargs["time_ids"].flatten(), cfg.addition_time_embed_dim).reshape(b, -1)
        add = torch.cat([added_cond_kwargs["text_embeds"], te.to(sample.dtype)], dim=-1)
        emb = emb + self.add_embedding(add)
        cond = self.controlnet_cond_embedding(controlnet_cond)
        if cond.shape[0] != b:
            cond = cond.repeat(b // cond.shape[0], 1, 1, 1)
        h = self.conv_in(sample) + cond
        feats = [h]
        for blk in self.down_blocks:
            h, outs = blk(h, emb, encoder_hidden_states)
            feats.extend(outs)
        h = self.mid_block(h, emb, encoder_hidden_states)
        down = [conv(f) * conditioning_scale for f, conv in zip(feats, self.controlnet_down_blocks)]
        return down, self.controlnet_mid_block(h) * conditioning_scale


def unet_forward(unet, sample, timestep, encoder_hidden_states, added_cond_kwargs, down_res=None, mid_res=None):
    """oracle.sdxl_unet.UNet2DConditionModel.forward with diffusers' additional residuals: every skip and the mid output get theirs
    added after the mid block, before the up path (with None: the plain forward, the same operations in the same order)"""
    cfg = unet.config
    b = sample.shape[0]
    t = timestep if torch.is_tensor(timestep) else torch.tensor([timestep], dtype=torch.float32)
    t = t.reshape(-1).expand(b)
    emb = unet.time_embedding(timestep_embedding(t, cfg.block_out_channels[0]).to(sample.dtype))
    te = timestep_embedding(added_cond_kwargs["time_ids"].flatten(), cfg.addition_time_embed_dim).reshape(b, -1)
    add = torch.cat([added_cond_kwargs["text_embeds"], te.to(added_cond_kwargs["text_embeds"].dtype)], dim=-1).to(emb.dtype)
    emb = emb + unet.add_embedding(add)
    h = unet.conv_in(sample)
    skips = [h]
    for blk in unet.down_blocks:
        h, outs = blk(h, emb, encoder_hidden_states)
        skips.extend(outs)
    h = unet.mid_block(h, emb, encoder_hidden_states)
    if down_res is not None:
        skips = [s + r for s, r in zip(skips, down_res)]
        h = h + mid_res
    for blk in unet.up_blocks:
        h = blk(h, skips, emb, encoder_hidden_states)
    return unet.conv_out(F.silu(unet.conv_norm_out(h)))


def keep(i, m, start, end):
    """diffusers controlnet_keep: 1.0 - float(i / m < start or (i + 1) / m > end)"""
    return 0.0 if (i / m < start or (i + 1) / m > end) else 1.0


@torch.no_grad()
def denoise(unet, controlnet, scheduler, latents, prompt_embeds, negative_prompt_embeds, pooled, negative_pooled, height, width,
            control_image, num_inference_steps, guidance_scale=5.0, conditioning_scale=1.0, controlnet_guidance_start=0.0,
            controlnet_guidance_end=1.0, t_start=0):
    """the CFG loop of StableDiffusionXLControlNetPipeline on pre-computed embeddings (guess_mode off): the ControlNet sees the
    CFG-duplicated, scaled latents and the prompt embeddings; its residuals times conditioning_scale * keep(i) go into the UNet.
    controlnet=None: the plain loop.  t_start: the loop runs timesteps[t_start:] (a scheduler that was given t_start itself has
    already cut its list)."""
    s = latents.shape[0]
    scheduler.set_timesteps(num_inference_steps)
    latents = latents * scheduler.init_noise_sigma
    tid = torch.tensor([[height, width, 0, 0, height, width]], dtype=prompt_embeds.dtype)
    ehs = torch.cat([negative_prompt_embeds, prompt_embeds], 0)
    added = {"text_embeds": torch.cat([negative_pooled, pooled], 0), "time_ids": tid.repeat(2 * s, 1)}
    ts = scheduler.timesteps if getattr(scheduler, "t_start", 0) else scheduler.timesteps[t_start:]
    m = len(ts)
    for i, t in enumerate(ts):
        x = scheduler.scale_model_input(torch.cat([latents] * 2), t)
        down = mid = None
        if controlnet is not None:
            g = conditioning_scale * keep(i, m, controlnet_guidance_start, controlnet_guidance_end)
            down, mid = controlnet(x, t, ehs, control_image, conditioning_scale=g, added_cond_kwargs=added)
        eps = unet_forward(unet, x, t, ehs, added, down, mid)
        u, c = eps.chunk(2)
        latents = scheduler.step(u + guidance_scale * (c - u), t, latents)[0]
    return latents
