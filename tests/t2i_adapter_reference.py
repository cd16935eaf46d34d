"""Test-local CPU fp32 restatement of diffusers 0.30 ``T2IAdapter`` (``adapter_type="full_adapter_xl"``: ``FullAdapterXL`` / ``AdapterBlock`` /
``AdapterResnetBlock``), of ``UNet2DConditionModel.forward`` with ``down_intrablock_additional_residuals`` on the SDXL block layout, and of
the CFG loop of ``StableDiffusionXLAdapterPipeline`` with ``adapter_conditioning_scale`` / ``adapter_conditioning_factor`` -- recalled from
the published sources; diffusers itself is not installed, so like the rest of the oracle's diffusers half this is UNPINNED against
diffusers.

Built from plain torch modules, the blocks of ``oracle.sdxl_unet`` and the schedulers of ``oracle.schedulers`` (or any object with their
surface); imports nothing from the product.  Parameter names follow diffusers' state dict, so
``imagharmony_amd.t2i_adapter.T2IAdapter.load_state_dict(RefT2IAdapter.state_dict())`` is strict.

A plain helper module; no fixtures, no pytest settings."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle.sdxl_unet import timestep_embedding


class RefAdapterResnetBlock(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.block1 = nn.Conv2d(c, c, 3, padding=1)
        self.act = nn.ReLU()
        self.block2 = nn.Conv2d(c, c, 1)

    def forward(self, x):
        return self.block2(self.act(self.block1(x))) + x


class RefAdapterBlock(nn.Module):
    def __init__(self, cin, cout, n, down=False):
        super().__init__()
        self.downsample = nn.AvgPool2d(2, stride=2, ceil_mode=True) if down else None
        self.in_conv = nn.Conv2d(cin, cout, 1) if cin != cout else None
        self.resnets = nn.Sequential(*[RefAdapterResnetBlock(cout) for _ in range(n)])

    def forward(self, x):
        if self.downsample is not None:
            x = self.downsample(x)
        if self.in_conv is not None:
            x = self.in_conv(x)
        return self.resnets(x)


class RefFullAdapterXL(nn.Module):
    def __init__(self, in_channels, channels, n, f):
        super().__init__()
        self.unshuffle = nn.PixelUnshuffle(f)
        self.conv_in = nn.Conv2d(in_channels * f * f, channels[0], 3, padding=1)
        c = channels
        self.body = nn.ModuleList([RefAdapterBlock(c[0], c[0], n), RefAdapterBlock(c[0], c[1], n), RefAdapterBlock(c[1], c[2], n, down=True),
                                   RefAdapterBlock(c[3], c[3], n)])

    def forward(self, x):
        x = self.conv_in(self.unshuffle(x))
        feats = []
        for blk in self.body:
            x = blk(x)
            feats.append(x)
        return feats


class RefT2IAdapter(nn.Module):
    def __init__(self, in_channels=3, channels=(320, 640, 1280, 1280), num_res_blocks=2, downscale_factor=16):
        super().__init__()
        self.adapter = RefFullAdapterXL(in_channels, tuple(channels), num_res_blocks, downscale_factor)

    def forward(self, x):
        return self.adapter(x)


def unet_forward(unet, sample, timestep, encoder_hidden_states, added_cond_kwargs, intrablock=None):
    """oracle.sdxl_unet.UNet2DConditionModel.forward with diffusers' down_intrablock_additional_residuals (four NCHW tensors, already
    scaled; batch 1 or the sample's): feature 0 onto the output of down block 0's downsampler, 1 and 2 onto the output of the last
    attention of down blocks 1 and 2 (block 1: before its downsampler), 3 onto the mid block's output when the shapes match.  The sum
    replaces the tensor for every later reader, the skip included.  None: the plain forward, the same operations in the same order."""
    cfg = unet.config
    b = sample.shape[0]
    t = timestep if torch.is_tensor(timestep) else torch.tensor([timestep], dtype=torch.float32)
    t = t.reshape(-1).expand(b)
    emb = unet.time_embedding(timestep_embedding(t, cfg.block_out_channels[0]).to(sample.dtype))
    te = timestep_embedding(added_cond_kwargs["time_ids"].flatten(), cfg.addition_time_embed_dim).reshape(b, -1)
    add = torch.cat([added_cond_kwargs["text_embeds"], te.to(added_cond_kwargs["text_embeds"].dtype)], dim=-1).to(emb.dtype)
    emb = emb + unet.add_embedding(add)
    res = list(intrablock) if intrablock is not None else []
    if intrablock is not None:
        assert len(res) == 4 and len(unet.down_blocks) == 3 and not unet.down_blocks[0].has_attn
    fit = lambda r: r if r.shape[0] == b else r.repeat(b // r.shape[0], 1, 1, 1)        # [uncond S | cond S] against S features: b % S picks the sample
    h = unet.conv_in(sample)
    skips = [h]
    for bi, blk in enumerate(unet.down_blocks):
        for i, r in enumerate(blk.resnets):
            h = r(h, emb)
            if blk.has_attn:
                h = blk.attentions[i](h, encoder_hidden_states)
                if res and i == len(blk.resnets) - 1:
                    h = h + fit(res.pop(0))              # CrossAttnDownBlock2D: additional_residuals, before the skip is appended
            skips.append(h)
        if blk.downsamplers is not None:
            h = blk.downsamplers[0](h)
            if res and not blk.has_attn:
                h = h + fit(res.pop(0))                  # DownBlock2D: ``sample += r`` mutates the tensor already appended as the skip
            skips.append(h)
    h = unet.mid_block(h, emb, encoder_hidden_states)
    if res and res[0].shape[1:] == h.shape[1:]:
        h = h + fit(res.pop(0))
    for blk in unet.up_blocks:
        h = blk(h, skips, emb, encoder_hidden_states)
    return unet.conv_out(F.silu(unet.conv_norm_out(h)))


@torch.no_grad()
def denoise(unet, adapter, scheduler, latents, prompt_embeds, negative_prompt_embeds, pooled, negative_pooled, height, width,
            control_image, num_inference_steps, guidance_scale=5.0, adapter_conditioning_scale=1.0, adapter_conditioning_factor=1.0):
    """the CFG loop of StableDiffusionXLAdapterPipeline on pre-computed embeddings: the adapter runs once, its features times
    adapter_conditioning_scale go into the UNet at the steps i < int(num_inference_steps * adapter_conditioning_factor).
    adapter=None: the plain loop."""
    s = latents.shape[0]
    scheduler.set_timesteps(num_inference_steps)
    latents = latents * scheduler.init_noise_sigma
    tid = torch.tensor([[height, width, 0, 0, height, width]], dtype=prompt_embeds.dtype)
    ehs = torch.cat([negative_prompt_embeds, prompt_embeds], 0)
    added = {"text_embeds": torch.cat([negative_pooled, pooled], 0), "time_ids": tid.repeat(2 * s, 1)}
    state = [f * adapter_conditioning_scale for f in adapter(control_image)] if adapter is not None else None
    ts = scheduler.timesteps
    for i, t in enumerate(ts):
        x = scheduler.scale_model_input(torch.cat([latents] * 2), t)
        intra = state if state is not None and i < int(len(ts) * adapter_conditioning_factor) else None
        eps = unet_forward(unet, x, t, ehs, added, intra)
        u, c = eps.chunk(2)
        latents = scheduler.step(u + guidance_scale * (c - u), t, latents)[0]
    return latents
