"""Perturbed-attention guidance (Ahn et al. 2024) restated from diffusers' published source around the oracle's own pieces, for the
tests: diffusers is not installed here, and oracle.pipeline.denoise cannot take a third chunk.  Imports nothing from the product.

  * PAGIdentitySelfAttn -- diffusers' PAGCFGIdentitySelfAttnProcessor2_0 / PAGIdentitySelfAttnProcessor2_0: the batch is
    [uncond | cond | perturbed] (or [cond | perturbed]); all chunks but the last go through the wrapped processor unchanged, the last
    one skips the attention map: out = to_out(to_v(x)), then the residual and the rescale as for the others.
  * oracle_pag -- PAGMixin._set_pag_attn_processor for the length of a ``with`` block: every entry of ``layers`` is re.search-ed in the
    names of the self-attention (attn1) modules, as diffusers >= 0.30 matches pag_applied_layers.
  * denoise_pag -- oracle.pipeline.denoise's loop with PAGMixin._prepare_perturbed_attention_guidance (the conditional rows once more)
    and _apply_perturbed_attention_guidance (eps = u + g (c - u) + s (c - p), or c + s (c - p) without CFG); guidance_rescale as
    StableDiffusionXLPAGPipeline applies it: rescale_noise_cfg(eps, c, phi), only with CFG."""
import contextlib
import re

import torch
import torch.nn as nn

from oracle.modules import IPAttnProcessor2_0
from oracle.pipeline import rescale_noise_cfg, set_scale


class PAGIdentitySelfAttn(nn.Module):
    def __init__(self, inner, k):
        super().__init__()
        self.inner, self.k = inner, int(k)

    def __call__(self, attn, hidden_states, encoder_hidden_states=None, attention_mask=None, temb=None, *args, **kwargs):
        assert encoder_hidden_states is None, "installed on self-attention layers only"
        n = hidden_states.shape[0] - self.k
        org = self.inner(attn, hidden_states[:n])
        x = hidden_states[n:]
        o = attn.to_out[1](attn.to_out[0](attn.to_v(x)))              # the attention map is the identity: the values themselves
        if attn.residual_connection:
            o = o + x
        return torch.cat([org, o / attn.rescale_output_factor], 0)


def pag_layer_names(unet, layers):
    """names of the attn1 modules that ``layers`` (a pattern or a list of patterns) chooses; ValueError for a pattern without a match"""
    pats = [layers] if isinstance(layers, str) else list(layers)
    attn1 = [n[:-len(".processor")] for n in unet.attn_processors if n.endswith("attn1.processor")]
    hit = []
    for pat in pats:
        m = [n for n in attn1 if re.search(pat, n) is not None]
        if not m:
            raise ValueError(f"cannot find a PAG layer to set the attention processor for: {pat}")
        hit += [n for n in m if n not in hit]
    return hit


@contextlib.contextmanager
def oracle_pag(unet, layers, k):
    """inside the block the last k samples of every forward of `unet` run identity self-attention in the chosen layers; the processors
    are put back on exit"""
    mods = dict(unet.named_modules())
    chosen = [mods[n] for n in pag_layer_names(unet, layers)]
    saved = [m.get_processor() for m in chosen]
    try:
        for m, p in zip(chosen, saved):
            m.set_processor(PAGIdentitySelfAttn(p, k))
        yield unet
    finally:
        for m, p in zip(chosen, saved):
            m.set_processor(p)


def combine(eps, guidance_scale, pag_scale, do_cfg, guidance_rescale=0.0):
    """PAGMixin._apply_perturbed_attention_guidance (+ rescale_noise_cfg as the PAG pipelines call it)"""
    if do_cfg:
        u, c, p = eps.chunk(3)
        out = u + guidance_scale * (c - u) + pag_scale * (c - p)
        if guidance_rescale > 0.0:
            out = rescale_noise_cfg(out, c, guidance_rescale)
        return out
    c, p = eps.chunk(2)
    return c + pag_scale * (c - p)


@torch.no_grad()
def denoise_pag(unet, scheduler, latents, prompt_embeds, negative_prompt_embeds, pooled, negative_pooled, height, width,
                num_inference_steps=30, guidance_scale=5.0, pag_scale=3.0, layers="mid", guidance_rescale=0.0):
    """oracle.pipeline.denoise with the perturbed member: batch [uncond | cond | perturbed] under CFG, else [cond | perturbed]"""
    s = latents.shape[0]
    do_cfg = guidance_scale > 1.0
    scheduler.set_timesteps(num_inference_steps)
    latents = latents * scheduler.init_noise_sigma
    tid = torch.tensor([[height, width, 0, 0, height, width]], dtype=prompt_embeds.dtype).repeat(s, 1)
    neg = do_cfg
    ehs = torch.cat(([negative_prompt_embeds] if neg else []) + [prompt_embeds, prompt_embeds], 0)
    text = torch.cat(([negative_pooled] if neg else []) + [pooled, pooled], 0)
    ids = torch.cat([tid] * (3 if neg else 2), 0)
    cond_scale = next(p.scale for p in unet.attn_processors.values() if isinstance(p, IPAttnProcessor2_0))
    set_scale(unet, cond_scale)
    with oracle_pag(unet, layers, s):
        for t in scheduler.timesteps:
            x = scheduler.scale_model_input(torch.cat([latents] * (3 if neg else 2)), t)
            eps = unet(x, t, encoder_hidden_states=ehs, added_cond_kwargs={"text_embeds": text, "time_ids": ids})[0]
            latents = scheduler.step(combine(eps, guidance_scale, pag_scale, do_cfg, guidance_rescale), t, latents)[0]
    return latents
