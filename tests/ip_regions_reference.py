"""fp32 torch restatement of regional image prompts, the reference the tests of imagharmony_amd.regions / csrc/xattn_regions.hip compare
against: the reference's IPAttnProcessor2_0 math (oracle/modules.py, attention_processor.py:364-465) with the per-image loop and
``scale * w_i * (ip_i * m_i)`` of diffusers' IPAdapterAttnProcessor2_0 (ip_adapter_masks, several images per adapter), and diffusers'
IPAdapterMaskProcessor.downsample (bicubic, fp32, not clamped) for the masks.  A plain helper module: no fixtures, no pytest settings.

``RegionsProcessor`` follows the oracle UNet's processor protocol (``__call__(attn, hidden_states, encoder_hidden_states=...)``), so it
plugs into oracle.sdxl_unet through ``set_attn_processor`` like oracle.modules' processors do."""
import math

import torch
import torch.nn.functional as F

from oracle import modules as om


def diffusers_grid(L, Hm, Wm):
    """IPAdapterMaskProcessor.downsample's float rule, verbatim: mask_h = int(sqrt(L / (Wm / Hm))), plus one if L does not divide"""
    ratio = Wm / Hm
    mask_h = int(math.sqrt(L / ratio))
    mask_h = int(mask_h) + int((L % int(mask_h)) != 0)
    return mask_h, L // mask_h


def downsample(masks, h, w):
    """masks fp32 [N, Hm, Wm] -> [N, h * w]: F.interpolate(mask.unsqueeze(0), size=(h, w), mode="bicubic").squeeze(0), flattened"""
    return F.interpolate(masks.float().unsqueeze(0), size=(h, w), mode="bicubic").squeeze(0).reshape(masks.shape[0], h * w)


def _heads(t, b, h):
    return t.view(b, -1, h, t.shape[-1] // h).transpose(1, 2)


def regions_attention(q, k, v, ks, vs, rows, weights, scale, heads):
    """q [B, L, C]; text k / v [B, Lk, C]; per image ks[i] / vs[i] [B, T, C]; rows [N, L]; -> [B, L, C] in q's dtype:
    sdpa(q, k, v) + sum_i scale * w_i * (sdpa(q, k_i, v_i) * m_i)"""
    b = q.shape[0]
    qh = _heads(q, b, heads)
    o = F.scaled_dot_product_attention(qh, _heads(k, b, heads), _heads(v, b, heads))
    o = o.transpose(1, 2).reshape(b, -1, q.shape[-1]).to(q.dtype)
    for i in range(len(ks)):
        io = F.scaled_dot_product_attention(qh, _heads(ks[i], b, heads), _heads(vs[i], b, heads))
        io = io.transpose(1, 2).reshape(b, -1, q.shape[-1]).to(q.dtype)
        m = rows[i].to(q.dtype)[None, :, None]
        o = o + scale * weights[i] * (io * m)
    return o


class RegionsProcessor(om.IPAttnProcessor2_0):
    """oracle.modules.IPAttnProcessor2_0 (a subclass: oracle.pipeline's loop finds and gates it like the plain one) with num_images masked image prompts: the encoder states end in num_images * num_tokens image
    tokens [r0 | r1 | ...].  masks: fp32 [N, Hm, Wm]; grid: {L: (h, w)} for the layers whose grid the caller knows, else the float rule."""

    def __init__(self, hidden_size, cross_attention_dim=None, scale=1.0, num_tokens=4, skip=False, masks=None, weights=None, grid=None):
        super().__init__(hidden_size, cross_attention_dim, scale=scale, num_tokens=num_tokens, skip=skip)
        self.masks = masks
        self.num_images = int(masks.shape[0])
        self.weights = [1.0] * self.num_images if weights is None else [float(w) for w in weights]
        self.grid = grid or {}

    def __call__(self, attn, hidden_states, encoder_hidden_states=None, attention_mask=None, temb=None):
        residual = hidden_states
        L = hidden_states.shape[1]
        q = attn.to_q(hidden_states)
        end = encoder_hidden_states.shape[1] - self.num_images * self.num_tokens
        text, ip = encoder_hidden_states[:, :end], encoder_hidden_states[:, end:]
        k, v = attn.to_k(text), attn.to_v(text)
        ks, vs, rows = [], [], None
        if not self.skip:
            h, w = self.grid.get(L) or diffusers_grid(L, self.masks.shape[1], self.masks.shape[2])
            rows = downsample(self.masks, h, w)
            for i in range(self.num_images):
                tok = ip[:, i * self.num_tokens:(i + 1) * self.num_tokens]
                ks.append(self.to_k_ip(tok))
                vs.append(self.to_v_ip(tok))
        o = regions_attention(q, k, v, ks, vs, rows, self.weights, self.scale, attn.heads)
        o = attn.to_out[1](attn.to_out[0](o))
        if attn.residual_connection:
            o = o + residual
        return o / attn.rescale_output_factor


def install(ou, masks, weights=None, grid=None):
    """replace every oracle IPAttnProcessor2_0 of the oracle UNet `ou` by a RegionsProcessor with the same weights -> the processors"""
    procs = dict(ou.attn_processors)
    for name, p in list(procs.items()):
        if isinstance(p, om.IPAttnProcessor2_0):
            r = RegionsProcessor(p.hidden_size, p.cross_attention_dim, scale=p.scale, num_tokens=p.num_tokens, skip=p.skip, masks=masks,
                                 weights=weights, grid=grid)
            r.load_state_dict(p.state_dict())
            procs[name] = r
    ou.set_attn_processor(procs)
    return procs
