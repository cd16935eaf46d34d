"""Test-local restatement of diffusers' FreeU (utils/torch_utils.py ``fourier_filter`` / ``apply_freeu``, recalled from the published
source; diffusers itself is not installed) with torch.fft, and a way to run the UNMODIFIED ``oracle.sdxl_unet.UNet2DConditionModel``
with it: ``UpBlock.forward``'s seven lines are restated here around the oracle's own submodules, with apply_freeu in front of the
concat, and bound to up blocks 0 and 1 for the length of a ``with`` block.  Nothing under oracle/ is edited; imports nothing from the
product.

A plain helper module; no fixtures, no pytest settings."""
import contextlib

import torch


def fourier_filter(x_in, threshold, scale, work=torch.float32):
    """x_in: [B, C, H, W].  diffusers computes in fp32 for bf16 inputs and for sides that are no powers of two, and in the input's
    own precision otherwise; this restatement computes in `work` throughout (fp32: the precision upstream gives a bf16 model; float64
    to pin the closed form) and returns `work`"""
    x = x_in.to(work)
    B, C, H, W = x.shape
    x_freq = torch.fft.fftn(x, dim=(-2, -1))
    x_freq = torch.fft.fftshift(x_freq, dim=(-2, -1))
    mask = torch.ones((B, C, H, W), dtype=work)
    crow, ccol = H // 2, W // 2
    mask[..., crow - threshold:crow + threshold, ccol - threshold:ccol + threshold] = scale
    x_freq = x_freq * mask
    x_freq = torch.fft.ifftshift(x_freq, dim=(-2, -1))
    return torch.fft.ifftn(x_freq, dim=(-2, -1)).real


def apply_freeu(resolution_idx, hidden_states, res_hidden_states, s1, s2, b1, b2):
    """-> (hidden_states, res_hidden_states) in the dtype they came in"""
    if resolution_idx not in (0, 1):
        return hidden_states, res_hidden_states
    b, s = (b1, s1) if resolution_idx == 0 else (b2, s2)
    half = hidden_states.shape[1] // 2
    hidden_states = hidden_states.clone()
    hidden_states[:, :half] = hidden_states[:, :half] * b
    res = fourier_filter(res_hidden_states, 1, s).to(res_hidden_states.dtype)
    return hidden_states, res


def _up_forward(blk, resolution_idx, freeu):
    """oracle.sdxl_unet.UpBlock.forward with apply_freeu in front of the concat"""
    def forward(h, skips, temb, ehs):
        for i, r in enumerate(blk.resnets):
            res = skips.pop()
            h, res = apply_freeu(resolution_idx, h, res, *freeu)
            h = torch.cat([h, res], dim=1)
            h = r(h, temb)
            if blk.has_attn:
                h = blk.attentions[i](h, ehs)
        if blk.upsamplers is not None:
            h = blk.upsamplers[0](h)
        return h
    return forward


@contextlib.contextmanager
def oracle_freeu(unet, s1, s2, b1, b2):
    """inside the block every forward of `unet` (an oracle UNet: its own forward, or tests/controlnet_reference.unet_forward, which
    calls the same up blocks) runs FreeU in up blocks 0 and 1; the modules themselves are left as they were"""
    blocks = list(unet.up_blocks)[:2]
    try:
        for i, blk in enumerate(blocks):
            blk.forward = _up_forward(blk, i, (s1, s2, b1, b2))
        yield unet
    finally:
        for blk in blocks:
            blk.__dict__.pop("forward", None)
