"""Dry recordings of the full-SDXL-width UNet forward at the resolutions the product accepts (test infrastructure: no GPU, no compute).

The forward is chosen by shape -- tile variants from tuning.json keyed by (M, N, K), the folded LayerNorm only at 64-aligned token
counts, the ragged self-attention below that, halo convs wherever a table entry names one -- so each geometry below records a
different launch set.  Shared by the CPU pins (tests/test_host_logic.py) and the GPU launch sweep (tests/test_gpu_resolutions.py)."""
import torch

# (S, Hl, Wl): S latents, UNet batch 2S (CFG)
RESOLUTIONS = [(1, 128, 128),                      # 1024^2, the benchmarked geometry: tuned variants
               (1, 112, 144), (1, 144, 112),       # 1152x896: generic tiles, ragged deepest level (1008 tokens), unfused LayerNorm
               (1, 96, 168), (1, 168, 96),         # 1344x768
               (1, 80, 192), (1, 192, 80),         # 1536x640: generic tiles, unfused GroupNorm
               (1, 64, 256), (1, 256, 64),         # 2048x512: M coincides with 128x128 -> the tuned halo convs at another H x W
               (1, 104, 152), (1, 152, 104),       # 832x1216: 988 tokens at the deepest level (not a multiple of 16)
               (2, 128, 128), (4, 128, 128)]       # num_samples 2 / PNS batch 4 at 1024^2


def sdxl_unet_meta(dtype=torch.bfloat16):
    """the full-width UNet with IP processors, uninitialised CPU weights (recording reads shapes and pointers only)"""
    from imagharmony_amd.ip_adapter import install_ip_processors
    from imagharmony_amd.unet import UNet2DConditionModel, UNetConfig
    with torch.device("meta"):
        u = UNet2DConditionModel(UNetConfig())
    u = u.to_empty(device="cpu").to(dtype)
    install_ip_processors(u, num_tokens=4, device="cpu", dtype=dtype, init="empty")
    return u


def record_forward(u, S, Hl, Wl, dtype=torch.bfloat16):
    """one dry-recorded forward at latent Hl x Wl, S latents (UNet batch 2S) -> the recording Ctx"""
    from imagharmony_amd.ctx import Ctx
    B = 2 * S
    ctx = Ctx("cpu", dtype, record=True, dry=True)
    st = u.prepare_conditioning(ctx, torch.zeros(B, 81, 2048), torch.zeros(B, 1280), torch.zeros(B, 6))
    st.t_value = torch.zeros(B)
    st.latents = torch.zeros(S, 4, Hl, Wl)
    u.emit_forward(ctx, st, S, Hl, Wl, cfg_dup=True)
    return ctx
