"""The cases of tests/test_gpu_controlnet_edit.py's trajectory tests and their CPU fp32 references (controlnet_edit_reference), computed
once per session and shared by both dtypes.  Everything here runs on the CPU and imports nothing from the product: the oracle models are
the ones tests/test_gpu_inpaint.py's build_pair / build_vae_pair and tests/test_gpu_controlnet.py's _ref_controlnet fill (same seeds), so
the product models those builders load carry the same weights.

A plain helper module; no fixtures, no pytest settings."""
import dataclasses
import functools

import torch

import controlnet_edit_reference as cer
from oracle import modules as om
from oracle.detfill import det_fill, det_randn
from oracle.pipeline import install_ip_processors
from oracle.sdxl_unet import UNet2DConditionModel as OracleUNet
from oracle.sdxl_unet import tiny_config
from oracle.vae import AutoencoderKL as OracleVAE
from oracle.vae import tiny_vae_config

T_TOKENS = 4
GUIDANCE = 5.0

# name -> dict(mode, cin, kind, H, W, S, glist, strength, steps, window, scale).  Steps that run, m = steps - t_start:
#   i2i.*      5 steps x 0.8 -> t_start 1, m = 4; window (0.25, 0.75) keeps steps 1 and 2 of the four and gates off 0 and 3
#   inp4.S1    4 steps x 0.75 -> t_start 1, m = 3; window (0, 0.7) gates off the last
#   inp4.S2    non-square 256 x 288, a generator list, 6 steps x 0.5 -> t_start 3, m = 3; window (0.3, 1) gates off the first
#   inp4.full  strength 1.0 (is_strength_max: pure noise), 3 steps, t_start 0; whole window
#   inp9.S1 / inp9.S2: the 9-channel UNet under the same two schedules (S2 square)
# the mask covers the left half of the image (half_mask); the ControlNet runs at scale 1.0 in the inpainting cases so that the branch
# stays visible where the blend overwrites the unmasked half
CASES = {
    "i2i.ddim": dict(mode="i2i", cin=4, kind="ddim", H=256, W=256, S=1, glist=False, strength=0.8, steps=5, window=(0.25, 0.75), scale=0.8),
    "i2i.dpmpp2m": dict(mode="i2i", cin=4, kind="dpmpp2m", H=256, W=256, S=1, glist=False, strength=0.8, steps=5, window=(0.25, 0.75), scale=0.8),
    "inp4.S1": dict(mode="inp", cin=4, kind="ddim", H=256, W=256, S=1, glist=False, strength=0.75, steps=4, window=(0.0, 0.7), scale=1.0),
    "inp4.S2": dict(mode="inp", cin=4, kind="euler", H=256, W=288, S=2, glist=True, strength=0.5, steps=6, window=(0.3, 1.0), scale=1.0),
    "inp4.full": dict(mode="inp", cin=4, kind="ddim", H=256, W=256, S=1, glist=False, strength=1.0, steps=3, window=(0.0, 1.0), scale=1.0),
    "inp9.S1": dict(mode="inp", cin=9, kind="ddim", H=256, W=256, S=1, glist=False, strength=0.75, steps=4, window=(0.0, 0.7), scale=1.0),
    "inp9.S2": dict(mode="inp", cin=9, kind="euler", H=256, W=256, S=2, glist=True, strength=0.5, steps=6, window=(0.3, 1.0), scale=1.0),
}


def image(H, W):
    return torch.rand(1, 3, H, W, generator=torch.Generator().manual_seed(3)) * 2 - 1


def control_image(H, W, seed=9):
    """tests/test_gpu_controlnet.py's _control_image at any size: in [0, 1], structure at every scale of the hint tower"""
    return det_randn((1, 3, H, W), seed).mul(0.25).add(0.5).clamp(0, 1)


def half_mask(H, W):
    m = torch.zeros(1, 1, H, W)
    m[..., :, :W // 2] = 1.0
    return m


def embeds(S):
    ocfg = tiny_config()
    cd = ocfg.cross_attention_dim
    return dict(prompt_embeds=det_randn((S, 77 + T_TOKENS, cd), 4), negative_prompt_embeds=det_randn((S, 77 + T_TOKENS, cd), 5),
                pooled_prompt_embeds=det_randn((S, ocfg.pooled_dim), 6), negative_pooled_prompt_embeds=det_randn((S, ocfg.pooled_dim), 7))


def gens(S, as_list, seed=11):
    return [torch.Generator().manual_seed(seed + s) for s in range(S)] if as_list else torch.Generator().manual_seed(seed)


@functools.lru_cache(maxsize=None)
def oracle_unet(cin):
    ocfg = dataclasses.replace(tiny_config(), in_channels=cin)
    with torch.no_grad():
        ou = det_fill(OracleUNet(ocfg), 5).eval()
        procs = install_ip_processors(ou, num_tokens=T_TOKENS, scale=0.8)
        for n, p in procs.items():
            if isinstance(p, om.IPAttnProcessor2_0):
                det_fill(p, 7, prefix=n)
    return ou


@functools.lru_cache(maxsize=None)
def oracle_vae():
    return det_fill(OracleVAE(tiny_vae_config()), 3).eval()


@functools.lru_cache(maxsize=None)
def ref_controlnet():
    """a 4-channel ControlNet of the tiny widths, det_filled -- zero convs included, so that the branch acts -- whatever the UNet's
    in_channels (tests/test_gpu_controlnet.py's _ref_controlnet("tiny"), the same object when that module is loaded)"""
    from test_gpu_controlnet import _ref_controlnet
    return _ref_controlnet("tiny")


@functools.lru_cache(maxsize=None)
def reference(name):
    """(the reference's final latents with the ControlNet, without it, the latent mask or None, t_start)"""
    c = CASES[name]
    ou, ov = oracle_unet(c["cin"]), oracle_vae()
    t_start = cer.t_start_of(c["steps"], c["strength"])
    img = image(c["H"], c["W"])
    mask = half_mask(c["H"], c["W"]) if c["mode"] == "inp" else None
    out = []
    for net in (ref_controlnet(), None):
        sch = cer.Sched(c["kind"], c["steps"], t_start)
        init = cer.prepare(ov, sch, img, c["S"], gens(c["S"], c["glist"]), c["strength"], mask=mask, nine=c["cin"] == 9)
        out.append(cer.edit_loop(ou, net, sch, init, embeds(c["S"]), c["H"], c["W"], control_image(c["H"], c["W"]), guidance_scale=GUIDANCE,
                                 conditioning_scale=c["scale"], controlnet_guidance_start=c["window"][0], controlnet_guidance_end=c["window"][1]))
    return out[0], out[1], init["m"], t_start
