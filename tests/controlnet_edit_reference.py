"""Test-local CPU fp32 restatement of the CFG loops of diffusers 0.30 ``StableDiffusionXLControlNetImg2ImgPipeline`` and
``StableDiffusionXLControlNetInpaintPipeline`` on pre-computed embeddings (guess_mode off, one ControlNet) -- recalled from the published
sources; diffusers itself is not installed, so like the rest of the oracle's diffusers half this is UNPINNED against diffusers
(DESIGN.md section 5).

Built from ``controlnet_reference`` (RefControlNet, unet_forward, keep), the oracle UNet / VAE / schedulers and ``multistep_reference``;
imports nothing from the product.  What the two upstream loops do per step i of the m = len(timesteps) steps that run (timesteps =
get_timesteps(num_inference_steps, strength), the list from t_start on):

    latent_model_input = scale_model_input(cat([latents] * 2), t)
    control_model_input = latent_model_input                                 # the 4-channel latents: taken BEFORE the concat below
    down, mid = controlnet(control_model_input, t, prompt_embeds, control_image, conditioning_scale * controlnet_keep[i])
    if num_channels_unet == 9: latent_model_input = cat([latent_model_input, mask, masked_image_latents], 1)      # the UNet only
    noise_pred = unet(latent_model_input, t, ..., down_block_additional_residuals=down, mid_block_additional_residual=mid)
    noise_pred = uncond + guidance_scale * (text - uncond)
    latents = scheduler.step(noise_pred, t, latents)
    if num_channels_unet == 4 (inpainting): init_latents_proper = image_latents, noised to timesteps[i + 1] on every step but the
        last; latents = (1 - mask) * init_latents_proper + mask * latents

with controlnet_keep[i] = 1 - float(i / m < start or (i + 1) / m > end).  The initial latents are the image-to-image / inpainting
pipelines' own (prepare_latents, prepare_mask_latents): a ControlNet makes no draws, so the generator order is the posterior noise of the
image, the add-noise noise and, with 9 channels, the posterior noise of the masked image.

A plain helper module; no fixtures, no pytest settings."""
import torch
import torch.nn.functional as F

import controlnet_reference as cr
from multistep_reference import RefDPMSolverMultistep
from oracle import modules as om
from oracle.pipeline import set_scale as oracle_set_scale
from oracle.schedulers import DDIMScheduler as OracleDDIM
from oracle.schedulers import EulerDiscreteScheduler as OracleEuler


def t_start_of(steps, strength):
    """get_timesteps: init_timestep = min(int(steps * strength), steps); t_start = max(steps - init_timestep, 0)"""
    return max(steps - min(int(steps * strength), steps), 0)


class Sched:
    """one scheduler of the loop, begun at t_start (get_timesteps + set_begin_index): ``ts`` the timesteps that run, ``pair(row)`` the
    (a, b) of scheduler.add_noise(x, noise, timesteps[row]) = a x + b noise, and the scale_model_input / step surface"""

    def __init__(self, kind, steps, t_start):
        self.kind, self.t_start = kind, t_start
        if kind == "dpmpp2m":
            self.s = RefDPMSolverMultistep(t_start=t_start)               # cuts its own list, begins its step index at t_start
            self.s.set_timesteps(steps)
            self.ts = self.s.timesteps
        else:
            self.s = OracleDDIM() if kind == "ddim" else OracleEuler()
            self.s.set_timesteps(steps)
            self.ts = self.s.timesteps[t_start:]
            if hasattr(self.s, "_i"):
                self.s._i = t_start
        self.init_noise_sigma = self.s.init_noise_sigma

    def pair(self, row):
        if self.kind == "ddim":
            ac = self.s.alphas_cumprod[int(self.s.timesteps[row])]
            return float(ac ** 0.5), float((1 - ac) ** 0.5)
        if self.kind == "euler":
            return 1.0, float(self.s.sigmas[row])
        a, b = RefDPMSolverMultistep._alpha_sigma(self.s.sigmas[row])      # DPMSolverMultistepScheduler.add_noise: alpha_t x + sigma_t noise
        return float(a), float(b)

    def scale_model_input(self, x, t):
        return self.s.scale_model_input(x, t)

    def step(self, eps, t, x):
        return self.s.step(eps, t, x)[0]


def _draw(shape, gens):
    if isinstance(gens, (list, tuple)):
        return torch.cat([torch.randn((1,) + tuple(shape[1:]), generator=g) for g in gens], 0)
    return torch.randn(tuple(shape), generator=gens)


@torch.no_grad()
def prepare(ov, sch, img, S, gens, strength, mask=None, nine=False):
    """prepare_latents / prepare_mask_latents over the oracle VAE -> dict(x = the initial latents, z = the image latents, n2 = the
    add-noise noise, m = the latent mask or None, mz = the masked-image latents or None).  img [1, 3, H, W] in [-1, 1]; mask
    [1, 1, H, W] of zeros and ones (inpainting) or None (image-to-image)."""
    per_sample = isinstance(gens, (list, tuple))
    h, w = img.shape[2] // 8, img.shape[3] // 8
    sf = ov.config.scaling_factor

    def posterior(x, noise):
        mean, logvar = ov.quant_conv(ov.encoder(x)).chunk(2, 1)
        n = noise.shape[0]
        return (mean.repeat(n, 1, 1, 1) + torch.exp(0.5 * logvar.clamp(-30, 20)).repeat(n, 1, 1, 1) * noise) * sf
    n1 = _draw((S if per_sample else 1, 4, h, w), gens)
    z = posterior(img, n1).repeat(S // n1.shape[0], 1, 1, 1)
    n2 = _draw((S, 4, h, w), gens)
    if mask is not None and strength == 1.0:                              # is_strength_max
        x = n2 * sch.init_noise_sigma
    else:
        a, b = sch.pair(sch.t_start)
        x = a * z + b * n2
    m = mz = None
    if mask is not None:
        m = F.interpolate(mask, size=(h, w)).repeat(S, 1, 1, 1)
        if nine:
            n3 = _draw((S if per_sample else 1, 4, h, w), gens)
            mz = posterior(img * (mask < 0.5), n3).repeat(S // n3.shape[0], 1, 1, 1)
    return dict(x=x, z=z, n2=n2, m=m, mz=mz)


@torch.no_grad()
def edit_loop(ou, controlnet, sch, init, emb, height, width, control_image, guidance_scale=5.0, conditioning_scale=1.0,
              controlnet_guidance_start=0.0, controlnet_guidance_end=1.0):
    """the loop of the module docstring.  ou: the oracle UNet (4 or 9 input channels), controlnet: a RefControlNet (4 channels) or None
    (the plain edit), sch: a Sched, init: prepare()'s result (m None: image-to-image, no blend), emb: dict(prompt_embeds,
    negative_prompt_embeds, pooled_prompt_embeds, negative_pooled_prompt_embeds) for S samples."""
    nine = ou.config.in_channels == 9
    x, z, n2, m, mz = (init[k] for k in ("x", "z", "n2", "m", "mz"))
    S = x.shape[0]
    pe, ne, po, no = (emb[k] for k in ("prompt_embeds", "negative_prompt_embeds", "pooled_prompt_embeds", "negative_pooled_prompt_embeds"))
    ids = torch.tensor([[height, width, 0, 0, height, width]], dtype=pe.dtype).repeat(2 * S, 1)
    ehs = torch.cat([ne, pe], 0)
    added = {"text_embeds": torch.cat([no, po], 0), "time_ids": ids}
    ip_scale = next(p.scale for p in ou.attn_processors.values() if isinstance(p, om.IPAttnProcessor2_0))
    oracle_set_scale(ou, ip_scale)                                         # the IP-scale window stays open: control_guidance_* = (0, 1)
    ts = sch.ts
    n = len(ts)
    for i, t in enumerate(ts):
        xin = sch.scale_model_input(torch.cat([x] * 2), t)
        down = mid = None
        if controlnet is not None:
            g = conditioning_scale * cr.keep(i, n, controlnet_guidance_start, controlnet_guidance_end)
            down, mid = controlnet(xin, t, ehs, control_image, conditioning_scale=g, added_cond_kwargs=added)
        if nine:
            xin = torch.cat([xin, torch.cat([m] * 2), torch.cat([mz] * 2)], 1)
        eps = cr.unet_forward(ou, xin, t, ehs, added, down, mid)
        u, c = eps.chunk(2)
        x = sch.step(u + guidance_scale * (c - u), t, x)
        if m is not None and not nine:
            p = z
            if i < n - 1:
                a, b = sch.pair(sch.t_start + i + 1)
                p = a * z + b * n2
            x = (1 - m) * p + m * x
    return x
