"""Denoise pipeline with the call surface of the reference's ``StableDiffusionXLCustomPipeline``
(ip_adapter/custom_pipelines.py:16-394) for the part that is on the hot path: pre-computed prompt
embeddings in, latents out.  Text encoders, the VAE decode and PIL post-processing are the rows
SURVEY.md 8(f) marks "next"; they can be plugged in (``vae_decode`` / ``text_encoder`` callables) but are
not part of this library.
"""
import types
from dataclasses import dataclass
from typing import Any, Callable, List, Optional, Union

import torch

from .attention_processor import IPAttnProcessor
from .denoise import DenoiseEngine
from .lora import LoRAPipelineMixin
from .schedulers import DDIMScheduler, get_timesteps


@dataclass
class StableDiffusionXLPipelineOutput:
    images: Any


def randn_latents(shape, generator=None, dtype=torch.float32):
    """diffusers ``randn_tensor``: one generator, or a list with one generator per sample
    (ip_adapter/utils.py:83-93 builds exactly that for a list of seeds)."""
    if isinstance(generator, (list, tuple)):
        if len(generator) != shape[0]:
            raise ValueError(f"got {len(generator)} generators for a batch of {shape[0]}")
        return torch.cat([torch.randn((1,) + tuple(shape[1:]), generator=g, device=g.device, dtype=dtype).cpu()
                          for g in generator], 0)
    dev = generator.device if generator is not None else "cpu"
    return torch.randn(tuple(shape), generator=generator, device=dev, dtype=dtype).cpu()


def decode_output(vae, vae_decode, latents, output_type, watermark=None):
    """custom_pipelines.py:365-386, the tail of every pipeline call and of generate_pns: 'latent' returns the latents; with ``vae`` (an
    ``imagharmony_amd.vae.AutoencoderKL``) the HIP decode, the watermark if any and the post-processing; else ``vae_decode(latents)``"""
    if output_type == "latent":
        return latents
    if vae is None:
        return vae_decode(latents)
    from .vae import decode_latents, postprocess
    image = decode_latents(vae, latents)
    if watermark is not None:
        image = watermark.apply_watermark(image)
    return postprocess(image, output_type)


# An edit's preparation (image-to-image, inpainting), stated once: the pipelines' __call__ and PNS over edits (pns.edit_prepare_fn,
# IPAdapterXL.generate_pns) both go through these three functions, so a PNS winner is the pipe's own call with that seed's generator.

def edit_moments(vae, img, per_sample, cin=4, strength_max=False, mask=None):
    """What an edit encodes, and at which batch -> (moments, masked_moments); either may be None.  The image's moments are read by a
    4-channel UNet and below strength 1.0 (is_strength_max); a 9-channel UNet also reads those of the masked image
    ``img * (mask < 0.5)`` (prepare_mask_latents), image and mask batch repeated to the larger of the two.  per_sample (the generator is
    a list): every image is encoded on its own, at batch 1 as diffusers encodes them, and read by index."""
    masked = None
    if cin == 9:
        B, Mb = img.shape[0], mask.shape[0]
        Bm = max(B, Mb)
        if Bm % B or Bm % Mb:
            raise ValueError(f"cannot pair an image batch of {B} with a mask batch of {Mb}")
        masked = img.repeat(Bm // B, 1, 1, 1) * (mask.repeat(Bm // Mb, 1, 1, 1) < 0.5)
    need_z = cin == 4 or not strength_max
    encode = (lambda x: torch.cat([vae.encode_moments(x[j:j + 1]) for j in range(x.shape[0])], 0)) if per_sample else vae.encode_moments
    return encode(img) if need_z else None, encode(masked) if masked is not None else None


def edit_draws(generator, S, B, h, w, Bm=None):
    """An edit's draws from ``generator`` (one, or a list with one per sample), in upstream's order -> (n1, n2, n3 or None), fp32 on the
    CPU: the posterior noise of the image (prepare_latents; one generator: one draw per image, B rows, repeated S // B times; a list: S
    rows), the add-noise noise (S rows) and -- Bm given: a 9-channel UNet with Bm masked images -- the posterior noise of the masked
    image (prepare_mask_latents).  The first draw is made even where nothing reads it, so that the order holds in every mode."""
    per_sample = isinstance(generator, (list, tuple))
    n1 = randn_latents((S if per_sample else B, 4, h, w), generator)
    n2 = randn_latents((S, 4, h, w), generator)
    return n1, n2, (randn_latents((S if per_sample else Bm, 4, h, w), generator) if Bm else None)


def edit_prepare(engine, scheduler, t_start, scaling, moments, draws, lmask=None, strength_max=False, masked_moments=None):
    """The hand-over: the initial latents of a schedule that starts at its row t_start -- and, inpainting (lmask: the latent mask), the
    blend / conv_in state -- written into the engine by one fused launch, under the schedule set_schedule has just set"""
    n1, n2, n3 = draws
    a, b = scheduler.add_noise_coefficients(t_start)
    if lmask is None:
        return engine.prepare_img2img(moments, n1, n2, scaling, a, b)
    return engine.prepare_inpaint(moments, n1, n2, scaling, a, b, lmask, strength_max=strength_max, masked_moments=masked_moments, n3=n3)


class _Call(types.SimpleNamespace):
    """One __call__ of a pipeline: its arguments by name (its locals() on entry) and, in four hooks, what that __call__ adds to the
    sequence of StableDiffusionXLCustomPipeline._run -- begin (its refusals; height / width), schedule_kw (the refusals that need the
    batch; set_schedule's extra keywords), condition (the engine calls around set_conditioning) and start (how the initial latents
    reach the engine: returned for denoise, or written into it and None).  The hooks go with the __call__, not with the pipe's class:
    the base class's __call__ on an image-to-image or inpainting pipe is a text-to-image call.  This class: text-to-image."""

    def __init__(self, ns):
        super().__init__(**{k: v for k, v in ns.items() if k != "self"})

    def begin(self, pipe):
        self.height = self.height or pipe.default_sample_size * pipe.vae_scale_factor      # :189-190
        self.width = self.width or pipe.default_sample_size * pipe.vae_scale_factor

    def schedule_kw(self, pipe, S):
        return {}

    def condition(self, pipe, eng):
        pag = pipe.pag_scale_of(self)           # (0.0: the call as it always was)
        eng.set_conditioning(self.prompt_embeds, self.negative_prompt_embeds, self.pooled_prompt_embeds, self.negative_pooled_prompt_embeds,
                             self.height, self.width, self.guidance_scale, guidance_rescale=self.guidance_rescale,
                             original_size=self.original_size, crops_coords_top_left=self.crops_coords_top_left, target_size=self.target_size,
                             **({"pag_scale": pag} if pag else {}))

    def start(self, pipe, eng, S):
        if self.latents is not None:
            return self.latents
        return randn_latents((S, 4, self.height // 8, self.width // 8), self.generator)       # prepare_latents :255-265


class _EditCall(_Call):
    """What the image-to-image and the inpainting __call__ share: the refusals around ``image``, the batch checks, the schedule truncated
    by ``strength`` and, in place of initial noise, the edit preparation above."""

    def __init__(self, ns, edit="image-to-image"):
        super().__init__(ns)
        self.edit, self.inpaint = edit, edit == "inpainting"

    def begin(self, pipe):
        if self.latents is not None:
            raise NotImplementedError(f"latents= is not supported by the {self.edit} path: the initial latents come from `image`")
        if self.image is None:
            raise ValueError(f"{self.edit} needs `image` (PIL, a list of PIL images or a tensor [B, 3, H, W])")
        if self.inpaint and self.mask_image is None:
            raise ValueError("inpainting needs `mask_image` (PIL, a list of PIL images or a tensor; white = repaint)")
        if torch.is_tensor(self.image) and self.image.dim() >= 3 and self.image.shape[-3] == 4:
            raise NotImplementedError("a 4-channel latent `image` is not supported: pass the image itself")
        if not 0.0 <= float(self.strength) <= 1.0:
            raise ValueError(f"strength must be in [0.0, 1.0], got {self.strength}")
        from .vae import preprocess, preprocess_mask
        self.img, self.mask = preprocess(self.image), None                   # image_processor.preprocess
        H, W = self.img.shape[2], self.img.shape[3]
        if self.inpaint:
            if (self.height or H, self.width or W) != (H, W):
                raise NotImplementedError(f"height / width {self.height} x {self.width} differ from the image's {H} x {W}: resize the image first")
            self.mask = preprocess_mask(self.mask_image, H, W)               # mask_processor.preprocess
        if getattr(pipe.vae, "tiny", False):
            pipe.vae.encode()                                                # AutoencoderTiny: its encoder's NotImplementedError
        if pipe.vae is None or not getattr(pipe.vae, "with_encoder", False):
            raise NotImplementedError(f"{self.edit} needs a VAE with its encoder: vae=AutoencoderKL(config, with_encoder=True)")
        self.height, self.width = H, W

    def schedule_kw(self, pipe, S):
        if isinstance(self.generator, (list, tuple)) and len(self.generator) != S:
            raise ValueError(f"got {len(self.generator)} generators for a batch of {S}")
        for what, t in (("an image", self.img), ("a mask", self.mask)):      # prepare_latents, prepare_mask_latents
            if t is not None and (S < t.shape[0] or S % t.shape[0]):
                raise ValueError(f"cannot duplicate {what} batch of {t.shape[0]} to {S} samples")
        pipe.scheduler.set_timesteps(self.num_inference_steps)
        _, self.t_start = get_timesteps(pipe.scheduler, self.num_inference_steps, self.strength)
        return dict(t_start=self.t_start, **({"inpaint": True} if self.inpaint else {}))

    def start(self, pipe, eng, S):
        from .vae import latent_mask
        h, w = self.height // 8, self.width // 8
        cin = pipe.unet.config.in_channels if self.inpaint else 4           # num_channels_unet
        strength_max = self.inpaint and float(self.strength) == 1.0         # is_strength_max
        moments, masked_moments = edit_moments(pipe.vae, self.img, isinstance(self.generator, (list, tuple)), cin, strength_max, self.mask)
        draws = edit_draws(self.generator, S, self.img.shape[0], h, w, Bm=max(self.img.shape[0], self.mask.shape[0]) if cin == 9 else None)
        edit_prepare(eng, pipe.scheduler, self.t_start, pipe.vae.config.scaling_factor, moments, draws,
                     latent_mask(self.mask, h, w) if self.inpaint else None, strength_max, masked_moments)


class StableDiffusionXLCustomPipeline(LoRAPipelineMixin):
    """(LoRAPipelineMixin: diffusers' load_lora_weights / set_adapters / fuse_lora ..., delegated to the UNet -- lora.py)"""
    vae_scale_factor = 8

    def __init__(self, unet, scheduler=None, device="cuda:0", dtype=torch.bfloat16, vae_decode: Optional[Callable] = None,
                 text_encoder: Optional[Callable] = None, use_graph=True, vae=None, watermark=None):
        """vae: an ``imagharmony_amd.vae.AutoencoderKL`` (HIP decode + post-processing for output_type 'pil' / 'np' /
        'pt'); ``vae_decode``: alternatively any callable latents -> images (its result is returned as is)."""
        self.unet = unet
        self.vae = vae
        self.watermark = watermark
        self.scheduler = scheduler or DDIMScheduler()
        self.device = torch.device(device)
        self.dtype = dtype
        self.vae_decode = vae_decode
        self.text_encoder = text_encoder
        self.default_sample_size = unet.config.sample_size
        self.engine = DenoiseEngine(unet, self.device, dtype, use_graph=use_graph)

    def to(self, device):
        self.device = torch.device(device)
        self.unet.to(self.device)
        self.engine = DenoiseEngine(self.unet, self.device, self.dtype, use_graph=self.engine.use_graph)
        return self

    def enable_vae_tiling(self):                                          # test.py:73
        if self.vae is None:
            raise NotImplementedError("no VAE attached (construct the pipeline with vae=AutoencoderKL)")
        self.vae.enable_tiling(True)

    def disable_vae_tiling(self):
        if self.vae is not None:
            self.vae.enable_tiling(False)

    def enable_freeu(self, s1, s2, b1, b2):
        """diffusers' pipe.enable_freeu: delegates to the UNet (unet.UNet2DConditionModel.enable_freeu); the next call records -- or
        picks from the engine's cache -- the plan of that setting.  SDXL's published values: s1 = 0.6, s2 = 0.4, b1 = 1.1, b2 = 1.2."""
        self.unet.enable_freeu(s1, s2, b1, b2)

    def disable_freeu(self):
        self.unet.disable_freeu()

    def set_pag_applied_layers(self, layers):
        """diffusers' PAGMixin.set_pag_applied_layers: delegates to the UNet (unet.UNet2DConditionModel.set_pag_applied_layers; None
        switches it off).  The layers take effect in calls with ``pag_scale > 0``."""
        self.unet.set_pag_applied_layers(layers)

    def pag_scale_of(self, c):
        """the PAG scale a call runs with: its pag_scale (a keyword of the classes that have none in their signature) where layers are
        chosen on the UNet, else 0.0 -- the call as it always was.  Refuses what is not built, before any GPU work."""
        kw = getattr(c, "kwargs", None) or {}
        scale = float(getattr(c, "pag_scale", None) or kw.get("pag_scale") or 0.0)
        adaptive = float(getattr(c, "pag_adaptive_scale", None) or kw.get("pag_adaptive_scale") or 0.0)
        if adaptive != 0.0:
            raise NotImplementedError("pag_adaptive_scale != 0 (the PAG scale decaying with the timestep) is not built")
        if scale < 0.0:
            raise ValueError(f"pag_scale must be >= 0, got {scale}")
        if scale == 0.0 or not getattr(self.unet, "pag_layers", None):
            return 0.0
        for what, other in (("a ControlNet", getattr(self, "controlnet", None)), ("a T2I-Adapter", getattr(self, "adapter", None)),
                            ("regional image prompts (ip_region_masks=)", kw.get("ip_region_masks"))):
            if other is not None:
                raise NotImplementedError(f"perturbed-attention guidance (pag_scale > 0) together with {what} is not built")
        return scale

    def set_scale(self, scale):                                           # custom_pipelines.py:17-20
        for p in self.unet.attn_processors.values():
            if isinstance(p, IPAttnProcessor):
                p.scale = scale

    def encode_prompt(self, prompt, num_images_per_prompt=1, do_classifier_free_guidance=True, negative_prompt=None,
                      **kw):
        if self.text_encoder is None:
            raise NotImplementedError("text encoders are outside the hot path (SURVEY.md 8f-4): pass prompt_embeds, or "
                                      "construct the pipeline with text_encoder=callable")
        return self.text_encoder(prompt, num_images_per_prompt=num_images_per_prompt,
                                 do_classifier_free_guidance=do_classifier_free_guidance, negative_prompt=negative_prompt)

    @torch.no_grad()
    def __call__(self, prompt=None, height=None, width=None, num_inference_steps: int = 50, guidance_scale: float = 5.0,
                 negative_prompt=None, num_images_per_prompt: int = 1, eta: float = 0.0,
                 generator: Optional[Union[torch.Generator, List[torch.Generator]]] = None, latents=None,
                 prompt_embeds=None, negative_prompt_embeds=None, pooled_prompt_embeds=None,
                 negative_pooled_prompt_embeds=None, output_type: Optional[str] = "pil", return_dict: bool = True,
                 control_guidance_start: float = 0.0, control_guidance_end: float = 1.0, guidance_rescale: float = 0.0,
                 callback=None, callback_steps: int = 1, original_size=None, crops_coords_top_left=(0, 0),
                 target_size=None, denoising_end: Optional[float] = None, step_noise: str = "generator",
                 pag_scale: float = 0.0, pag_adaptive_scale: float = 0.0, **kwargs):
        """``pag_scale`` > 0 with layers chosen (set_pag_applied_layers): perturbed-attention guidance, diffusers'
        StableDiffusionXLPAGPipeline -- per sample one more UNet batch member, conditioned like the conditional one and with identity
        self-attention maps in the chosen layers; eps = u + g (c - u) + pag_scale (c - p), or c + pag_scale (c - p) at
        guidance_scale <= 1; guidance_rescale applies to that sum.  pag_scale = 0 or no layers: the call as it always was.
        ``pag_adaptive_scale`` != 0 is refused (NotImplementedError).
        ``output_type`` defaults to "pil" as the reference does (custom_pipelines.py:42), so ``test.py:43``'s
        ``images[0].save(...)`` works; that needs a VAE (``vae=`` / ``vae_decode=``) -- without one the call fails
        BEFORE denoising with a clear error (pass output_type="latent" for latents).  The default scheduler is
        DDIM (BASELINE.json's metric; IP-Adapter convention) -- stock SDXL ships EulerDiscrete: pass
        ``scheduler=EulerDiscreteScheduler()`` for that.
        ``step_noise`` (stochastic schedulers: SDE-DPM-Solver++, Euler ancestral): "generator" (default) draws the per-step noise from
        ``generator`` on the host, in diffusers' order; "seeded" generates it on the device from the generators' seeds (step_seed_table:
        one generator -> its initial_seed() with lane = sample index, a list -> each generator's own seed with lane 0), so that a seed
        reproduces its image whatever the batch -- it needs a generator (ValueError without one)."""
        return self._run(_Call(locals()))

    def _run(self, c: _Call):
        """The call sequence of every pipeline class, once; c: the __call__'s arguments and hooks.  Refusals of arguments that only one
        __call__ has come before, in that __call__."""
        self._refuse(c.output_type, c.eta, c.kwargs)
        self.pag_scale_of(c)
        self.step_seed_table(c.step_noise, c.generator, None)
        masks, weights = c.kwargs.get("ip_region_masks"), c.kwargs.get("ip_region_weights")
        if masks is None and weights is not None:
            raise ValueError("ip_region_weights= comes with ip_region_masks=")
        if masks is not None and (getattr(self, "controlnet", None) is not None or getattr(self, "adapter", None) is not None):
            raise NotImplementedError("regional image prompts (ip_region_masks=) under a ControlNet or a T2I-Adapter are not built")
        c.begin(self)
        if masks is None:
            return self._denoise(c)
        # regional image prompts: prompt_embeds carry text + N * num_tokens tokens; the masks are prepared at the call's height x width
        from .regions import IPRegions
        regions = masks if isinstance(masks, IPRegions) else IPRegions.from_masks(masks, c.height, c.width, weights,
                                                                                  binarize=c.kwargs.get("binarize", True))
        try:
            self.engine.set_ip_regions(regions)
            return self._denoise(c)
        finally:
            self.engine.set_ip_regions(None)        # a later plain call sees num_images == 1 and no regions

    def _denoise(self, c: _Call):
        if c.prompt_embeds is None:
            c.prompt_embeds, c.negative_prompt_embeds, c.pooled_prompt_embeds, c.negative_pooled_prompt_embeds = \
                self.encode_prompt(c.prompt, c.num_images_per_prompt, c.guidance_scale > 1.0, c.negative_prompt)
        if c.pooled_prompt_embeds is None:
            raise ValueError("pooled_prompt_embeds must be passed together with prompt_embeds")     # check_inputs
        S = c.prompt_embeds.shape[0]
        schedule_kw = c.schedule_kw(self, S)
        eng = self.engine
        c.condition(self, eng)
        seed_tab = self.step_seed_table(c.step_noise, c.generator, S)
        eng.set_schedule(self.scheduler, c.num_inference_steps, c.control_guidance_start, c.control_guidance_end,
                         denoising_end=c.denoising_end, **schedule_kw, **({"seeded_noise": True} if seed_tab else {}))
        latents = c.start(self, eng, S)
        out = eng.denoise(latents, callback=c.callback, callback_steps=c.callback_steps, **self._noise_kw(eng, seed_tab, c.generator)).clone()
        out = self._output(out, c.output_type)
        return StableDiffusionXLPipelineOutput(images=out) if c.return_dict else (out,)

    @staticmethod
    def step_seed_table(step_noise, generator, S):
        """step_noise = "generator": None.  "seeded": (seeds, lanes) for DenoiseEngine.denoise(step_seeds=, step_lanes=) -- one generator:
        its initial_seed() for every sample with lanes 0 .. S - 1; a list of S generators: each one's own initial_seed(), lane 0.
        S = None only validates (before any GPU work).  ValueError: another value, or "seeded" without a generator."""
        if step_noise not in ("generator", "seeded"):
            raise ValueError(f'step_noise must be "generator" or "seeded", not {step_noise!r}')
        if step_noise == "generator":
            return None
        if generator is None:
            raise ValueError('step_noise="seeded" derives the step noise from the generator\'s seed: pass generator=')
        if S is None:
            return ()
        if isinstance(generator, (list, tuple)):
            if len(generator) != S:
                raise ValueError(f"got {len(generator)} generators for a batch of {S}")
            return [int(g.initial_seed()) for g in generator], [0] * S
        return [int(generator.initial_seed())] * S, list(range(S))

    @staticmethod
    def _noise_kw(eng, seed_tab, generator):
        """denoise()'s noise arguments: the seed table under a seeded schedule (a deterministic scheduler ignores the flag and draws
        nothing), else the generator as before"""
        if seed_tab and eng.seeded:
            return dict(step_seeds=seed_tab[0], step_lanes=seed_tab[1])
        return dict(generator=generator)

    def _refuse(self, output_type, eta, kwargs):
        if output_type != "latent" and self.vae is None and self.vae_decode is None:
            raise NotImplementedError("output_type=%r needs a VAE: construct the pipeline with "
                                      "vae=imagharmony_amd.vae.AutoencoderKL(...) or vae_decode=callable, or pass "
                                      "output_type='latent'" % (output_type,))
        if eta not in (0, 0.0):
            raise NotImplementedError("eta != 0 (stochastic DDIM) is not supported: the device-resident step is the "
                                      "deterministic x' = cx*x + ce*eps update (the reference runs eta = 0)")
        for k in ("negative_original_size", "negative_target_size", "prompt_2", "negative_prompt_2", "cross_attention_kwargs"):
            if kwargs.get(k) is not None:
                raise NotImplementedError(f"{k} is not supported on this path (custom_pipelines.py:23-56 accepts it for diffusers' sake)")

    def _output(self, out, output_type):
        return out if output_type == "latent" else decode_output(self.vae, self.vae_decode, out, output_type, self.watermark)


class StableDiffusionXLImg2ImgCustomPipeline(StableDiffusionXLCustomPipeline):
    """SDXL image-to-image with diffusers' ``StableDiffusionXLImg2ImgPipeline`` call surface (0.30) for what this path supports: the
    init image is encoded by the HIP VAE encoder (``vae=AutoencoderKL(..., with_encoder=True)``), noised to step t_start of the
    schedule (get_timesteps) by one fused launch, and denoised from there by the device-resident loop.  ``IPAdapterXL(pipe, ...)
    .generate(pil_image=..., image=init, strength=...)`` forwards image / strength here through its **kwargs, as the reference does.

    Known difference: diffusers rounds the initial latents to the pipeline dtype (prepare_latents runs in prompt_embeds.dtype); this
    loop keeps them in fp32, as the text-to-image path keeps its latents."""

    @torch.no_grad()
    def __call__(self, prompt=None, image=None, strength: float = 0.3, num_inference_steps: int = 50, denoising_start=None,
                 denoising_end: Optional[float] = None, guidance_scale: float = 5.0, negative_prompt=None,
                 num_images_per_prompt: int = 1, eta: float = 0.0,
                 generator: Optional[Union[torch.Generator, List[torch.Generator]]] = None, latents=None,
                 prompt_embeds=None, negative_prompt_embeds=None, pooled_prompt_embeds=None,
                 negative_pooled_prompt_embeds=None, output_type: Optional[str] = "pil", return_dict: bool = True,
                 control_guidance_start: float = 0.0, control_guidance_end: float = 1.0, guidance_rescale: float = 0.0,
                 callback=None, callback_steps: int = 1, original_size=None, crops_coords_top_left=(0, 0),
                 target_size=None, aesthetic_score: float = 6.0, negative_aesthetic_score: float = 2.5, step_noise: str = "generator",
                 pag_scale: float = 0.0, pag_adaptive_scale: float = 0.0, **kwargs):
        """aesthetic_score / negative_aesthetic_score are accepted and unused: SDXL base has requires_aesthetics_score=False.
        pag_scale / pag_adaptive_scale: as the text-to-image call.
        step_noise: as the text-to-image call ("seeded": the step noise of a stochastic scheduler from the generators' seeds; the rows
        read are the schedule's rows t_start .. -- the device step counter, not the count of steps that ran).
        Refused: denoising_start (refiner hand-off), a 4-channel latent ``image``, ``latents=``, eta != 0 (NotImplementedError);
        strength outside [0, 1] or a schedule that truncates to no step (ValueError)."""
        if denoising_start is not None:
            raise NotImplementedError("denoising_start (the refiner hand-off) is not supported on this path")
        return self._run(_EditCall(locals()))


class StableDiffusionXLInpaintCustomPipeline(StableDiffusionXLCustomPipeline):
    """SDXL inpainting with diffusers' ``StableDiffusionXLInpaintPipeline`` call surface (0.30) for what this path supports: the edit is
    confined to ``mask_image`` (white = repaint).  The mode follows ``unet.config.in_channels`` as upstream's ``num_channels_unet``:

    * 4 (SDXL base): after every step the region outside the mask is replaced by the init image's latents, noised to the next
      timestep (``__call__``: ``latents = (1 - init_mask) * init_latents_proper + init_mask * latents``) -- here inside the recorded
      step, in the CFG + scheduler launch, so the loop stays graph replays with no host work;
    * 9 (the published SDXL inpainting UNet): conv_in reads ``cat([scale_model_input(latents), mask, masked_image_latents], 1)``; no
      blend.

    The image and (9 channels) the masked image are encoded by the HIP VAE encoder (``vae=AutoencoderKL(..., with_encoder=True)``).
    Draws from ``generator`` (one, or a list with one per sample), in upstream's order: the posterior noise of ``image``
    (prepare_latents), the add-noise noise, then -- 9 channels only -- the posterior noise of ``masked_image`` (prepare_mask_latents).
    Upstream also encodes the masked image and makes the third draw for a 4-channel UNet, where nothing reads the result: this path
    skips both.  With a 9-channel UNet at ``strength == 1.0`` nothing reads the image latents either: the encoder pass is skipped, the
    first draw is still made so that the order above holds in every mode.  ``IPAdapterXL(pipe, ...).generate(pil_image=..., image=init,
    mask_image=mask, strength=...)`` reaches this class through its **kwargs.

    Not supported: soft masks (``mask_processor.blur``), ``padding_mask_crop`` / ``apply_overlay``, the refiner hand-off.  Known
    difference, as for image-to-image: the latents stay fp32 where diffusers rounds them to the pipeline dtype."""

    @torch.no_grad()
    def __call__(self, prompt=None, image=None, mask_image=None, masked_image_latents=None, height=None, width=None,
                 padding_mask_crop=None, strength: float = 0.9999, num_inference_steps: int = 50, denoising_start=None,
                 denoising_end: Optional[float] = None, guidance_scale: float = 7.5, negative_prompt=None,
                 num_images_per_prompt: int = 1, eta: float = 0.0,
                 generator: Optional[Union[torch.Generator, List[torch.Generator]]] = None, latents=None,
                 prompt_embeds=None, negative_prompt_embeds=None, pooled_prompt_embeds=None,
                 negative_pooled_prompt_embeds=None, output_type: Optional[str] = "pil", return_dict: bool = True,
                 control_guidance_start: float = 0.0, control_guidance_end: float = 1.0, guidance_rescale: float = 0.0,
                 callback=None, callback_steps: int = 1, original_size=None, crops_coords_top_left=(0, 0),
                 target_size=None, aesthetic_score: float = 6.0, negative_aesthetic_score: float = 2.5, step_noise: str = "generator",
                 pag_scale: float = 0.0, pag_adaptive_scale: float = 0.0, **kwargs):
        """height / width default to the preprocessed image's size (anything else is refused: resize the image first).
        pag_scale / pag_adaptive_scale: as the text-to-image call; the perturbed member runs under the 4-channel blend and through the
        9-channel conv_in like the other two.
        aesthetic_score / negative_aesthetic_score are accepted and unused, as for image-to-image; step_noise as there.
        Refused before any GPU work -- NotImplementedError: padding_mask_crop, masked_image_latents=, a 4-channel latent ``image``,
        latents=, denoising_start, eta != 0; ValueError: no image, no mask_image, a mask that cannot be brought to the image's size and
        batch, strength outside [0, 1] or a schedule that truncates to no step."""
        if denoising_start is not None:
            raise NotImplementedError("denoising_start (the refiner hand-off) is not supported on this path")
        if padding_mask_crop is not None:
            raise NotImplementedError("padding_mask_crop (crop, inpaint, overlay) is not supported on this path")
        if masked_image_latents is not None:
            raise NotImplementedError("masked_image_latents= is not supported: the masked image is encoded from `image` and `mask_image`")
        return self._run(_EditCall(locals(), "inpainting"))


def prepare_control_image(image, height, width):
    """diffusers StableDiffusionXLControlNetPipeline.prepare_image with VaeImageProcessor(do_normalize=False): a PIL image (or a list of
    them) or a float tensor [n, 3, H, W] / [3, H, W] in [0, 1] -> float32 [n, 3, height, width] in [0, 1], resized when the size
    differs (PIL: Lanczos, upstream's default resample; tensors: bilinear), NOT normalised to [-1, 1]"""
    if torch.is_tensor(image):
        img = image.detach().to("cpu", torch.float32)
        if img.dim() == 3:
            img = img[None]
        if img.dim() != 4 or img.shape[1] != 3:
            raise ValueError(f"control image tensor {tuple(image.shape)}: expected [n, 3, H, W] in [0, 1]")
        if tuple(img.shape[2:]) != (height, width):
            img = torch.nn.functional.interpolate(img, size=(height, width), mode="bilinear", align_corners=False)
        return img.contiguous()
    import numpy as np
    from PIL import Image
    imgs = list(image) if isinstance(image, (list, tuple)) else [image]
    out = []
    for im in imgs:
        if not isinstance(im, Image.Image):
            raise ValueError(f"control image of type {type(im).__name__}: a PIL image, a list of PIL images or a float tensor")
        im = im.convert("RGB")
        if im.size != (width, height):
            im = im.resize((width, height), resample=Image.LANCZOS)
        out.append(torch.from_numpy(np.asarray(im, dtype=np.float32) / 255.0).permute(2, 0, 1))
    return torch.stack(out, 0).contiguous()


class _ControlNetCall(_Call):
    """text-to-image under a ControlNet: the control image (the call's ``image``), the ControlNet's window, the branch's engine calls.
    Every hook goes through super(), so the class also stacks in front of _EditCall (_ControlNetEditCall)."""
    control_arg = "image"

    def begin(self, pipe):
        super().begin(pipe)
        self.cond = prepare_control_image(getattr(self, self.control_arg), self.height, self.width)

    def schedule_kw(self, pipe, S):
        if self.cond.shape[0] not in (1, S):
            raise ValueError(f"{self.cond.shape[0]} control images for {S} samples: one image, or one per sample")
        return dict(super().schedule_kw(pipe, S), controlnet_guidance_start=float(self.controlnet_guidance_start),
                    controlnet_guidance_end=float(self.controlnet_guidance_end))

    def condition(self, pipe, eng):
        eng.set_controlnet(pipe.controlnet)
        super().condition(pipe, eng)
        eng.set_control_image(self.cond, conditioning_scale=float(self.controlnet_conditioning_scale))


class _ControlNetEditCall(_ControlNetCall, _EditCall):
    """an edit under a ControlNet: _EditCall's image / mask / strength and preparation, _ControlNetCall's branch.  The control image is
    ``control_image``, at the edit's height and width; the window travels next to t_start, so it counts the steps that run.  A ControlNet
    makes no draws: the generator order is the edit's own."""
    control_arg = "control_image"


def check_controlnet_args(control, name, scale, guess_mode, start, end):
    """what every ControlNet __call__ (and generate_pns) refuses before any GPU work"""
    if guess_mode:
        raise NotImplementedError("guess_mode is not supported on this path")
    if isinstance(scale, (list, tuple)):
        raise NotImplementedError("a list of conditioning scales belongs to MultiControlNetModel, which is not supported")
    if control is None:
        raise ValueError(f"the ControlNet pipeline needs `{name}`: the control image (PIL or a float tensor [n, 3, H, W] in [0, 1])")
    if not 0.0 <= float(start) <= float(end) <= 1.0:
        raise ValueError(f"controlnet guidance window [{start}, {end}] must satisfy 0 <= start <= end <= 1")


class _ControlNetPipe:
    """what the ControlNet pipeline classes share, in front of their base in the MRO: the ``.controlnet`` attribute (which IPAdapterXL
    looks for), the constructor's refusal of several nets, to() and the engine's set_controlnet"""

    def __init__(self, unet, controlnet, scheduler=None, device="cuda:0", dtype=torch.bfloat16, **kw):
        if isinstance(controlnet, (list, tuple)) or hasattr(controlnet, "nets"):
            raise NotImplementedError("several ControlNets (MultiControlNetModel) are not supported: pass one ControlNetModel")
        super().__init__(unet, scheduler=scheduler, device=device, dtype=dtype, **kw)
        self.controlnet = controlnet
        self.engine.set_controlnet(controlnet)

    def to(self, device):
        super().to(device)
        self.controlnet.to(self.device)
        self.engine.set_controlnet(self.controlnet)
        return self


class StableDiffusionXLControlNetCustomPipeline(_ControlNetPipe, StableDiffusionXLCustomPipeline):
    """Text-to-image under a ControlNet, with diffusers' ``StableDiffusionXLControlNetPipeline`` call surface (0.30) for what this path
    builds: one ``controlnet.ControlNetModel``, one control image (or one per sample), ``controlnet_conditioning_scale`` and a guidance
    window.  The pipe exposes ``.controlnet``, so ``IPAdapterXL(pipe, ...)`` installs ``CNAttnProcessor2_0`` on it (ip_adapter/ip_adapter.py:
    126-133) and ``IPAdapterXL.generate(..., image=, controlnet_conditioning_scale=)`` reaches ``__call__`` through its **kwargs.

    Naming: upstream's ControlNet pipelines call their window ``control_guidance_start / _end``; the reference's custom pipeline uses those
    names for the IP-scale window (custom_pipelines.py:326-329) and they keep that meaning here.  The ControlNet's window is
    ``controlnet_guidance_start / controlnet_guidance_end``.

    The image-to-image and inpainting variants are StableDiffusionXLControlNetImg2ImgCustomPipeline / ...InpaintCustomPipeline below.
    Not built: ``guess_mode``, several ControlNets (``MultiControlNetModel`` / a list) (NotImplementedError)."""

    @torch.no_grad()
    def __call__(self, prompt=None, image=None, height=None, width=None, num_inference_steps: int = 50, guidance_scale: float = 5.0,
                 negative_prompt=None, num_images_per_prompt: int = 1, eta: float = 0.0,
                 generator: Optional[Union[torch.Generator, List[torch.Generator]]] = None, latents=None,
                 prompt_embeds=None, negative_prompt_embeds=None, pooled_prompt_embeds=None,
                 negative_pooled_prompt_embeds=None, output_type: Optional[str] = "pil", return_dict: bool = True,
                 controlnet_conditioning_scale: float = 1.0, guess_mode: bool = False,
                 controlnet_guidance_start: float = 0.0, controlnet_guidance_end: float = 1.0,
                 control_guidance_start: float = 0.0, control_guidance_end: float = 1.0, guidance_rescale: float = 0.0,
                 callback=None, callback_steps: int = 1, original_size=None, crops_coords_top_left=(0, 0),
                 target_size=None, denoising_end: Optional[float] = None, step_noise: str = "generator",
                 pag_scale: float = 0.0, pag_adaptive_scale: float = 0.0, **kwargs):
        """pag_scale / pag_adaptive_scale: the base call's arguments; perturbed-attention guidance next to this conditioner is not built
        and refused where it would be on (NotImplementedError).
        image: the control image -- PIL, a list of PIL images or a float tensor [1 | S, 3, H, W] in [0, 1] -- resized to (height, width),
        not normalised; one image serves every sample.  Everything else as StableDiffusionXLCustomPipeline.__call__.
        Refused before any GPU work: guess_mode, a list of scales (NotImplementedError); no image, a window outside 0 <= start <= end <= 1
        (ValueError)."""
        check_controlnet_args(image, "image", controlnet_conditioning_scale, guess_mode, controlnet_guidance_start, controlnet_guidance_end)
        return self._run(_ControlNetCall(locals()))


class StableDiffusionXLControlNetImg2ImgCustomPipeline(_ControlNetPipe, StableDiffusionXLImg2ImgCustomPipeline):
    """Image-to-image under a ControlNet, with diffusers' ``StableDiffusionXLControlNetImg2ImgPipeline`` call surface (0.30) for what this
    path builds: ``image`` is the init image, encoded and noised to step t_start as in StableDiffusionXLImg2ImgCustomPipeline;
    ``control_image`` steers the steps that run through one ``controlnet.ControlNetModel``.  The recorded step is the text-to-image
    ControlNet step -- the branch over the 4-channel latents, then the UNet with the gated injections -- started at row t_start.

    The ControlNet's window is ``controlnet_guidance_start / controlnet_guidance_end`` (``control_guidance_*`` stays the IP-scale
    window) and counts the m = steps - t_start steps that run: diffusers' ``controlnet_keep`` over ``len(timesteps)``.
    Not built: ``guess_mode``, several ControlNets, a list of scales (NotImplementedError)."""

    @torch.no_grad()
    def __call__(self, prompt=None, image=None, control_image=None, strength: float = 0.3, num_inference_steps: int = 50,
                 denoising_start=None, denoising_end: Optional[float] = None, guidance_scale: float = 5.0, negative_prompt=None,
                 num_images_per_prompt: int = 1, eta: float = 0.0,
                 generator: Optional[Union[torch.Generator, List[torch.Generator]]] = None, latents=None,
                 prompt_embeds=None, negative_prompt_embeds=None, pooled_prompt_embeds=None,
                 negative_pooled_prompt_embeds=None, output_type: Optional[str] = "pil", return_dict: bool = True,
                 controlnet_conditioning_scale: float = 1.0, guess_mode: bool = False,
                 controlnet_guidance_start: float = 0.0, controlnet_guidance_end: float = 1.0,
                 control_guidance_start: float = 0.0, control_guidance_end: float = 1.0, guidance_rescale: float = 0.0,
                 callback=None, callback_steps: int = 1, original_size=None, crops_coords_top_left=(0, 0),
                 target_size=None, aesthetic_score: float = 6.0, negative_aesthetic_score: float = 2.5, step_noise: str = "generator",
                 pag_scale: float = 0.0, pag_adaptive_scale: float = 0.0, **kwargs):
        """pag_scale / pag_adaptive_scale: the parent call's arguments; perturbed-attention guidance under a ControlNet is not built and
        refused where it would be on (NotImplementedError).
        control_image: PIL, a list of PIL images or a float tensor [1 | S, 3, H, W] in [0, 1], brought to the init image's height and
        width, not normalised; one image serves every sample.  Everything else as StableDiffusionXLImg2ImgCustomPipeline.__call__.
        Refused before any GPU work: guess_mode, a list of scales (NotImplementedError); no control_image, a window outside
        0 <= start <= end <= 1 (ValueError); and what the image-to-image call refuses."""
        check_controlnet_args(control_image, "control_image", controlnet_conditioning_scale, guess_mode, controlnet_guidance_start,
                              controlnet_guidance_end)
        if denoising_start is not None:
            raise NotImplementedError("denoising_start (the refiner hand-off) is not supported on this path")
        return self._run(_ControlNetEditCall(locals()))


class StableDiffusionXLControlNetInpaintCustomPipeline(_ControlNetPipe, StableDiffusionXLInpaintCustomPipeline):
    """Inpainting under a ControlNet, with diffusers' ``StableDiffusionXLControlNetInpaintPipeline`` call surface (0.30) for what this
    path builds.  Both modes of StableDiffusionXLInpaintCustomPipeline run next to the branch, in one recorded step and with no launch
    more than the text-to-image ControlNet step: with a 4-channel UNet the masked blend rides in the CFG + scheduler launch; with a
    9-channel UNet only the UNet's conv_in reads [mask | masked-image latents] -- the ControlNet is a 4-channel model and reads the
    scaled latents alone (upstream: ``control_model_input = latent_model_input``, taken before the concat).  ``ControlNetModel.from_unet``
    on a 9-channel UNet stays refused: build the ControlNet from a 4-channel config of the same widths.

    Window naming and counting as in StableDiffusionXLControlNetImg2ImgCustomPipeline.
    Not built: ``guess_mode``, several ControlNets, a list of scales (NotImplementedError)."""

    @torch.no_grad()
    def __call__(self, prompt=None, image=None, mask_image=None, control_image=None, masked_image_latents=None, height=None, width=None,
                 padding_mask_crop=None, strength: float = 0.9999, num_inference_steps: int = 50, denoising_start=None,
                 denoising_end: Optional[float] = None, guidance_scale: float = 7.5, negative_prompt=None,
                 num_images_per_prompt: int = 1, eta: float = 0.0,
                 generator: Optional[Union[torch.Generator, List[torch.Generator]]] = None, latents=None,
                 prompt_embeds=None, negative_prompt_embeds=None, pooled_prompt_embeds=None,
                 negative_pooled_prompt_embeds=None, output_type: Optional[str] = "pil", return_dict: bool = True,
                 controlnet_conditioning_scale: float = 1.0, guess_mode: bool = False,
                 controlnet_guidance_start: float = 0.0, controlnet_guidance_end: float = 1.0,
                 control_guidance_start: float = 0.0, control_guidance_end: float = 1.0, guidance_rescale: float = 0.0,
                 callback=None, callback_steps: int = 1, original_size=None, crops_coords_top_left=(0, 0),
                 target_size=None, aesthetic_score: float = 6.0, negative_aesthetic_score: float = 2.5, step_noise: str = "generator",
                 pag_scale: float = 0.0, pag_adaptive_scale: float = 0.0, **kwargs):
        """pag_scale / pag_adaptive_scale: the parent call's arguments; perturbed-attention guidance under a ControlNet is not built and
        refused where it would be on (NotImplementedError).
        control_image: as for StableDiffusionXLControlNetImg2ImgCustomPipeline, at the init image's height and width.  Everything else
        as StableDiffusionXLInpaintCustomPipeline.__call__, defaults included.
        Refused before any GPU work: guess_mode, a list of scales (NotImplementedError); no control_image, a window outside
        0 <= start <= end <= 1 (ValueError); and what the inpainting call refuses."""
        check_controlnet_args(control_image, "control_image", controlnet_conditioning_scale, guess_mode, controlnet_guidance_start,
                              controlnet_guidance_end)
        if denoising_start is not None:
            raise NotImplementedError("denoising_start (the refiner hand-off) is not supported on this path")
        if padding_mask_crop is not None:
            raise NotImplementedError("padding_mask_crop (crop, inpaint, overlay) is not supported on this path")
        if masked_image_latents is not None:
            raise NotImplementedError("masked_image_latents= is not supported: the masked image is encoded from `image` and `mask_image`")
        return self._run(_ControlNetEditCall(locals(), "inpainting"))


def prepare_adapter_image(image):
    """diffusers ``_preprocess_adapter_image``: a PIL image (or a list of them) -> float32 [n, 3, H, W] in [0, 1] (``/ 255``, not normalised);
    a float tensor [n, 3, H, W] / [3, H, W] in [0, 1] passes through.  Nothing is resized: the adapter's features are tied to the pixels,
    and a control image of another size than the call's is refused (T2IAdapter.check_image)."""
    if torch.is_tensor(image):
        img = image.detach().to("cpu", torch.float32)
        return (img[None] if img.dim() == 3 else img).contiguous()
    import numpy as np
    from PIL import Image
    imgs = list(image) if isinstance(image, (list, tuple)) else [image]
    out = []
    for im in imgs:
        if torch.is_tensor(im):
            out.append(im.detach().to("cpu", torch.float32).reshape((-1,) + tuple(im.shape[-2:])))
            continue
        if not isinstance(im, Image.Image):
            raise ValueError(f"adapter image of type {type(im).__name__}: a PIL image, a list of PIL images or a float tensor")
        out.append(torch.from_numpy(np.asarray(im.convert("RGB"), dtype=np.float32) / 255.0).permute(2, 0, 1))
    if len({tuple(t.shape) for t in out}) != 1:
        raise ValueError("the adapter images of one call must share one size")
    return torch.stack(out, 0).contiguous()


def check_adapter_args(image, scale, factor):
    """what the adapter __call__ (and generate_pns) refuses before any GPU work"""
    if image is None:
        raise ValueError("the T2I-Adapter pipeline needs `image`: the control image (PIL or a float tensor [n, 3, H, W] in [0, 1])")
    if isinstance(scale, (list, tuple)):
        raise NotImplementedError("a list of conditioning scales belongs to MultiAdapter, which is not supported")
    if not 0.0 <= float(factor) <= 1.0:
        raise ValueError(f"adapter_conditioning_factor {factor} must lie in [0, 1]")


class _AdapterCall(_Call):
    """text-to-image under a T2I-Adapter: the control image (the call's ``image``) fixes height / width unless they are given, the
    adapter's scale and factor travel to the engine"""

    def begin(self, pipe):
        self.cond = prepare_adapter_image(self.image)
        if self.cond.dim() != 4:
            raise ValueError(f"adapter image {tuple(self.cond.shape)}: expected [n, 3, H, W]")
        self.height = self.height or int(self.cond.shape[2])               # upstream's _default_height_width: the image's
        self.width = self.width or int(self.cond.shape[3])
        pipe.adapter.check_image(self.cond, self.height, self.width)
        super().begin(pipe)

    def schedule_kw(self, pipe, S):
        if self.cond.shape[0] not in (1, S):
            raise ValueError(f"{self.cond.shape[0]} adapter images for {S} samples: one image, or one per sample")
        return dict(super().schedule_kw(pipe, S), adapter_conditioning_factor=float(self.adapter_conditioning_factor))

    def condition(self, pipe, eng):
        eng.set_adapter(pipe.adapter)
        super().condition(pipe, eng)
        eng.set_adapter_image(self.cond, conditioning_scale=float(self.adapter_conditioning_scale))


class StableDiffusionXLAdapterCustomPipeline(StableDiffusionXLCustomPipeline):
    """Text-to-image under a T2I-Adapter, with diffusers' ``StableDiffusionXLAdapterPipeline`` call surface (0.30) for what this path
    builds: one ``t2i_adapter.T2IAdapter`` ("full_adapter_xl"), one control image (or one per sample), ``adapter_conditioning_scale`` and
    ``adapter_conditioning_factor`` (the fraction of the steps, from the first, that get the features).  The adapter runs once per
    control image -- a second call with the same image computes nothing --; the recorded step is the text-to-image step plus four gated
    adds.  The pipe exposes ``.adapter``; ``IPAdapterXL.generate(..., image=, adapter_conditioning_scale=, adapter_conditioning_factor=)``
    reaches ``__call__`` through its **kwargs.  Every sampler and ``step_noise`` mode of the base pipeline works unchanged.

    Not built: the adapter in image-to-image / inpainting, together with a ControlNet, several adapters (``MultiAdapter`` / a list), the
    SD-1.x adapter types (NotImplementedError)."""

    def __init__(self, unet, adapter, scheduler=None, device="cuda:0", dtype=torch.bfloat16, **kw):
        if isinstance(adapter, (list, tuple)) or hasattr(adapter, "adapters"):
            raise NotImplementedError("several adapters (MultiAdapter / a list of adapters) are not supported: pass one T2IAdapter")
        super().__init__(unet, scheduler=scheduler, device=device, dtype=dtype, **kw)
        self.adapter = adapter
        self.engine.set_adapter(adapter)

    def to(self, device):
        super().to(device)
        self.adapter.to(self.device)
        self.engine.set_adapter(self.adapter)
        return self

    @torch.no_grad()
    def __call__(self, prompt=None, image=None, height=None, width=None, num_inference_steps: int = 50, guidance_scale: float = 5.0,
                 negative_prompt=None, num_images_per_prompt: int = 1, eta: float = 0.0,
                 generator: Optional[Union[torch.Generator, List[torch.Generator]]] = None, latents=None,
                 prompt_embeds=None, negative_prompt_embeds=None, pooled_prompt_embeds=None,
                 negative_pooled_prompt_embeds=None, output_type: Optional[str] = "pil", return_dict: bool = True,
                 adapter_conditioning_scale: float = 1.0, adapter_conditioning_factor: float = 1.0,
                 control_guidance_start: float = 0.0, control_guidance_end: float = 1.0, guidance_rescale: float = 0.0,
                 callback=None, callback_steps: int = 1, original_size=None, crops_coords_top_left=(0, 0),
                 target_size=None, denoising_end: Optional[float] = None, step_noise: str = "generator",
                 pag_scale: float = 0.0, pag_adaptive_scale: float = 0.0, **kwargs):
        """pag_scale / pag_adaptive_scale: the base call's arguments; perturbed-attention guidance next to this conditioner is not built
        and refused where it would be on (NotImplementedError).
        image: the control image -- PIL, a list of PIL images or a float tensor [1 | S, 3, H, W] in [0, 1] --, not normalised and not
        resized: its sides are multiples of 2 x the adapter's downscale factor (32) and equal height / width (which default to the
        image's); one image serves every sample.  Everything else as StableDiffusionXLCustomPipeline.__call__.
        Refused before any GPU work: a list of scales (NotImplementedError); no image, an image of another size, a factor outside
        [0, 1] (ValueError)."""
        check_adapter_args(image, adapter_conditioning_scale, adapter_conditioning_factor)
        return self._run(_AdapterCall(locals()))
