"""Adapter API of the reference (ip_adapter/ip_adapter.py) on the HIP hot path.

``install_ip_processors`` is ``IPAdapter.set_ip_adapter`` (ip_adapter.py:99-125): attn1 layers get
``AttnProcessor2_0``, attn2 layers get ``IPAttnProcessor2_0`` whose image-prompt branch is active only
under ``down_blocks.2.attentions.1`` (:117; the ``target_blocks`` argument is ignored upstream, :75).
"""
import torch

from .attention_processor import AttnProcessor2_0, CNAttnProcessor2_0, IPAttnProcessor2_0

ACTIVE_BLOCK = "down_blocks.2.attentions.1"


def install_ip_processors(unet, num_tokens=4, scale=1.0, device=None, dtype=torch.float16, init="default"):
    cfg = unet.config
    procs = {}
    for name in unet.attn_processors.keys():
        cross = None if name.endswith("attn1.processor") else cfg.cross_attention_dim
        if name.startswith("mid_block"):
            hidden = cfg.block_out_channels[-1]
        elif name.startswith("up_blocks"):
            hidden = list(reversed(cfg.block_out_channels))[int(name[len("up_blocks.")])]
        else:
            hidden = cfg.block_out_channels[int(name[len("down_blocks.")])]
        if cross is None:
            procs[name] = AttnProcessor2_0()
        else:
            if init == "empty":      # skip the (slow) CPU kaiming init: weights are loaded / filled afterwards
                with torch.device("meta"):
                    p = IPAttnProcessor2_0(hidden, cross, scale=scale, num_tokens=num_tokens, skip=ACTIVE_BLOCK not in name)
                p = p.to_empty(device=device or "cpu").to(dtype)
            else:
                p = IPAttnProcessor2_0(hidden, cross, scale=scale, num_tokens=num_tokens, skip=ACTIVE_BLOCK not in name)
                p = p.to(device=device, dtype=dtype)
            procs[name] = p
    unet.set_attn_processor(procs)
    return procs


def set_scale(unet, scale):
    """IPAdapter.set_scale (ip_adapter.py:179-182) / StableDiffusionXLCustomPipeline.set_scale (custom_pipelines.py:17-20)"""
    for p in unet.attn_processors.values():
        if isinstance(p, IPAttnProcessor2_0):
            p.scale = scale


def set_ip_regions(unet, regions):
    """regional image prompts (regions.IPRegions: N masks over the picture, N weights) on every IP / ControlNet cross-attention
    processor of `unet`, or None to take them off: the encoder states then end in N * num_tokens image tokens [r0 | r1 | ...].  Every
    processor slices that many tokens off (the skip=True ones too, as they always slice num_tokens); the ones with an image-prompt
    branch apply image i where mask i says."""
    from .regions import IPRegions
    if regions is not None and not isinstance(regions, IPRegions):
        raise TypeError(f"set_ip_regions takes an imagharmony_amd.regions.IPRegions or None, not {type(regions).__name__}")
    for p in unet.attn_processors.values():
        if isinstance(p, (IPAttnProcessor2_0, CNAttnProcessor2_0)):
            p.num_images = regions.n if regions is not None else 1
            p.regions = regions


# --------------------------------------------------------------------------------------------
# Adapter classes (API surface of ip_adapter/ip_adapter.py:69-478 for the SDXL variants)
# --------------------------------------------------------------------------------------------
import os
from typing import List

from .modules import HarmonyAttention, ImageProjModel, MLPProjModel, Resampler  # noqa: E402,F401
from .utils import get_generator  # noqa: E402

IPAttnProcessor = IPAttnProcessor2_0


def _prompts(prompt, negative_prompt, n=None):
    """the reference's prompt defaults (ip_adapter.py:200-212); n given: a single prompt is broadcast to a list of n"""
    prompt = prompt if prompt is not None else "best quality, high quality"
    negative_prompt = negative_prompt if negative_prompt is not None else \
        "monochrome, lowres, bad anatomy, worst quality, low quality"
    if n is not None and not isinstance(prompt, List):
        prompt = [prompt] * n
    if n is not None and not isinstance(negative_prompt, List):
        negative_prompt = [negative_prompt] * n
    return prompt, negative_prompt


def _default_batch(n_seeds):
    """PNS candidates stacked per UNet forward: as many as a rank holds, up to 4"""
    import torch.distributed as dist
    world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
    return min(4, (n_seeds + world - 1) // world)


class IPAdapter:
    """``IPAdapter.__init__`` / ``set_ip_adapter`` / ``load_ip_adapter`` / ``get_image_embeds`` / ``set_scale``
    (ip_adapter.py:70-182).  Differences, all behaviour-compatible: the compute dtype is a parameter (the
    reference hard-codes fp16 in 8 places), ``number_class_crossattention`` may be None (ip_adapter.py:85
    crashes), the ``.safetensors`` branch works (ip_adapter.py:137-147 writes a missing key), and an already
    constructed CLIP vision model / pre-computed CLIP embeddings may be supplied (no network here)."""

    def __init__(self, sd_pipe, image_encoder_path, ip_ckpt, device, num_tokens=4, target_blocks=None,
                 number_class_crossattention=None, image_encoder=None, dtype=torch.float16, clip_embeddings_dim=1280,
                 clip_hidden_size=1280, clip_image_processor=None, image_encoder_backend="transformers"):
        """image_encoder_backend: what ``image_encoder_path`` is loaded into -- "transformers" (default): the stock
        CLIPVisionModelWithProjection; "hip": imagharmony_amd.clip_vision.CLIPVisionEncoder (the tower on this library's kernels).  An
        ``image_encoder`` passed in is used as it is, whichever of the two it is."""
        if image_encoder_backend not in ("transformers", "hip"):
            raise ValueError(f"image_encoder_backend={image_encoder_backend!r}: 'transformers' or 'hip'")
        self.image_encoder_backend = image_encoder_backend
        self.device = device
        self.dtype = dtype
        self.image_encoder_path = image_encoder_path
        self.ip_ckpt = ip_ckpt
        self.num_tokens = num_tokens
        self.pipe = sd_pipe.to(self.device)
        self.set_ip_adapter()
        self.image_encoder = image_encoder
        self.clip_image_processor = clip_image_processor
        if image_encoder is not None and clip_image_processor is None:
            from transformers import CLIPImageProcessor                                     # ip_adapter.py:84
            self.clip_image_processor = CLIPImageProcessor()
        if image_encoder is None and image_encoder_path is not None and image_encoder_backend == "hip":
            from transformers import CLIPImageProcessor
            from .clip_vision import CLIPVisionEncoder
            self.image_encoder = CLIPVisionEncoder.from_pretrained(image_encoder_path, device=self.device, dtype=dtype)
            self.clip_image_processor = clip_image_processor or CLIPImageProcessor()
        elif image_encoder is None and image_encoder_path is not None:
            from transformers import CLIPImageProcessor, CLIPVisionModelWithProjection       # ip_adapter.py:81-84
            self.image_encoder = CLIPVisionModelWithProjection.from_pretrained(image_encoder_path).to(self.device, dtype=dtype)
            self.clip_image_processor = CLIPImageProcessor()
        self.clip_embeddings_dim = getattr(getattr(self.image_encoder, "config", None), "projection_dim", clip_embeddings_dim)
        self.clip_hidden_size = getattr(getattr(self.image_encoder, "config", None), "hidden_size", clip_hidden_size)
        self.number_class_crossattention = (number_class_crossattention.to(self.device, dtype=dtype)
                                            if number_class_crossattention is not None else None)
        self.image_proj_model = self.init_proj()
        if ip_ckpt is not None:
            self.load_ip_adapter()

    def _g(self, module):
        """the conditioning module as a replayed hipGraph (modules.Graphed): get_image_embeds runs the 0.8 ms replay, not an eager pass
        of ~45 launches; CPU tensors (the host-logic tests) go straight through"""
        from .modules import Graphed
        cache = self.__dict__.setdefault("_graphed", {})
        w = cache.get(id(module))
        if w is None or w.module is not module:
            w = cache[id(module)] = Graphed(module)
        return w

    def init_proj(self):                                                  # ip_adapter.py:91-97
        return ImageProjModel(cross_attention_dim=self.pipe.unet.config.cross_attention_dim,
                              clip_embeddings_dim=self.clip_embeddings_dim,
                              clip_extra_context_tokens=self.num_tokens).to(self.device, dtype=self.dtype)

    def set_ip_adapter(self):                                             # ip_adapter.py:99-133
        install_ip_processors(self.pipe.unet, num_tokens=self.num_tokens, device=self.device, dtype=self.dtype)
        cn = getattr(self.pipe, "controlnet", None)                       # :126-133: text-only cross-attention there
        if cn is not None:
            for c in (getattr(cn, "nets", None) or [cn]):
                c.set_attn_processor(CNAttnProcessor2_0(num_tokens=self.num_tokens))

    def load_ip_adapter(self, state_dict=None):                           # ip_adapter.py:135-154
        if state_dict is None:
            from .checkpoint import load_ip_adapter_file
            state_dict = load_ip_adapter_file(self.ip_ckpt)
        self.image_proj_model.load_state_dict(state_dict["image_proj"])
        if self.number_class_crossattention is not None:
            self.number_class_crossattention.load_state_dict(state_dict["composed_adapter"])
        ip_layers = torch.nn.ModuleList(self.pipe.unet.attn_processors.values())     # keys '<idx>.to_k_ip.weight'
        ip_layers.load_state_dict(state_dict["ip_adapter"])

    def _clip_embeds(self, pil_image, clip_image_embeds):
        if pil_image is not None:
            if self.image_encoder is None or self.clip_image_processor is None:
                raise NotImplementedError("the CLIP image encoder is the step before the hot path (SURVEY.md 8f-4): "
                                          "pass clip_image_embeds or construct with image_encoder_path")
            imgs = pil_image if isinstance(pil_image, (list, tuple)) else [pil_image]
            px = self.clip_image_processor(images=imgs, return_tensors="pt").pixel_values
            return self.image_encoder(px.to(self.device, dtype=self.dtype)).image_embeds
        return clip_image_embeds.to(self.device, dtype=self.dtype)

    @torch.inference_mode()
    def fused_clip_embeds(self, pil_image=None, clip_image_embeds=None, extra_prompt_embeds=None):
        """CLIP image embedding with the harmony-aware correction added: ``clip + HA(text, clip)`` (ip_adapter.py:163-173).
        Also the target the default PNS judge scores previews against (imagharmony_amd.pns.ClipPreferenceJudge)."""
        clip_image_embeds = self._clip_embeds(pil_image, clip_image_embeds)
        if extra_prompt_embeds is not None and self.number_class_crossattention is not None:
            extra = extra_prompt_embeds.to(self.device, self.dtype)
            clip_image_embeds = clip_image_embeds + self._g(self.number_class_crossattention)(extra, clip_image_embeds)   # :170-173
        return clip_image_embeds

    @torch.inference_mode()
    def get_image_embeds(self, pil_image=None, clip_image_embeds=None, extra_prompt_embeds=None):   # ip_adapter.py:158-177
        clip_image_embeds = self.fused_clip_embeds(pil_image, clip_image_embeds, extra_prompt_embeds)
        image_prompt_embeds = self._g(self.image_proj_model)(clip_image_embeds)
        uncond_image_prompt_embeds = self._g(self.image_proj_model)(torch.zeros_like(clip_image_embeds))
        return image_prompt_embeds, uncond_image_prompt_embeds

    def _hidden_states(self, pil_image, instead):
        """the Plus variants' input: the penultimate CLIP hidden states [B, 257, hidden] of the images and of an all-zero image"""
        if self.image_encoder is None or self.clip_image_processor is None:
            raise NotImplementedError(f"CLIP image encoder not attached: pass {instead}")
        imgs = pil_image if isinstance(pil_image, (list, tuple)) else [pil_image]
        px = self.clip_image_processor(images=imgs, return_tensors="pt").pixel_values.to(self.device, dtype=self.dtype)
        return (self.image_encoder(px, output_hidden_states=True).hidden_states[-2],
                self.image_encoder(torch.zeros_like(px), output_hidden_states=True).hidden_states[-2])

    def set_scale(self, scale):                                           # ip_adapter.py:179-182
        set_scale(self.pipe.unet, scale)

    def generate(self, pil_image=None, clip_image_embeds=None, prompt=None, negative_prompt=None, scale=1.0,
                 num_samples=4, seed=None, guidance_scale=7.5, num_inference_steps=30, prompt_embeds=None, **kwargs):
        """Base (SD-1.x style) generate, ip_adapter.py:184-247: the pipe's ``encode_prompt`` returns (cond, uncond)
        and the pipe takes no pooled embeddings.  ``prompt_embeds`` = that 2-tuple when no text encoder is attached."""
        self.set_scale(scale)
        if pil_image is not None:
            n = len(pil_image) if isinstance(pil_image, (list, tuple)) else 1
        else:
            n = clip_image_embeds.size(0)
        prompt, negative_prompt = _prompts(prompt, negative_prompt, n)
        extra = {k: kwargs.pop(k) for k in ("uncond_clip_image_embeds",) if k in kwargs}   # IPAdapterPlus / Full, no CLIP attached
        ipe, uipe = self.get_image_embeds(pil_image=pil_image, clip_image_embeds=clip_image_embeds, **extra)
        bs, seq_len, _ = ipe.shape
        tile = lambda t: t.repeat(1, num_samples, 1).view(bs * num_samples, seq_len, -1)        # :216-220
        ipe, uipe = tile(ipe), tile(uipe)
        if prompt_embeds is None:
            prompt_embeds = self.pipe.encode_prompt(prompt, device=self.device, num_images_per_prompt=num_samples,
                                                    do_classifier_free_guidance=True, negative_prompt=negative_prompt)
        pe, ne = prompt_embeds[0], prompt_embeds[1]
        pe = torch.cat([pe.to(ipe.device, self.dtype), ipe], dim=1)                             # :230-231
        ne = torch.cat([ne.to(ipe.device, self.dtype), uipe], dim=1)
        self.generator = get_generator(seed, kwargs.pop("generator_device", "cpu"))
        return self.pipe(prompt_embeds=pe, negative_prompt_embeds=ne, guidance_scale=guidance_scale,
                         num_inference_steps=num_inference_steps, generator=self.generator, **kwargs).images

    # shared tail of the generate() variants
    def _run(self, image_prompt_embeds, uncond_image_prompt_embeds, prompt, negative_prompt, num_samples, seed,
             num_inference_steps, embeds, kwargs):
        bs, seq_len, _ = image_prompt_embeds.shape
        tile = lambda t: t.repeat(1, num_samples, 1).view(bs * num_samples, seq_len, -1)        # ip_adapter.py:302-306
        image_prompt_embeds, uncond_image_prompt_embeds = tile(image_prompt_embeds), tile(uncond_image_prompt_embeds)
        if embeds is None:
            embeds = self.pipe.encode_prompt(prompt, num_images_per_prompt=num_samples, do_classifier_free_guidance=True,
                                             negative_prompt=negative_prompt)
        pe, ne, ppe, npe = embeds
        dev = image_prompt_embeds.device
        pe = torch.cat([pe.to(dev, self.dtype), image_prompt_embeds], dim=1)                    # :321-322
        ne = torch.cat([ne.to(dev, self.dtype), uncond_image_prompt_embeds], dim=1)
        self.generator = get_generator(seed, kwargs.pop("generator_device", "cpu"))
        return self.pipe(prompt_embeds=pe, negative_prompt_embeds=ne, pooled_prompt_embeds=ppe,
                         negative_pooled_prompt_embeds=npe, num_inference_steps=num_inference_steps,
                         generator=self.generator, **kwargs).images


class IPAdapterXL(IPAdapter):
    """ip_adapter.py:249-340."""

    def __init__(self, sd_pipe, image_encoder_path, ip_ckpt, device, num_tokens=4, target_blocks=None, inference=False,
                 number_class_crossattention=None, **kw):
        self.inference = inference
        super().__init__(sd_pipe, image_encoder_path, ip_ckpt, device, num_tokens=num_tokens, target_blocks=target_blocks,
                         number_class_crossattention=number_class_crossattention, **kw)

    def generate(self, pil_image=None, prompt=None, negative_prompt=None, extra_text=None, scale=1.0, num_samples=4,
                 seed=None, num_inference_steps=30, clip_image_embeds=None, prompt_embeds=None, extra_prompt_embeds=None,
                 **kwargs):
        """Same arguments as the reference; additionally ``clip_image_embeds`` / ``prompt_embeds`` (a 4-tuple as
        returned by encode_prompt) / ``extra_prompt_embeds`` may be given when no encoders are attached."""
        self.set_scale(scale)
        # a stray number_class_crossattention= (test.py:38) travels on to the pipeline inside **kwargs, as upstream;
        # StableDiffusionXLCustomPipeline.__call__ here ignores unknown keywords like diffusers' stock pipeline does
        if pil_image is None and clip_image_embeds is not None:     # pre-computed CLIP embeddings carry the batch
            n = clip_image_embeds.size(0)
        else:
            n = 1 if not isinstance(pil_image, (list, tuple)) else len(pil_image)
        prompt, negative_prompt = _prompts(prompt, negative_prompt, n)
        if extra_prompt_embeds is None and extra_text is not None:      # ip_adapter.py:285-297 (NameError upstream if None)
            extra_prompt_embeds = self.pipe.encode_prompt(extra_text, num_images_per_prompt=num_samples,
                                                          do_classifier_free_guidance=True,
                                                          negative_prompt=negative_prompt)[0]
        ipe, uipe = self.get_image_embeds(pil_image=pil_image, clip_image_embeds=clip_image_embeds,
                                          extra_prompt_embeds=extra_prompt_embeds)
        return self._run(ipe, uipe, prompt, negative_prompt, num_samples, seed, num_inference_steps, prompt_embeds, kwargs)


    def generate_regions(self, regions, prompt=None, negative_prompt=None, scale=1.0, num_samples=4, seed=None,
                         num_inference_steps=30, prompt_embeds=None, **kwargs):
        """Several image prompts for one picture, each where its mask says ("this reference for the left half, that one for the
        right"): diffusers' ``ip_adapter_masks`` with several images per adapter.  regions: a list of dicts with
        ``pil_image`` or ``clip_image_embeds`` ([1, D]), ``mask`` (PIL, or a tensor [height, width]; white = here), ``weight`` (default
        1.0) and optionally ``extra_text`` or ``extra_prompt_embeds`` -- each region goes through get_image_embeds, with its own
        HarmonyAttention correction.  The image tokens are concatenated [text | r0 | r1 | ...], the unconditional ones the same way, and
        reach the pipe with ``ip_region_masks= / ip_region_weights=``; height / width (kwargs) are the pipe's defaults unless given.
        ``binarize=False`` (kwargs) keeps soft masks.  The text-to-image, image-to-image and inpainting pipes take regions; the
        ControlNet and adapter pipes refuse them.  Afterwards the pipe is as it was: a plain ``generate`` sees one image prompt."""
        regions = list(regions)
        if not regions or not all(isinstance(r, dict) and r.get("mask") is not None for r in regions):
            raise ValueError("generate_regions takes a list of dicts, each with `mask` and `pil_image` or `clip_image_embeds`")
        self.set_scale(scale)
        prompt, negative_prompt = _prompts(prompt, negative_prompt, 1)
        ipes, uipes = [], []
        for r in regions:
            extra = r.get("extra_prompt_embeds")
            if extra is None and r.get("extra_text") is not None:
                extra = self.pipe.encode_prompt(r["extra_text"], num_images_per_prompt=num_samples, do_classifier_free_guidance=True,
                                                negative_prompt=negative_prompt)[0]
            ipe, uipe = self.get_image_embeds(pil_image=r.get("pil_image"), clip_image_embeds=r.get("clip_image_embeds"),
                                              extra_prompt_embeds=extra)
            if ipe.shape[0] != 1:
                raise ValueError(f"a region carries one image, got a batch of {ipe.shape[0]}")
            ipes.append(ipe)
            uipes.append(uipe)
        kwargs = dict(kwargs, ip_region_masks=[r["mask"] for r in regions], ip_region_weights=[float(r.get("weight", 1.0)) for r in regions])
        return self._run(torch.cat(ipes, 1), torch.cat(uipes, 1), prompt, negative_prompt, num_samples, seed, num_inference_steps,
                         prompt_embeds, kwargs)

    @torch.no_grad()
    def generate_pns(self, seeds, pil_image=None, prompt=None, negative_prompt=None, extra_text=None, scale=1.0,
                     preview_steps=10, num_inference_steps=30, guidance_scale=5.0, scorer=None, batch=None,
                     clip_image_embeds=None, prompt_embeds=None, extra_prompt_embeds=None, height=None, width=None,
                     output_type="pil", step_noise="global", image=None, mask_image=None, strength=None, judge_preprocess="torch",
                     control_image=None, controlnet_conditioning_scale=1.0, adapter_image=None, adapter_conditioning_scale=1.0,
                     adapter_conditioning_factor=1.0, preview_vae=None, **schedule_kw):
        """Preference-guided noise selection (README.md:27, assets/1.png) around ``generate``: every candidate seed gets
        a ``preview_steps`` denoise, a judge scores the previews, the best NOISE gets the full ``num_inference_steps``
        denoise.  Candidates are sharded over the ranks of an initialised torch.distributed group (one process per
        GPU; no per-step collective).  ``scorer`` (latents [S,4,h,w] -> [S]) defaults to the CLIP-space judge when a
        VAE and a CLIP vision model are attached, else to the latent statistic of ``pns.default_scorer``.
        ``batch`` = preview candidates stacked per UNet forward on a rank; None (default) = as many as the rank holds, up
        to 4 (BASELINE.json configs[4] runs 4 per GPU): a stacked forward costs 1.27x less per candidate than one at a
        time on MI355X (bench.py ``stacked_candidates`` / ``pns_two_stage``); the final denoise is batch 1 either way.
        Under a stochastic scheduler on the pipe (SDE-DPM-Solver++, Euler ancestral) ``step_noise`` chooses the per-step noise of the
        previews and the final denoise (pns.two_stage_fns has the details): "global" (default) takes it from torch's global generator, so a
        seed fixes the initial noise only; "seed" generates it on the device from each candidate's own seed (lane 0), so a seed fixes
        its whole trajectory, stacked or alone, on any rank.
        ``judge_preprocess``: how the default CLIP judge gets from decoded previews to the encoder's input -- "torch" (default): the chain
        of torch ops of ``pns.ClipPreferenceJudge.preprocess``; "hip": one imh_clip_preprocess launch straight into the HIP vision tower's
        patch buffer (``CLIPVisionEncoder.embed_decoded``); it needs ``image_encoder_backend="hip"`` (ValueError before any GPU work).
        On an image-to-image or inpainting pipe the candidates are EDITS of ``image`` (and, inpainting, ``mask_image``; white = repaint) at
        ``strength`` (default: the pipe's own, 0.3 / 0.9999): the image -- and, for a 9-channel UNet, the masked image -- is encoded once,
        and for candidate seed s every draw comes from ``torch.Generator("cpu").manual_seed(s)`` in the pipe's order (posterior noise of
        the image, add-noise noise, 9 channels: posterior noise of the masked image; pns.edit_draws).  The winner's latents are therefore the
        bits of ``pipe(image=, [mask_image=,] strength=, num_inference_steps=num_inference_steps, generator=[that generator],
        output_type="latent")`` -- with ``step_noise="seed"`` under a stochastic scheduler, of that call with ``step_noise="seeded"``.
        height / width follow the image there.
        On a pipe with a ControlNet (``pipe.controlnet``: the text-to-image, image-to-image and inpainting ControlNet pipelines)
        ``control_image`` is required -- on the text-to-image one too, where ``image=`` stays refused -- and steers every candidate at
        ``controlnet_conditioning_scale``: it is prepared at the call's height / width and set on the engine once per call, one image for
        every stacked candidate; the ControlNet's window travels in ``controlnet_guidance_start / controlnet_guidance_end``.  A ControlNet
        makes no draws, so the contract above holds with ``control_image=`` (and the scale and window) added to the pipe's call.  On a
        pipe without a ControlNet ``control_image`` is refused (ValueError).
        On a pipe with a T2I-Adapter (``pipe.adapter``: StableDiffusionXLAdapterCustomPipeline) ``adapter_image`` is required (``image=`` stays
        refused) and steers the previews and the final denoise at ``adapter_conditioning_scale`` / ``adapter_conditioning_factor`` (counted
        per stage): one control image serves every candidate, its features are computed once per call.  An adapter makes no draws, so the
        winner's latents are the bits of the pipe's own call with ``image=adapter_image``, the scale and the factor, and that seed's
        generator.  On a pipe without an adapter ``adapter_image`` is refused (ValueError).
        ``preview_vae`` (default None: ``pipe.vae``): the VAE whose ``decode`` the default CLIP judge sees the previews through -- an
        ``AutoencoderTiny`` decodes a preview in 35 small launches; its fp32 NCHW image is what either ``judge_preprocess`` takes.  The
        winner's image still comes from ``pipe.vae``; a custom ``scorer`` never sees it.
        Returns dict(images, best_seed, scores, latents)."""
        from . import pns
        from .pipeline import (StableDiffusionXLImg2ImgCustomPipeline, StableDiffusionXLInpaintCustomPipeline, _ControlNetPipe,
                               check_controlnet_args, decode_output, edit_moments, prepare_control_image)
        seeds = list(seeds)                       # consumed more than once below: a generator passed as `seeds` must survive that
        if schedule_kw.get("pag_scale") or schedule_kw.get("pag_adaptive_scale"):
            raise NotImplementedError("perturbed-attention guidance (pag_scale=) is not built for generate_pns: use generate")
        if judge_preprocess not in ("torch", "hip"):
            raise ValueError(f"judge_preprocess={judge_preprocess!r}: 'torch' or 'hip'")
        if judge_preprocess == "hip" and not hasattr(self.image_encoder, "embed_decoded"):
            raise ValueError('judge_preprocess="hip" needs the HIP CLIP vision tower as the image encoder '
                             '(image_encoder_backend="hip" / image_encoder=CLIPVisionEncoder)')
        pipe = self.pipe
        controlnet = pipe.controlnet if isinstance(pipe, _ControlNetPipe) else None          # (the three classes that carry .controlnet)
        if controlnet is None and control_image is not None:
            raise ValueError("control_image= belongs to a ControlNet pipeline: this pipe has no .controlnet")
        if controlnet is not None:
            check_controlnet_args(control_image, "control_image", controlnet_conditioning_scale, schedule_kw.pop("guess_mode", False),
                                  schedule_kw.get("controlnet_guidance_start", 0.0), schedule_kw.get("controlnet_guidance_end", 1.0))
        t2i = getattr(pipe, "adapter", None)
        if t2i is None and adapter_image is not None:
            raise ValueError("adapter_image= belongs to a T2I-Adapter pipeline: this pipe has no .adapter")
        if t2i is not None:
            from .pipeline import check_adapter_args, prepare_adapter_image
            if adapter_image is None:
                raise ValueError("PNS on a T2I-Adapter pipe needs adapter_image= (the control image)")
            check_adapter_args(adapter_image, adapter_conditioning_scale, adapter_conditioning_factor)
            ad_img = prepare_adapter_image(adapter_image)
            if ad_img.dim() != 4 or ad_img.shape[0] != 1:
                raise ValueError(f"PNS runs its candidates under one adapter image, got {tuple(ad_img.shape)}")
            height, width = height or int(ad_img.shape[2]), width or int(ad_img.shape[3])
            t2i.check_image(ad_img, height, width)
            schedule_kw["adapter_conditioning_factor"] = float(adapter_conditioning_factor)
        inpaint = isinstance(pipe, StableDiffusionXLInpaintCustomPipeline)
        edit = inpaint or isinstance(pipe, StableDiffusionXLImg2ImgCustomPipeline)
        if edit:
            img, mask, strength = self._pns_edit_inputs(image, mask_image, strength, preview_steps, num_inference_steps, output_type, step_noise)
            height, width = int(img.shape[2]), int(img.shape[3])
        else:
            if image is not None or mask_image is not None or strength is not None:
                raise ValueError("image= / mask_image= / strength= belong to an image-to-image or inpainting pipeline")
            if output_type != "latent" and pipe.vae is None and pipe.vae_decode is None:
                raise NotImplementedError("output_type=%r needs a VAE on the pipeline; pass output_type='latent'" % (output_type,))
            height = height or pipe.default_sample_size * pipe.vae_scale_factor
            width = width or pipe.default_sample_size * pipe.vae_scale_factor
        h, w = height // 8, width // 8
        control = prepare_control_image(control_image, height, width) if controlnet is not None else None
        if control is not None and control.shape[0] != 1:
            raise ValueError(f"PNS runs its candidates under one control image, got a batch of {control.shape[0]}")
        fused, cond = self._pns_setup(scale, pil_image, clip_image_embeds, prompt, negative_prompt, extra_text, prompt_embeds, extra_prompt_embeds)
        S = max(1, int(_default_batch(len(seeds)) if batch is None else batch))
        eng = pipe.engine
        if controlnet is not None:
            eng.set_controlnet(controlnet)
        if t2i is not None:
            eng.set_adapter(t2i)
        if edit:
            # everything a candidate shares is computed once, the moments at batch 1 as the pipelines encode a per-sample-generator call;
            # a candidate costs its draws, one fused initial-latents launch (stacked ``batch`` per call) and the truncated denoise
            from .vae import latent_mask
            concat = inpaint and pipe.unet.config.in_channels == 9
            moments, masked_moments = edit_moments(pipe.vae, img, True, 9 if concat else 4, float(strength) == 1.0, mask)
            prepare = pns.edit_prepare_fn(eng, pipe.scheduler, pipe.vae.config.scaling_factor, moments, h, w, strength,
                                          mask=latent_mask(mask, h, w) if inpaint else None, masked_moments=masked_moments, concat=concat)
            stages = pns.edit_two_stage_fns(eng, pipe.scheduler, prepare, strength, preview_steps, num_inference_steps,
                                            step_noise=step_noise, inpaint=inpaint, **schedule_kw)
        else:
            stages = pns.two_stage_fns(eng, pipe.scheduler, preview_steps, num_inference_steps, step_noise=step_noise, **schedule_kw)
        if scorer is None:
            scorer = self._default_scorer(pipe.vae if preview_vae is None else preview_vae, fused, judge_preprocess)
        state = {"n": None}

        def stacked(stage):
            """the stage function behind a re-conditioning whenever the stack size changes"""
            def fn(noise, **kw):
                n = noise.shape[0]
                if state["n"] != n:
                    eng.set_conditioning(*(t.repeat(*([n] + [1] * (t.ndim - 1))) for t in cond), height, width, guidance_scale=guidance_scale)
                    if control is not None and state["n"] is None:
                        # once per call, behind the first conditioning; later re-conditionings prepare the hint and the ControlNet's
                        # caches again for their stack size themselves (DenoiseEngine.set_conditioning -> _prepare_control)
                        eng.set_control_image(control, conditioning_scale=float(controlnet_conditioning_scale))
                    if t2i is not None:
                        # the same image at every re-conditioning: the features are computed at the first and kept (set_adapter_image)
                        eng.set_adapter_image(ad_img, conditioning_scale=float(adapter_conditioning_scale))
                    state["n"] = n
                return stage(noise, **kw)
            return fn

        r = pns.run_pns(stacked(stages[0]), seeds, (1, 4, h, w), scorer=scorer, device=self.device, final_fn=stacked(stages[1]), batch=S,
                        pass_seeds=edit or step_noise == "seed")
        out = decode_output(pipe.vae, pipe.vae_decode, r["latents"], output_type)
        return dict(images=out, best_seed=r["best_seed"], scores=r["scores"], latents=r["latents"])

    def _pns_setup(self, scale, pil_image, clip_image_embeds, prompt, negative_prompt, extra_text, prompt_embeds, extra_prompt_embeds):
        """what the candidates of a generate_pns call share -> (the fused CLIP embedding the default judge scores against, the conditioning
        of one sample (pe, ne, ppe, npe) with the image tokens appended)"""
        self.set_scale(scale)
        pipe = self.pipe
        prompt, negative_prompt = _prompts(prompt, negative_prompt)
        if extra_prompt_embeds is None and extra_text is not None:
            extra_prompt_embeds = pipe.encode_prompt(extra_text, num_images_per_prompt=1, do_classifier_free_guidance=True,
                                                     negative_prompt=negative_prompt)[0]
        fused = self.fused_clip_embeds(pil_image, clip_image_embeds, extra_prompt_embeds)
        ipe = self._g(self.image_proj_model)(fused)
        uipe = self._g(self.image_proj_model)(torch.zeros_like(fused))
        if prompt_embeds is None:
            prompt_embeds = pipe.encode_prompt(prompt, num_images_per_prompt=1, do_classifier_free_guidance=True,
                                               negative_prompt=negative_prompt)
        pe, ne, ppe, npe = prompt_embeds
        pe = torch.cat([pe.to(ipe.device, self.dtype), ipe], dim=1)
        ne = torch.cat([ne.to(ipe.device, self.dtype), uipe], dim=1)
        return fused, (pe, ne, ppe.to(ipe.device), npe.to(ipe.device))

    def _default_scorer(self, vae, fused, judge_preprocess):
        """the CLIP-space judge when a VAE and a CLIP vision model are attached, else the latent statistic"""
        from . import pns
        if vae is None or self.image_encoder is None:
            return pns.default_scorer
        from .vae import decode_latents
        return pns.ClipPreferenceJudge(lambda z: decode_latents(vae, z), self.image_encoder, fused,
                                       **({"preprocess_backend": "hip"} if judge_preprocess == "hip" else {}))

    def _pns_edit_inputs(self, image, mask_image, strength, preview_steps, num_inference_steps, output_type, step_noise):
        """generate_pns on an image-to-image / inpainting pipe (its docstring states the contract): the refusals, all before any GPU work
        -> (the preprocessed image [1, 3, H, W], the mask [1, 1, H, W] or None, the strength)"""
        from .pipeline import StableDiffusionXLInpaintCustomPipeline
        from .schedulers import get_timesteps
        from .vae import preprocess, preprocess_mask
        pipe = self.pipe
        inpaint = isinstance(pipe, StableDiffusionXLInpaintCustomPipeline)
        if step_noise not in ("global", "seed"):
            raise ValueError(f'step_noise must be "global" or "seed", not {step_noise!r}')
        if image is None:
            raise NotImplementedError("generate_pns on an image-to-image / inpainting pipe selects among EDITS of image= (PIL or a tensor "
                                      "[1, 3, H, W]); text-to-image schedules on such a pipe are not supported")
        if inpaint and mask_image is None:
            raise ValueError("PNS on an inpainting pipe needs mask_image= (white = repaint)")
        if not inpaint and mask_image is not None:
            raise ValueError("mask_image= belongs to an inpainting pipeline")
        if strength is None:
            strength = 0.9999 if inpaint else 0.3
        if not 0.0 <= float(strength) <= 1.0:
            raise ValueError(f"strength must be in [0.0, 1.0], got {strength}")
        if output_type != "latent" and pipe.vae is None and pipe.vae_decode is None:
            raise NotImplementedError("output_type=%r needs a VAE on the pipeline; pass output_type='latent'" % (output_type,))
        if getattr(pipe.vae, "tiny", False):
            pipe.vae.encode()                                    # AutoencoderTiny: its encoder's NotImplementedError
        if pipe.vae is None or not getattr(pipe.vae, "with_encoder", False):
            raise NotImplementedError("an edit needs a VAE with its encoder: vae=AutoencoderKL(config, with_encoder=True)")
        for steps in (preview_steps, num_inference_steps):
            pipe.scheduler.set_timesteps(steps)
            get_timesteps(pipe.scheduler, steps, strength)       # a stage that truncates to no step: the pipelines' ValueError
        img = preprocess(image)
        if img.shape[0] != 1:
            raise ValueError(f"PNS edits one image (the candidates are its seeds), got a batch of {img.shape[0]}")
        mask = None
        if inpaint:
            mask = preprocess_mask(mask_image, int(img.shape[2]), int(img.shape[3]))
            if mask.shape[0] != 1:
                raise ValueError(f"PNS edits one image under one mask, got a mask batch of {mask.shape[0]}")
        return img, mask, strength


class IPAdapterPlus(IPAdapter):
    """ip_adapter.py:344-374: Resampler (12 heads, width = the UNet's cross-attention dim) over the penultimate CLIP
    hidden states; base ``generate``."""

    def init_proj(self):                                                  # ip_adapter.py:347-360
        cd = self.pipe.unet.config.cross_attention_dim
        return Resampler(dim=cd, depth=4, dim_head=64, heads=12, num_queries=self.num_tokens,
                         embedding_dim=self.clip_hidden_size, output_dim=cd, ff_mult=4).to(self.device, dtype=self.dtype)

    @torch.inference_mode()
    def get_image_embeds(self, pil_image=None, clip_image_embeds=None, uncond_clip_image_embeds=None):      # :362-374
        """clip_image_embeds here = penultimate hidden states [B, 257, hidden] (as upstream names them); without an
        attached CLIP model pass them together with ``uncond_clip_image_embeds`` (hidden states of a zero image)."""
        if pil_image is not None:
            clip_image_embeds, uncond_clip_image_embeds = self._hidden_states(pil_image, "clip_image_embeds (hidden states)")
        if uncond_clip_image_embeds is None:
            raise NotImplementedError("pass uncond_clip_image_embeds (CLIP hidden states of an all-zero image)")
        c = clip_image_embeds.to(self.device, self.dtype)
        u = uncond_clip_image_embeds.to(self.device, self.dtype)
        return self._g(self.image_proj_model)(c), self._g(self.image_proj_model)(u)


class IPAdapterFull(IPAdapterPlus):
    """ip_adapter.py:377-386: every hidden-state token through the MLP projection."""

    def init_proj(self):
        return MLPProjModel(cross_attention_dim=self.pipe.unet.config.cross_attention_dim,
                            clip_embeddings_dim=self.clip_hidden_size).to(self.device, dtype=self.dtype)


class IPAdapterPlusXL(IPAdapter):
    """ip_adapter.py:389-478: Resampler over the penultimate CLIP hidden states."""

    def init_proj(self):                                                  # ip_adapter.py:391-403
        return Resampler(dim=1280, depth=4, dim_head=64, heads=20, num_queries=self.num_tokens,
                         embedding_dim=self.clip_hidden_size, output_dim=self.pipe.unet.config.cross_attention_dim,
                         ff_mult=4).to(self.device, dtype=self.dtype)

    @torch.inference_mode()
    def get_image_embeds(self, pil_image=None, clip_hidden_states=None, uncond_clip_hidden_states=None):   # :405-417
        if pil_image is not None:
            clip_hidden_states, uncond_clip_hidden_states = self._hidden_states(pil_image, "clip_hidden_states")
        c = clip_hidden_states.to(self.device, self.dtype)
        u = uncond_clip_hidden_states.to(self.device, self.dtype)
        return self._g(self.image_proj_model)(c), self._g(self.image_proj_model)(u)

    def generate(self, pil_image=None, prompt=None, negative_prompt=None, scale=1.0, num_samples=4, seed=None,
                 num_inference_steps=30, clip_hidden_states=None, uncond_clip_hidden_states=None, prompt_embeds=None,
                 **kwargs):
        self.set_scale(scale)
        if pil_image is None and clip_hidden_states is not None:
            n = clip_hidden_states.size(0)
        else:
            n = 1 if not isinstance(pil_image, (list, tuple)) else len(pil_image)
        prompt, negative_prompt = _prompts(prompt, negative_prompt, n)
        ipe, uipe = self.get_image_embeds(pil_image, clip_hidden_states, uncond_clip_hidden_states)
        return self._run(ipe, uipe, prompt, negative_prompt, num_samples, seed, num_inference_steps, prompt_embeds, kwargs)
