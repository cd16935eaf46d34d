"""imagharmony_amd -- the MI355X-native (gfx950) SDXL denoising hot path of IMAGHarmony.

Host code is Python on PyTorch-ROCm (device memory, streams, torch.distributed only); the
arithmetic runs in hand-written HIP kernels behind the C ABI of ``libimh_hip.so`` (include/imh.h).
"""
__version__ = "0.1.0"

# the reference package's exports (ip_adapter/__init__.py:1-11), resolved lazily so that importing the package
# does not import torch
__all__ = ["IPAdapter", "IPAdapterPlus", "IPAdapterPlusXL", "IPAdapterXL", "IPAdapterFull"]
# the CLIP vision tower on the HIP path (clip_vision.py), lazily as well
_CLIP = ("CLIPVisionEncoder", "CLIPVisionEncoderConfig")
# ... and the CLIP text towers (clip_text.py)
_CLIP_TEXT = ("CLIPTextEncoder", "CLIPTextEncoderConfig")


# the pipelines, lazily too: text-to-image (custom_pipelines.py), image-to-image and inpainting (diffusers' SDXL img2img / inpaint call surfaces)
_PIPELINES = ("StableDiffusionXLCustomPipeline", "StableDiffusionXLImg2ImgCustomPipeline", "StableDiffusionXLInpaintCustomPipeline",
              "StableDiffusionXLControlNetCustomPipeline", "StableDiffusionXLControlNetImg2ImgCustomPipeline",
              "StableDiffusionXLControlNetInpaintCustomPipeline", "StableDiffusionXLAdapterCustomPipeline")
# the SDXL ControlNet (controlnet.py): the model whose residuals the UNet forward adds to its skips
_CONTROLNET = ("ControlNetModel",)
# the SDXL T2I-Adapter (t2i_adapter.py): the once-per-image net whose four features the UNet's down path adds
_T2I_ADAPTER = ("T2IAdapter",)
# diffusers' AutoencoderTiny decoder (tiny_vae.py): the preview VAE of generate_pns(preview_vae=), or a pipeline's vae=
_TINY_VAE = ("AutoencoderTiny", "TinyVAEConfig")
# regional image prompts (regions.py): N masks over the picture and N weights for IPAdapterXL.generate_regions / ip_region_masks=
_REGIONS = ("IPRegions",)
# the schedulers of the device-resident loop (schedulers.py): the two linear ones and the multistep / ancestral ones
_SCHEDULERS = ("DDIMScheduler", "EulerDiscreteScheduler", "DPMSolverMultistepScheduler", "EulerAncestralDiscreteScheduler")
# the seeded step noise restated in numpy (noise.py): seeded_randn / seed_rows, the yardstick of the device generator
_NOISE = ("seeded_randn", "seed_rows")
# the CLIP judge's preprocessing restated in numpy (imageops.py): the yardstick of imh_clip_preprocess
_IMAGEOPS = ("clip_preprocess_reference", "clip_geometry")


def __getattr__(name):
    if name in __all__:
        from . import ip_adapter
        return getattr(ip_adapter, name)
    if name in _CLIP:
        from . import clip_vision
        return getattr(clip_vision, name)
    if name in _CLIP_TEXT:
        from . import clip_text
        return getattr(clip_text, name)
    if name in _PIPELINES:
        from . import pipeline
        return getattr(pipeline, name)
    if name in _CONTROLNET:
        from . import controlnet
        return getattr(controlnet, name)
    if name in _T2I_ADAPTER:
        from . import t2i_adapter
        return getattr(t2i_adapter, name)
    if name in _TINY_VAE:
        from . import tiny_vae
        return getattr(tiny_vae, name)
    if name in _REGIONS:
        from . import regions
        return getattr(regions, name)
    if name in _SCHEDULERS:
        from . import schedulers
        return getattr(schedulers, name)
    if name in _NOISE:
        from . import noise
        return getattr(noise, name)
    if name in _IMAGEOPS:
        from . import imageops
        return getattr(imageops, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
