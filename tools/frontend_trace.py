"""CPU only, no library: the call trace of the host front end -- every engine, scheduler and VAE-encoder call the pipelines'
``__call__`` and ``IPAdapterXL.generate_pns`` make, in order, with their arguments -- on recording fakes.

    python tools/frontend_trace.py [out.json]

Tensors are logged as shape + SHA-1 of their fp32 bytes, scalars as they are, other objects by type name.  The fakes compute with
element-wise fp32 arithmetic only (no reduction, no matmul), so the hashes depend on the front end's draws and on nothing else.
``tests/golden/frontend_trace.json`` is this tool's output at the commit before the pipelines shared one call skeleton;
``tests/test_frontend_trace_host.py`` compares case by case.

Cases: {text-to-image, image-to-image, 4-channel inpainting at strength 0.5, 9-channel inpainting at strength 1.0, ControlNet} x {one
generator, a list} x step_noise {"generator", "seeded"} on S = 2, 64 x 64, 6 steps of Euler ancestral, output_type="latent"; and
generate_pns (5 seeds, batch 2, an explicit scorer) over text-to-image, image-to-image and 9-channel inpainting at strength 1.0, under
step_noise "global" and "seed".  Three more cases run one class's ``__call__`` on another class's pipe: text-to-image on an image-to-image
and on an inpainting pipe, image-to-image on an inpainting pipe.  A ``__call__`` is the call of the class that defines it."""
import hashlib
import json
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imagharmony_amd import pipeline as P                                     # noqa: E402
from imagharmony_amd.ip_adapter import IPAdapterXL                            # noqa: E402
from imagharmony_amd.schedulers import EulerAncestralDiscreteScheduler       # noqa: E402

S, SIDE, STEPS = 2, 64, 6


def enc(v):
    """a logged value: JSON scalars as they are, tensors as [shape, sha1 of the fp32 bytes], containers element-wise, the rest by type"""
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    if torch.is_tensor(v):
        return ["tensor", list(v.shape), hashlib.sha1(v.detach().to("cpu", torch.float32).contiguous().numpy().tobytes()).hexdigest()]
    if isinstance(v, (list, tuple)):
        return [enc(x) for x in v]
    if isinstance(v, dict):
        return {str(k): enc(x) for k, x in sorted(v.items())}
    return type(v).__name__


def ramp(*shape, mod=17, scale=1.0 / 16, shift=0):
    """a deterministic tensor of exact fp32 values"""
    n = 1
    for s in shape:
        n *= s
    return (((torch.arange(n) + shift) % mod).float() * scale).reshape(shape)


class RecEngine:
    """logs every method call; ``seeded`` follows set_schedule as on the engine (a stochastic scheduler here); prepare_* and denoise compute
    a per-sample element-wise function of what they are given, so that a PNS score tells the candidates apart"""

    def __init__(self, log):
        self.log, self.seeded, self.lat, self.steps, self.t_start = log, False, None, 0, 0

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)

        def call(*a, **k):
            self.log.append([name, enc(a), enc(k)])
            effect = getattr(type(self), "_" + name, None)
            return effect(self, *a, **k) if effect is not None else None
        return call

    def _set_schedule(self, scheduler, steps, *a, **kw):
        self.steps, self.t_start, self.seeded = int(steps), int(kw.get("t_start", 0)), bool(kw.get("seeded_noise"))

    @staticmethod
    def _rows(t, n):
        return t[torch.arange(n) % t.shape[0]]

    def _prepare_img2img(self, moments, n1, n2, scaling, a, b):
        n = n2.shape[0]
        self.lat = (self._rows(moments, n) + self._rows(n1, n)) * (a * scaling) + n2 * b

    def _prepare_inpaint(self, moments, n1, n2, scaling, a, b, mask, strength_max=False, masked_moments=None, n3=None):
        n = n2.shape[0]
        self.lat = n2.clone() if strength_max else (self._rows(moments, n) + self._rows(n1, n)) * (a * scaling) + n2 * b
        if n3 is not None:
            self.lat = self.lat + (self._rows(masked_moments, n) + self._rows(n3, n)) * 0.25

    def _denoise(self, latents, step_seeds=None, **kw):
        out = (self.lat if latents is None else latents.float()) * (0.5 + 0.125 * (self.steps - self.t_start))
        if step_seeds is not None:
            out = out + torch.tensor([float(int(s) % 7) for s in step_seeds]).view(-1, 1, 1, 1)
        return out


class RecVAE:
    with_encoder = True
    config = types.SimpleNamespace(scaling_factor=0.5)

    def __init__(self, log):
        self.log = log

    def encode_moments(self, x):
        self.log.append(["vae.encode_moments", enc((x,)), {}])
        z = x[:, :, ::8, ::8]
        return torch.cat([z, z[:, :1] * 0.5], 1).contiguous()


class RecScheduler(EulerAncestralDiscreteScheduler):
    log = None

    def set_timesteps(self, n, *a, **k):
        self.log.append(["scheduler.set_timesteps", enc((n,) + a), enc(k)])
        return super().set_timesteps(n, *a, **k)

    def add_noise_coefficients(self, t_start):
        self.log.append(["scheduler.add_noise_coefficients", enc((t_start,)), {}])
        return super().add_noise_coefficients(t_start)


def bare_pipe(cls, log, cin=4):
    pipe = cls.__new__(cls)
    pipe.unet = types.SimpleNamespace(config=types.SimpleNamespace(in_channels=cin, sample_size=SIDE // 8), attn_processors={})
    pipe.engine, pipe.vae, pipe.vae_decode, pipe.watermark, pipe.text_encoder = RecEngine(log), RecVAE(log), None, None, None
    pipe.scheduler = RecScheduler()
    pipe.scheduler.log = log
    pipe.default_sample_size = SIDE // 8
    pipe.controlnet = types.SimpleNamespace()
    return pipe


def image():
    return ramp(1, 3, SIDE, SIDE)


def mask():
    m = torch.zeros(1, 1, SIDE, SIDE)
    m[..., 16:48, 8:40] = 1.0
    return m


MODES = {
    "txt2img": (P.StableDiffusionXLCustomPipeline, 4, lambda: {}),
    "img2img": (P.StableDiffusionXLImg2ImgCustomPipeline, 4, lambda: dict(image=image(), strength=0.5)),
    "inpaint4_s0.5": (P.StableDiffusionXLInpaintCustomPipeline, 4, lambda: dict(image=image(), mask_image=mask(), strength=0.5)),
    "inpaint9_s1.0": (P.StableDiffusionXLInpaintCustomPipeline, 9, lambda: dict(image=image(), mask_image=mask(), strength=1.0)),
    "controlnet": (P.StableDiffusionXLControlNetCustomPipeline, 4,
                   lambda: dict(image=ramp(1, 3, SIDE, SIDE, mod=13, scale=1.0 / 16), controlnet_conditioning_scale=0.75,
                                controlnet_guidance_start=0.25, controlnet_guidance_end=0.75)),
}


def pipeline_case(mode, gen_list, step_noise, on=None):
    """on: the class of the pipe where it is not the mode's own -- a class's __call__ on another class's pipe (the GPU tests run
    text-to-image and image-to-image that way on image-to-image and inpainting pipes) is that class's call"""
    cls, cin, extra = MODES[mode]
    log = []
    pipe = bare_pipe(on or cls, log, cin)
    gen = [torch.Generator("cpu").manual_seed(100 + i) for i in range(S)] if gen_list else torch.Generator("cpu").manual_seed(7)
    out = cls.__call__(pipe, prompt_embeds=ramp(S, 5, 6), negative_prompt_embeds=ramp(S, 5, 6, shift=3),
                       pooled_prompt_embeds=ramp(S, 4, shift=5), negative_pooled_prompt_embeds=ramp(S, 4, shift=7),
                       num_inference_steps=STEPS, guidance_scale=4.0, generator=gen, output_type="latent", step_noise=step_noise,
                       guidance_rescale=0.25, denoising_end=None, **extra())
    log.append(["return", enc((out.images,)), {}])
    return log


PNS_MODES = {
    "txt2img": (P.StableDiffusionXLCustomPipeline, 4, lambda: dict(height=SIDE, width=SIDE)),
    "img2img": (P.StableDiffusionXLImg2ImgCustomPipeline, 4, lambda: dict(image=image(), strength=0.5)),
    "inpaint9_s1.0": (P.StableDiffusionXLInpaintCustomPipeline, 9, lambda: dict(image=image(), mask_image=mask(), strength=1.0)),
}


def pns_case(mode, step_noise):
    cls, cin, extra = PNS_MODES[mode]
    log = []
    ip = IPAdapterXL.__new__(IPAdapterXL)
    ip.pipe = bare_pipe(cls, log, cin)
    ip.device, ip.dtype, ip.image_encoder, ip.clip_image_processor, ip.number_class_crossattention = "cpu", torch.float32, None, None, None
    ip.image_proj_model = None
    ip._g = lambda m: (lambda x: (x * 0.5).view(x.shape[0], 2, 6))
    r = ip.generate_pns([11, 7, 3, 19, 5], clip_image_embeds=ramp(1, 12, shift=2),
                        prompt_embeds=(ramp(1, 5, 6), ramp(1, 5, 6, shift=3), ramp(1, 4, shift=5), ramp(1, 4, shift=7)),
                        preview_steps=4, num_inference_steps=STEPS, guidance_scale=4.0, batch=2, output_type="latent",
                        scorer=lambda lat: lat[:, 0, 0, 0] + lat[:, 1, 1, 1] * 0.5, step_noise=step_noise, **extra())
    log.append(["return", enc((r["best_seed"], r["scores"].tolist(), r["latents"], r["images"])), {}])
    return log


def cases():
    """{case name: a function that runs it and returns its log}"""
    out = {}
    for mode in MODES:
        for gen_list in (False, True):
            for step_noise in ("generator", "seeded"):
                name = f"pipe/{mode}/{'list' if gen_list else 'one'}/{step_noise}"
                out[name] = (lambda m=mode, g=gen_list, s=step_noise: pipeline_case(m, g, s))
    for mode, on in (("txt2img", "img2img"), ("txt2img", "inpaint9_s1.0"), ("img2img", "inpaint4_s0.5")):
        out[f"cross/{mode}/on/{on}"] = (lambda m=mode, o=on: pipeline_case(m, True, "seeded", on=MODES[o][0]))
    for mode in PNS_MODES:
        for step_noise in ("global", "seed"):
            out[f"pns/{mode}/{step_noise}"] = (lambda m=mode, s=step_noise: pns_case(m, s))
    return out


def trace():
    return {name: run() for name, run in cases().items()}


if __name__ == "__main__":
    text = json.dumps(trace(), indent=0, sort_keys=True) + "\n"
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
