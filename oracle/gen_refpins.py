"""Mint tests/golden/refpin_*.pt: what the reference's OWN code returns for the cases the CPU tests pin the oracle
and the host code against (verbatim import, oracle/refshim.py).  Needs the reference tree refshim reads:

    python -m oracle.gen_refpins

The tests read these fixtures and never import the reference themselves.  Inputs and weights are regenerated from
seeds (oracle.detfill) and the test doubles below, so a fixture holds the reference's outputs -- plus, where the
reference writes or reads a file, that file's contents (a converted checkpoint) or the digests of its tensors (an
ip_adapter.bin and the weights loaded from it).

  refpin_convert_bin.pt    convert_bin.py's regrouping of fake_training_checkpoint()
  refpin_denoise_loop.pt   the final latents of custom_pipelines.py's __call__ for every LOOP_CASES entry
  refpin_state_dicts.pt    parameter names / shapes of four reference modules and two of their outputs
  refpin_legacy_attn.npz   the torch<2 processors (attention_processor.py:60-241) on two golden attention cases: their
                           outputs as float32 differences from the 2_0 outputs in attn_<case>.pt (a few ulps, so the
                           zip-compressed file stays small; adding them back restores the outputs bit for bit), and
                           their attention maps
  refpin_ipadapter.pt      what IPAdapterXL / IPAdapterPlusXL hand to the pipeline, get_generator, and the
                           ip_adapter.bin / the weights load_ip_adapter reads from it (as digests, see digest())
"""
import contextlib
import hashlib
import importlib.util
import io
import os

import numpy as np
import torch

from .detfill import det_fill, det_randn

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
HALF = torch.float16


# ---- convert_bin.py ------------------------------------------------------------------------------------------------
def fake_training_checkpoint():
    """an accelerate-style training state dict: UNet weights (dropped by the converter) + the three adapter groups"""
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g)
    return {"unet.conv_in.weight": r(8, 4, 3, 3),
            "image_proj_model.proj.weight": r(16, 8), "image_proj_model.proj.bias": r(16),
            "image_proj_model.norm.weight": r(4), "image_proj_model.norm.bias": r(4),
            "adapter_modules.1.to_k_ip.weight": r(8, 6), "adapter_modules.1.to_v_ip.weight": r(8, 6),
            "adapter_modules.3.to_k_ip.weight": r(8, 6), "adapter_modules.3.to_v_ip.weight": r(8, 6),
            "composed_modules.fc1.weight": r(5, 3), "composed_modules.ln.bias": r(5)}


# ---- the denoise loop (ip_adapter/custom_pipelines.py __call__) ------------------------------------------------------
LOOP_CASES = [("ddim", {}), ("euler", {}),
              ("ddim", dict(control_guidance_start=0.3, control_guidance_end=0.7)),
              ("ddim", dict(denoising_end=0.6)),
              ("ddim", dict(guidance_rescale=0.7, original_size=(512, 384), crops_coords_top_left=(16, 32), target_size=(256, 256)))]


def loop_inputs(cfg):
    """(latents, prompt / negative embeds, pooled / negative pooled) of every LOOP_CASES run"""
    cd = cfg.cross_attention_dim
    return (det_randn((1, 4, 32, 32), 3), det_randn((1, 81, cd), 4), det_randn((1, 81, cd), 5),
            det_randn((1, cfg.pooled_dim), 6), det_randn((1, cfg.pooled_dim), 7))


def _ref_loop(kind, kw):
    """the reference's own loop on the oracle's tiny UNet carrying the REFERENCE's processor classes"""
    from . import refshim
    from .schedulers import DDIMScheduler, EulerDiscreteScheduler
    from .sdxl_unet import UNet2DConditionModel, tiny_config
    Pipe, ap = refshim.load_pipeline_class()
    cfg = tiny_config()
    u = det_fill(UNet2DConditionModel(cfg), 5).eval()
    procs = {}
    for name in u.attn_processors.keys():                       # ip_adapter.py:102-123
        if name.endswith("attn1.processor"):
            procs[name] = ap.AttnProcessor2_0()
        else:
            hidden = {"mid_block": cfg.block_out_channels[-1]}.get(name.split(".")[0])
            if hidden is None:
                bid = int(name.split(".")[1])
                hidden = (list(reversed(cfg.block_out_channels)) if name.startswith("up_blocks") else cfg.block_out_channels)[bid]
            skip = "down_blocks.2.attentions.1" not in name
            p = ap.IPAttnProcessor2_0(hidden_size=hidden, cross_attention_dim=cfg.cross_attention_dim, scale=0.8,
                                      num_tokens=4, skip=skip)
            procs[name] = det_fill(p, 7, prefix=name)
    u.set_attn_processor(procs)

    class _U(torch.nn.Module):                                   # the reference passes cross_attention_kwargs / return_dict
        def __init__(s):
            super().__init__()
            s.u = u
            s.config = type("C", (), {"in_channels": cfg.in_channels})()

        @property
        def attn_processors(s):
            return s.u.attn_processors

        def forward(s, x, t, encoder_hidden_states=None, cross_attention_kwargs=None, added_cond_kwargs=None, return_dict=False):
            return s.u(x, t, encoder_hidden_states=encoder_hidden_states, added_cond_kwargs=added_cond_kwargs)

    class _Cfg:
        num_train_timesteps = 1000

    s = DDIMScheduler() if kind == "ddim" else EulerDiscreteScheduler()
    orig, orig_step = s.set_timesteps, s.step
    s.set_timesteps = lambda n, device=None: orig(n)            # the reference passes device=
    s.order, s.config = 1, _Cfg()
    s.step = lambda eps, t, lat, return_dict=False, **k: orig_step(eps, t, lat)

    pipe = Pipe.__new__(Pipe)
    pipe.unet, pipe.scheduler, pipe.default_sample_size, pipe.watermark = _U(), s, 32, None
    lat, pe, ne, po, no = loop_inputs(cfg)
    return pipe(prompt_embeds=pe, negative_prompt_embeds=ne, pooled_prompt_embeds=po, negative_pooled_prompt_embeds=no,
                height=256, width=256, num_inference_steps=4, guidance_scale=5.0, latents=lat.clone(),
                output_type="latent", **kw).images


# ---- state-dict interchange ------------------------------------------------------------------------------------------
def state_dict_modules(ns):
    """(name, module) of the four modules whose state dicts the project's must interchange with, as classes of `ns`"""
    from .gen_golden import HA_CFG, RES_TEST
    with contextlib.redirect_stdout(io.StringIO()):           # HarmonyAttention prints upstream
        return [("harmony", ns.HarmonyAttention(**HA_CFG)), ("imageproj", ns.ImageProjModel(2048, 1280, 4)),
                ("resampler", ns.Resampler(**RES_TEST)), ("ipattn", ns.IPAttnProcessor2_0(640, 2048))]


SD_SEED = 51


def state_dict_outputs(mods):
    """HarmonyAttention and Resampler outputs on seeded inputs, the modules filled by det_fill(SD_SEED)"""
    m = dict(mods)
    with contextlib.redirect_stdout(io.StringIO()):
        ha = det_fill(m["harmony"], SD_SEED)(det_randn((1, 77, 2048), 1), det_randn((1, 1280), 2))
    return {"ha_out": ha, "res_out": det_fill(m["resampler"], SD_SEED)(det_randn((2, 257, 1280), 3))}


# ---- legacy (torch < 2) processors -------------------------------------------------------------------------------------
LEGACY_CASES = ["c1280_t4", "c128_t32"]


# ---- IPAdapterXL / IPAdapterPlusXL host orchestration: test doubles shared by the fixture and the tests -----------------
class FakePipe:
    def __init__(self, unet):
        self.unet, self.calls, self.encoded = unet, [], []

    def to(self, device):
        return self

    def encode_prompt(self, prompt, num_images_per_prompt=1, do_classifier_free_guidance=True, negative_prompt=None, **kw):
        self.encoded.append((tuple(prompt) if isinstance(prompt, list) else prompt, num_images_per_prompt,
                             tuple(negative_prompt) if isinstance(negative_prompt, list) else negative_prompt))
        n = (len(prompt) if isinstance(prompt, list) else 1) * num_images_per_prompt
        seed = sum(map(ord, "".join(prompt) if isinstance(prompt, list) else prompt)) % 997
        cd = self.unet.config.cross_attention_dim
        return (det_randn((n, 77, cd), seed).to(HALF), det_randn((n, 77, cd), seed + 1).to(HALF),
                det_randn((n, 32), seed + 2).to(HALF), det_randn((n, 32), seed + 3).to(HALF))

    def __call__(self, **kw):
        self.calls.append(kw)
        return type("O", (), {"images": ["img"] * kw["prompt_embeds"].shape[0]})()


class FakeProc:                   # CLIPImageProcessor stand-in
    def __call__(self, images=None, return_tensors=None):
        arr = np.stack([np.asarray(im, dtype=np.float32).mean(axis=(0, 1)) for im in images])
        return type("B", (), {"pixel_values": torch.from_numpy(arr)})()


class FakeClip(torch.nn.Module):  # CLIPVisionModelWithProjection stand-in: pixel statistics -> [B, 128]
    config = type("C", (), {"projection_dim": 128, "hidden_size": 64})()

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(det_randn((3, 128), 77), requires_grad=False)

    def forward(self, px, output_hidden_states=False):
        return type("O", (), {"image_embeds": ((px.float() / 255.0) @ self.w.float()).to(px.dtype)})()   # an fp16 model returns fp16


class FakeClipH(torch.nn.Module):  # vision model with hidden states: the PlusXL path reads hidden_states[-2]
    config = type("C", (), {"projection_dim": 128, "hidden_size": 64})()

    def forward(self, px, output_hidden_states=False):
        base = (px.float() / 255.0).unsqueeze(1).repeat(1, 9, 1)                   # [B, 9 tokens, 3]
        w = det_randn((3, 64), 78)
        hs = [(base * (i + 1)) @ w for i in range(3)]
        return type("O", (), {"hidden_states": [h.to(px.dtype) for h in hs]})()


def adapter_modules(mod_ns):
    """the projection + HarmonyAttention modules with identical seeded weights, as classes of `mod_ns`"""
    proj = det_fill(mod_ns.ImageProjModel(cross_attention_dim=256, clip_embeddings_dim=128, clip_extra_context_tokens=4), 5)
    with contextlib.redirect_stdout(io.StringIO()):
        ha = mod_ns.HarmonyAttention(image_hidden_size=128, text_context_dim=256, inter_dim=512, cross_heads=8,
                                     reshape_blocks=8, cross_value_dim=64, scale=1.0, fusion_method="cross_attention")
    return proj.to(HALF), det_fill(ha, 3).to(HALF)


def fake_image(seed):
    from PIL import Image
    return Image.fromarray((np.random.RandomState(seed).rand(24, 20, 3) * 255).astype("uint8"))


XL_KWARGS = dict(prompt="lions", negative_prompt="blurry", extra_text="eight sheep", scale=0.6, num_samples=1, seed=42,
                 num_inference_steps=7, guidance_scale=5.0, height=256, width=256)
PLUS_CFG = dict(dim=128, depth=2, dim_head=32, heads=4, num_queries=16, embedding_dim=64, output_dim=256, ff_mult=2)
PLUS_KWARGS = dict(prompt=None, negative_prompt=None, scale=0.9, num_samples=2, seed=7, num_inference_steps=5, guidance_scale=4.0)
GENERATOR_SEEDS = (None, 5, [1, 2, 3])
NCA = "<number_class_crossattention>"      # stands for the module object generate() was handed


def record_call(kw, nca=None):
    """a pipeline call's kwargs in plain data: tensors as they are, a Generator as ("generator", seed), the module passed
    through as number_class_crossattention as NCA"""
    rec = {}
    for k, v in kw.items():
        if torch.is_tensor(v):
            rec[k] = v.detach().clone()
        elif isinstance(v, torch.Generator):
            rec[k] = ("generator", v.initial_seed())
        elif nca is not None and v is nca:
            rec[k] = NCA
        else:
            rec[k] = v
    return rec


def processor_table(procs):
    """{name: ("AttnProcessor2_0",) | ("IPAttnProcessor2_0", hidden, cross_dim, num_tokens, skip, to_k_ip shape, scale)}"""
    tab = {}
    for k, p in procs.items():
        kind = type(p).__name__
        if kind == "AttnProcessor2_0":
            tab[k] = (kind,)
        else:
            tab[k] = (kind, p.hidden_size, p.cross_attention_dim, p.num_tokens, p.skip, tuple(p.to_k_ip.weight.shape), p.scale)
    return tab


def digest(sd):
    """[(key, shape, dtype, sha256 of the float32 values)] of a state dict: exact equality without storing the weights"""
    return [(k, tuple(v.shape), str(v.dtype), hashlib.sha256(v.detach().float().contiguous().numpy().tobytes()).hexdigest())
            for k, v in sd.items()]


def _ref_adapter(ref):
    from .sdxl_unet import UNet2DConditionModel, tiny_config
    out = {}

    # IPAdapterXL (ip_adapter.py:249-340): constructed without __init__, which would download CLIP weights
    r_unet = det_fill(UNet2DConditionModel(tiny_config()), 5)
    r = ref.IPAdapterXL.__new__(ref.IPAdapterXL)
    r.device, r.num_tokens, r.pipe = "cpu", 4, FakePipe(r_unet)
    r.image_encoder, r.clip_image_processor = FakeClip(), FakeProc()
    r.image_proj_model, r.number_class_crossattention = adapter_modules(ref)
    r.set_ip_adapter()                                                            # ip_adapter.py:99-125
    with contextlib.redirect_stdout(io.StringIO()):
        images = r.generate(fake_image(0), number_class_crossattention=r.number_class_crossattention, **XL_KWARGS)
    out["xl"] = {"processors": processor_table(r_unet.attn_processors), "encoded": r.pipe.encoded,
                 "call": record_call(r.pipe.calls[-1], r.number_class_crossattention), "images": images}

    # IPAdapterPlusXL (ip_adapter.py:389-478)
    r = ref.IPAdapterPlusXL.__new__(ref.IPAdapterPlusXL)
    r.device, r.num_tokens, r.pipe = "cpu", 16, FakePipe(det_fill(UNet2DConditionModel(tiny_config()), 5))
    r.image_encoder, r.clip_image_processor = FakeClipH(), FakeProc()
    r.image_proj_model = det_fill(ref.Resampler(**PLUS_CFG), 9).to(HALF)
    r.set_ip_adapter()
    images = r.generate(fake_image(1), **PLUS_KWARGS)
    out["plusxl"] = {"encoded": r.pipe.encoded, "call": record_call(r.pipe.calls[-1]), "images": images}

    # get_generator (ip_adapter/utils.py:83-93)
    gens = []
    for seed in GENERATOR_SEEDS:
        a = ref.get_generator(seed, "cpu")
        if a is None:
            gens.append(None)
        elif isinstance(a, list):
            gens.append([g.initial_seed() for g in a])
        else:
            gens.append((a.initial_seed(), torch.randn(4, generator=a)))
    out["get_generator"] = gens

    # load_ip_adapter (ip_adapter.py:135-154) of a checkpoint in the reference's own format, written from a donor adapter
    donor_unet = det_fill(UNet2DConditionModel(tiny_config()), 5)
    donor = ref.IPAdapterXL.__new__(ref.IPAdapterXL)
    donor.device, donor.num_tokens, donor.pipe = "cpu", 4, FakePipe(donor_unet)
    donor.set_ip_adapter()
    for n, p in donor_unet.attn_processors.items():
        det_fill(p, 21, prefix=n)
    proj, ha = adapter_modules(ref)
    layers = torch.nn.ModuleList(donor_unet.attn_processors.values())
    ckpt = {"image_proj": det_fill(proj, 31).state_dict(), "ip_adapter": layers.state_dict(),
            "composed_adapter": det_fill(ha, 33).state_dict()}
    path = os.path.join(OUT, "_refpin_ip_adapter.bin")
    torch.save(ckpt, path)
    try:
        r = ref.IPAdapterXL.__new__(ref.IPAdapterXL)
        r.device, r.num_tokens, r.pipe, r.ip_ckpt = "cpu", 4, FakePipe(det_fill(UNet2DConditionModel(tiny_config()), 5)), path
        r.image_proj_model, r.number_class_crossattention = adapter_modules(ref)
        r.set_ip_adapter()
        with contextlib.redirect_stdout(io.StringIO()):
            r.load_ip_adapter()
    finally:
        os.remove(path)
    out["checkpoint"] = {grp: digest(sd) for grp, sd in ckpt.items()}
    out["loaded"] = {"image_proj": digest(r.image_proj_model.state_dict()),
                     "composed_adapter": digest(r.number_class_crossattention.state_dict()),
                     "ip_adapter": digest(torch.nn.ModuleList(r.pipe.unet.attn_processors.values()).state_dict())}
    return out


@torch.no_grad()
def main():
    from . import refshim
    from .gen_golden import ATTN_CASES, attn_inputs, make_attn
    ref = refshim.load()
    os.makedirs(OUT, exist_ok=True)

    spec = importlib.util.spec_from_file_location("_ref_convert_bin", os.path.join(refshim.REF, "convert_bin.py"))
    conv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(conv)
    src, dst = os.path.join(OUT, "_refpin_training.bin"), os.path.join(OUT, "_refpin_converted.bin")
    torch.save(fake_training_checkpoint(), src)
    try:
        assert conv.convert_checkpoint_to_ip_adapter(src, dst)
        converted = torch.load(dst)
    finally:
        for f in (src, dst):
            if os.path.exists(f):
                os.remove(f)
    torch.save({"out": converted}, os.path.join(OUT, "refpin_convert_bin.pt"))

    torch.save({"cases": LOOP_CASES, "latents": [_ref_loop(kind, kw) for kind, kw in LOOP_CASES]},
               os.path.join(OUT, "refpin_denoise_loop.pt"))

    mods = state_dict_modules(ref)
    torch.save({"keys": {n: [(k, tuple(v.shape)) for k, v in m.state_dict().items()] for n, m in mods}, "seed": SD_SEED,
                **state_dict_outputs(mods)}, os.path.join(OUT, "refpin_state_dicts.pt"))

    legacy = {}
    for case in LEGACY_CASES:
        b, l, c, h, cd, nt, t, scale = ATTN_CASES[case]
        hs, ehs = attn_inputs(case)
        g = torch.load(os.path.join(OUT, f"attn_{case}.pt"))                 # the 2_0 processors' outputs (gen_golden.py)
        p = det_fill(ref.IPAttnProcessor(c, cd, scale=scale, num_tokens=t), 17, prefix="proc.")
        ip = p(make_attn(case, cross=True), hs, encoder_hidden_states=ehs)
        sa = ref.AttnProcessor()(make_attn(case, cross=False), hs)
        for name, y, base in (("ip", ip, g["ip_skip0"]), ("self", sa, g["self"])):
            d = y - base
            assert torch.equal(base + d, y), (case, name)                     # the stored difference restores y bit for bit
            legacy[f"{case}.{name}_minus_2_0"] = d.numpy()
        legacy[f"{case}.attn_map"] = p.attn_map.numpy()
    np.savez_compressed(os.path.join(OUT, "refpin_legacy_attn.npz"), **legacy)

    torch.save(_ref_adapter(ref), os.path.join(OUT, "refpin_ipadapter.pt"))
    for f in sorted(os.listdir(OUT)):
        if f.startswith("refpin_"):
            print(f, os.path.getsize(os.path.join(OUT, f)))


if __name__ == "__main__":
    main()
