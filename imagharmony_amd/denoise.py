"""The denoise loop of ip_adapter/custom_pipelines.py:249-363 as a device-resident loop.

One denoise step = [UNet forward on the CFG-duplicated latent] + [CFG combine + scheduler.step] +
[step counter += 1], recorded ONCE into a C++ plan and captured into a hipGraph; the 30-step loop is
30 graph replays with no host work in between: timesteps, scheduler coefficients, the Euler input
scale and the per-step IP-scale gate (control_guidance_start/end, custom_pipelines.py:326-329) are
device tables indexed by a device-resident step counter.  Inpainting (diffusers StableDiffusionXLInpaintPipeline) keeps that shape: the
masked blend upstream applies on the host after every scheduler.step is part of the recorded step (it rides in the CFG + scheduler
launch and reads its add_noise pair from one more table), and a 9-channel UNet reads [mask | masked-image latents] from a
step-invariant buffer inside conv_in.  A ControlNet branch (set_controlnet) is recorded in front of the UNet in any of these modes: it reads the
4-channel latents alone, and neither inpainting mode adds a launch to it.
"""
import collections
import functools
import hashlib
import os

import torch

from . import lib as L
from .ctx import Ctx
from .unet import StepState

# XCD cell policy measured once per (device, UNet batch, latent size, dtype) and process: every engine (and fork) of that shape reuses it
_XCD_PICK = {}

# inpainting state the recorded plan points at; a call copies into them (prepare_inpaint) and re-records nothing
INPAINT_BUFFERS = ("inp_z", "inp_noise", "inp_mask", "conv_in_extra")
# what a plan that ends with the general step (EW_CFG_MSTEP) points at besides: the six-column table, the history slot and the noise
# bank -- or, under a seeded schedule, the samples' seed rows
GENERAL_STEP = ("coef6_tab", "hist", "noise_bank", "seed_rows")
# THE list of StepState members that are valid exactly as long as one recorded plan is: what the plan cache stores and restores.  The
# other two places that move such members from one StepState to another are written as differences from it:
PLAN_STATE = ("t_table", "coef_tab", "in_scale_tab", "ip_scale_tab", "temb_table", "blend_tab") + GENERAL_STEP
# - a new conditioning (set_conditioning) keeps the schedule's tables, the latents, the counter and the inpainting buffers, but not the
#   time-embedding rows: they were computed from the previous conditioning's aug_emb
_CARRIED = (set(PLAN_STATE) - {"temb_table"}) | {"latents", "step"} | set(INPAINT_BUFFERS)
# - a fork has its own (zeroed) general-step state, like its latents, shares the other tables and records its own time-embedding rows
_FORK_OWN = ("hist", "noise_bank", "seed_rows")
_FORK_SHARED = set(PLAN_STATE) - set(_FORK_OWN) - {"temb_table"}
# ... and the engine's members of the same lifetime: the step count, the plan(s) and what they write, the context that owns the
# time-embedding rows of the UNet and of the ControlNet, the conditioners' per-schedule tables
_PLAN_ENGINE = ("steps", "init_noise_sigma", "plan", "noise_pred", "plan_tail", "np_full", "_temb_ctx", "cn_scale_tab", "_cn_temb", "ad_gate_tab")


# What tells one recorded plan of a conditioning from another (set_schedule); used by name, compared and hashed as the tuple it is:
#   scheduler (the class name), num_train_timesteps, num_inference_steps, control_guidance_start / _end (the IP-scale window),
#   denoising_end, ip_scale (the IP processors' scale, the value of the gating table), steps (the row behind the last step that runs),
#   tables (SHA-1 of every table the plan reads, the IP gating table included), controlnet (SHA-1 of cn_scale_tab; None: no branch),
#   inpaint (None | "blend" | "concat"), adapter ((SHA-1 of ad_gate_tab, conditioning scale); None: no T2I-Adapter), seeded,
#   regions (IPRegions.digest(): SHA-1 of N, the weights and the mask bytes) -- a trailing field that exists only on the key of a plan
#   with regional image prompts: a key without them is the thirteen-field tuple it always was (``.regions`` reads None), so it compares,
#   hashes, slices and serialises as before, and PlanKey(...) equals PlanKey(..., regions=None)
_KEY_FIELDS = ("scheduler num_train_timesteps num_inference_steps control_guidance_start control_guidance_end "
               "denoising_end ip_scale steps tables controlnet inpaint adapter seeded")
#   freeu (the UNet's (s1, s2, b1, b2), unet.enable_freeu) -- the same way: a trailing field that exists only on the key of a plan recorded
#   with FreeU enabled, behind regions where both are set; a key without it is the tuple it always was and ``.freeu`` reads None
#   pag ((SHA-1 of the chosen attn1 layers' names, the PAG scale); unet.set_pag_applied_layers, set_conditioning(pag_scale=)) -- the same
#   way again, the last of the trailing fields: it exists only on the key of a plan recorded with perturbed-attention guidance on
_KEY_EXTRAS = ("regions", "freeu", "pag")


@functools.lru_cache(maxsize=None)
def _key_variant(extras):
    """the key class that carries the trailing fields `extras` (a non-empty subset of _KEY_EXTRAS, in that order); the others read None"""
    cls = collections.namedtuple("PlanKey" + "".join(n.capitalize() for n in extras), _KEY_FIELDS + " " + " ".join(extras))
    for n in _KEY_EXTRAS:
        if n not in extras:
            setattr(cls, n, None)
    return cls


class PlanKey(collections.namedtuple("PlanKey", _KEY_FIELDS)):
    __slots__ = ()
    regions = None
    freeu = None
    pag = None

    def __new__(cls, *args, regions=None, freeu=None, pag=None, **kw):
        if len(args) == len(cls._fields) + 1:
            args, regions = args[:-1], args[-1]
        if freeu is not None:
            freeu = tuple(float(v) for v in freeu)
        if pag is not None:
            pag = (str(pag[0]), float(pag[1]))
        extras = {n: v for n, v in (("regions", regions), ("freeu", freeu), ("pag", pag)) if v is not None}
        if not extras:
            return super().__new__(cls, *args, **kw)
        return _key_variant(tuple(extras))(*args, **kw, **extras)


def _move(names, src, dst):
    for k in names:
        setattr(dst, k, getattr(src, k, None))       # (None: a StepState has no coef_tab until set_schedule gives it one)


class PlanRecord:
    """One entry of the plan cache: every member of PLAN_STATE and _PLAN_ENGINE as it was when the plan was recorded."""
    __slots__ = PLAN_STATE + _PLAN_ENGINE

    def __init__(self, eng):
        _move(PLAN_STATE, eng.st, self)
        _move(_PLAN_ENGINE, eng, self)

    def restore(self, eng):
        _move(PLAN_STATE, self, eng.st)
        _move(_PLAN_ENGINE, self, eng)


# What a conditioning is, for the one case in which an engine keeps two: switching perturbed-attention guidance on or off changes the
# UNet batch, so the other mode's caches and recorded plans cannot serve -- but they are still right for their own mode, and a call that
# switches back with the same inputs picks them up again instead of projecting and recording anew
_COND_STATE = ("st", "_cond_ctx", "_cond_in", "_cond_fp", "_plans", "S", "H", "W", "T_total", "do_cfg", "guidance", "guidance_rescale",
               "cfg_role", "pag", "pag_scale")


class _CondRecord:
    __slots__ = _COND_STATE

    def __init__(self, eng):
        _move(_COND_STATE, eng, self)

    def restore(self, eng):
        _move(_COND_STATE, self, eng)
        eng.plan, eng._sched_key = None, None          # set_schedule picks the plan out of the restored cache


class DenoiseEngine:
    # Every member the engine reads exists on every engine: the ones below start from these defaults (immutable values, so the class can
    # hold them -- an engine put together without the constructor reads them too), the rest is set by the constructor.
    # the conditioning (set_conditioning)
    st = None
    S = H = W = T_total = None
    do_cfg, guidance, guidance_rescale = False, None, 0.0
    cfg_role = None          # 0 / 1: this engine computes one half of the CFG pair (denoise_cfg_split)
    _cond_ctx = None         # the context that owns aug_emb and the K / V caches
    _cond_in = None          # (ehs, text, ids) as the UNet got them: the ControlNet's caches are computed from the same
    # the current plan and what lives as long as it does (_PLAN_ENGINE; set_schedule, _record)
    plan = noise_pred = None
    plan_tail = None         # cfg_role engines: the second plan (CFG combine + scheduler step + step++) ...
    np_full = None           # ... and the [2, S, ...] buffer of both halves it reads
    steps = init_noise_sigma = None
    _temb_ctx = _cn_temb = None      # the context that owns the time-embedding rows; the ControlNet's rows in it
    _sched_key = None
    xcd_cells = None         # the XCD cell shape picked when the plan is first recorded (_pick_xcd_cells) ...
    xcd_times_ms = None      # ... and {candidate: median forward ms} of the pick it came from
    _is_fork = False
    t_start = 0              # image-to-image: the first step of the schedule that runs (set_schedule)
    inpaint = None           # None | "blend" (4-channel UNet: masked blend in the step) | "concat" (9-channel UNet: conv_in reads the mask)
    general = False          # the schedule steps through the six-column table (EW_CFG_MSTEP): multistep / ancestral samplers (set_schedule)
    stochastic = False       # ... and reads a noise row per step
    seeded = False           # ... which the step generates from st.seed_rows instead of reading a bank (set_schedule(seeded_noise=True))
    # the ControlNet state (an engine without one carries nothing)
    controlnet = None        # a controlnet.ControlNetModel whose branch is recorded in front of the UNet (set_controlnet)
    cn = None                # its state: dict(image, scale, hint, cond = StepState with its aug_emb / K,V caches) (set_control_image)
    cn_scale_tab = None      # fp32 [steps] conditioning_scale * keep(i) of the current schedule (set_schedule)
    # the T2I-Adapter state, likewise
    adapter = None           # a t2i_adapter.T2IAdapter whose four features are added inside the UNet's down path (set_adapter)
    ad = None                # its state: dict(image, scale, feats = four NHWC tensors, ctx) (set_adapter_image)
    ad_gate_tab = None       # fp32 [steps] 1 / 0 per step of the current schedule (set_schedule(adapter_conditioning_factor=))
    # regional image prompts (regions.py; an engine without them records, launches and returns what it always did)
    regions = None           # an IPRegions: the cross-attention layers with an image-prompt branch record csrc/xattn_regions.hip's launch (set_ip_regions)
    # perturbed-attention guidance (set_conditioning(pag_scale=) with unet.set_pag_applied_layers; off: the engine is what it always was)
    pag = False              # the conditioning carries one more block of S rows, [uncond | cond | perturbed] / [cond | perturbed]
    pag_scale = 0.0          # ... and the step adds pag_scale * (cond - perturbed)
    _cond_fp = None          # fingerprint of what the current conditioning was computed from (None: not taken) ...
    _cond_stash = None       # ... and the conditioning of the other PAG mode, kept across a switch with its caches and plans (_CondRecord)

    def __init__(self, unet, device, dtype=torch.bfloat16, use_graph=True):
        """Touches no device: the eager context is made on first use, so the "no CPU path" ImhError of a non-ROCm device surfaces at the
        first launch (or the first set_conditioning), not here."""
        self.unet, self.device, self.dtype, self.use_graph = unet, torch.device(device), dtype, use_graph
        # XCD cell shapes tried when the plan is first recorded (_pick_xcd_cells): the byte-count model, 4 x 2 and 8 x 1 cells, and
        # 4 x 2 with the GEGLU launches left to the model (13); the choice sticks for the life of the engine
        # (IMH_XCD_AUTOTUNE=0: model only)
        self.xcd_candidates = (0, 3, 2, 13) if os.environ.get("IMH_XCD_AUTOTUNE", "1") != "0" else (0,)
        self._plans = {}         # recorded plans by schedule key (two-stage PNS alternates a preview and a final schedule per image)
        self.max_cached_plans = int(os.environ.get("IMH_MAX_CACHED_PLANS", "3"))      # each pins ~2 GB of activation buffers at 1024^2

    @functools.cached_property
    def eager(self):
        """the context of the few launches outside a plan (the step counter's reset, the initial latents): made on first use"""
        return Ctx(self.device, self.dtype)

    # -- what the two conditioners (ControlNet, T2I-Adapter) share --
    @staticmethod
    def _whole_pair_only(half, what):
        if half:
            raise NotImplementedError(f"an engine that holds one half of the CFG pair (cfg_role) does not run a {what}")

    def _drop_plans(self, doomed):
        """drops the current plan and the cached plans whose key `doomed` holds for: they point at state that is going away"""
        self._plans = {k: v for k, v in self._plans.items() if not doomed(k)}
        self.plan, self._sched_key = None, None

    def _check_weights_epoch(self):
        """the K / V caches, aug_emb, the time-embedding rows and the recorded plans derive from the UNet's weights, and PlanKey has no
        field for them: a LoRA merge (lora.LoRAState.apply) after set_conditioning is refused instead of computing from stale copies"""
        ctx = self._cond_ctx             # (it owns the caches, so it carries the epoch they were computed at; forks share it)
        if ctx is not None and getattr(ctx, "weights_epoch", 0) != getattr(self.unet, "lora_epoch", 0):
            raise RuntimeError("weights changed since set_conditioning (a LoRA was loaded, re-weighted or unloaded): call set_conditioning again")

    @staticmethod
    def _image_fits(image, S, height, width):
        """a stored control image serves S samples at height x width: one image or one per sample, at that size"""
        return tuple(image.shape[2:]) == (height, width) and image.shape[0] in (1, S)

    # -- regional image prompts (opt-in) --
    def _regions_alone(self, what, other):
        if self.regions is not None and other:
            raise NotImplementedError(f"regional image prompts together with {what} are not built")

    def set_ip_regions(self, regions):
        """regions: a regions.IPRegions (N masks over the picture, N weights), or None to switch them off.  BEFORE set_conditioning: the
        prompt embeddings of that conditioning end in N * num_tokens image tokens, and the K / V caches are projected per image.  The
        UNet's IP processors get num_images / regions here (ip_adapter.set_ip_regions); the masks reach the plan as fp32 rows per token
        grid, resized once per grid on the CPU (IPRegions.rows) and kept alive by the plan that reads them.  The regions' digest is part
        of the plan key.  Not built, refused here and where the other side is set: cfg_role, a ControlNet, a T2I-Adapter."""
        from .regions import IPRegions
        if regions is not None and not isinstance(regions, IPRegions):
            raise TypeError(f"set_ip_regions takes an imagharmony_amd.regions.IPRegions or None, not {type(regions).__name__}")
        if regions is not None:
            for what, other in (("a ControlNet", self.controlnet), ("a T2I-Adapter", self.adapter), ("cfg_role (the CFG split)", self.cfg_role)):
                if other is not None:
                    raise NotImplementedError(f"regional image prompts together with {what} are not built")
        self.regions = regions
        self._sync_regions()

    # -- T2I-Adapter (opt-in, like the ControlNet; the two exclude each other) --
    def set_adapter(self, adapter):
        """adapter: an imagharmony_amd.t2i_adapter.T2IAdapter on the engine's device, or None to switch the injections off.  The next
        set_schedule picks (or records) the plan of that mode: the plans with and without the adapter of one schedule coexist."""
        if adapter is not None:
            if isinstance(adapter, (list, tuple)) or hasattr(adapter, "adapters"):
                raise NotImplementedError("several adapters (MultiAdapter / a list of adapters) are not supported: one T2IAdapter")
            if not hasattr(adapter, "prepare_features"):
                raise TypeError(f"set_adapter takes an imagharmony_amd.t2i_adapter.T2IAdapter, not {type(adapter).__name__}")
            if self.controlnet is not None:
                raise NotImplementedError("a T2I-Adapter together with a ControlNet is not built")
            self._whole_pair_only(self.cfg_role is not None, "T2I-Adapter")
            self._regions_alone("a T2I-Adapter", True)
        if adapter is not self.adapter:
            swap = self.adapter is not None and adapter is not None
            if swap:
                self.ad = None                           # another model: its features go, and every plan recorded with them
            self._drop_plans(lambda k: swap and k.adapter is not None)
        self.adapter = adapter

    @torch.no_grad()
    def set_adapter_image(self, image, conditioning_scale=1.0):
        """The per-image state of the adapter: its four features, computed here, once, outside the step, and kept until the image
        changes (a call with the same image and another scale computes nothing).  image: float [1 | S, 3, height, width] in [0, 1]: one
        control image may serve every stacked sample.  conditioning_scale is part of the plan key, so set_schedule follows this call."""
        if self.adapter is None:
            raise L.ImhError("set_adapter_image needs an adapter: set_adapter first")
        self.adapter.check_image(image)
        old = self.ad
        same = old is not None and old["image"].shape == image.shape and torch.equal(old["image"], image.detach().to("cpu", torch.float32))
        if same:
            old["scale"] = float(conditioning_scale)     # the same image: the features (and the plans that point at them) stay
        else:
            img = image.detach().to("cpu", torch.float32).clone()
            ctx = Ctx(self.device, self.dtype)           # fresh context: the features must outlive pooled buffers
            feats = self.adapter.prepare_features(ctx, img, img.shape[2] // 8, img.shape[3] // 8)
            self.ad = dict(image=img, scale=float(conditioning_scale), feats=feats, ctx=ctx)
        self._drop_plans(lambda k: not same and k.adapter is not None)     # a plan recorded with the adapter points at the previous features

    @staticmethod
    def adapter_gate_table(n, t_start, factor):
        """[n] floats: 1 where loop index i of the m = n - t_start steps that run satisfies i < int(m * factor) (diffusers
        StableDiffusionXLAdapterPipeline: ``if i < int(num_inference_steps * adapter_conditioning_factor)``), else 0, at rows t_start + i;
        rows before t_start (never read) hold 1, as in gate_table"""
        m = n - t_start
        k = int(m * float(factor))
        return [1.0] * t_start + [1.0 if i < k else 0.0 for i in range(m)]

    # -- ControlNet (opt-in; an engine without one records, launches and returns what it always did) --
    def set_controlnet(self, controlnet):
        """controlnet: an imagharmony_amd.controlnet.ControlNetModel on the engine's device, or None to switch the branch off.  The next
        set_schedule picks (or records) the plan of that mode: the plans with and without the branch of one schedule coexist."""
        if controlnet is not None:
            if isinstance(controlnet, (list, tuple)) or hasattr(controlnet, "nets"):
                raise NotImplementedError("several ControlNets (MultiControlNetModel) are not supported: one ControlNetModel")
            if not hasattr(controlnet, "controlnet_down_blocks") or not hasattr(controlnet, "prepare_hint"):
                raise TypeError(f"set_controlnet takes an imagharmony_amd.controlnet.ControlNetModel, not {type(controlnet).__name__}")
            self._whole_pair_only(self.cfg_role is not None, "ControlNet")
            if self.adapter is not None:
                raise NotImplementedError("a ControlNet together with a T2I-Adapter is not built")
            self._regions_alone("a ControlNet", True)
        if controlnet is not self.controlnet:
            swap = self.controlnet is not None and controlnet is not None
            if swap:
                self.cn = None                           # another model: its caches go, and every cached plan
            self._drop_plans(lambda k: swap)
        self.controlnet = controlnet

    @torch.no_grad()
    def set_control_image(self, image, conditioning_scale=1.0):
        """The per-image state of the ControlNet branch, computed once, outside the step: the hint controlnet_cond_embedding(image)
        (NHWC [Sh, H/8, W/8, C0], Sh = 1 or S: one control image may serve every stacked sample) and -- here or at the next
        set_conditioning, whichever comes later -- the ControlNet's aug_emb and the text-only K / V^T caches of its cross-attention
        layers.  image: float [1 | S, 3, height, width] in [0, 1].  conditioning_scale enters the per-schedule gate table, so
        set_schedule follows this call."""
        if self.controlnet is None:
            raise L.ImhError("set_control_image needs a ControlNet: set_controlnet first")
        self.cn = dict(image=image, scale=float(conditioning_scale), hint=None, cond=None)
        self._drop_plans(lambda k: k.controlnet is not None)      # a plan recorded with the branch points at the previous hint
        if self.st is not None and self._cond_in is not None:
            self._prepare_control()

    def _prepare_control(self):
        cn, net = self.cn, self.controlnet
        self._whole_pair_only(self.cfg_role is not None, "ControlNet")
        img = cn["image"]
        if img.dim() != 4 or img.shape[0] not in (1, self.S):
            raise L.ImhError(f"control image {tuple(img.shape)}: one image or one per sample ({self.S}) as [n, 3, H, W]")
        ctx = Ctx(self.device, self.dtype)       # fresh context: the hint and the caches must outlive pooled buffers
        cn["hint"] = net.prepare_hint(ctx, img, self.H, self.W)
        ehs, text, ids = self._cond_in
        cn["cond"] = net.prepare_conditioning(ctx, ehs, text, ids)
        cn["ctx"] = ctx

    @staticmethod
    def gate_table(n, t_start, start, end, value):
        """[n] floats: `value` where the window keeps step i of the m = n - t_start steps that run (custom_pipelines.py:319-329;
        diffusers controlnet_keep: 1 - (i / m < start or (i + 1) / m > end)), 0 where it does not, at rows t_start + i; rows before
        t_start (never read) hold `value`"""
        m = n - t_start
        return [float(value)] * t_start + [0.0 if (i / m < start) or ((i + 1) / m > end) else float(value) for i in range(m)]

    # -- conditioning (once per image / per PNS run; shared by every candidate seed) --
    @torch.no_grad()
    def set_conditioning(self, prompt_embeds, negative_prompt_embeds, pooled, negative_pooled, height, width,
                         guidance_scale=5.0, guidance_rescale=0.0, original_size=None, crops_coords_top_left=(0, 0),
                         target_size=None, cfg_role=None, pag_scale=0.0):
        """prompt_embeds: [S, 77+T, 2048] (IP tokens already concatenated, ip_adapter.py:321-322).
        pag_scale > 0 with layers chosen on the UNet (unet.set_pag_applied_layers): perturbed-attention guidance (diffusers PAGMixin).
        Every conditioning row set -- the prompt embeddings behind every cross-attention layer's K / V cache, image tokens included,
        text_embeds, time_ids, so also aug_emb and the time-embedding rows -- gets one more block, the positive rows again:
        [neg | pos | pos], or [pos | pos] without CFG; the UNet runs that block with identity self-attention maps in the chosen layers
        and the step adds pag_scale * (cond - perturbed).  pag_scale = 0, or no layers chosen: the call as it always was.  Refused
        (NotImplementedError): together with cfg_role, a ControlNet, a T2I-Adapter, regional image prompts.
        Switching the mode keeps the other mode's conditioning aside with its plans; the next call that switches back with the same
        inputs, guidance and weights gets it back and records nothing.
        original_size / crops_coords_top_left / target_size: SDXL micro-conditioning (custom_pipelines.py:277-293),
        default (height, width), (0, 0), (height, width).
        cfg_role = 0 / 1: this engine computes only the unconditional / the conditional half of the CFG pair (UNet batch S
        instead of 2S); the halves are exchanged every step by denoise_cfg_split (two ranks share one candidate's denoise:
        the serial tail of the two-stage PNS schedule)."""
        if cfg_role not in (None, 0, 1):
            raise ValueError("cfg_role must be None, 0 (unconditional half) or 1 (conditional half)")
        self._whole_pair_only(cfg_role is not None and self.controlnet is not None, "ControlNet")
        self._whole_pair_only(cfg_role is not None and self.adapter is not None, "T2I-Adapter")
        self._regions_alone("cfg_role (the CFG split)", cfg_role is not None)
        self._regions_alone("a ControlNet", self.controlnet is not None)
        self._regions_alone("a T2I-Adapter", self.adapter is not None)
        self._sync_regions()
        pag = float(pag_scale) > 0.0 and bool(getattr(self.unet, "pag_layers", None))
        if pag:
            for what, other in (("cfg_role (the CFG split)", cfg_role), ("a ControlNet", self.controlnet), ("a T2I-Adapter", self.adapter),
                                ("regional image prompts", self.regions)):
                if other is not None:
                    raise NotImplementedError(f"perturbed-attention guidance together with {what} is not built")
        if pag or self.pag or self._cond_stash is not None or getattr(self.unet, "pag_layers", None):
            # PAG is in play (layers chosen, or a mode to switch from): the conditionings are fingerprinted, and the one of the other mode
            # is kept across the switch.  An engine that never meets PAG skips all of this and carries none of its state
            fp = self._cond_fingerprint((prompt_embeds, negative_prompt_embeds, pooled, negative_pooled),
                                        (height, width, float(guidance_scale), float(guidance_rescale), original_size,
                                         tuple(crops_coords_top_left), target_size, cfg_role, float(pag_scale) if pag else 0.0))
            cur = _CondRecord(self) if self.st is not None and self._cond_fp is not None else None
            stash, self._cond_stash = self._cond_stash, None
            if cur is not None and cur.pag != pag:
                self._cond_stash = cur            # the other mode's conditioning outlives the switch
            elif stash is not None and stash.pag != pag:
                self._cond_stash = stash
            if stash is not None and fp is not None and stash.pag == pag and stash._cond_fp == fp:
                stash.restore(self)               # (its StepState comes back with it: the latents, the counter and the tables its plans point at)
                return self.st
            self.pag, self.pag_scale, self._cond_fp = pag, float(pag_scale) if pag else 0.0, fp
        elif self._cond_fp is not None:
            self._cond_fp = None                  # (a fingerprint taken while PAG was in play does not describe this conditioning)
        self._plans, self.plan = {}, None        # every recorded plan points into the previous conditioning's caches
        self.cfg_role = cfg_role
        self.do_cfg = guidance_scale > 1.0                                   # custom_pipelines.py:223
        self.guidance = float(guidance_scale)
        self.guidance_rescale = float(guidance_rescale)                      # :351-354 (only with CFG)
        S = prompt_embeds.shape[0]
        osz, tsz = tuple(original_size or (height, width)), tuple(target_size or (height, width))
        ids = torch.tensor([list(osz) + list(crops_coords_top_left) + list(tsz)], dtype=torch.float32).repeat(S, 1)   # :277-293
        if pag:                                                              # diffusers PAGMixin._prepare_perturbed_attention_guidance
            neg = [negative_prompt_embeds] if self.do_cfg else []
            ehs = torch.cat(neg + [prompt_embeds, prompt_embeds], 0)
            text = torch.cat(([negative_pooled] if self.do_cfg else []) + [pooled, pooled], 0)
            ids = torch.cat([ids] * (len(neg) + 2), 0)
        elif self.do_cfg and cfg_role is None:                               # :295-298 -- order [uncond | cond]
            ehs = torch.cat([negative_prompt_embeds, prompt_embeds], 0)
            text = torch.cat([negative_pooled, pooled], 0)
            ids = torch.cat([ids, ids], 0)
        elif self.do_cfg and cfg_role == 0:
            ehs, text = negative_prompt_embeds, negative_pooled
        else:
            ehs, text = prompt_embeds, pooled
        ctx = Ctx(self.device, self.dtype)      # fresh context: the K/V caches must outlive pooled buffers
        st = self.unet.prepare_conditioning(ctx, ehs, text, ids)
        self._cond_ctx = ctx
        ctx.weights_epoch = getattr(self.unet, "lora_epoch", 0)       # unet.lora_epoch as these caches saw it (_check_weights_epoch)
        self.S, self.H, self.W = S, height // 8, width // 8
        self.T_total = ehs.shape[1]
        old = self.st
        self.st = st
        if old is not None:                      # keep per-run tables
            _move(_CARRIED, old, st)
        self._cond_in = (ehs, text, ids)
        if self.cn is not None:
            self.cn["hint"] = self.cn["cond"] = None      # the ControlNet's caches belong to the previous conditioning (and size)
            img = self.cn["image"]
            if img.dim() == 4 and not self._image_fits(img, S, height, width):
                # the previous call's control image does not fit this conditioning (an edit's size follows its image): it is dropped,
                # not prepared at the wrong size; set_control_image sets this call's (set_schedule insists on one)
                self.cn = None
            elif self.controlnet is not None:
                self._prepare_control()
        if self.ad is not None and not self._image_fits(self.ad["image"], S, height, width):
            self.ad = None                        # the previous call's control image does not fit this size or batch: set_adapter_image sets this call's
        return st

    def _cond_fingerprint(self, tensors, scalars):
        """SHA-1 of everything a conditioning is computed from, for the switch of PAG modes (set_conditioning); None where the engine
        carries state the fingerprint does not cover (a ControlNet, an adapter, regions) or a tensor is missing"""
        if self.controlnet is not None or self.adapter is not None or self.regions is not None or any(not torch.is_tensor(t) for t in tensors):
            return None
        fp = hashlib.sha1(repr((scalars, getattr(self.unet, "lora_epoch", 0), str(self.dtype))).encode())
        for t in tensors:
            t = t.detach().to("cpu").contiguous()
            fp.update(repr((tuple(t.shape), str(t.dtype))).encode())
            fp.update(t.view(torch.uint8).numpy().tobytes())
        return fp.hexdigest()

    def _pag_key(self):
        """the PAG field of the plan key: (digest of the chosen layers' names, the scale), or None with PAG off"""
        if not self.pag:
            return None
        names = self.unet.pag_layer_names()
        if not names:
            raise L.ImhError("the conditioning carries the perturbed block but the UNet's PAG layers were cleared: set_pag_applied_layers, or set_conditioning again")
        return hashlib.sha1("\n".join(names).encode()).hexdigest(), self.pag_scale

    # -- schedule tables --
    def set_schedule(self, scheduler, num_inference_steps, control_guidance_start=0.0, control_guidance_end=1.0,
                     denoising_end=None, t_start=0, inpaint=False, seeded_noise=False, controlnet_guidance_start=0.0,
                     controlnet_guidance_end=1.0, adapter_conditioning_factor=1.0):
        """inpaint: the schedule of an inpainting call (prepare_inpaint).  On a 4-channel UNet every step then ends with upstream's masked
        blend, latents = (1 - m) * add_noise(z, n, timesteps[i + 1]) + m * latents, whose add_noise pair comes from blend_tab: row r holds
        scheduler.add_noise_coefficients(r + 1), the last row that runs (1, 0) -- the image latents themselves.  On a 9-channel UNet there is
        no blend; conv_in reads the mask and the masked-image latents.  Either way the plan differs from the text-to-image one under the
        same schedule, so the mode is part of the plan key.
        t_start > 0 (image-to-image, diffusers get_timesteps): the loop runs timesteps[t_start:] -- the device step counter starts at
        t_start, so the full schedule's tables, time-embedding rows and recorded plan serve; denoising_end then cuts the truncated list
        and the IP-scale gating window counts it.
        A scheduler with ``general_step`` (schedulers.DPMSolverMultistepScheduler, EulerAncestralDiscreteScheduler) hands over a six-column
        table, tables(t_start)["coef6"], in place of ``coef``; the plan then ends with EW_CFG_MSTEP.  Its row at t_start is first order, so
        a text-to-image and an image-to-image call get different tables -- and, the table being part of the fingerprint, different plans --
        exactly where the rows differ.  Allocated here for such a schedule: st.hist, fp32 [S, 4, H, W] (the previous data prediction, when
        the scheduler needs one), and st.noise_bank, fp32 [num_inference_steps, S, 4, H, W], for a stochastic scheduler: row r is the
        noise of step r, filled by denoise() before the loop.  At 1024^2 the bank is 4 * 128 * 128 * 4 B = 256 KiB per step and sample,
        about 8 MB per sample for 30 steps.
        seeded_noise=True (a stochastic scheduler; ignored by a deterministic one, whose plan is what it was): no bank.  The plan ends
        with the seeded step (imh.h imh_step_seeded, same launch count), which generates row *step's noise from st.seed_rows, int32 bits of
        adapter_conditioning_factor (an engine with a T2I-Adapter and its image set): the adapter's features are added in the first
        int(steps that run * factor) steps (adapter_gate_table); the table and the conditioning scale are part of the plan key.
        uint32 [S, 4] = (seed low, seed high, lane, 0) per sample (noise.seed_rows) -- 16 bytes per sample that denoise(step_seeds=...)
        fills before the loop.  The noise is then a pure function of (seed, lane, table row, element): the same on any rank, alone or
        stacked, eager or graph.  The flag is part of the plan key; the bank plan and the seeded plan of one schedule coexist."""
        st, dev = self.st, self.device
        t_start = int(t_start)
        self._check_weights_epoch()
        self._regions_alone("cfg_role (the CFG split)", self.cfg_role is not None)
        self._regions_alone("a ControlNet", self.controlnet is not None)
        self._regions_alone("a T2I-Adapter", self.adapter is not None)
        have, want = self._images_in_caches(), self.regions.n if self.regions is not None else 1
        if have is not None and have != want:
            raise L.ImhError(f"the conditioning's K / V caches hold {have} image prompt(s) per sample, the regions {want}: "
                             f"set_ip_regions comes before set_conditioning")
        if not 0 <= t_start < int(num_inference_steps):
            raise ValueError(f"t_start {t_start} outside the schedule of {num_inference_steps} steps")
        from .attention_processor import IPAttnProcessor2_0
        base = next((p.scale for p in self.unet.attn_processors.values() if isinstance(p, IPAttnProcessor2_0)), 1.0)
        # the key carries a fingerprint of the tables themselves (timesteps, coefficients, input scale, init sigma): a scheduler instance
        # configured differently (betas, spacing, prediction type) under the same class name must not reuse another schedule's plan
        scheduler.set_timesteps(num_inference_steps)
        general = bool(getattr(scheduler, "general_step", False))
        tab = scheduler.tables(t_start) if general else scheduler.tables()
        fp = hashlib.sha1()
        for k in ("timesteps", "coef", "in_scale") + (("coef6",) if general else ()):      # every table the plan reads
            v = tab.get(k)
            fp.update(b"-" if v is None else v.detach().to("cpu", torch.float64).contiguous().numpy().tobytes())
        fp.update(repr(float(tab["init_noise_sigma"])).encode())
        n = num_inference_steps
        if denoising_end is not None and isinstance(denoising_end, float) and 0 < denoising_end < 1:
            # custom_pipelines.py:303-311: stop once t falls below the cut-off; the gating window below then counts
            # the truncated list, as upstream does (image-to-image: the list from t_start on, as diffusers' img2img cuts it)
            cutoff = int(round(1000 - denoising_end * 1000))
            n = max(int((tab["timesteps"] >= cutoff).sum().item()), t_start)
        m = n - t_start                                                      # steps that run: table rows t_start .. n - 1
        # custom_pipelines.py:319-329 over the m steps that run, at rows t_start + i; the rows before t_start are never read (base
        # there, so that a text-to-image and an image-to-image call with the same window share one gating table and plan)
        gate = self.gate_table(n, t_start, control_guidance_start, control_guidance_end, base)
        # the gating table is part of what the recorded plan reads: its fingerprint is part of the key
        fp.update(torch.tensor(gate, dtype=torch.float32).numpy().tobytes())
        mode = None
        if inpaint:
            mode = "concat" if self.unet.config.in_channels == 9 else "blend"
        stochastic = general and bool(getattr(scheduler, "stochastic", False))
        seeded = bool(seeded_noise) and stochastic
        cn_gate = cn_key = None
        if self.controlnet is not None:
            if self.cn is None:
                raise L.ImhError("a ControlNet is set but no control image: set_control_image before set_schedule")
            cn_gate = self.gate_table(n, t_start, controlnet_guidance_start, controlnet_guidance_end, self.cn["scale"])
            cn_key = hashlib.sha1(torch.tensor(cn_gate, dtype=torch.float32).numpy().tobytes()).hexdigest()
        ad_gate = ad_key = None
        if self.adapter is not None:
            if self.ad is None:
                raise L.ImhError("a T2I-Adapter is set but no control image: set_adapter_image before set_schedule")
            if inpaint or t_start:
                raise NotImplementedError("the T2I-Adapter runs text-to-image schedules (image-to-image / inpainting with an adapter are not built)")
            ad_gate = self.adapter_gate_table(n, t_start, adapter_conditioning_factor)
            ad_key = (hashlib.sha1(torch.tensor(ad_gate, dtype=torch.float32).numpy().tobytes()).hexdigest(), self.ad["scale"])
        key = PlanKey(type(scheduler).__name__, int(getattr(scheduler, "num_train_timesteps", 1000)), int(num_inference_steps),
                      float(control_guidance_start), float(control_guidance_end), denoising_end, float(base), n, fp.hexdigest(),
                      controlnet=cn_key, inpaint=mode, adapter=ad_key, seeded=seeded,
                      regions=self.regions.digest() if self.regions is not None else None, freeu=getattr(self.unet, "freeu", None),
                      pag=self._pag_key())
        self.t_start = t_start
        self.inpaint = mode
        self.general = general
        self.stochastic = stochastic
        self.seeded = seeded
        hit = self._plans.get(key)
        if hit is not None:
            # a schedule this engine has run under this conditioning: its tables, time-embedding rows and recorded plan are still there
            # (the plan's launches point at them), so a preview / final alternation re-records nothing
            hit.restore(self)
            self._sched_key = key
            return
        st.t_table = tab["timesteps"].to(dev)
        st.coef_tab = tab["coef"].contiguous().to(dev) if tab.get("coef") is not None else None
        st.coef6_tab = st.hist = st.noise_bank = st.seed_rows = None
        if general:
            if tuple(tab["coef6"].shape) != (int(num_inference_steps), 6):
                raise L.ImhError(f"the scheduler's coef6 table is {tuple(tab['coef6'].shape)}, expected ({int(num_inference_steps)}, 6)")
            st.coef6_tab = tab["coef6"].to(torch.float32).contiguous().to(dev)
            if getattr(scheduler, "needs_history", False):
                st.hist = torch.zeros(self.S, 4, self.H, self.W, dtype=torch.float32, device=dev)
            if self.seeded:
                st.seed_rows = torch.zeros(self.S, 4, dtype=torch.int32, device=dev)
            elif self.stochastic:
                st.noise_bank = torch.zeros(int(num_inference_steps), self.S, 4, self.H, self.W, dtype=torch.float32, device=dev)
        st.in_scale_tab = tab["in_scale"].to(dev) if tab["in_scale"] is not None else None
        st.ip_scale_tab = torch.tensor(gate, dtype=torch.float32, device=dev)
        st.blend_tab = self.blend_table(scheduler, num_inference_steps, n).to(dev) if mode == "blend" else None
        self.cn_scale_tab = torch.tensor(cn_gate, dtype=torch.float32, device=dev) if cn_gate is not None else None
        self.ad_gate_tab = torch.tensor(ad_gate, dtype=torch.float32, device=dev) if ad_gate is not None else None
        if st.step is None:
            st.step = torch.zeros(1, dtype=torch.int32, device=dev)
        self.steps = n
        self.init_noise_sigma = float(tab["init_noise_sigma"])
        self.plan = None                         # table pointers changed
        self._sched_key = key

    @staticmethod
    def blend_table(scheduler, num_inference_steps, n):
        """fp32 [num_inference_steps, 2]: row r = scheduler.add_noise_coefficients(r + 1) -- upstream's add_noise(image_latents, noise,
        timesteps[i + 1]) after step i (DDIM: alphas_cumprod[t]; Euler after set_begin_index and one step: sigmas[step_index]) -- and
        (1, 0) from row n - 1 on: after the last step that runs (n as set_schedule counts it under denoising_end) the unmasked region
        is the image latents themselves.  The scheduler's timesteps must be set."""
        rows = [scheduler.add_noise_coefficients(r + 1) if r < n - 1 else (1.0, 0.0) for r in range(int(num_inference_steps))]
        return torch.tensor(rows, dtype=torch.float32)

    def fork(self):
        """A second engine on the SAME weights and the SAME conditioning (K/V caches, aug_emb) with its own latents,
        step counter, activation buffers and plan: lets several PNS candidates be in flight on one GPU (one HIP
        stream each), so that kernels of independent candidates fill the CUs a batch-1 kernel leaves idle."""
        e = DenoiseEngine(self.unet, self.device, self.dtype, self.use_graph)
        e._is_fork = True                        # never tunes: it may record while its parent is running on another stream
        _move(("do_cfg", "guidance", "guidance_rescale", "S", "H", "W", "T_total", "steps", "init_noise_sigma", "_cond_ctx", "cfg_role",
               "xcd_candidates", "xcd_cells", "t_start", "inpaint", "general", "stochastic", "seeded"), self, e)
        if self.pag:
            _move(("pag", "pag_scale"), self, e)
        # shared, read-only during denoising: the ControlNet's hint, caches and table, the adapter's features and gate table
        _move(("controlnet", "cn", "cn_scale_tab", "adapter", "ad", "ad_gate_tab", "regions"), self, e)
        st = StepState()
        src = self.st
        st.aug_emb, st.kv = src.aug_emb, src.kv                      # shared, read-only during denoising
        _move(_FORK_SHARED, src, st)                                 # (the mask, image latents and noise are the fork's own: _record)
        for k in _FORK_OWN:                                          # the general step's state is the fork's own, like its latents
            v = getattr(src, k)
            setattr(st, k, None if v is None else torch.zeros_like(v))
        st.step = torch.zeros(1, dtype=torch.int32, device=self.device)
        e.st = st
        return e

    def _images_in_caches(self):
        """image prompts per sample the K / V caches of the current conditioning were projected for (None: not known here)"""
        if self._cond_in is None or self.st is None or not getattr(self.st, "kv", None):
            return None
        rows = self._cond_in[0].shape[0]
        return next((int(kv.k2.shape[0]) // rows for kv in self.st.kv.values() if kv.k2 is not None), None)

    def _sync_regions(self):
        """the UNet's processors carry this engine's regions (or none) whenever it projects K / V or records: engines that share a UNet
        may differ in them"""
        from .ip_adapter import set_ip_regions
        set_ip_regions(self.unet, self.regions)

    def _record(self):
        st = self.st
        self._sync_regions()
        if st.latents is None or tuple(st.latents.shape) != (self.S, 4, self.H, self.W):
            st.latents = torch.zeros(self.S, 4, self.H, self.W, dtype=torch.float32, device=self.device)
        split = self.do_cfg and self.cfg_role is not None
        if self.inpaint and split:
            raise NotImplementedError("inpainting runs on an engine that holds both halves of the CFG pair (cfg_role = None)")
        if self.unet.config.in_channels == 9 and self.inpaint != "concat":
            raise L.ImhError("a UNet with in_channels = 9 runs inpainting schedules only (set_schedule(..., inpaint=True), prepare_inpaint)")
        want = {"blend": (("inp_z", 4), ("inp_noise", 4), ("inp_mask", 1)), "concat": (("conv_in_extra", 5),)}.get(self.inpaint, ())
        for k, c in want:
            if getattr(st, k) is None or tuple(getattr(st, k).shape) != (self.S, c, self.H, self.W):
                setattr(st, k, torch.zeros(self.S, c, self.H, self.W, dtype=torch.float32, device=self.device))
        # the time-embedding rows of every step of this schedule under this conditioning: once here, not five launches per step
        self._temb_ctx = Ctx(self.device, self.dtype)          # (its pool owns the table for the life of the plan)
        self.unet.precompute_temb(self._temb_ctx, st, st.t_table)
        cst = self._cn_temb = None
        if self.controlnet is not None:
            self._whole_pair_only(split, "ControlNet")
            if self.cn is None or self.cn.get("hint") is None or self.cn.get("cond") is None or self.cn_scale_tab is None:
                raise L.ImhError("the ControlNet branch needs set_conditioning, set_control_image and then set_schedule")
            from .controlnet import control_state
            # the UNet's latents / counter / tables, the ControlNet's conditioning.  Under an inpainting schedule too the branch reads the
            # 4-channel latents alone: a 9-channel UNet's conv_in_extra is not part of its state (diffusers' ControlNet inpainting pipeline
            # takes control_model_input before the concat), and the blend rides in the CFG + scheduler launch below as without a branch
            cst = control_state(st, self.cn["cond"])
            self.controlnet.precompute_temb(self._temb_ctx, cst, st.t_table)
            self._cn_temb = cst.temb_table
        if not split and self.use_graph and len(self.xcd_candidates) > 1 and self.xcd_cells is None:
            pk = (self.device.index or 0, self.S, self.H, self.W, str(self.dtype), bool(self.do_cfg)) + ((True,) if self.pag else ())
            if pk not in _XCD_PICK and not self._is_fork:
                _XCD_PICK[pk] = self._pick_xcd_cells()
            self.xcd_cells = _XCD_PICK[pk][0] if pk in _XCD_PICK else 0
            if pk in _XCD_PICK:
                self.xcd_times_ms = _XCD_PICK[pk][1]
        rec = Ctx(self.device, self.dtype, record=True)
        rec.xcd_cells = self.xcd_cells or 0
        control = None
        if cst is not None:
            # the ControlNet branch, then the UNet that consumes its residuals, in ONE plan on one stream: a linear capture
            control = self.controlnet.emit_forward(rec, cst, self.S, self.H, self.W, cfg_dup=self.do_cfg, hint=self.cn["hint"],
                                                   tab=self.cn_scale_tab)
        extra = {"control": control} if control is not None else {}
        if self.adapter is not None:
            self._whole_pair_only(split, "T2I-Adapter")
            if self.ad is None or self.ad_gate_tab is None:
                raise L.ImhError("the T2I-Adapter needs set_adapter_image and then set_schedule")
            img = self.ad["image"]
            if not self._image_fits(img, self.S, 8 * self.H, 8 * self.W):
                raise L.ImhError(f"adapter image {tuple(img.shape)}: one image or one per sample ({self.S}) at {8 * self.H} x {8 * self.W}")
            from .t2i_adapter import AdapterResiduals
            extra["adapter"] = AdapterResiduals(self.ad["feats"], scale=self.ad["scale"], tab=self.ad_gate_tab, step=st.step)
        if self.pag:
            if split or control is not None or self.adapter is not None:
                raise NotImplementedError("perturbed-attention guidance runs on a whole engine without a ControlNet or a T2I-Adapter")
            extra["pag"] = self.S             # [uncond | cond | perturbed]: the perturbed block reads the same S latents
        out = self.unet.emit_forward(rec, st, self.S, self.H, self.W, cfg_dup=self.do_cfg and not split, **extra)
        if split:
            # this rank's half of the noise prediction ends the forward plan; the CFG combine + scheduler step + step counter are a
            # second tiny plan over BOTH halves ([uncond | cond] = the layout the fused step reads), run after the per-step exchange
            if self.use_graph:
                rec.capture()
            pred = torch.empty((2,) + tuple(out.shape), dtype=out.dtype, device=self.device)
            tail = Ctx(self.device, self.dtype, record=True)
            self._emit_step_tail(tail, pred)
        else:
            rec.tag = 70
            pred, tail = out, rec
            self._emit_step_tail(rec, out)
        if self.use_graph:
            tail.capture()
        self.plan, self.noise_pred = rec, out
        self.plan_tail, self.np_full = (tail, pred) if split else (None, None)
        self._remember_plan()

    def _emit_step_tail(self, ctx, pred):
        """The end of a step, recorded into ctx: rescale_noise_cfg's factor where asked for (custom_pipelines.py:351-354), then ONE launch
        for the CFG combine and the scheduler step -- EW_CFG_STEP, or for the multistep / ancestral samplers EW_CFG_MSTEP with the
        six-column row, the history slot and the step's noise row (a seeded schedule: no bank, the launch generates the row from the
        samples' seed rows, imh.h imh_step_seeded); upstream's masked blend rides in either (no extra launch, no extra pass over the
        latents) -- then step++.  pred: the noise prediction, [uncond | cond] under CFG -- the forward's output, or on a cfg_role engine
        the buffer of both ranks' halves (such an engine always combines and never blends).  Under perturbed-attention guidance pred
        ends in the perturbed block and both launches run their three-term form (imh.h: i2 = 1, the PAG scale in f3 / f0)."""
        st, S, HW = self.st, self.S, self.H * self.W
        fac = None
        pag, ps = int(self.pag), self.pag_scale if self.pag else 0.0
        if self.do_cfg and self.guidance_rescale > 0.0:
            fac = ctx.new(S, dtype=torch.float32)
            ctx.ew(L.EW_CFG_RESCALE, fac, a=pred, i=(S, HW, pag, 0, 0, 0), f=(ps, 0.0, self.guidance, self.guidance_rescale), descr="cfg.rescale")
        blend = dict(x2=st.inp_z, noise=st.inp_noise, mask=st.inp_mask, blend_tab=st.blend_tab) if self.inpaint == "blend" else {}
        if self.general:
            op, tab, descr = L.EW_CFG_MSTEP, st.coef6_tab, "cfg+mstep+seeded" if self.seeded else "cfg+mstep"
            more = dict(hist=st.hist, bank=st.noise_bank, seeds=st.seed_rows if self.seeded else None)
        else:
            op, tab, descr, more = L.EW_CFG_STEP, st.coef_tab, "cfg+step", {}
        ctx.ew(op, st.latents, a=pred, w=fac, tab=tab, step=st.step, i=(S, HW, pag, int(self.do_cfg), S if blend else 0, 0),
               f=(0.0, 0.0, self.guidance, ps), descr=descr + ("+pag" if pag else "") + ("+blend" if blend else ""), **more, **blend)
        ctx.ew(L.EW_STEP_SET, st.step, i=(0, 0, 0, 0, 0, 0), descr="step++")

    def _remember_plan(self):
        if self._sched_key is None:
            return
        self._plans[self._sched_key] = PlanRecord(self)
        while len(self._plans) > self.max_cached_plans:              # (each plan keeps ~2 GB of activation buffers alive at 1024^2)
            self._plans.pop(next(iter(self._plans)))

    def _pick_xcd_cells(self):
        """Which XCD cell shape this box prefers for the GEMM / conv launches of the forward (imh_gemm_args.xcd): the byte-count model
        (0), or 4 x 2 (3) / 8 x 1 (2) cells over M x N everywhere.  Bit-identical results either way; the faster one differs from box to box
        (fresh MI355X boxes, same build: the model is 0.3 ms per forward ahead on a 19.9-ms box and 0.4 ms behind on 21.5-ms boxes,
        profiles/r04_forward_ab_xcd_cells*.json), so it is measured once per engine: each candidate's forward is recorded,
        captured and replayed a few times; the winner's plan is then recorded for real by _record()."""
        st = self.st
        times = {}
        for cells in self.xcd_candidates:
            rec = Ctx(self.device, self.dtype, record=True)
            rec.xcd_cells = cells
            self.unet.emit_forward(rec, st, self.S, self.H, self.W, cfg_dup=self.do_cfg, **({"pag": self.S} if self.pag else {}))
            rec.capture()
            ts = []
            for i in range(11):
                self.eager.ew(L.EW_STEP_SET, st.step, i=(0, 1, 0, 0, 0, 0), descr="step=0")
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); rec.replay(); e1.record()
                torch.cuda.synchronize(self.device)
                if i:                                      # the first replay is the warm-up
                    ts.append(e0.elapsed_time(e1))
            ts.sort()
            times[cells] = ts[len(ts) // 2]                # median of ten: the candidates are 1-2 % apart
            del rec
        self.xcd_times_ms = times
        return min(times, key=times.get), times

    @staticmethod
    def draw_step_noise(shape, steps, generator=None):
        """the per-step noise of a stochastic scheduler, fp32 [steps, *shape]: one randn_latents(shape, generator) call per step that
        runs, in step order -- the order in which diffusers' scheduler.step consumes the generator (a generator list: one draw per
        sample and step).  The caller makes the initial-latents draws first."""
        from .pipeline import randn_latents
        return torch.stack([randn_latents(tuple(shape), generator) for _ in range(int(steps))], 0)

    def _start_general_step(self, generator=None, step_noise=None, step_seeds=None, step_lanes=None):
        """before the loop of a plan that ends with EW_CFG_MSTEP: the history slot is zeroed (the first row that runs is first order and
        has ch = 0, but 0 * NaN is NaN: stale contents must not be relied on to be finite), and a stochastic scheduler's noise goes into
        rows t_start .. steps - 1 of the bank, so that the loop itself stays graph replays with no host work in between.  Under a seeded
        schedule there is no bank: the samples' seed rows (16 bytes each) are copied instead, and generator / step_noise are refused."""
        st = self.st
        if not self.seeded and (step_seeds is not None or step_lanes is not None):
            raise L.ImhError("step_seeds= / step_lanes= need a seeded schedule: set_schedule(..., seeded_noise=True) with a stochastic scheduler")
        if self.seeded:
            if generator is not None or step_noise is not None:
                raise L.ImhError("a seeded schedule takes its step noise from step_seeds=: generator= / step_noise= are refused")
            if step_seeds is None:
                raise L.ImhError("a seeded schedule needs step_seeds= (one 64-bit seed per sample)")
            from .noise import seed_rows
            step_seeds = list(step_seeds) if isinstance(step_seeds, (list, tuple)) else [step_seeds]
            if len(step_seeds) != self.S:
                raise L.ImhError(f"{len(step_seeds)} step_seeds for {self.S} samples")
            rows = seed_rows(step_seeds, step_lanes)                     # ValueError: a seed outside [0, 2**64)
            st.seed_rows.copy_(torch.from_numpy(rows.view("int32")))
        if st.hist is not None:
            st.hist.zero_()
        if self.seeded:
            return
        if not self.stochastic:
            if step_noise is not None:
                raise L.ImhError("step_noise= is for stochastic schedulers; this schedule draws no noise")
            return
        m = self.steps - self.t_start
        shape = (self.S, 4, self.H, self.W)
        if step_noise is None:
            step_noise = self.draw_step_noise(shape, m, generator)
        if tuple(step_noise.shape) != (m,) + shape:
            raise L.ImhError(f"step_noise {tuple(step_noise.shape)} for {m} steps of {shape}")
        st.noise_bank[self.t_start:self.steps].copy_(step_noise.to(self.device, torch.float32))

    @torch.no_grad()
    def denoise_cfg_split(self, latents, exchange, step_seeds=None, step_lanes=None):
        """One candidate's denoise shared by TWO ranks (engines with cfg_role 0 and 1 on the same conditioning and noise): per step
        each runs the UNet on its half of the CFG pair, `exchange(mine [S*HW*4...]) -> (uncond, cond)` swaps the halves (pns.
        pair_exchange: one all_gather of [S, HW, 4] values over xGMI), and both apply the identical combine + scheduler step, so
        the latents stay bit-equal on the two ranks without further traffic.  The two-stage PNS tail (assets/1.png: the judged-best
        noise x the full denoise) is then `steps` batch-S forwards deep instead of batch-2S ones.
        A multistep scheduler's tail plan ends with the same EW_CFG_MSTEP as the one-rank plan.  Stochastic schedulers (SDE-DPM-Solver++,
        Euler ancestral) are refused here under a bank schedule: the two ranks would have to fill identical noise banks.  Under a seeded
        schedule (set_schedule(..., seeded_noise=True)) with ``step_seeds`` they run: the tail plan ends with the seeded step on both
        ranks, and each generates the identical noise from the seeds without talking."""
        if self.cfg_role is None or not self.do_cfg:
            raise L.ImhError("denoise_cfg_split needs an engine whose conditioning was set with cfg_role = 0 / 1 and guidance > 1")
        if self.stochastic and not (self.seeded and step_seeds is not None):
            raise NotImplementedError("denoise_cfg_split does not run stochastic schedulers: both ranks would need identical noise banks "
                                      "(a seeded schedule with step_seeds= needs none)")
        if self.t_start or self.inpaint:
            raise NotImplementedError("denoise_cfg_split runs whole text-to-image schedules (t_start = 0, no inpainting)")
        self._check_weights_epoch()
        if self.plan is None:
            self._record()
        st = self.st
        st.latents.copy_(latents.to(self.device, torch.float32) * self.init_noise_sigma)
        if self.general:
            self._start_general_step(step_seeds=step_seeds, step_lanes=step_lanes)
        elif step_seeds is not None:
            raise L.ImhError("step_seeds= need a seeded schedule: set_schedule(..., seeded_noise=True) with a stochastic scheduler")
        self.eager.ew(L.EW_STEP_SET, st.step, i=(0, 1, 0, 0, 0, 0), descr="step=0")
        for _ in range(self.steps):
            self.plan.replay()
            un, co = exchange(self.noise_pred)
            self.np_full[0].copy_(un); self.np_full[1].copy_(co)
            self.plan_tail.replay()
        return st.latents

    @torch.no_grad()
    def prepare_img2img(self, moments, n1, n2, scaling, add_a, add_b):
        """image-to-image initial latents (diffusers StableDiffusionXLImg2ImgPipeline.prepare_latents) written straight into the engine's
        latent buffer by one fused fp32 launch: add_a * scaling * (mean + std * n1) + add_b * n2.  moments: the VAE's quant_conv output
        NHWC [M, h, w, 8] fp32 (M images; sample s reads s % M), n1: posterior noise [N, 4, h, w] (sample s reads s % N), n2: the
        add-noise noise [S, 4, h, w]; (add_a, add_b) = scheduler.add_noise_coefficients(t_start).  Then denoise(None)."""
        if self.plan is None:
            self._record()
        st = self.st
        dev = self.device
        self.eager.img2img_init(st.latents, moments.to(dev, torch.float32).contiguous(), n1.to(dev, torch.float32).contiguous(),
                                n2.to(dev, torch.float32).contiguous(), scaling, add_a, add_b)
        return st.latents

    @torch.no_grad()
    def prepare_inpaint(self, moments, n1, n2, scaling, add_a, add_b, mask, strength_max=False, masked_moments=None, n3=None):
        """inpainting state and initial latents (diffusers StableDiffusionXLInpaintPipeline.prepare_latents / prepare_mask_latents), copied
        into the buffers the recorded plan points at; under set_schedule(..., inpaint=True).  moments / n1 / n2 / scaling as
        prepare_img2img; mask: the latent mask [M, 1, h, w] of zeros and ones (1 = repaint; sample s reads mask s % M).
        Initial latents: add_noise(z, n2, t_start) = add_a * z + add_b * n2, or with strength_max (upstream's is_strength_max, strength
        == 1) n2 * init_noise_sigma.  4-channel UNet: the image latents z (the init op with (a, b) = (1, 0)), n2 and the mask feed the
        blend of every step.  9-channel UNet: masked_moments / n3 = the encoder moments and posterior noise of the masked image; conv_in
        reads [mask | scaling * posterior sample] at every step (moments / n1 may be None with strength_max: nothing reads z).
        Then denoise(None)."""
        if not self.inpaint:
            raise L.ImhError("prepare_inpaint needs an inpainting schedule: set_schedule(..., inpaint=True)")
        if self.plan is None:
            self._record()
        st, dev = self.st, self.device
        f32 = lambda t: t.to(dev, torch.float32).contiguous()
        S, H, W = self.S, self.H, self.W
        if mask.dim() != 4 or tuple(mask.shape[1:]) != (1, H, W) or S % mask.shape[0]:
            raise L.ImhError(f"prepare_inpaint: latent mask {tuple(mask.shape)} for {S} samples of {H} x {W}")
        mask = f32(mask).repeat(S // mask.shape[0], 1, 1, 1)
        n2 = f32(n2)
        if strength_max:
            st.latents.copy_(n2 * self.init_noise_sigma)
        else:
            self.eager.img2img_init(st.latents, f32(moments), f32(n1), n2, scaling, add_a, add_b)
        if self.inpaint == "blend":
            self.eager.img2img_init(st.inp_z, f32(moments), f32(n1), n2, scaling, 1.0, 0.0, descr="inpaint.z")
            st.inp_noise.copy_(n2)
            st.inp_mask.copy_(mask)
        else:
            if masked_moments is None or n3 is None:
                raise L.ImhError("prepare_inpaint: a 9-channel UNet needs the masked image's moments and posterior noise")
            mz = torch.empty(S, 4, H, W, dtype=torch.float32, device=dev)
            self.eager.img2img_init(mz, f32(masked_moments), f32(n3), n2, scaling, 1.0, 0.0, descr="inpaint.masked_z")
            st.conv_in_extra[:, :1].copy_(mask)
            st.conv_in_extra[:, 1:].copy_(mz)
        return st.latents

    @torch.no_grad()
    def denoise(self, latents, callback=None, callback_steps=1, generator=None, step_noise=None, step_seeds=None, step_lanes=None):
        """latents: [S, 4, H/8, W/8] unit-variance noise (CPU or device), or None: the latent buffer already holds the initial latents
        (prepare_img2img).  Runs the steps t_start .. steps - 1 of the schedule (t_start = 0 unless set_schedule was given one).  Returns
        final fp32 latents (output_type='latent' of custom_pipelines.py:365-379).  callback(i, t, latents) every ``callback_steps``
        steps (:359-363; i counts the steps that run from 0) is the only thing that makes the host wait inside the loop.
        A stochastic scheduler (SDE-DPM-Solver++, Euler ancestral) reads one noise row per step: ``step_noise``, fp32 [steps that run,
        S, 4, H/8, W/8], or drawn here from ``generator`` (draw_step_noise: one randn_latents call per step, in step order, after the
        caller's initial-latents draws -- diffusers' order; None: torch's global generator, as diffusers).  It is copied into the
        device noise bank BEFORE the loop (about 8 MB per sample for 30 steps at 1024^2), so the loop is still graph replays only.
        Under a seeded schedule (set_schedule(..., seeded_noise=True)) ``step_seeds`` is required instead: one integer in [0, 2**64) per
        sample, with ``step_lanes`` (default 0 each; the sample indices where one seed serves the batch).  16 bytes per sample are copied,
        nothing is drawn; generator= / step_noise= are refused there, and step_seeds= anywhere else."""
        if self.cfg_role is not None and self.do_cfg:
            raise L.ImhError("this engine holds one half of the CFG pair (cfg_role): use denoise_cfg_split")
        self._check_weights_epoch()
        if self.inpaint and latents is not None:
            raise L.ImhError("an inpainting schedule starts from prepare_inpaint: denoise(None)")
        if self.plan is None:
            if latents is None:
                raise L.ImhError("denoise(None) needs the initial latents in place (prepare_img2img / prepare_inpaint) under the current schedule")
            self._record()
        st = self.st
        if latents is not None:
            st.latents.copy_(latents.to(self.device, torch.float32) * self.init_noise_sigma)     # prepare_latents :255-265
        t0 = self.t_start
        if self.general:
            self._start_general_step(generator, step_noise, step_seeds, step_lanes)
        elif step_noise is not None:
            raise L.ImhError("step_noise= is for stochastic schedulers; this schedule draws no noise")
        elif step_seeds is not None or step_lanes is not None:
            raise L.ImhError("step_seeds= / step_lanes= need a seeded schedule: set_schedule(..., seeded_noise=True) with a stochastic scheduler")
        self.eager.ew(L.EW_STEP_SET, st.step, i=(t0, 1, 0, 0, 0, 0), descr="step=t_start")
        for i in range(t0, self.steps):                                     # :325 -- no host work per step
            self.plan.replay()
            if callback is not None and (i - t0) % callback_steps == 0:
                torch.cuda.current_stream(self.device).synchronize()
                callback(i - t0, st.t_table[i].item(), st.latents)
        return st.latents
