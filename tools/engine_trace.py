"""CPU only: what a real ``DenoiseEngine`` records and caches, on a tiny UNet with uninitialised weights and dry recording contexts.

    python tools/engine_trace.py [out.json]

Every ``Ctx`` the engine makes is a dry recording one (the name ``Ctx`` of the ``denoise`` module is replaced; ``use_graph=False``, so
nothing captures and the XCD pick never runs).  ``tests/golden/engine_trace.json`` is this tool's output at the commit before the engine
got one plan record and one step tail; ``tests/test_engine_trace_host.py`` compares case by case.

``python tools/engine_trace.py --args [out.json]`` writes ``tests/golden/engine_args.json``: per plan case and plan (the tail plan of a
``cfg_role`` engine second) the launch count and the SHA-1 over the exact arguments of every launch (tools/forward_trace.py
args_digest), taken at the commit before Ctx got one recorder and shared argument packers.

Per plan case: the launch count of the forward part and a SHA-1 over its (tag, kind, descr, shape, epilogue) list; in clear, every op
from the first tail op on (``cfg.rescale`` or ``cfg+...``), of both plans of a ``cfg_role`` engine: kind, element-wise op code, descr,
tag, i0..i5, f0..f3 and every pointer field resolved to the NAME of the engine buffer it points at (null: a null pointer, "?": none of
the named buffers); the plan key as a list, and steps / t_start / inpaint / general / stochastic / seeded.

Two things do not record dry and are replaced on the model objects: ``ControlNetModel.prepare_hint`` and ``T2IAdapter.
prepare_features`` refuse a recording context (they are eager, once per image), so the tool's models return zero tensors of the shapes
those would return.  The engine's calls are the real ones.

Two sequence cases are event lists: the plan cache (hits, eviction order, what set_control_image / set_adapter_image / set_conditioning
drop) and ``fork()`` (per engine and StepState attribute: the same object, a fresh zero tensor of the same shape, an equal value, or
the fork's own object; attributes that are None or absent on both sides are left out, and so is the eager context)."""
import hashlib
import json
import os
import sys
from unittest import mock

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from forward_trace import args_digest                                          # noqa: E402
from imagharmony_amd import denoise as D                                       # noqa: E402
from imagharmony_amd import lib as L                                           # noqa: E402
from imagharmony_amd import schedulers as hs                                   # noqa: E402
from imagharmony_amd.ctx import Ctx                                            # noqa: E402

DTYPE, SIDE, TOKENS = torch.bfloat16, 256, 4
PTR_FIELDS = ("a", "b", "y", "w", "bias", "tab", "step", "x2", "noise", "mask", "blend_tab")
ST_BUFFERS = ("latents", "coef_tab", "coef6_tab", "step", "hist", "noise_bank", "seed_rows", "inp_z", "inp_noise", "inp_mask", "blend_tab")


class DryCtx(Ctx):
    """a dry recording context whatever was asked for, which also keeps the element-wise op code of every recorded op"""

    def __init__(self, device, dtype=torch.bfloat16, record=False, dry=False):
        super().__init__("cpu", dtype, record=True, dry=True)
        self.ew_ops = {}          # op index -> element-wise op code

    def _emit(self, kind, args, ew_op=0, **kw):
        self.ew_ops[len(self.tags)] = int(ew_op)
        return super()._emit(kind, args, ew_op=ew_op, **kw)


# ------------------------------------------------------------------------------------------------------------------ models
_MODELS = {}


def _config(in_channels=4):
    from imagharmony_amd.unet import UNetConfig
    return UNetConfig(block_out_channels=(64, 128, 256), transformer_layers_per_block=(1, 1, 2), attention_head_dim=(1, 2, 4),
                      cross_attention_dim=256, addition_time_embed_dim=64, projection_class_embeddings_input_dim=128 + 6 * 64,
                      sample_size=32, in_channels=in_channels)


def unet(in_channels=4):
    key = ("unet", in_channels)
    if key not in _MODELS:
        from imagharmony_amd.ip_adapter import install_ip_processors
        from imagharmony_amd.unet import UNet2DConditionModel
        with torch.device("meta"):
            u = UNet2DConditionModel(_config(in_channels))
        u = u.to_empty(device="cpu").to(DTYPE)
        install_ip_processors(u, num_tokens=TOKENS, device="cpu", dtype=DTYPE, init="empty")
        _MODELS[key] = u
    return _MODELS[key]


def controlnet():
    if "cn" not in _MODELS:
        from imagharmony_amd.attention_processor import CNAttnProcessor2_0
        from imagharmony_amd.controlnet import ControlNetModel
        with torch.device("meta"):
            cn = ControlNetModel(_config())
        cn = cn.to_empty(device="cpu").to(DTYPE)
        cn.set_attn_processor(CNAttnProcessor2_0(num_tokens=TOKENS))
        c0 = cn.config.block_out_channels[0]
        cn.prepare_hint = lambda ctx, image, Hl, Wl: torch.zeros(image.shape[0], Hl, Wl, c0, dtype=DTYPE)
        _MODELS["cn"] = cn
    return _MODELS["cn"]


def adapter():
    if "ad" not in _MODELS:
        from imagharmony_amd.t2i_adapter import T2IAdapter
        c = (64, 128, 256, 256)
        with torch.device("meta"):
            ad = T2IAdapter(channels=c)
        ad.prepare_features = lambda ctx, image, Hl, Wl: [torch.zeros(image.shape[0], Hl // d, Wl // d, ch, dtype=DTYPE)
                                                          for d, ch in zip((2, 2, 4, 4), c)]
        _MODELS["ad"] = ad
    return _MODELS["ad"]


def control_image(shift=0):
    return (((torch.arange(3 * SIDE * SIDE) + shift) % 17).float() / 16).reshape(1, 3, SIDE, SIDE)


# ------------------------------------------------------------------------------------------------------------------ an engine
def engine(S=1, in_channels=4, guidance=5.0, rescale=0.0, cfg_role=None, cn=False, ad=False):
    u = unet(in_channels)
    eng = D.DenoiseEngine(u, "cpu", DTYPE, False)
    if cn:
        eng.set_controlnet(controlnet())
        eng.set_control_image(control_image(), 0.75)
    if ad:
        eng.set_adapter(adapter())
        eng.set_adapter_image(control_image(), 0.75)
    condition(eng, S, guidance, rescale, cfg_role)
    return eng


def condition(eng, S=1, guidance=5.0, rescale=0.0, cfg_role=None):
    cd, pd = eng.unet.config.cross_attention_dim, eng.unet.config.pooled_dim
    eng.set_conditioning(torch.zeros(S, 77 + TOKENS, cd), torch.zeros(S, 77 + TOKENS, cd), torch.zeros(S, pd), torch.zeros(S, pd), SIDE, SIDE,
                         guidance_scale=guidance, guidance_rescale=rescale, cfg_role=cfg_role)


def _is_tail(descr):
    return descr == "cfg.rescale" or descr.startswith("cfg+")


def _buffer_names(eng, ctxs):
    names = {}
    for k in ST_BUFFERS:
        t = getattr(eng.st, k, None)
        if t is not None:
            names.setdefault(t.data_ptr(), k)
    if eng.cfg_role is not None and eng.do_cfg:
        names.setdefault(eng.np_full.data_ptr(), "np_full")
    names.setdefault(eng.noise_pred.data_ptr(), "noise_pred")
    for c in ctxs:
        for t, o in zip(c.tags, c._ops):
            if t[2] == "cfg.rescale":
                names.setdefault(o[1].y, "rescale_factor")
    return names


def _op(ctx, j, names):
    tag, kind, descr = ctx.tags[j][:3]
    a = ctx._ops[j][1]
    e = a.ew if kind == L.OP_STEP_SEEDED else a
    ptr = {k: (names.get(getattr(e, k), "?") if getattr(e, k) else None) for k in PTR_FIELDS}
    if kind == L.OP_STEP_SEEDED:
        ptr["seeds"] = names.get(a.seeds, "?") if a.seeds else None
    return dict(kind=int(kind), ew_op=ctx.ew_ops[j], descr=descr, tag=int(tag), i=[e.i0, e.i1, e.i2, e.i3, e.i4, e.i5],
                f=[e.f0, e.f1, e.f2, e.f3], ptr=ptr)


def _forward(ctx, n):
    rows = [(t[0], t[1], t[2], t[5], sorted(t[6].items()) if isinstance(t[6], dict) else t[6]) for t in ctx.tags[:n]]
    return dict(launches=n, sha1=hashlib.sha1(repr(rows).encode()).hexdigest())


def plan_trace(eng, args=False):
    """records the plan of the engine's current schedule and describes it"""
    eng._record()
    split = eng.cfg_role is not None and eng.do_cfg
    rec = eng.plan
    ctxs = [rec] + ([eng.plan_tail] if split else [])
    names = _buffer_names(eng, ctxs)
    n = next((j for j, t in enumerate(rec.tags) if _is_tail(t[2])), len(rec.tags))
    out = dict(forward=_forward(rec, n), tail=[_op(rec, j, names) for j in range(n, len(rec.tags))])
    if split:
        out["plan_tail"] = [_op(eng.plan_tail, j, names) for j in range(len(eng.plan_tail.tags))]
    if args:
        out["args"] = [list(args_digest(c)) for c in ctxs]
    out["key"] = list(eng._sched_key)
    out["state"] = dict(steps=eng.steps, t_start=eng.t_start, inpaint=eng.inpaint, general=eng.general, stochastic=eng.stochastic,
                        seeded=eng.seeded)
    return out


def plan_case(scheduler, steps=4, schedule=None, **engine_kw):
    def run(args=False):
        eng = engine(**engine_kw)
        eng.set_schedule(scheduler(), steps, **(schedule or {}))
        return plan_trace(eng, args)
    return run


SDE = lambda: hs.DPMSolverMultistepScheduler(algorithm_type="sde-dpmsolver++")       # noqa: E731

PLAN_CASES = {
    "plan/ddim_g5": plan_case(hs.DDIMScheduler),
    "plan/ddim_g5_rescale0.7": plan_case(hs.DDIMScheduler, rescale=0.7),
    "plan/ddim_g1": plan_case(hs.DDIMScheduler, guidance=1.0),
    "plan/euler": plan_case(hs.EulerDiscreteScheduler),
    "plan/dpm": plan_case(hs.DPMSolverMultistepScheduler, 5),
    "plan/sde_bank": plan_case(SDE, 5),
    "plan/euler_a_bank": plan_case(hs.EulerAncestralDiscreteScheduler),
    "plan/euler_a_seeded": plan_case(hs.EulerAncestralDiscreteScheduler, schedule=dict(seeded_noise=True)),
    "plan/ddim_tstart2": plan_case(hs.DDIMScheduler, 6, dict(t_start=2)),
    "plan/blend_ddim_tstart2": plan_case(hs.DDIMScheduler, 6, dict(t_start=2, inpaint=True)),
    "plan/blend_euler_a_seeded": plan_case(hs.EulerAncestralDiscreteScheduler, 5, dict(inpaint=True, seeded_noise=True), rescale=0.7),
    "plan/concat9_ddim": plan_case(hs.DDIMScheduler, schedule=dict(inpaint=True), in_channels=9),
    "plan/split0_ddim_rescale0.7": plan_case(hs.DDIMScheduler, rescale=0.7, cfg_role=0),
    "plan/split1_euler_a_seeded": plan_case(hs.EulerAncestralDiscreteScheduler, schedule=dict(seeded_noise=True), cfg_role=1),
    "plan/controlnet_t2i": plan_case(hs.DDIMScheduler, schedule=dict(controlnet_guidance_start=0.25, controlnet_guidance_end=0.75), cn=True),
    "plan/controlnet_blend_tstart2": plan_case(hs.EulerDiscreteScheduler, 6, dict(t_start=2, inpaint=True), cn=True),
    "plan/adapter_factor0.5": plan_case(hs.DDIMScheduler, schedule=dict(adapter_conditioning_factor=0.5), ad=True),
    "plan/s2_sde_seeded_rescale0.7": plan_case(SDE, 5, dict(seeded_noise=True), S=2, rescale=0.7),
}


# ------------------------------------------------------------------------------------------------------------------ sequences
def cache_sequence():
    """max_cached_plans = 3.  A / D are recorded with the ControlNet, B / C without: A, B, A (hit), C, D (evicts A); a new control image
    leaves the plans without a ControlNet entry; then the adapter: one image under two scales, another image, a new conditioning"""
    eng = engine(cn=True)
    eng.max_cached_plans = 3
    log, seen = [], {}
    cn, ad = controlnet(), adapter()
    sched = {"A": (hs.DDIMScheduler, 4), "B": (hs.EulerDiscreteScheduler, 4), "C": (hs.DDIMScheduler, 5), "D": (hs.EulerDiscreteScheduler, 5)}

    def keys():
        return [list(k) for k in eng._plans]

    def schedule(name, what):
        cls, n = sched[name]
        eng.set_schedule(cls(), n)
        how = "hit"
        if eng.plan is None:
            how = "record"
            eng._record()
        log.append([f"schedule {name} {what}", how, f"plan#{seen.setdefault(id(eng.plan), len(seen))}", list(eng._sched_key), keys()])

    def event(name):
        log.append([name, eng.plan is None, eng._sched_key is None, keys()])

    keep = []                                     # (evicted plans stay alive, so that no later plan reuses an id)
    for name, with_cn in (("A", True), ("B", False), ("A", True), ("C", False), ("D", True)):
        eng.set_controlnet(cn if with_cn else None)
        schedule(name, "controlnet" if with_cn else "plain")
        keep.append(eng.plan)
    eng.set_controlnet(cn)
    eng.set_control_image(control_image(3), 0.5)
    event("set_control_image")
    eng.set_controlnet(None)
    eng.set_adapter(ad)
    img = control_image()
    eng.set_adapter_image(img, 1.0)
    event("set_adapter_image scale 1.0")
    feats = eng.ad["feats"]
    schedule("A", "adapter")
    keep.append(eng.plan)
    eng.set_adapter_image(img.clone(), 0.5)
    event("set_adapter_image same image, scale 0.5")
    log.append(["features kept by identity", eng.ad["feats"] is feats])
    schedule("A", "adapter")
    keep.append(eng.plan)
    eng.set_adapter_image(control_image(5), 0.5)
    event("set_adapter_image another image")
    log.append(["features kept by identity", eng.ad["feats"] is feats])
    condition(eng)
    event("set_conditioning")
    return log


def _relation(a, b):
    if a is None and b is None:
        return None
    if a is None or b is None:
        return "the engine's alone" if b is None else "the fork's alone"
    if torch.is_tensor(b):
        if a is b:
            return "same"
        if torch.is_tensor(a) and a.shape == b.shape and a.dtype == b.dtype and not b.any():
            return "zeros"
        return "own"
    if isinstance(b, (bool, int, float, str, tuple, torch.dtype, torch.device)):
        return "value" if type(a) is type(b) and a == b else f"differs: {b!r}"
    return "same" if a is b else "own"


def fork_sequence():
    eng = engine(cn=True)
    eng.set_schedule(SDE(), 5, seeded_noise=True)
    eng._record()
    eng.st.hist.fill_(1.0)
    eng.st.seed_rows.fill_(1)
    f = eng.fork()
    out = {}
    conditioners = {"controlnet", "cn", "cn_scale_tab", "adapter", "ad", "ad_gate_tab"}
    for prefix, a, b, more in (("engine", eng, f, conditioners), ("st", eng.st, f.st, set())):
        for k in sorted((set(vars(a)) | set(vars(b)) | more) - {"eager", "_eager"}):
            r = _relation(getattr(a, k, None), getattr(b, k, None))
            if r is not None:
                out[f"{prefix}.{k}"] = r
    return out


def dry(fn):
    """fn, run with every Ctx the engine makes a dry recording one"""
    def run(*a, **kw):
        with mock.patch.object(D, "Ctx", DryCtx), torch.no_grad():
            return fn(*a, **kw)
    return run


def cases():
    """{case name: a function that runs it under dry contexts and returns what it logged}"""
    out = {name: dry(fn) for name, fn in PLAN_CASES.items()}
    out["sequence/plan_cache"] = dry(cache_sequence)
    out["sequence/fork"] = dry(fork_sequence)
    return out


def trace():
    return {name: run() for name, run in cases().items()}


def args_trace():
    """{plan case: per plan [launch count, SHA-1] of args_digest}: tests/golden/engine_args.json (python tools/engine_trace.py --args)"""
    return {name: dry(fn)(args=True)["args"] for name, fn in PLAN_CASES.items()}


if __name__ == "__main__":
    if sys.argv[1:2] == ["--args"]:
        del sys.argv[1]
        trace = args_trace
    text = "{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, sort_keys=True)}" for k, v in sorted(trace().items())) + "\n}\n"
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
