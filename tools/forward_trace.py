"""CPU only: what ``UNet2DConditionModel.emit_forward`` and ``ControlNetModel.emit_forward`` record, launch for launch, at full SDXL
width with uninitialised weights under dry recording contexts.

    python tools/forward_trace.py [out.json]

``tests/golden/forward_trace.json`` is this tool's output at the commit before unet.py / controlnet.py got one encoder base class, one
GroupNorm front end and lost three A/B switches; ``tests/test_forward_trace_host.py`` compares case by case.

Per forward case (the whole recording context, step-invariant conditioning included):
  * ``launches``: the launch count;
  * ``sha1``: SHA-1 over the rows (tag, kind, descr, shape, sorted epilogue) of ``ctx.tags``;
  * ``sha1_alias``: SHA-1 over those rows plus the buffer aliasing of each launch -- every ``c_void_p`` field of the recorded argument
    struct (both structs of a two-problem launch) in ``_fields_`` order, each address replaced by the index of its first appearance in
    the recording (null stays null): which launch reads what which launch wrote, and which pool buffer is reused where;
  * ``descr``: {descr: count}, so that a mismatch can be read.

Per model (``model/...``): SHA-1 of ``list(state_dict())``, of ``list(attn_processors)`` and of the names ``attn2_modules()`` yields --
parameter names and processor order.

Cases: the 13 geometries of ``tests/forward_recordings.RESOLUTIONS`` under the default switches; each of the module switches that
build the reference side of a GPU comparison (FOLD_LAYERNORM, GN_FUSE, GN_STATS_HANDOVER, and the last two together: the ``own_stats``
configuration of tests/test_gpu_gnstats.py) off at (1, 128, 128) and (1, 112, 144); the 9-channel inpainting UNet; the ControlNet
branch followed by the UNet that consumes it, in one context; the T2I-Adapter's four injections."""
import ctypes as C
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import forward_recordings as FR                                                # noqa: E402
from imagharmony_amd import unet as U                                          # noqa: E402
from imagharmony_amd.ctx import Ctx                                            # noqa: E402

DTYPE = torch.bfloat16
AB_GEOMETRIES = ((1, 128, 128), (1, 112, 144))
AB = {"fold_layernorm_off": dict(FOLD_LAYERNORM=False),
      "gn_fuse_off": dict(GN_FUSE=False),
      "gn_stats_off": dict(GN_STATS_HANDOVER=False),
      "own_stats": dict(GN_FUSE=False, GN_STATS_HANDOVER=False)}


# ------------------------------------------------------------------------------------------------------------------ models
_MODELS = {}


def unet(in_channels=4):
    key = ("unet", in_channels)
    if key not in _MODELS:
        if in_channels == 4:
            _MODELS[key] = FR.sdxl_unet_meta(DTYPE)
        else:
            from imagharmony_amd.ip_adapter import install_ip_processors
            with torch.device("meta"):
                u = U.UNet2DConditionModel(U.UNetConfig(in_channels=in_channels))
            u = u.to_empty(device="cpu").to(DTYPE)
            install_ip_processors(u, num_tokens=4, device="cpu", dtype=DTYPE, init="empty")
            _MODELS[key] = u
    return _MODELS[key]


def controlnet():
    if "cn" not in _MODELS:
        from imagharmony_amd.attention_processor import CNAttnProcessor2_0
        from imagharmony_amd.controlnet import ControlNetModel
        with torch.device("meta"):
            cn = ControlNetModel(U.UNetConfig())
        cn = cn.to_empty(device="cpu").to(DTYPE)
        cn.set_attn_processor(CNAttnProcessor2_0(num_tokens=4))          # ONE object on every layer, as IPAdapter.set_ip_adapter installs it
        _MODELS["cn"] = cn
    return _MODELS["cn"]


# ------------------------------------------------------------------------------------------------------------------ describing a recording
def _pointers(a):
    """every c_void_p field of an argument struct in _fields_ order (a nested struct's in place)"""
    out = []
    for name, typ in a._fields_:
        if typ is C.c_void_p:
            out.append(getattr(a, name))
        elif isinstance(typ, type) and issubclass(typ, C.Structure):
            out.extend(_pointers(getattr(a, name)))
    return out


def describe(ctx):
    rows, alias, first, hist = [], [], {}, {}
    for t, o in zip(ctx.tags, ctx._ops):
        row = (t[0], t[1], t[2], t[5], sorted(t[6].items()) if isinstance(t[6], dict) else t[6])
        rows.append(row)
        structs = list(o[1]) if isinstance(o[1], C.Array) else [o[1]]
        alias.append(row + ([None if not p else first.setdefault(p, len(first)) for s in structs for p in _pointers(s)],))
        hist[t[2]] = hist.get(t[2], 0) + 1
    return dict(launches=len(rows), sha1=hashlib.sha1(repr(rows).encode()).hexdigest(),
                sha1_alias=hashlib.sha1(repr(alias).encode()).hexdigest(), descr=hist)


def _sha1_names(names):
    return hashlib.sha1("\n".join(names).encode()).hexdigest()


def model_case(get):
    def run():
        m = get()
        return dict(state_dict=_sha1_names(list(m.state_dict())), attn_processors=_sha1_names(list(m.attn_processors)),
                    attn2_modules=_sha1_names([n for n, _ in m.attn2_modules()]))
    return run


# ------------------------------------------------------------------------------------------------------------------ the forward cases
def _conditioned(u, ctx, S, Hl, Wl):
    """-> (StepState of a plan step: step counter and timestep table, conditioning inputs)"""
    B = 2 * S
    cond = (torch.zeros(B, 81, u.config.cross_attention_dim), torch.zeros(B, u.config.pooled_dim), torch.zeros(B, 6))
    st = u.prepare_conditioning(ctx, *cond)
    st.t_table, st.step = torch.zeros(4), torch.zeros(1, dtype=torch.int32)
    st.latents = torch.zeros(S, 4, Hl, Wl)
    return st, cond


def unet_case(S, Hl, Wl, flags=None):
    def run():
        old = {k: getattr(U, k) for k in (flags or {})}
        try:
            for k, v in (flags or {}).items():
                setattr(U, k, v)
            return describe(FR.record_forward(unet(), S, Hl, Wl, DTYPE))
        finally:
            for k, v in old.items():
                setattr(U, k, v)
    return run


def unet9_case(S, Hl, Wl):
    def run():
        u = unet(9)
        B = 2 * S
        ctx = Ctx("cpu", DTYPE, record=True, dry=True)
        st = u.prepare_conditioning(ctx, torch.zeros(B, 81, 2048), torch.zeros(B, 1280), torch.zeros(B, 6))
        st.t_value = torch.zeros(B)
        st.latents = torch.zeros(S, 4, Hl, Wl)
        st.conv_in_extra = torch.zeros(S, 5, Hl, Wl)
        u.emit_forward(ctx, st, S, Hl, Wl, cfg_dup=True)
        return describe(ctx)
    return run


def controlnet_case(S, Hl, Wl):
    """the branch, then the UNet with control=, in one context (tests/test_controlnet_host.py::_record at full width)"""
    def run():
        from imagharmony_amd.controlnet import control_state
        u, cn = unet(), controlnet()
        ctx = Ctx("cpu", DTYPE, record=True, dry=True)
        st, cond = _conditioned(u, ctx, S, Hl, Wl)
        cst = control_state(st, cn.prepare_conditioning(ctx, *cond))
        hint = torch.zeros(1, Hl, Wl, u.config.block_out_channels[0], dtype=DTYPE)
        control = cn.emit_forward(ctx, cst, S, Hl, Wl, hint=hint, tab=torch.zeros(4))
        u.emit_forward(ctx, st, S, Hl, Wl, cfg_dup=True, control=control)
        return describe(ctx)
    return run


def adapter_case(S, Hl, Wl):
    def run():
        from imagharmony_amd.t2i_adapter import AdapterResiduals
        u = unet()
        ctx = Ctx("cpu", DTYPE, record=True, dry=True)
        st, _ = _conditioned(u, ctx, S, Hl, Wl)
        feats = [torch.zeros(1, Hl // d, Wl // d, ch, dtype=DTYPE) for d, ch in zip((2, 2, 4, 4), (320, 640, 1280, 1280))]
        u.emit_forward(ctx, st, S, Hl, Wl, cfg_dup=True, adapter=AdapterResiduals(feats, scale=0.75, tab=torch.zeros(4), step=st.step))
        return describe(ctx)
    return run


def cases():
    """{case name: a function that records it and returns what it logged}"""
    geo = lambda g: "x".join(str(v) for v in g)        # noqa: E731
    out = {f"unet/{geo(g)}": unet_case(*g) for g in FR.RESOLUTIONS}
    for name, flags in AB.items():
        for g in AB_GEOMETRIES:
            out[f"unet/ab/{name}/{geo(g)}"] = unet_case(*g, flags=flags)
    out["unet9/1x128x128"] = unet9_case(1, 128, 128)
    for g in AB_GEOMETRIES:
        out[f"controlnet/{geo(g)}"] = controlnet_case(*g)
        out[f"adapter/{geo(g)}"] = adapter_case(*g)
    out["model/unet"] = model_case(unet)
    out["model/unet9"] = model_case(lambda: unet(9))
    out["model/controlnet"] = model_case(controlnet)
    return out


def trace():
    with torch.no_grad():
        return {name: run() for name, run in cases().items()}


if __name__ == "__main__":
    text = "{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, sort_keys=True)}" for k, v in sorted(trace().items())) + "\n}\n"
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
