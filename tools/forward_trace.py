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

``python tools/forward_trace.py --args [out.json]`` writes ``tests/golden/forward_args.json``: per forward case and per ``direct/...`` case
[launch count, SHA-1] over the exact arguments of every launch (``args_digest``): every scalar field, every pointer as (allocation,
byte offset), the prefetch fields -- taken at the commit before Ctx got one recorder and shared argument packers.

Per model (``model/...``): SHA-1 of ``list(state_dict())``, of ``list(attn_processors)`` and of the names ``attn2_modules()`` yields --
parameter names and processor order.

Cases: the 13 geometries of ``tests/forward_recordings.RESOLUTIONS`` under the default switches; each of the module switches that
build the reference side of a GPU comparison (FOLD_LAYERNORM, GN_FUSE, GN_STATS_HANDOVER, and the last two together: the ``own_stats``
configuration of tests/test_gpu_gnstats.py) off at (1, 128, 128) and (1, 112, 144); the 9-channel inpainting UNet; the ControlNet
branch followed by the UNet that consumes it, in one context; the T2I-Adapter's four injections.  ``--args`` only: ``direct/...``, single calls of the Ctx
methods, one per branch of an argument packer that no forward above reaches (``DIRECT``)."""
import bisect
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
from imagharmony_amd import lib as L                                           # noqa: E402
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


def _values(a, where):
    """every field of an argument struct in _fields_ order (a nested struct's in place): a pointer as where(address), the rest as it is"""
    out = []
    for name, typ in a._fields_:
        v = getattr(a, name)
        if typ is C.c_void_p:
            out.append(where(v))
        elif isinstance(typ, type) and issubclass(typ, C.Structure):
            out.extend(_values(v, where))
        else:
            out.append(v)
    return out


def args_digest(ctx):
    """-> (launch count, SHA-1) over the exact arguments of every recorded launch, prefetch fields included: per ``ctx._ops`` row the plan
    kind and every field of its struct(s); a pointer as None or (ordinal of the allocation it lies in, byte offset), the allocations being
    the storages of ``ctx.keep`` numbered by first appearance here.  A pointer into no allocation is an error of this tool."""
    ctx.finalize_prefetch()
    spans = {}
    for t in ctx.keep:
        st = t.untyped_storage()
        if st.nbytes():
            spans[st.data_ptr()] = st.nbytes()
    bases = sorted(spans)
    ordinal = {}

    def where(p):
        if not p:
            return None
        i = bisect.bisect_right(bases, p) - 1
        if i < 0 or p >= bases[i] + spans[bases[i]]:
            raise RuntimeError(f"args_digest: launch {len(rows)} holds the pointer {p:#x}, which lies in no tensor the context keeps")
        return ordinal.setdefault(bases[i], len(ordinal)), p - bases[i]

    rows = []
    for kind, a, _cold in ctx._ops:
        rows.append([int(kind)] + [v for s in (list(a) if isinstance(a, C.Array) else [a]) for v in _values(s, where)])
    return len(rows), hashlib.sha1(repr(rows).encode()).hexdigest()


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
    def run(what=describe):
        old = {k: getattr(U, k) for k in (flags or {})}
        try:
            for k, v in (flags or {}).items():
                setattr(U, k, v)
            return what(FR.record_forward(unet(), S, Hl, Wl, DTYPE))
        finally:
            for k, v in old.items():
                setattr(U, k, v)
    return run


def unet9_case(S, Hl, Wl):
    def run(what=describe):
        u = unet(9)
        B = 2 * S
        ctx = Ctx("cpu", DTYPE, record=True, dry=True)
        st = u.prepare_conditioning(ctx, torch.zeros(B, 81, 2048), torch.zeros(B, 1280), torch.zeros(B, 6))
        st.t_value = torch.zeros(B)
        st.latents = torch.zeros(S, 4, Hl, Wl)
        st.conv_in_extra = torch.zeros(S, 5, Hl, Wl)
        u.emit_forward(ctx, st, S, Hl, Wl, cfg_dup=True)
        return what(ctx)
    return run


def controlnet_case(S, Hl, Wl):
    """the branch, then the UNet with control=, in one context (tests/test_controlnet_host.py::_record at full width)"""
    def run(what=describe):
        from imagharmony_amd.controlnet import control_state
        u, cn = unet(), controlnet()
        ctx = Ctx("cpu", DTYPE, record=True, dry=True)
        st, cond = _conditioned(u, ctx, S, Hl, Wl)
        cst = control_state(st, cn.prepare_conditioning(ctx, *cond))
        hint = torch.zeros(1, Hl, Wl, u.config.block_out_channels[0], dtype=DTYPE)
        control = cn.emit_forward(ctx, cst, S, Hl, Wl, hint=hint, tab=torch.zeros(4))
        u.emit_forward(ctx, st, S, Hl, Wl, cfg_dup=True, control=control)
        return what(ctx)
    return run


def adapter_case(S, Hl, Wl):
    def run(what=describe):
        from imagharmony_amd.t2i_adapter import AdapterResiduals
        u = unet()
        ctx = Ctx("cpu", DTYPE, record=True, dry=True)
        st, _ = _conditioned(u, ctx, S, Hl, Wl)
        feats = [torch.zeros(1, Hl // d, Wl // d, ch, dtype=DTYPE) for d, ch in zip((2, 2, 4, 4), (320, 640, 1280, 1280))]
        u.emit_forward(ctx, st, S, Hl, Wl, cfg_dup=True, adapter=AdapterResiduals(feats, scale=0.75, tab=torch.zeros(4), step=st.step))
        return what(ctx)
    return run


# ------------------------------------------------------------------------------------------------------------------ the direct-call cases
# What the model forwards above never call (or never with these arguments): each case is one dry context and zero tensors of the smallest
# shape the packer takes, one case per branch of the packer's code.  The product runs several of them eagerly; the packers are the same.
def _z(*shape, dtype=DTYPE):
    return torch.zeros(*shape, dtype=dtype)


def _f(*shape):
    return torch.zeros(*shape, dtype=torch.float32)


def _i(*shape):
    return torch.zeros(*shape, dtype=torch.int32)


def _ln(n=64):
    return _f(n), _f(n), 1e-5


def _gs(B, C_, sub=4, nblk=1):
    from imagharmony_amd.ctx import GnStats
    return GnStats(_f(B, nblk, C_ // sub, 2), nblk, sub, 0, C_)


def _spec(srcs, groups=16):
    from imagharmony_amd.ctx import GnSpec
    n = sum(g.C for g in srcs)
    return GnSpec(srcs, _z(n), _z(n), groups, 1e-5)


def _xattn(ctx, regions, **kw):
    """one 64-query, 64-key, one-head fused cross-attention with a second key set of 64 (per image)"""
    n = kw.pop("n_img", 1)
    a = (_z(64, 64), _z(64, 64), _z(64, 64), _z(64, 64), _z(64, 64), 1, 1, 64, 64, 64, 64, 64, 0.125)
    if regions:
        return ctx.cross_attention_regions(*a, _z(n * 64, 64), _z(64, n * 64), 64, 64, 64, n * 64, n, _f(n, 64), **kw)
    return ctx.cross_attention(*a, **kw)


def _attn(ctx, **kw):
    return ctx.attention(_z(64, 64), _z(64, 64), _z(64, 64), _z(64, 64), 1, 1, 64, 64, 64, 64, 64, 64, 64, 0.125, **kw)


def _halo_conv(ctx, gn, two):
    x, x2 = _z(1, 16, 16, 64), (_z(1, 16, 16, 64) if two else None)
    return ctx.conv3x3(x, _z(160, 9 * (128 if two else 64)), cfg=(7128, 160, 1), gn=gn, x2=x2)


def _mstep(ctx, **kw):
    return ctx.ew(L.EW_CFG_MSTEP, _f(1, 4, 8, 8), a=_z(2, 8, 8, 4), tab=_f(4, 8), step=_i(1), n=256, i=(1, 64, 0, 0, 0, 0), **kw)


def _clip(ctx, dtype):
    return ctx.clip_preprocess(_f(1, 3, 16, 20), torch.zeros(1, 3 * 14 * 14 + 4, dtype=dtype), 14, 14, (0.5, 0.4, 0.3), (0.2, 0.3, 0.4))


DIRECT = {
    "gemm/ln_row_own_stats": lambda c: c.gemm(_z(64, 64), _z(64, 64), flags=L.GF_LN_ROW, ln=_ln(), cfg=(64, 64, 1)),
    "gemm/ln_col_own_stats": lambda c: c.gemm(_z(64, 64), _z(128, 64), flags=L.GF_LN_COL, ln=_ln(), cfg=(64, 64, 1)),
    "gemm/split_k": lambda c: c.gemm(_z(64, 128), _z(64, 128), bias=_z(64), cfg=(64, 64, 2)),
    "gemm/stats_out_epilogue": lambda c: c.gemm(_z(64, 64), _z(128, 64), stats_out=True, cfg=(64, 64, 1)),
    "gemm/stats_out_no_epilogue": lambda c: c.gemm(_z(64, 64), _z(128, 64), stats_out=True, cfg=(8256, 128, 1)),
    "gemm/stats_out_split_k": lambda c: c.gemm(_z(64, 128), _z(128, 128), stats_out=True, cfg=(64, 64, 2)),
    "gemm/out_f32": lambda c: c.gemm(_z(64, 64), _z(64, 64), flags=L.GF_OUT_F32, out_dtype=torch.float32, cfg=(64, 64, 1)),
    "gemm_dual/plain": lambda c: c.gemm_dual(dict(x=_z(64, 64), w=_z(64, 64)), dict(x=_z(64, 64), w=_z(64, 64), bias=_z(64))),
    "gemm_dual/ln_own_stats": lambda c: (lambda x: c.gemm_dual(dict(x=x, w=_z(64, 64), flags=L.GF_LN_ROW, ln=_ln()),
                                                               dict(x=_z(64, 64), w=x, flags=L.GF_LN_COL, ln=_ln())))(_z(64, 64)),
    "gemm_dual/ln_caller_stats": lambda c: (lambda x, st: c.gemm_dual(dict(x=x, w=_z(64, 64), flags=L.GF_LN_ROW, ln=_ln() + (st,)),
                                                                      dict(x=_z(64, 64), w=x, flags=L.GF_LN_COL, ln=_ln() + (st,))))(
        _z(64, 64), (_f(64, 1, 2), 1)),
    "conv3x3/pad1_stride2": lambda c: c.conv3x3(_z(1, 4, 6, 64), _z(64, 576), bias=_z(64), stride=2, pad=1, cfg=(64, 64, 1)),
    "conv3x3/gn_table": lambda c: _halo_conv(c, (_f(1, 64, 2), True), False),
    "conv3x3/gn_spec": lambda c: _halo_conv(c, (_spec([_gs(1, 64)]), False), False),
    "conv3x3/gn_spec_two_sources": lambda c: _halo_conv(c, (_spec([_gs(1, 64), _gs(1, 64, nblk=2)]), True), True),
    "attention/plain": _attn,
    "attention/k2_scale_tab": lambda c: _attn(c, k2=_z(64, 64), vt2=_z(64, 64), Lk2=4, Lk2_pad=64, ldk2=64, ldvt2=64, scale2=0.5,
                                              scale2_tab=_f(4), step=_i(1)),
    "cross_attention/ln_own_stats": lambda c: _xattn(c, False, ln=_ln()),
    "cross_attention_regions/plain": lambda c: _xattn(c, True),
    "cross_attention_regions/weights_ln_own_stats": lambda c: _xattn(c, True, n_img=2, weights=_f(2), ln=_ln(), scale2_tab=_f(4), step=_i(1)),
    "cross_attention_regions/ln_caller_stats": lambda c: _xattn(c, True, ln=_ln() + ((_f(64, 1, 2), 1),)),
    "attention_small": lambda c: c.attention_small(_z(8, 32), _z(12, 32), _z(12, 48), 2, 2, 4, 6, 16, 24, 0.25),
    "attention_enc/full": lambda c: (lambda qkv: c.attention_enc(qkv[:, :32], qkv[:, 32:64], qkv[:, 64:], 1, 1, 64, 32))(_z(64, 96)),
    "attention_enc/causal": lambda c: c.attention_enc(_z(64, 32), _z(64, 32), _z(64, 32), 1, 1, 64, 32, scale=0.5, causal=True),
    "gn_stats": lambda c: c.gn_stats(_z(1, 8, 8, 32), sub=2),
    "gn_table/one_source": lambda c: c.gn_table(_gs(1, 32, 2), _z(32), _z(32), 16, 1e-5, 64),
    "gn_table/two_sources": lambda c: c.gn_table([_gs(1, 64), _gs(1, 32, nblk=2)], None, None, 8, 1e-6, 64),
    "gn_apply": lambda c: c.gn_apply(_z(1, 8, 8, 32), _f(1, 32, 2), True),
    "gn_table_apply/two_sources": lambda c: c.gn_table_apply(_z(1, 64, 96), _spec([_gs(1, 64), _gs(1, 32, nblk=2)], 8), True),
    "groupnorm/own_stats": lambda c: c.groupnorm(_z(1, 64, 32), _z(32), _z(32), 16, 1e-5, True),
    "groupnorm/caller_stats": lambda c: c.groupnorm(_z(1, 64, 32), _z(32), _z(32), 16, 1e-5, False, stats=_gs(1, 32, 2)),
    "layernorm": lambda c: c.layernorm(_z(2, 32, 64), _z(64), _z(64), 1e-5),
    "ew/mstep_hist_bank": lambda c: _mstep(c, hist=_f(1, 4, 8, 8), bank=_f(4, 1, 4, 8, 8), f=(5.0, 0.0, 0.0, 0.0)),
    "ew/mstep_seeds": lambda c: _mstep(c, hist=_f(1, 4, 8, 8), seeds=_i(1, 4), noise_stream=3),
    "ew/x2_noise_mask_blend_tab": lambda c: _mstep(c, x2=_f(1, 5, 8, 8), noise=_f(1, 4, 8, 8), mask=_f(1, 1, 8, 8), blend_tab=_f(4, 2)),
    "randn_seeded/raw": lambda c: c.randn_seeded(_i(1, 4), 64, row=7, noise_stream=2, raw=True),
    "randn_seeded/step": lambda c: c.randn_seeded(_i(2, 4), 64, step=_i(1)),
    "clip_preprocess/bf16": lambda c: _clip(c, torch.bfloat16),
    "clip_preprocess/f16": lambda c: _clip(c, torch.float16),
    "clip_preprocess/f32": lambda c: _clip(c, torch.float32),
    "control_add/plain": lambda c: c.control_add(_z(2, 8, 8, 32), _z(1, 8, 8, 32), scale=0.5),
    "control_add/tab_gn_sub": lambda c: c.control_add(_z(2, 8, 8, 32), _z(1, 8, 8, 32), tab=_f(4), step=_i(1), gn_sub=2),
    "gather_rows/plain": lambda c: c.gather_rows(_z(16, 64), _i(8)),
    "gather_rows/add": lambda c: c.gather_rows(_z(16, 64), _i(8), add=_z(4, 64)),
    "concat": lambda c: c.concat(_z(1, 8, 8, 32), _z(1, 8, 8, 64)),
    "silu": lambda c: c.silu(_z(2, 64)),
}


def direct_case(call):
    def run(what=describe):
        ctx = Ctx("cpu", DTYPE, record=True, dry=True)
        call(ctx)
        return what(ctx)
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


def digest(ctx):
    return list(args_digest(ctx))


def args_cases():
    """{case name: a function that records it and returns [launch count, SHA-1] of args_digest}: every forward case of cases() and the
    direct-call cases"""
    runs = {name: run for name, run in cases().items() if not name.startswith("model/")}
    runs.update({f"direct/{name}": direct_case(call) for name, call in DIRECT.items()})
    return {name: (lambda run=run: run(what=digest)) for name, run in runs.items()}


def trace():
    with torch.no_grad():
        return {name: run() for name, run in cases().items()}


if __name__ == "__main__":
    if sys.argv[1:2] == ["--args"]:                  # python tools/forward_trace.py --args [out.json]: tests/golden/forward_args.json
        del sys.argv[1]
        with torch.no_grad():
            trace = lambda: {name: run() for name, run in args_cases().items()}        # noqa: E731
            text = "{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in sorted(trace().items())) + "\n}\n"
    else:
        text = "{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, sort_keys=True)}" for k, v in sorted(trace().items())) + "\n}\n"
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
