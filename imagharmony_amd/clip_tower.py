"""What the two CLIP towers (clip_text.py, clip_vision.py) have in common: the parameter holders of the encoder stack with transformers'
names, the per-layer launch sequence, the packed [Wq; Wk; Wv] copies, the per-batch-size plan cache, and the readers of a config and of
a saved checkpoint directory.  What differs stays in the towers: the embedding front end, the tail after the last layer, the refusals."""
import json
import os
from dataclasses import fields

import torch
import torch.nn as nn

from . import lib as L
from .derived import derived

ACT = {"gelu": L.GF_ACT_GELU, "quick_gelu": L.GF_ACT_QGELU}       # config.hidden_act -> the fc1 epilogue


# ------------------------------------------------------------------ parameter holders
class _Attention(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        h = cfg.hidden_size
        self.k_proj, self.v_proj, self.q_proj, self.out_proj = nn.Linear(h, h), nn.Linear(h, h), nn.Linear(h, h), nn.Linear(h, h)


class _MLP(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.fc1 = nn.Linear(cfg.hidden_size, cfg.intermediate_size)
        self.fc2 = nn.Linear(cfg.intermediate_size, cfg.hidden_size)


class _Layer(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.self_attn = _Attention(cfg)
        self.layer_norm1 = nn.LayerNorm(cfg.hidden_size, eps=cfg.layer_norm_eps)
        self.mlp = _MLP(cfg)
        self.layer_norm2 = nn.LayerNorm(cfg.hidden_size, eps=cfg.layer_norm_eps)


class _Encoder(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.layers = nn.ModuleList([_Layer(cfg) for _ in range(cfg.num_hidden_layers)])


# ------------------------------------------------------------------ construction
def config_from_any(cls, cfg, section):
    """the config dataclass ``cls`` from an instance of it, a dict (config.json, possibly a full CLIP config with a ``section`` --
    ``text_config`` / ``vision_config`` -- whose projection_dim lives at the top level) or any object with these attributes"""
    if isinstance(cfg, cls):
        return cls(**{f.name: getattr(cfg, f.name) for f in fields(cls)})
    if isinstance(cfg, dict):
        proj = cfg.get("projection_dim")
        if section in cfg and "hidden_size" not in cfg:
            cfg = dict(cfg[section])
            if proj is not None:
                cfg["projection_dim"] = proj
        get = cfg.get
    else:
        get = lambda k, d=None: getattr(cfg, k, d)      # noqa: E731
    kw = {}
    for f in fields(cls):
        v = get(f.name, None)
        if v is not None:
            kw[f.name] = type(f.default)(v)
    return cls(**kw)


def load_directory(path, make, device=None, dtype=None):
    """``config.json`` + ``model.safetensors`` or ``pytorch_model.bin`` of a directory transformers saved -> the tower.
    ``make(config dict, state dict)`` -> (the module, the state dict in the module's key spelling); loaded strictly, then moved / cast."""
    with open(os.path.join(path, "config.json")) as f:
        cfg = json.load(f)
    st = os.path.join(path, "model.safetensors")
    if os.path.exists(st):
        from safetensors.torch import load_file
        sd = load_file(st, device="cpu")
    elif os.path.exists(os.path.join(path, "pytorch_model.bin")):
        sd = torch.load(os.path.join(path, "pytorch_model.bin"), map_location="cpu")
    else:
        raise FileNotFoundError(f"{path}: neither model.safetensors nor pytorch_model.bin")
    enc, sd = make(cfg, sd)
    enc.load_state_dict(sd, strict=True)
    if device is not None or dtype is not None:
        enc.to(device=device, dtype=dtype)
    return enc


# ------------------------------------------------------------------ emission
def pack_qkv(layers):
    """per layer ``wqkv`` [3 hidden, hidden] = [Wq; Wk; Wv] and ``bqkv`` [3 hidden]: Q, K and V of a layer come out of ONE GEMM"""
    d = dict(wqkv=[], bqkv=[])
    for ly in layers:
        a = ly.self_attn
        d["wqkv"].append(torch.cat([a.q_proj.weight, a.k_proj.weight, a.v_proj.weight], 0).detach().contiguous())
        d["bqkv"].append(torch.cat([a.q_proj.bias, a.k_proj.bias, a.v_proj.bias], 0).detach().contiguous())
    return d


def layernorm(ctx, norm, x, descr):
    return ctx.layernorm(x, norm.weight.detach(), norm.bias.detach(), norm.eps, descr=descr)


def emit_layers(ctx, layers, wqkv, bqkv, x, B, heads, n, hd, act, causal, pre):
    """the pre-LayerNorm transformer layers over x [B * n, heads * hd] (n tokens per sample): per layer LayerNorm -> one [Wq; Wk; Wv]
    GEMM -> attention straight on the packed QKV buffer -> out_proj + residual -> LayerNorm -> fc1 + ``act`` -> fc2 + residual, tagged
    1 + layer index, descr ``pre`` + name.  -> [x, every layer's output]: they all stay live (hidden_states)"""
    hid = heads * hd
    hidden = [x]
    for i, ly in enumerate(layers):
        ctx.tag = 1 + i
        t = layernorm(ctx, ly.layer_norm1, x, pre + "ln1")
        qkv = ctx.gemm(t, wqkv[i], bias=bqkv[i], descr=pre + "qkv")
        ctx.free(t)
        o = ctx.attention_enc(qkv[:, :hid], qkv[:, hid:2 * hid], qkv[:, 2 * hid:], B, heads, n, hd, causal=causal, descr=pre + "attn")
        ctx.free(qkv)
        a = ly.self_attn.out_proj
        x1 = ctx.gemm(o, a.weight.detach(), bias=a.bias.detach(), residual=x, descr=pre + "out_proj")
        ctx.free(o)
        t = layernorm(ctx, ly.layer_norm2, x1, pre + "ln2")
        f = ctx.gemm(t, ly.mlp.fc1.weight.detach(), bias=ly.mlp.fc1.bias.detach(), flags=act, descr=pre + "fc1")
        ctx.free(t)
        x = ctx.gemm(f, ly.mlp.fc2.weight.detach(), bias=ly.mlp.fc2.bias.detach(), residual=x1, descr=pre + "fc2")
        ctx.free(f)
        ctx.free(x1)
        hidden.append(x)
    return hidden


def plan_record(ctx, **rec):
    """what a tower's ``_record`` returns: the recording context, captured into a hipGraph unless IMH_GRAPHED=0 (a dry context only
    records), and the buffers the tower fills before and reads after a replay"""
    if not ctx.dry and os.environ.get("IMH_GRAPHED", "1") != "0":
        ctx.capture()
    return dict(ctx=ctx, **rec)


class Tower(nn.Module):
    """the caches of a tower: the derived copies of its weights and, per batch size, the plan recorded with them.  A subclass has
    ``_pack()`` -> the dict of derived copies and ``_record(B, ..., ctx=None)`` -> plan_record(...)"""

    def __init__(self):
        super().__init__()
        self._derived = None        # (key, dict): derived.derived's slot
        self._plans = {}            # batch size -> recorded plan

    def derived(self):
        """``_pack()``'s copies, rebuilt when any parameter changes (loaded, moved, cast or modified in place); the recorded plans hold
        pointers into them and are dropped with them"""
        ps = list(self.parameters())

        def build():
            self._plans = {}
            with torch.no_grad():
                return self._pack()
        return derived(self, "_derived", ps, build, where=[(p.dtype, p.device) for p in ps])     # (per call: no str() of 500 devices)

    def _plan(self, B, **shape):
        """the plan for batch size B, recorded now if there is none for the present weights or it was recorded at another ``shape``
        (text: the sequence length).  Call it under inference_mode(False): the plan's buffers outlive the call as normal tensors."""
        self.derived()
        plan = self._plans.get(B)
        if plan is None or any(plan[k] != v for k, v in shape.items()):
            plan = self._plans[B] = self._record(B, **shape)
        return plan
