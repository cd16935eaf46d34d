"""CLIP text towers (CLIP-L, OpenCLIP bigG) on the HIP path: the two text encoders behind the SDXL prompt
(ip_adapter.py:285-297,308-319 -> diffusers StableDiffusionXLPipeline.encode_prompt; imagharmony_amd.text.SDXLPromptEncoder).

``CLIPTextEncoder`` has the parameter names and shapes of transformers' ``CLIPTextModel`` (``with_projection=False``) or
``CLIPTextModelWithProjection`` (``with_projection=True``), so ``load_state_dict(hf.state_dict(), strict=True)`` works, and the call
surface ``SDXLPromptEncoder`` uses: ``enc(input_ids, output_hidden_states=True)`` -> ``out[0]`` / ``.hidden_states[-2]`` /
``.last_hidden_state`` / ``.pooler_output`` / ``.text_embeds``; ``.config``; ``.parameters()`` / ``.to()`` / ``.dtype``.

``forward`` issues launches of libimh_hip.so only: one row gather for token + position embedding, per layer LayerNorm -> one
[Wq; Wk; Wv] GEMM -> ``imh_attention_enc_causal`` straight on the packed QKV buffer -> out_proj + residual -> LayerNorm -> fc1 +
(quick-)GELU -> fc2 + residual, the final LayerNorm over all rows, a second row gather for the EOS pooling and, with projection, the
bias-free text_projection GEMM.  The launch sequence is recorded once per batch size into a plan, captured into a hipGraph and replayed
on later calls; the token ids and the EOS rows live in plan-owned int32 buffers that are refilled (validated on the host) before each
replay.  The only thing left to transformers on the inference path is the tokenizer.  The layer stack, the packed QKV copies, the plan
cache and the checkpoint readers are clip_tower.py's, shared with the vision tower.
"""
from dataclasses import dataclass

import torch
import torch.nn as nn

from .clip_tower import ACT, Tower, _Encoder, config_from_any, emit_layers, layernorm, load_directory, pack_qkv, plan_record
from .ctx import Ctx


@dataclass
class CLIPTextEncoderConfig:
    vocab_size: int = 49408             # defaults: CLIP-L (openai/clip-vit-large-patch14), SDXL's text_encoder
    hidden_size: int = 768
    intermediate_size: int = 3072
    num_hidden_layers: int = 12
    num_attention_heads: int = 12
    max_position_embeddings: int = 77
    projection_dim: int = 768
    layer_norm_eps: float = 1e-5
    hidden_act: str = "quick_gelu"
    eos_token_id: int = 2               # what the published SDXL checkpoints carry: pooling at argmax(ids) (see eos_positions)

    @classmethod
    def clip_l(cls, **kw):
        """CLIP-L: hidden 768, 12 heads of 64, 12 layers, MLP 3072, quick_gelu"""
        return cls(**kw)

    @classmethod
    def open_clip_bigg(cls, **kw):
        """OpenCLIP bigG (SDXL's text_encoder_2): hidden 1280, 20 heads of 64, 32 layers, MLP 5120, erf GELU, projection 1280"""
        return cls(**{**dict(hidden_size=1280, intermediate_size=5120, num_hidden_layers=32, num_attention_heads=20,
                             projection_dim=1280, hidden_act="gelu"), **kw})

    @classmethod
    def from_any(cls, cfg):
        """from a dict (config.json, possibly a full CLIP config with a ``text_config`` section) or any object with these attributes"""
        return config_from_any(cls, cfg, "text_config")


def eos_positions(input_ids, eos_token_id):
    """the position whose final-layer-normed hidden row is the pooled output, per row of input_ids [B, L] -- transformers' rule:
    ``eos_token_id == 2`` (configs from before the id was corrected, the published SDXL ones among them): argmax of the ids, the
    end-of-text token being the largest id of the vocabulary; otherwise the FIRST position equal to ``eos_token_id`` (the padding
    may be the same token).  A row without the token pools position 0, as upstream.  Host code: -> int64 [B] on the CPU."""
    ids = torch.as_tensor(input_ids).detach().to("cpu", torch.int32)
    if eos_token_id == 2:
        return ids.argmax(dim=-1).to(torch.int64)
    return (ids == eos_token_id).to(torch.int32).argmax(dim=-1).to(torch.int64)


def normalise_keys(sd, with_projection):
    """state-dict keys in the spelling of THIS module's parameters, from either spelling of a checkpoint: transformers 4.x wrote the
    ``text_model.`` prefix for CLIPTextModel and CLIPTextModelWithProjection alike (the published SDXL checkpoints), the installed 5.x
    keeps it only under CLIPTextModelWithProjection.  A persisted ``embeddings.position_ids`` buffer is dropped, and so is a
    ``text_projection.weight`` that a tower without projection has no use for."""
    out = {}
    for k, v in sd.items():
        k = k[len("text_model."):] if k.startswith("text_model.") else k
        if k.endswith("embeddings.position_ids"):
            continue
        if k.startswith("text_projection."):
            if with_projection:
                out[k] = v
            continue
        out[("text_model." + k) if with_projection else k] = v
    return out


class _Embeddings(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.token_embedding = nn.Embedding(cfg.vocab_size, cfg.hidden_size)
        self.position_embedding = nn.Embedding(cfg.max_position_embeddings, cfg.hidden_size)


class _TextModel(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.embeddings = _Embeddings(cfg)
        self.encoder = _Encoder(cfg)
        self.final_layer_norm = nn.LayerNorm(cfg.hidden_size, eps=cfg.layer_norm_eps)


class CLIPTextEncoderOutput:
    """attribute access like transformers' output classes, and ``out[i]`` over the fields that are set, in their order:
    (last_hidden_state, pooler_output[, hidden_states]) without projection, (text_embeds, last_hidden_state[, hidden_states]) with it"""

    def __init__(self, last_hidden_state, pooler_output, text_embeds=None, hidden_states=None):
        self.last_hidden_state, self.pooler_output, self.text_embeds = last_hidden_state, pooler_output, text_embeds
        self.hidden_states, self.attentions = hidden_states, None

    def to_tuple(self):
        t = (self.last_hidden_state, self.pooler_output) if self.text_embeds is None else (self.text_embeds, self.last_hidden_state)
        return t + ((self.hidden_states,) if self.hidden_states is not None else ())

    def __getitem__(self, i):
        return getattr(self, i) if isinstance(i, str) else self.to_tuple()[i]


class CLIPTextEncoder(Tower):
    def __init__(self, config=None, with_projection=False, **kw):
        super().__init__()
        self.config = CLIPTextEncoderConfig.from_any(config) if config is not None else CLIPTextEncoderConfig(**kw)
        cfg = self.config
        if cfg.hidden_size % cfg.num_attention_heads:
            raise ValueError("hidden_size must divide by num_attention_heads")
        self.with_projection = bool(with_projection)
        if self.with_projection:        # CLIPTextModelWithProjection: text_model.* + text_projection
            self.text_model = _TextModel(cfg)
            self.text_projection = nn.Linear(cfg.hidden_size, cfg.projection_dim, bias=False)
        else:                           # CLIPTextModel (transformers 5.x): the tower's parts at the top level
            tm = _TextModel(cfg)
            self.embeddings, self.encoder, self.final_layer_norm = tm.embeddings, tm.encoder, tm.final_layer_norm
        self.requires_grad_(False)

    @property
    def tower(self):
        """the module that owns embeddings / encoder / final_layer_norm"""
        return self.text_model if self.with_projection else self

    # ------------------------------------------------------------------ construction
    @classmethod
    def from_hf(cls, module):
        """copy config and weights from a transformers ``CLIPTextModel`` / ``CLIPTextModelWithProjection`` (same device and dtype)"""
        proj = hasattr(module, "text_projection")
        enc = cls(CLIPTextEncoderConfig.from_any(module.config), with_projection=proj)
        p = next(module.parameters())
        enc.to(device=p.device, dtype=p.dtype)
        enc.load_state_dict(normalise_keys(module.state_dict(), proj), strict=True)
        return enc

    @classmethod
    def from_pretrained(cls, path, with_projection=None, device=None, dtype=None):
        """``config.json`` + ``model.safetensors`` or ``pytorch_model.bin`` of a saved ``CLIPTextModel`` / ``CLIPTextModelWithProjection``
        directory, written by transformers 4.x or 5.x (normalise_keys).  with_projection=None: as the checkpoint (it has a
        ``text_projection.weight`` or not)."""
        def make(cfg, sd):
            proj = "text_projection.weight" in sd if with_projection is None else with_projection
            return cls(CLIPTextEncoderConfig.from_any(cfg), with_projection=proj), normalise_keys(sd, proj)
        return load_directory(path, make, device, dtype)

    @property
    def dtype(self):
        return self.tower.embeddings.token_embedding.weight.dtype

    @property
    def device(self):
        return self.tower.embeddings.token_embedding.weight.device

    # ------------------------------------------------------------------ derived caches
    def _pack(self):
        """per layer ``wqkv`` [3 hidden, hidden] = [Wq; Wk; Wv] and ``bqkv`` (Tower.derived)"""
        return pack_qkv(self.tower.encoder.layers)

    # ------------------------------------------------------------------ forward
    def _refuse(self, input_ids, attention_mask, position_ids, output_attentions):
        """-> the ids on the host (int64 [B, L]); every refusal comes before a Ctx exists"""
        cfg = self.config
        if cfg.hidden_act not in ACT:
            raise NotImplementedError(f"CLIPTextEncoder: hidden_act={cfg.hidden_act!r} is not implemented ('gelu' or 'quick_gelu')")
        hd = cfg.hidden_size // cfg.num_attention_heads
        if hd % 8 or hd > 128:
            raise NotImplementedError(f"CLIPTextEncoder: head dim {hd} must be a multiple of 8 up to 128 (imh_attention_enc_causal)")
        if cfg.hidden_size % 64 or cfg.intermediate_size % 64:
            raise NotImplementedError(f"CLIPTextEncoder: hidden_size {cfg.hidden_size} and intermediate_size {cfg.intermediate_size} must "
                                      f"be multiples of 64 (the contraction step of imh_gemm)")
        if attention_mask is not None:
            raise NotImplementedError("CLIPTextEncoder: attention_mask is not implemented (SDXL's encode_prompt passes none: padding is attended)")
        if position_ids is not None:
            raise NotImplementedError("CLIPTextEncoder: position_ids is not implemented (positions are 0 .. L-1)")
        if output_attentions:
            raise NotImplementedError("CLIPTextEncoder: output_attentions is not implemented (the attention probabilities never leave the kernel)")
        if input_ids is None or input_ids.dim() != 2 or input_ids.dtype.is_floating_point or input_ids.numel() == 0:
            raise ValueError("CLIPTextEncoder: input_ids must be a non-empty integer tensor [B, L]")
        if input_ids.shape[1] > cfg.max_position_embeddings:
            raise NotImplementedError(f"CLIPTextEncoder: sequence length {input_ids.shape[1]} exceeds max_position_embeddings = "
                                      f"{cfg.max_position_embeddings}")
        ids = input_ids.detach().to("cpu", torch.int64)
        lo, hi = int(ids.min()), int(ids.max())
        if lo < 0 or hi >= cfg.vocab_size:
            raise ValueError(f"CLIPTextEncoder: token ids span [{lo}, {hi}], the vocabulary is [0, {cfg.vocab_size})")
        return ids

    def _record(self, B, Ls, ctx=None):
        """record one forward at batch size B, sequence length Ls (into ``ctx``: a recording context of the caller's, e.g. a dry one) ->
        dict(ctx, ids / eos (int32 index buffers), hidden (list of [B*Ls, hidden]), last, pooled, embeds, Ls)"""
        cfg, tm, d = self.config, self.tower, self.derived()
        heads = cfg.num_attention_heads
        ctx = ctx or Ctx(self.device, self.dtype, record=True)
        ids = ctx.zeros(B * Ls, dtype=torch.int32)     # token ids, row b * Ls + l; refilled before every replay
        eos = ctx.zeros(B, dtype=torch.int32)          # b * Ls + eos position of row b; likewise
        x = ctx.gather_rows(tm.embeddings.token_embedding.weight.detach(), ids,
                            add=tm.embeddings.position_embedding.weight.detach()[:Ls], descr="clip_text.embed")
        hidden = emit_layers(ctx, tm.encoder.layers, d["wqkv"], d["bqkv"], x, B, heads, Ls, cfg.hidden_size // heads, ACT[cfg.hidden_act],
                             causal=True, pre="clip_text.")
        ctx.tag = 99
        last = layernorm(ctx, tm.final_layer_norm, hidden[-1], "clip_text.final_layer_norm")
        pooled = ctx.gather_rows(last, eos, descr="clip_text.eos_pool")
        embeds = None
        if self.with_projection:
            embeds = ctx.gemm(pooled, self.text_projection.weight.detach(), descr="clip_text.text_projection")
        return plan_record(ctx, ids=ids, eos=eos, hidden=hidden, last=last, pooled=pooled, embeds=embeds, Ls=Ls)

    @torch.no_grad()
    def forward(self, input_ids=None, attention_mask=None, position_ids=None, output_attentions=False, output_hidden_states=False, **_):
        ids = self._refuse(input_ids, attention_mask, position_ids, output_attentions)
        cfg = self.config
        B, Ls = ids.shape
        hid = cfg.hidden_size
        rows = torch.arange(B, dtype=torch.int64) * Ls + eos_positions(ids, cfg.eos_token_id)      # < B * Ls by construction
        with torch.inference_mode(False):       # the plan's buffers outlive this call: normal tensors, also under inference_mode callers
            plan = self._plan(B, Ls=Ls)
            plan["ids"].copy_(ids.reshape(-1).to(torch.int32))
            plan["eos"].copy_(rows.to(torch.int32))
            plan["ctx"].replay()
            hs = tuple(h.view(B, Ls, hid).clone() for h in plan["hidden"]) if output_hidden_states else None
            return CLIPTextEncoderOutput(last_hidden_state=plan["last"].view(B, Ls, hid).clone(), pooler_output=plan["pooled"].clone(),
                                         text_embeds=plan["embeds"].clone() if plan["embeds"] is not None else None, hidden_states=hs)
