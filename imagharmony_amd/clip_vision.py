"""CLIP vision tower (ViT-H/14, ViT-bigG/14) on the HIP path: the image encoder behind the IP-Adapter image prompt
(ip_adapter/ip_adapter.py:81-84,163-164,411-415) and the PNS judge (imagharmony_amd.pns.ClipPreferenceJudge).

``CLIPVisionEncoder`` has the parameter names and shapes of transformers' ``CLIPVisionModelWithProjection`` (its
``vision_model.pre_layrnorm`` spelling included), so ``load_state_dict(hf.state_dict(), strict=True)`` works, and the call
surface the adapters and the judge use: ``enc(pixel_values[, output_hidden_states=True])`` -> ``.image_embeds`` /
``.last_hidden_state`` / ``.hidden_states``; ``.config``; ``.parameters()`` / ``.to()`` / ``.dtype``.

``forward`` issues launches of libimh_hip.so only: the patch embedding as a GEMM over the 14 x 14 x 3 patches (the im2col is a
torch view / reshape, K = 588 zero-padded to a multiple of 64), LayerNorm launches, one [Wq; Wk; Wv] GEMM per layer,
``imh_attention_enc`` straight on the packed QKV buffer, and the bias / erf-GELU / residual epilogues of ``imh_gemm``.  The launch
sequence is recorded once per batch size into a plan, captured into a hipGraph and replayed on later calls.  The layer stack, the packed
QKV copies, the plan cache and the checkpoint readers are clip_tower.py's, shared with the text towers.
"""
from dataclasses import dataclass
from types import SimpleNamespace

import torch
import torch.nn as nn

from . import lib as L
from .clip_tower import Tower, _Encoder, config_from_any, emit_layers, layernorm, load_directory, pack_qkv, plan_record
from .ctx import Ctx


@dataclass
class CLIPVisionEncoderConfig:
    hidden_size: int = 1664             # defaults: ViT-bigG/14, the clip_embeddings_dim = 1280 tower of IPAdapterXL
    intermediate_size: int = 8192
    num_hidden_layers: int = 48
    num_attention_heads: int = 16
    image_size: int = 224
    patch_size: int = 14
    projection_dim: int = 1280
    layer_norm_eps: float = 1e-5
    hidden_act: str = "gelu"

    @classmethod
    def vit_h(cls, **kw):
        """ViT-H/14 (IP-Adapter Plus XL): hidden 1280, 16 heads of 80, 32 layers, projection 1024"""
        return cls(**{**dict(hidden_size=1280, intermediate_size=5120, num_hidden_layers=32, num_attention_heads=16,
                             projection_dim=1024), **kw})

    @classmethod
    def vit_bigg(cls, **kw):
        """ViT-bigG/14: hidden 1664, 16 heads of 104, 48 layers, projection 1280"""
        return cls(**kw)

    @classmethod
    def from_any(cls, cfg):
        """from a dict (config.json, possibly a full CLIP config with a ``vision_config`` section) or any object with these attributes"""
        return config_from_any(cls, cfg, "vision_config")


class _Embeddings(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        n = (cfg.image_size // cfg.patch_size) ** 2 + 1
        self.class_embedding = nn.Parameter(torch.randn(cfg.hidden_size))
        self.patch_embedding = nn.Conv2d(3, cfg.hidden_size, kernel_size=cfg.patch_size, stride=cfg.patch_size, bias=False)
        self.position_embedding = nn.Embedding(n, cfg.hidden_size)


class _VisionModel(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.embeddings = _Embeddings(cfg)
        self.pre_layrnorm = nn.LayerNorm(cfg.hidden_size, eps=cfg.layer_norm_eps)      # (sic: the checkpoint's spelling)
        self.encoder = _Encoder(cfg)
        self.post_layernorm = nn.LayerNorm(cfg.hidden_size, eps=cfg.layer_norm_eps)


class CLIPVisionEncoder(Tower):
    def __init__(self, config=None, **kw):
        super().__init__()
        self.config = CLIPVisionEncoderConfig.from_any(config) if config is not None else CLIPVisionEncoderConfig(**kw)
        cfg = self.config
        if cfg.hidden_size % cfg.num_attention_heads or cfg.image_size % cfg.patch_size:
            raise ValueError("hidden_size must divide by num_attention_heads and image_size by patch_size")
        self.vision_model = _VisionModel(cfg)
        self.visual_projection = nn.Linear(cfg.hidden_size, cfg.projection_dim, bias=False)
        self.requires_grad_(False)

    # ------------------------------------------------------------------ construction
    @classmethod
    def from_hf(cls, module):
        """copy config and weights from a transformers ``CLIPVisionModelWithProjection`` (same device and dtype)"""
        enc = cls(CLIPVisionEncoderConfig.from_any(module.config))
        p = next(module.parameters())
        enc.to(device=p.device, dtype=p.dtype)
        enc.load_state_dict(module.state_dict(), strict=True)
        return enc

    @classmethod
    def from_pretrained(cls, path, device=None, dtype=None):
        """``config.json`` + ``model.safetensors`` or ``pytorch_model.bin`` of a saved ``CLIPVisionModelWithProjection`` directory"""
        def make(cfg, sd):      # embeddings.position_ids: a buffer older checkpoints persist
            return cls(CLIPVisionEncoderConfig.from_any(cfg)), {k: v for k, v in sd.items() if not k.endswith("embeddings.position_ids")}
        return load_directory(path, make, device, dtype)

    @property
    def dtype(self):
        return self.visual_projection.weight.dtype

    @property
    def device(self):
        return self.visual_projection.weight.device

    @property
    def num_positions(self):
        return (self.config.image_size // self.config.patch_size) ** 2 + 1

    # ------------------------------------------------------------------ derived caches
    PATCH_K_ALIGN = 64      # imh_gemm contracts in steps of 64: 3 * 14 * 14 = 588 -> 640

    def _pack(self):
        """packed / padded copies of the weights (Tower.derived): per layer ``wqkv`` [3 hidden, hidden] = [Wq; Wk; Wv] and ``bqkv``;
        ``patch_w`` [hidden, K'] (K = 3 p p zero-padded to a multiple of 64); ``cls_pos`` = class embedding + position row 0"""
        emb = self.vision_model.embeddings
        pw = emb.patch_embedding.weight.detach()
        k = pw[0].numel()
        kp = (k + self.PATCH_K_ALIGN - 1) // self.PATCH_K_ALIGN * self.PATCH_K_ALIGN
        patch_w = pw.new_zeros(pw.shape[0], kp)
        patch_w[:, :k] = pw.reshape(pw.shape[0], k)
        return dict(patch_w=patch_w, patch_k=k, cls_pos=(emb.class_embedding.detach() + emb.position_embedding.weight.detach()[0]).contiguous(),
                    **pack_qkv(self.vision_model.encoder.layers))

    # ------------------------------------------------------------------ forward
    def _refuse(self, pixel_values, interpolate_pos_encoding, output_attentions):
        cfg = self.config
        if cfg.hidden_act != "gelu":
            raise NotImplementedError(f"CLIPVisionEncoder: hidden_act={cfg.hidden_act!r} is not implemented (erf GELU only; "
                                      f"quick_gelu towers are out of scope)")
        if interpolate_pos_encoding:
            raise NotImplementedError("CLIPVisionEncoder: interpolate_pos_encoding is not implemented")
        if output_attentions:
            raise NotImplementedError("CLIPVisionEncoder: output_attentions is not implemented (the attention probabilities never leave the kernel)")
        if pixel_values.dim() != 4 or pixel_values.shape[1] != 3 or tuple(pixel_values.shape[-2:]) != (cfg.image_size, cfg.image_size):
            raise NotImplementedError(f"CLIPVisionEncoder: pixel_values {tuple(pixel_values.shape)} must be [B, 3, {cfg.image_size}, "
                                      f"{cfg.image_size}] (config.image_size; no position interpolation)")

    def _record(self, B, ctx=None):
        """record one forward at batch size B (into ``ctx``: a recording context of the caller's, e.g. a dry one) -> dict(ctx, patches
        (input buffer), hidden (list of [B*n, hidden]), embeds)"""
        cfg, vm, d = self.config, self.vision_model, self.derived()
        hid, heads, n, npatch = cfg.hidden_size, cfg.num_attention_heads, self.num_positions, self.num_positions - 1
        ctx = ctx or Ctx(self.device, self.dtype, record=True)
        patches = ctx.zeros(B * npatch, d["patch_w"].shape[1])         # im2col rows; the K padding stays zero
        emb = ctx.new(B * n, hid)
        pos = vm.embeddings.position_embedding.weight.detach()
        emb.view(B, n, hid)[:, 0] = d["cls_pos"]                       # class token + position 0: the same for every image and call
        for b in range(B):                                             # patch rows of image b + their position rows, in the epilogue
            ctx.gemm(patches[b * npatch:(b + 1) * npatch], d["patch_w"], out=emb[b * n + 1:(b + 1) * n], residual=pos[1:],
                     descr="clip.patch_embed")
        x = layernorm(ctx, vm.pre_layrnorm, emb, "clip.pre_layrnorm")
        hidden = emit_layers(ctx, vm.encoder.layers, d["wqkv"], d["bqkv"], x, B, heads, n, hid // heads, L.GF_ACT_GELU, causal=False, pre="clip.")
        ctx.tag = 99
        # post_layernorm is per row: normalise every row, project the class rows (row stride n * hidden)
        pl = layernorm(ctx, vm.post_layernorm, hidden[-1], "clip.post_layernorm")
        embeds = ctx.gemm(pl.view(B, n * hid)[:, :hid], self.visual_projection.weight.detach(), descr="clip.visual_projection")
        return plan_record(ctx, patches=patches, hidden=hidden, embeds=embeds)

    def _replay(self, plan, B, output_hidden_states):
        """replay a plan whose ``patches`` are filled -> the output object (clones: the next call overwrites the plan's buffers)"""
        n, hid = self.num_positions, self.config.hidden_size
        plan["ctx"].replay()
        out = SimpleNamespace(image_embeds=plan["embeds"].clone(), last_hidden_state=plan["hidden"][-1].view(B, n, hid).clone(),
                              hidden_states=None, attentions=None)
        if output_hidden_states:
            out.hidden_states = tuple(h.view(B, n, hid).clone() for h in plan["hidden"])
        return out

    @torch.no_grad()
    def forward(self, pixel_values, output_hidden_states=False, interpolate_pos_encoding=False, output_attentions=False, **_):
        self._refuse(pixel_values, interpolate_pos_encoding, output_attentions)
        if pixel_values.device != self.device or pixel_values.dtype != self.dtype:
            raise L.ImhError(f"CLIPVisionEncoder: pixel_values on {pixel_values.device} / {pixel_values.dtype}, the encoder on "
                             f"{self.device} / {self.dtype}")
        cfg = self.config
        B, p, g = pixel_values.shape[0], cfg.patch_size, cfg.image_size // cfg.patch_size
        with torch.inference_mode(False):       # the plan's buffers outlive this call: normal tensors, also under inference_mode callers
            plan = self._plan(B)
            # im2col as a view: [B, 3, g, p, g, p] -> [B, g, g, 3, p, p] = one row of 3 p p per patch, Conv2d's weight order
            rows = pixel_values.detach().reshape(B, 3, g, p, g, p).permute(0, 2, 4, 1, 3, 5).reshape(B * g * g, 3 * p * p)
            plan["patches"][:, :3 * p * p].copy_(rows)
            return self._replay(plan, B, output_hidden_states)

    @torch.no_grad()
    def embed_decoded(self, images, output_hidden_states=False):
        """decoded images [S, 3, H, W] fp32 in [-1, 1] on the encoder's device (what ``vae.decode`` returns) -> the object ``forward``
        returns for ``ClipPreferenceJudge.preprocess(images)``: one ``imh_clip_preprocess`` launch (Ctx.clip_preprocess: clamp, antialiased
        bicubic to the shortest edge, centre crop, CLIP mean / std, one rounding to the run dtype) writes the patch rows straight into the
        recorded plan's ``patches`` buffer, then the plan replays.  No torch op touches the pixels."""
        from .imageops import CLIP_MEAN, CLIP_STD
        cfg = self.config
        if cfg.hidden_act != "gelu":
            raise NotImplementedError(f"CLIPVisionEncoder: hidden_act={cfg.hidden_act!r} is not implemented (erf GELU only)")
        if images.dim() != 4 or images.shape[1] != 3:
            raise NotImplementedError(f"CLIPVisionEncoder.embed_decoded: images {tuple(images.shape)} must be [S, 3, H, W]")
        if images.device != self.device or images.dtype != torch.float32:
            raise L.ImhError(f"CLIPVisionEncoder.embed_decoded: images on {images.device} / {images.dtype}, expected {self.device} / torch.float32")
        B = images.shape[0]
        with torch.inference_mode(False):
            plan = self._plan(B)
            eager = self.__dict__.get("_eager")          # one eager context for the encoder's life, not one per preview group
            if eager is None or eager.device != self.device or eager.dtype != self.dtype:
                eager = self.__dict__["_eager"] = Ctx(self.device, self.dtype)
            eager.clip_preprocess(images.detach().contiguous(), plan["patches"], cfg.image_size, cfg.patch_size, CLIP_MEAN, CLIP_STD,
                                  descr="clip.preprocess")
            return self._replay(plan, B, output_hidden_states)
