"""Regional image prompts: several image prompts per sample, each with a mask over the picture and a weight -- diffusers'
``ip_adapter_masks`` with several images per adapter (``IPAdapterMaskProcessor``, ``IPAdapterAttnProcessor2_0``), on the fused
cross-attention launch of csrc/xattn_regions.hip:

    O[b, q, h] = softmax(q K_text^T) V_text + sum_i  g(step) * w_i * m_i[q] * softmax(q K_i^T) V_i

``IPRegions`` carries the N masks as fp32 ``[N, Hm, Wm]`` on the CPU and the N weights.  A layer with ``L = h * w`` query tokens reads the
masks resized to its token grid (bicubic, fp32, on the CPU, not clamped -- as diffusers does it), once per call and grid; the rows are
uploaded as fp32 ``[N, h * w]``.  None of this is on the hot path.

The grid of a layer:
  * the recorded forward knows it (the latent grid divided by the layer's down factor) and hands it over;
  * the eager ``__call__`` of a processor sees only ``L`` and takes ``token_grid(L, Hm, Wm)``: integer arithmetic on the mask's aspect
    ratio, ``h = isqrt(L * Hm // Wm)``, ``w = L // h``, and it requires ``h * w == L`` and ``h * Wm == w * Hm``.  diffusers computes
    ``int(sqrt(L / (Wm / Hm)))`` in floating point (plus one if L does not divide) and pads or truncates a mask whose grid does not
    match, with a warning; here a token count that is no grid of the mask's aspect ratio is a ``ValueError``.
"""
import hashlib
import math

import torch
import torch.nn.functional as F

MAX_IMAGES = 8          # include/imh_regions.h IMH_REGIONS_MAX_IMAGES


def token_grid(L, Hm, Wm):
    """(h, w) of a layer with L query tokens under masks of Hm x Wm: h * w == L and h : w == Hm : Wm exactly, else ValueError"""
    L, Hm, Wm = int(L), int(Hm), int(Wm)
    if L < 1 or Hm < 1 or Wm < 1:
        raise ValueError(f"token_grid: L={L}, mask {Hm} x {Wm} must be positive")
    h = math.isqrt(L * Hm // Wm)
    w = L // h if h else 0
    if h < 1 or h * w != L or h * Wm != w * Hm:
        raise ValueError(f"{L} query tokens are no grid of the masks' aspect ratio {Hm} x {Wm}")
    return h, w


def prepare_masks(masks, height, width, binarize=True):
    """diffusers' IPAdapterMaskProcessor defaults restated: grayscale; PIL input resized with Lanczos to height x width; values in
    [0, 1]; binarised at 0.5 (binarize=False keeps soft masks).  A tensor mask must already be [height, width] or [N, height, width].
    -> fp32 [N, height, width] on the CPU."""
    height, width = int(height), int(width)
    if torch.is_tensor(masks):
        masks = [masks] if masks.dim() == 2 else list(masks) if masks.dim() == 3 else None
        if masks is None:
            raise ValueError("a tensor mask is [height, width] or [N, height, width]")
    elif not isinstance(masks, (list, tuple)):
        masks = [masks]
    out = []
    for m in masks:
        if torch.is_tensor(m):
            if tuple(m.shape) != (height, width):
                raise ValueError(f"a tensor mask must already be [{height}, {width}], got {tuple(m.shape)}")
            t = m.detach().to("cpu", torch.float32)
        else:
            import numpy as np
            from PIL import Image
            if not isinstance(m, Image.Image):
                raise ValueError(f"a mask is a PIL image or a tensor, not {type(m).__name__}")
            im = m.convert("L").resize((width, height), resample=Image.LANCZOS)
            t = torch.from_numpy(np.asarray(im, dtype=np.float32) / 255.0)
        if binarize:
            t = (t >= 0.5).to(torch.float32)
        out.append(t.contiguous())
    if not 1 <= len(out) <= MAX_IMAGES:
        raise ValueError(f"{len(out)} masks: a sample takes 1 .. {MAX_IMAGES} regional image prompts")
    return torch.stack(out).contiguous()


class IPRegions:
    """N regional image prompts of one call: masks fp32 [N, Hm, Wm] on the CPU (prepare_masks), weights (default all 1.0)"""

    def __init__(self, masks, weights=None):
        masks = torch.as_tensor(masks)
        if masks.dim() != 3 or not 1 <= masks.shape[0] <= MAX_IMAGES or masks.numel() == 0:
            raise ValueError(f"masks must be [N, Hm, Wm] with N = 1 .. {MAX_IMAGES}, got {tuple(masks.shape)}")
        self.masks = masks.detach().to("cpu", torch.float32).contiguous()
        self.n = int(masks.shape[0])
        w = [1.0] * self.n if weights is None else [float(v) for v in weights]
        if len(w) != self.n:
            raise ValueError(f"{len(w)} weights for {self.n} masks")
        self.weights = tuple(w)
        self._rows = {}

    @classmethod
    def from_masks(cls, masks, height, width, weights=None, binarize=True):
        return cls(prepare_masks(masks, height, width, binarize), weights)

    @property
    def size(self):
        return int(self.masks.shape[1]), int(self.masks.shape[2])

    def digest(self):
        """SHA-1 of N, the weights and the mask bytes: what a recorded plan with these regions depends on"""
        h = hashlib.sha1()
        h.update(repr((self.n, self.size, self.weights)).encode())
        h.update(self.masks.numpy().tobytes())
        return h.hexdigest()

    def downsample(self, h, w):
        """the masks on an h x w token grid, fp32 [N, h * w] on the CPU: F.interpolate(bicubic, align_corners=False), not clamped"""
        return F.interpolate(self.masks[None], size=(int(h), int(w)), mode="bicubic", align_corners=False)[0].reshape(self.n, int(h) * int(w)).contiguous()

    def rows(self, device, grid=None, tokens=None):
        """-> (mask rows fp32 [N, h * w], weights fp32 [N]) on `device` for a layer of that token grid (grid = (h, w), or tokens = L
        through token_grid); computed and uploaded once per grid and device"""
        if grid is None:
            grid = token_grid(tokens, *self.size)
        key = (int(grid[0]), int(grid[1]), str(torch.device(device)))
        r = self._rows.get(key)
        if r is None:
            r = self._rows[key] = (self.downsample(*grid).to(device), torch.tensor(self.weights, dtype=torch.float32).to(device))
        return r
