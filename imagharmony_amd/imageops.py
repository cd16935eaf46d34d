"""Host restatement of ``imh_clip_preprocess`` (include/imh.h): decoded images [S, 3, H, W] in [-1, 1] -> the patch rows the CLIP vision
tower's first GEMM contracts, in numpy float64.  It is to the image kernel what ``noise.py`` is to the seeded generator: the
specification the CPU tests hold against torch (``pns.ClipPreferenceJudge.preprocess`` + the im2col of ``CLIPVisionEncoder.forward``) and
the GPU tests hold the kernel against.  Nothing here runs on the product path.

Steps, per value: u = clamp(x / 2 + 0.5, 0, 1); antialiased bicubic (A = -0.5) to (nh, nw), separable, the filter of torch's
``upsample_bicubic2d_aa`` (``aa_tables``); clamp to [0, 1]; centre crop to size x size at (top, left); (v - mean_c) / std_c; row
``s g^2 + gy g + gx`` holds the 3 p p values of patch (gy, gx) in Conv2d's weight order (c, py, px).
"""
import math

import numpy as np

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
A = -0.5


def clip_geometry(H, W, size):
    """(nh, nw, top, left) of CLIPImageProcessor's resize-shortest-edge + centre crop, as ClipPreferenceJudge.preprocess derives them
    (Python's round: ties to even)"""
    H, W, size = int(H), int(W), int(size)
    sc = size / min(H, W)
    nh, nw = max(size, round(H * sc)), max(size, round(W * sc))
    return nh, nw, (nh - size) // 2, (nw - size) // 2


def cubic(x):
    """the bicubic convolution kernel with A = -0.5 (Keys), support [-2, 2]"""
    x = np.abs(np.asarray(x, dtype=np.float64))
    near = ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0
    far = (((x - 5.0) * x + 8.0) * x - 4.0) * A
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


def aa_taps(n_in, n_out, i):
    """output index i of one axis -> (first tap, weights float64 summing to 1): scale = in / out; support = 2 scale when downsampling
    (scale >= 1), else 2; centre = scale (i + 0.5); taps j in [max(0, int(centre - support + 0.5)), min(in, int(centre + support + 0.5)));
    weight cubic((j - centre + 0.5) / max(scale, 1)), normalised"""
    scale = n_in / n_out
    support = 2.0 * scale if scale >= 1.0 else 2.0
    inv = 1.0 / scale if scale >= 1.0 else 1.0
    centre = scale * (i + 0.5)
    lo = max(0, int(centre - support + 0.5))
    hi = min(int(n_in), int(centre + support + 0.5))
    w = cubic((np.arange(lo, hi) - centre + 0.5) * inv)
    return lo, w / w.sum()


def aa_tables(n_in, n_out):
    """the whole axis: (first [n_out] int, count [n_out] int, weights [n_out, max count] float64, zero beyond a row's count)"""
    taps = [aa_taps(n_in, n_out, i) for i in range(int(n_out))]
    first = np.array([t[0] for t in taps], dtype=np.int64)
    count = np.array([len(t[1]) for t in taps], dtype=np.int64)
    wts = np.zeros((int(n_out), int(count.max())), dtype=np.float64)
    for i, (_, w) in enumerate(taps):
        wts[i, :len(w)] = w
    return first, count, wts


def aa_matrix(n_in, n_out):
    """the axis as a dense [n_out, n_in] matrix"""
    first, count, wts = aa_tables(n_in, n_out)
    m = np.zeros((int(n_out), int(n_in)), dtype=np.float64)
    for i in range(int(n_out)):
        m[i, first[i]:first[i] + count[i]] = wts[i, :count[i]]
    return m


def clip_tap_bounds(n_in, n_out, patch):
    """(columns, taps): upper bounds of the source window of ``patch`` consecutive outputs of one axis and of one output's tap count --
    what the launcher sizes the kernel's LDS by: x1 - x0 <= (patch - 1) scale + 2 support + 1 and taps <= 2 support + 1"""
    scale = n_in / n_out
    support = 2.0 * scale if scale >= 1.0 else 2.0
    return int(math.floor((patch - 1) * scale + 2.0 * support)) + 2, int(math.floor(2.0 * support)) + 2


def clip_preprocess_reference(images, size=224, patch=14, mean=CLIP_MEAN, std=CLIP_STD):
    """images [S, 3, H, W] (array-like, [-1, 1] nominal) -> patch rows [S g^2, 3 patch^2] float64, g = size // patch"""
    x = np.asarray(images, dtype=np.float64)
    if x.ndim != 4 or x.shape[1] != 3:
        raise ValueError(f"images {x.shape} must be [S, 3, H, W]")
    size, patch = int(size), int(patch)
    if size % patch:
        raise ValueError(f"size {size} is no multiple of patch {patch}")
    S, _, H, W = x.shape
    nh, nw, top, left = clip_geometry(H, W, size)
    u = np.clip(x / 2 + 0.5, 0.0, 1.0)
    my = aa_matrix(H, nh)[top:top + size]                 # only the cropped rows / columns are ever needed
    mx = aa_matrix(W, nw)[left:left + size]
    v = np.einsum("xw,schw->schx", mx, u)                 # horizontal, then vertical
    v = np.einsum("yh,schx->scyx", my, v)
    v = np.clip(v, 0.0, 1.0)
    v = (v - np.asarray(mean, dtype=np.float64).reshape(1, 3, 1, 1)) / np.asarray(std, dtype=np.float64).reshape(1, 3, 1, 1)
    g = size // patch
    return v.reshape(S, 3, g, patch, g, patch).transpose(0, 2, 4, 1, 3, 5).reshape(S * g * g, 3 * patch * patch)
