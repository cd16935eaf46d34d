"""FreeU at the up blocks' skip concat, restated in numpy float64 (include/imh.h IMH_EW_CONCAT, the form with i2 > 0, is the
specification of the launch; csrc/elementwise.hip freeu_concat_kernel the product's code).

What diffusers does (utils/torch_utils.py, restated from its published source).  ``apply_freeu(resolution_idx, hidden, res_hidden, s1,
s2, b1, b2)`` runs in every ResNet step of up blocks 0 and 1, right before ``torch.cat([hidden, res_hidden], 1)``:

    hidden[:, :C // 2] = hidden[:, :C // 2] * b          b = b1 in up block 0, b2 in up block 1
    res_hidden = fourier_filter(res_hidden, threshold=1, scale=s)          s = s1 / s2

and ``fourier_filter(x, threshold, scale)`` is, per (sample, channel) plane of H x W,

    X = fftshift(fftn(x));  X[crow - threshold : crow + threshold, ccol - threshold : ccol + threshold] *= scale;  ifftn(ifftshift(X)).real

with crow, ccol = H // 2, W // 2 (in fp32 for bf16 inputs and for sides that are no powers of two).

The closed form.  fftshift puts frequency k of an axis of length N at index (k + N // 2) mod N, so index N // 2 holds frequency 0 and
index N // 2 - 1 holds frequency -1, for even and odd N alike.  With threshold = 1 the box [N // 2 - 1, N // 2 + 1) is therefore the
frequency set {-1, 0} on each axis: the mask scales the four components X[u, v], (u, v) in {-1, 0}^2, and leaves the rest alone.  The
filter is linear, so

    out = x + (s - 1) * low,      low(y, x) = Re( (1 / HW) * sum_{(u, v) in {-1, 0}^2} X[u, v] * exp(2 pi i (u y / H + v x / W)) ),
    X[u, v] = sum_{y', x'} x(y', x') * exp(-2 pi i (u y' / H + v x' / W)).

Written with t = 2 pi y / H and p = 2 pi x / W, the four components need seven real plane sums,

    S = sum x,  (Ac, As) = sum x * (cos t, sin t),  (Bc, Bs) = sum x * (cos p, sin p),  (Dc, Ds) = sum x * (cos(t + p), sin(t + p)),
    HW * low = S + (Ac cos t + As sin t) + (Bc cos p + Bs sin p) + (Dc cos(t + p) + Ds sin(t + p))

(nine, the outer product of (1, cos t, sin t) and (1, cos p, sin p), if cos(t + p) and sin(t + p) are expanded).  The mask is
asymmetric -- frequency -1 is scaled, frequency +1 is not -- and ``.real`` drops what that leaves imaginary: a real plane cos t with
H > 2 has half its weight at -1 and half at +1, so it comes out as x * (1 + (s - 1) / 2), not s * x.  At N = 2 the frequencies -1 and
+1 are the same (Nyquist) component, the box covers the whole axis, and cos t = (-1)^y comes out as s * x.  That is upstream's
behaviour and is reproduced, not corrected.

These functions are the yardstick the kernel is held against (tests/test_freeu_host.py pins them to an FFT restatement)."""
import numpy as np


def _axis(n):
    a = 2.0 * np.pi * np.arange(n, dtype=np.float64) / n
    return np.cos(a), np.sin(a)


def fourier_low(x):
    """x: float64 [..., H, W, C] (NHWC planes) -> low, the same shape: the four masked Fourier components' real part"""
    x = np.asarray(x, dtype=np.float64)
    H, W = x.shape[-3], x.shape[-2]
    ct, st = (v[:, None, None] for v in _axis(H))
    cp, sp = (v[None, :, None] for v in _axis(W))
    cd, sd = ct * cp - st * sp, st * cp + ct * sp

    def S(w):
        return (x * w).sum(axis=(-3, -2), keepdims=True)
    one = np.ones((1, 1, 1))
    low = S(one) + (S(ct) * ct + S(st) * st) + (S(cp) * cp + S(sp) * sp) + (S(cd) * cd + S(sd) * sd)
    return low / float(H * W)


def fourier_filter(x, scale):
    """diffusers fourier_filter(x, threshold=1, scale) on NHWC planes: float64 [..., H, W, C] -> the same shape"""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim < 3 or x.shape[-3] < 2 or x.shape[-2] < 2:
        raise ValueError(f"fourier_filter takes [..., H, W, C] with H, W >= 2, got {x.shape}")
    return x + (float(scale) - 1.0) * fourier_low(x)


def freeu_concat(hidden, skip, scaled, b, s):
    """The FreeU concat, unrounded: hidden [B, H, W, C1], skip [B, H, W, C2] (the values of the compute dtype, as float64) ->
    float64 [B, H, W, C1 + C2] = [hidden with its first `scaled` channels times b | fourier_filter(skip, s)].  The launch rounds the
    scaled and the filtered channels to the compute dtype once; it carries b and s as fp32."""
    hidden, skip = np.asarray(hidden, dtype=np.float64), np.asarray(skip, dtype=np.float64)
    if hidden.ndim != 4 or skip.ndim != 4 or hidden.shape[:3] != skip.shape[:3]:
        raise ValueError(f"freeu_concat takes NHWC tensors of one grid, got {hidden.shape} and {skip.shape}")
    if not 0 <= int(scaled) <= hidden.shape[-1]:
        raise ValueError(f"{scaled} scaled channels of {hidden.shape[-1]}")
    h = hidden.copy()
    h[..., :int(scaled)] *= float(b)
    return np.concatenate([h, fourier_filter(skip, s)], axis=-1)


def unet_settings(freeu, block):
    """(b, s) of up block `block` under freeu = (s1, s2, b1, b2), diffusers' argument order; None for blocks 2 and up or without FreeU"""
    if freeu is None or block > 1:
        return None
    s1, s2, b1, b2 = (float(v) for v in freeu)
    return (b1, s1) if block == 0 else (b2, s2)
