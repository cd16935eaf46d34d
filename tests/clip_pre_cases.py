"""Inputs, float64 references and bounds shared by tests/test_clip_preprocess_host.py and tests/test_gpu_clip_preprocess.py.
A plain helper module (no fixtures, no pytest settings).

Images per case, S = 3: image 0 is a +-1 checkerboard of blocks a few output pixels wide -- the bicubic over- and undershoots at every
edge, so the clamp BEHIND the resize bites; image 1 is 1.6 x standard normal -- a third of its values lie outside [-1, 1], so the clamp in
FRONT of it bites; image 2 is a smooth ramp plus small noise (nothing clamps)."""
import math

import numpy as np
import torch

from imagharmony_amd import imageops

SIZE, PATCH = 28, 14                      # the tiny CLIP config of the tests
SHAPES = [(40, 56), (56, 40), (31, 50), (72, 40), (16, 24), (28, 28)]
FULL = (1024, 1024, 224, 14)

# fp32 bounds, absolute, in normalised units ((v - mean) / std: values in about [-1.8, 2.2]); profiles/clip_judge_parity.json has the
# measurements.  Each is 4 x the largest difference measured on the first run over the cases it covers.
# torch against the restatement: the margin covers the order of torch's fp32 sums and -- the larger part at 1024 -- its fp32 tap
# positions: torch forms centre = scale (i + 0.5) in fp32, whose ulp near coordinate 1000 is 6e-5, so a tap's weight is off by about
# 1e-5 there; hence one bound for the 28-pixel cases and one for 1024 -> 224.  Both measurements are below 1e-4, beyond which the
# restatement would be wrong, not loose.
HOST_MEASURED = {"small": 1.61e-5, "full": 5.94e-5}        # restatement (float64) vs torch CPU fp32, max over the cases of the group
assert max(HOST_MEASURED.values()) <= 1e-4
HOST_BOUND = {k: 4 * v for k, v in HOST_MEASURED.items()}
# kernel against the restatement: the kernel takes its tap positions as exact integer ratios (csrc/image.hip), so what is left is the
# order and the fused multiply-adds of its fp32 sums and one fp32 rounding per weight
KERNEL_MEASURED = 2.03e-6                  # kernel fp32 rows vs restatement, max over the cases (first GPU run)
KERNEL_BOUND = 4 * KERNEL_MEASURED

_CACHE = {}


def images(H, W, size, S=3):
    """[S, 3, H, W] fp32 (CPU), deterministic per shape"""
    g = torch.Generator().manual_seed(1000 * H + W)
    blk = max(1, int(round(3 * min(H, W) / size)))
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    board = (((yy // blk + xx // blk) % 2) * 2 - 1).float()
    x = torch.empty(S, 3, H, W)
    for s in range(S):
        if s % 3 == 0:
            x[s] = board * torch.tensor([1.0, -1.0, 0.9]).view(3, 1, 1)
        elif s % 3 == 1:
            x[s] = torch.randn(3, H, W, generator=g) * 1.6
        else:
            ramp = (yy.float() / H + xx.float() / W) - 1.0
            x[s] = ramp + 0.05 * torch.randn(3, H, W, generator=g)
    return x


def case(H, W, size=SIZE, patch=PATCH, S=3):
    """dict(x fp32 [S, 3, H, W], ref float64 rows [S g g, 3 p p]) computed once per shape and left unchanged"""
    key = (H, W, size, patch, S)
    if key not in _CACHE:
        x = images(H, W, size, S)
        _CACHE[key] = dict(x=x, ref=torch.from_numpy(imageops.clip_preprocess_reference(x.numpy(), size, patch)))
    return _CACHE[key]


def ulp(ref, dtype):
    """ulp of `dtype` at |ref| (float64 tensor): 2^(floor(log2 |ref|) - explicit mantissa bits), the subnormal spacing below the smallest normal"""
    bits, emin = {torch.bfloat16: (7, -126), torch.float16: (10, -14), torch.float32: (23, -126)}[dtype]
    e = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** emin)))
    return torch.pow(2.0, e - bits)


def bound_for(ref, dtype):
    """per-element absolute bound of the kernel's rows in `dtype` against the float64 reference: fp32 rows carry KERNEL_BOUND (sum
    order); bf16 / fp16 rows one rounding (half an ulp of the reference value) on top of it"""
    if dtype == torch.float32:
        return torch.full_like(ref, KERNEL_BOUND)
    return 0.5 * ulp(ref, dtype) + KERNEL_BOUND


def torch_rows(x, size, patch):
    """ClipPreferenceJudge.preprocess in fp32 on x's device, then the im2col of CLIPVisionEncoder.forward -> [S g g, 3 p p] fp32"""
    from imagharmony_amd.pns import ClipPreferenceJudge
    j = ClipPreferenceJudge.__new__(ClipPreferenceJudge)
    j.image_size = size
    px = j.preprocess(x)
    S, g = x.shape[0], size // patch
    return px.reshape(S, 3, g, patch, g, patch).permute(0, 2, 4, 1, 3, 5).reshape(S * g * g, 3 * patch * patch)


def padded_k(patch):
    k = 3 * patch * patch
    return (k + 63) // 64 * 64


assert math.isclose(SIZE / PATCH, 2.0)
