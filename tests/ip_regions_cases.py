"""Inputs of the kernel-level tests of regional image prompts, shared by tests/test_ip_regions_host.py (CPU: the restatement's own
dtype error on these inputs) and tests/test_gpu_ip_regions.py (GPU: csrc/xattn_regions.hip against the restatement).  Everything is
derived from seeds (oracle.detfill); a plain helper module."""
import torch
import torch.nn.functional as F

import ip_regions_reference as rr
from oracle.detfill import det_randn

C_, H, CD, NT = 128, 2, 128, 77          # width, heads, cross-attention width, text tokens
TOL = {torch.float16: 1.5e-3, torch.bfloat16: 1.2e-2}      # tests/test_gpu_processors.py: the project's bound for this processor
SCALE = 0.8

# parity cases: name -> (B, grid (h, w), image tokens T, N, weights); soft (bicubic) masks
PARITY = {
    "n1_60_t4": (2, (6, 10), 4, 1, (1.0,)),
    "n2_144_t16": (2, (12, 12), 16, 2, (1.0, 0.5)),
    "n4_60_t4": (2, (6, 10), 4, 4, (1.0, 0.5, 0.75, 0.25)),
    "n2_128_t33": (1, (8, 16), 33, 2, (1.0, 0.5)),
}


def inputs(B, Lq, T, N, seed=1):
    """fp32 on the CPU: token rows x [B * Lq, C], to_q / to_k / to_v / to_k_ip / to_v_ip weights, text tokens [B, 77, CD], image tokens
    [B, N * T, CD] ([r0 | r1 | ...])"""
    s = seed * 100
    return dict(x=det_randn((B * Lq, C_), s + 1), wq=det_randn((C_, C_), s + 2, C_ ** -0.5),
                wk=det_randn((C_, CD), s + 3, CD ** -0.5), wv=det_randn((C_, CD), s + 4, CD ** -0.5),
                wk_ip=det_randn((C_, CD), s + 5, CD ** -0.5), wv_ip=det_randn((C_, CD), s + 6, CD ** -0.5),
                text=det_randn((B, NT, CD), s + 7), ip=det_randn((B, N * T, CD), s + 8), B=B, Lq=Lq, T=T, N=N)


def block_masks(N, Hm=45, Wm=77):
    """N 0 / 1 masks of Hm x Wm: vertical stripes that overlap nowhere, mask i = stripe i (N = 1: the left half)"""
    m = torch.zeros(N, Hm, Wm)
    S = max(N, 2)
    for i in range(N):
        m[i, :, i * Wm // S:(i + 1) * Wm // S] = 1.0
    return m


def soft_rows(N, grid, Hm=45, Wm=77):
    """the stripes resized to the token grid as diffusers does (bicubic, not clamped; 45 x 77 is no multiple of any grid here, so the
    edges are soft and overshoot [0, 1]): rows fp32 [N, h * w]"""
    return rr.downsample(block_masks(N, Hm, Wm), *grid)


def reference(inp, rows, weights, scale=SCALE, dtype=torch.float32):
    """the restatement on these inputs, every tensor and operation in `dtype` on the CPU -> [B * Lq, C] in dtype"""
    f = lambda t: t.to(dtype)
    B, Lq, T, N = inp["B"], inp["Lq"], inp["T"], inp["N"]
    q = F.linear(f(inp["x"]).view(B, Lq, C_), f(inp["wq"]))
    k, v = F.linear(f(inp["text"]), f(inp["wk"])), F.linear(f(inp["text"]), f(inp["wv"]))
    ks = [F.linear(f(inp["ip"][:, i * T:(i + 1) * T]), f(inp["wk_ip"])) for i in range(N)]
    vs = [F.linear(f(inp["ip"][:, i * T:(i + 1) * T]), f(inp["wv_ip"])) for i in range(N)]
    return rr.regions_attention(q, k, v, ks, vs, rows, list(weights), scale, H).reshape(B * Lq, C_)


def parity_case(name):
    B, grid, T, N, weights = PARITY[name]
    inp = inputs(B, grid[0] * grid[1], T, N, seed=sum(map(ord, name)))
    return inp, soft_rows(N, grid), weights
