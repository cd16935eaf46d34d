"""Operands for which an attention launch has ONE right answer (tests/test_gpu_exact_attention.py; the conditions on these operands are
checked on the CPU by tests/test_attention_needles_host.py), after tests/exact_operands.py: softmax is made a SELECTION.

Keys carry +-1 codes.  For a head dim d the code has two parts of n dims, n the largest power of two with 2 n <= d (32 for d = 64, 16 for
40 and 36, 64 for 128, 32 for 80), the remaining dims are zero: code c = [s_a H_n[c % n] | s_b H_n[(c // n) % n]], the two signs from
c // n^2, H_n the Sylvester Hadamard matrix -- 4 n^2 distinct codes (4096 for d = 64).  Two different codes agree in at most one part:
their dot product is <= n, a code's with itself 2 n.  A query is A times the code of its needle key, A the smallest power of two with
A n scale >= 32: every operand value is exact in bf16 and fp16, every raw score an exact integer in fp32, the needle scores A 2 n scale
nats (64 for d = 64, A = 8, scale = 1/8) and every other key at least 32 nats less.  exp(-32) = 1.3e-14: over 4096 keys the off-needle
softmax mass stays below 2^-24 -- 2^12 below half a unit in the last place of fp16 -- which assert_premise checks in float64 for every
row; it is a condition on the operands, not a measured tolerance.

Row classes, mixed in every launch (a row's class follows from the keys that share its needle's code):
  single needle   O[i] = V[pi(i)]; pi(i) = (i odd + c) mod Lk strides across tiles, differs per batch and head and, where Lq >= Lk, hits
                  every real key; V of such keys uses every mantissa bit of T.
  equal group     g in {2, 4, 64, 128} keys {1, 16, 32, 64, Lk / 4, Lk / 2} apart share one code: O[i] is their mean (V = s {1, 2} for
                  g >= 64, s k / 4 with k of 1 .. 16 for g <= 4, the sign s a function of (batch, head, dim) alone: the mean is a
                  value of T, never 0, and l = g is a power of two whose reciprocal is exact).  A key counted twice, or in the numerator but not in l, or a wrong merge weight moves it.
  poisoned pad    every key of [Lk, Lk_pad) repeats the code of a real needle (the first pad that of the LAST real key) with V = -100.
  causal          every fourth row's needle code is repeated two keys later, in its future: a key past the diagonal halves that row
                  (and the rows from there on, which do see both, get the mean of the pair).
  two key sets    a key of the second set carries the first part of a code only (the second part is zero), so a query selects in it
                  the keys that share the first part of its needle's code, 32 nats over the rest; V = s k / 2 with k of 1 .. 8 (s {1, 2} and
                  groups of <= 2 for the images of a regions launch), scale2 and the regions' weights powers of two, masks of {0, 1, 0.5}:
                  V1 + sum_i w_i m_i V2_i is a value of T.

The expected value is stated from the operands themselves: per key set the mean of V over the keys whose integer score equals the row
maximum (float64), the weighted sum over the key sets, rounded once.  A kernel's p = exp2(fma(s, c, -m c)) of a needle differs from 1 by
the rounding of m c (a few 1e-6), which rounds to 1 in T; its l is then g (1 +- a few 1e-6) and O the statement's value times that: with
the statement's value IN T there is no rounding tie such a perturbation could flip, so equality decides and no tolerance is chosen.

A plain helper module: no GPU needed to import it, no fixtures, no pytest settings."""
import math

import torch

from exact_operands import full_mantissa

F64 = torch.float64
GAP_NATS = 32.0                  # every off-needle key scores at least this much less than the needle
MASS = 2.0 ** -24                # bound on the off-needle softmax mass of every row
POISON = -100.0
GROUP_SIZES = (2, 4, 64, 128)

# ---- the shapes of tests/test_gpu_exact_attention.py (the host test checks the premises of every one of them) ----
SELF_SHAPES = [(2, 2, 64), (1, 3, 128), (1, 2, 192), (2, 2, 256), (2, 1, 320), (1, 2, 384), (1, 1, 448), (1, 4, 512), (1, 2, 1024), (1, 1, 4096),
               (2, 20, 1024)]                                                        # (B, H, Lq): Lq = 64 {1 .. 8, 16, 64} tiles with B H <= 4; key quarters
SELF_MASKED = [(1, 2, 63, 64), (2, 3, 1, 64), (1, 2, 100, 128), (2, 2, 988, 1024), (1, 1, 4031, 4096)]     # (B, H, Lk, Lk_pad)
SELF_K2 = [(2, 2, 256, 77, 4), (1, 2, 128, 77, 16), (1, 3, 192, 77, 70), (2, 1, 100, 130, 4), (1, 2, 64, 130, 16), (1, 1, 320, 130, 70)]   # (B, H, Lq, nt, nip)
CROSS = [(2, 2, 100, 77, 4, 0), (1, 5, 128, 77, 70, 1), (2, 10, 256, 130, 4, 2), (1, 2, 256, 130, 0, 3), (2, 5, 256, 77, 0, 0), (1, 10, 128, 130, 70, 3),
         (1, 5, 100, 130, 70, 2), (2, 2, 128, 77, 0, 1), (2, 20, 1024, 77, 4, 2)]     # (B, H, Lq, nt, nip, ln); the last: 320 items, 8 of 40 per XCD as half items
REGIONS = [(2, 2, 144, 77, 4, 1), (1, 2, 100, 77, 16, 3), (2, 2, 60, 130, 33, 8), (1, 5, 256, 77, 4, 3)]    # (B, H, Lq, nt, T, n_img)
SMALL = [(2, 2, 64, 64, 64, 64, "lds"), (1, 3, 65, 65, 40, 64, "lds"), (2, 2, 77, 77, 40, 64, "lds"), (1, 2, 273, 273, 64, 64, "lds"),
         (1, 2, 273, 273, 128, 40, "lds"), (2, 2, 77, 77, 40, 64, "pitch"), (1, 2, 77, 77, 36, 64, "dq36"), (1, 1, 273, 273, 128, 128, "big")]
#          (B, H, Lq, Lk, dq, dv, which kernel: LDS-resident, or the fallback by row pitch / by dq % 8 / above 150 KB of LDS)
ENC = [(2, 2, 77, 64), (1, 2, 257, 80), (1, 3, 200, 64), (1, 1, 257, 64), (2, 1, 77, 80)]      # (B, H, L, d); 200 = three tiles and a ragged one


def small_lds_bytes(Lk, dq, dv):
    """LDS bytes of the K^T / V-resident kernel, as attention_small_launch computes them"""
    lkp = (Lk + 63) // 64 * 64
    return (dq * lkp + Lk * dv) * 2 + (4 * lkp + 4 * dq) * 4


def pad64(n):
    return (n + 63) // 64 * 64


# ------------------------------------------------------------------------------------------------ codes
def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def hadamard(n):
    h = torch.ones(1, 1, dtype=F64)
    while h.shape[0] < n:
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    assert h.shape[0] == n, "a power of two"
    return h


def part(d):
    """width of one code part: the largest power of two n with 2 n <= d"""
    n = 1
    while 4 * n <= d:
        n *= 2
    return n


def n_codes(d):
    return 4 * part(d) ** 2


def amplitude(d, scale):
    """smallest power of two A with A n scale >= GAP_NATS"""
    a = 1.0
    while a * part(d) * scale < GAP_NATS:
        a *= 2
    return a


def code(ids, d, first_part_only=False):
    """ids (long, any shape) of [0, 4 n^2) -> float64 [..., d]"""
    n = part(d)
    hn = hadamard(n)
    ids = ids.long()
    assert int(ids.min()) >= 0 and int(ids.max()) < 4 * n * n
    a, b, s = ids % n, (ids // n) % n, ids // (n * n)
    sa, sb = 1.0 - 2.0 * (s & 1).double(), 1.0 - 2.0 * (s >> 1).double()
    out = torch.zeros(*ids.shape, d, dtype=F64)
    out[..., :n] = sa[..., None] * hn[a]
    if not first_part_only:
        out[..., n:2 * n] = sb[..., None] * hn[b]
    return out


def balanced_ids(d):
    """the codes whose two parts are both non-constant Hadamard rows: mean 0, variance 1 over the head's dims when 2 n == d (the rows a
    LayerNorm with identity affine leaves alone)"""
    n = part(d)
    ids = torch.arange(4 * n * n)
    return ids[(ids % n != 0) & ((ids // n) % n != 0)]


# ------------------------------------------------------------------------------------------------ pi, groups, poison
_ODD = [3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67, 71, 73, 79, 83, 89, 97]


def pi_rows(B, H, Lq, Lk, seed=0):
    """[B, H, Lq] long: row i of (b, h) selects key (i odd + c) mod Lk, odd coprime to Lk and different from head to head"""
    out = torch.empty(B, H, Lq, dtype=torch.long)
    ok = [p for p in _ODD if math.gcd(p, Lk) == 1]
    i = torch.arange(Lq)
    for b in range(B):
        for h in range(H):
            t = b * H + h + seed
            out[b, h] = (i * ok[t % len(ok)] + 17 * t + 5) % Lk
    return out


def key_layout(Lk, Lk_pad, seed=0, gmax=128, groups=True):
    """-> (src [Lk_pad] long, kind [Lk_pad] long).  src[j]: the key whose code key j carries -- j itself, the first member of its equal
    group, or for a pad key a real key (for key Lk the last real key).  kind[j]: 0 a key of its own, g a member of a group of g, -1 pad.
    Groups are placed greedily, at most half of the real keys in groups."""
    g_ = _gen(1000 + seed)
    src, kind = torch.arange(Lk_pad), torch.zeros(Lk_pad, dtype=torch.long)
    used, budget = torch.zeros(Lk, dtype=torch.bool), Lk // 2
    specs = [(2, Lk // 2), (4, Lk // 4), (2, 1), (2, 16), (2, 32), (2, 64), (4, 1), (4, 16), (4, 32), (4, 64), (64, 1), (128, 1), (64, 16),
             (128, 16), (64, 32), (64, 64), (128, 32)]
    for g, sp in specs if groups else []:
        span = (g - 1) * sp
        if g > gmax or sp < 1 or span >= Lk or g > budget:
            continue
        for _ in range(16):
            j0 = int(torch.randint(0, Lk - span, (1,), generator=g_))
            m = j0 + sp * torch.arange(g)
            if not bool(used[m].any()):
                used[m], src[m], kind[m] = True, j0, g
                budget -= g
                break
    if Lk_pad > Lk:
        r = torch.randint(0, Lk, (Lk_pad - Lk,), generator=g_)
        r[0] = Lk - 1
        src[Lk:], kind[Lk:] = src[r], -1
    return src, kind


def values(kind, B, H, dv, dtype, seed, grid=None):
    """V [B, Lp, H, dv] in T by the key's kind: every mantissa bit for a key of its own, s k / 4 with k of 1 .. 16 for groups of <= 4, s k
    with k of {1, 2} for larger ones, POISON for pads; grid = (den, kmax): s k / den with k of 1 .. kmax for every real key instead.
    s = +-1 depends on (batch, head, dim) alone -- the same in every key set of a problem -- so no mean and no sum over key sets cancels: a
    statement's value that is exactly 0 has no relative margin (a kernel's 1e-14 of off-needle mass is a nonzero bf16 value)"""
    sgn = 1.0 - 2.0 * torch.randint(0, 2, (B, 1, H, dv), generator=_gen(77)).double()
    Lp = kind.shape[0]
    g_ = _gen(2000 + seed)
    shape = (B, Lp, H, dv)
    kd = kind.view(1, Lp, 1, 1)
    if grid is None:
        v = full_mantissa(shape, 3000 + seed, F64).to(dtype).double()
        q4 = sgn * torch.randint(1, 17, shape, generator=g_).double() / 4
        t3 = sgn * torch.randint(1, 3, shape, generator=g_).double()
        v = torch.where((kd > 0) & (kd <= 4), q4, v)
        v = torch.where(kd > 4, t3, v)
    else:
        den, kmax = grid
        v = sgn * torch.randint(1, kmax + 1, shape, generator=g_).double() / den
    v = torch.where(kd < 0, torch.full_like(v, POISON), v)
    return v.to(dtype)


# ------------------------------------------------------------------------------------------------ problems
class KeySet:
    """k [B, Lp, H, d], v [B, Lp, H, dv] in T in the LOGICAL order (the launch's layouts are the GPU test's business); the first Lk keys are
    real; w: the set's weight in the output; roww float64 [Lq] or None: a further weight per query row (the regions' masks)"""

    def __init__(self, k, v, Lk, kind, w=1.0, roww=None):
        self.k, self.v, self.Lk, self.Lp, self.kind, self.w, self.roww = k, v, Lk, k.shape[1], kind, float(w), roww


class Problem:
    def __init__(self, q, sets, scale, dtype, A, causal=False, what=""):
        self.q, self.sets, self.scale, self.dtype, self.A, self.causal, self.what = q, sets, float(scale), dtype, A, causal, what
        self._sol = None

    def to(self, dev):
        """the same problem with its operands on `dev` (the statement is then computed there)"""
        p = Problem(self.q.to(dev), [KeySet(s.k.to(dev), s.v.to(dev), s.Lk, s.kind, s.w, None if s.roww is None else s.roww.to(dev))
                                     for s in self.sets], self.scale, self.dtype, self.A, self.causal, self.what)
        return p


def _keys_from_ids(ids, d, dtype, first_part_only=False):
    """ids [B, H, Lp] -> k [B, Lp, H, d] in T"""
    return code(ids, d, first_part_only).permute(0, 2, 1, 3).contiguous().to(dtype)


def single_set(B, H, Lq, Lk, Lk_pad, dtype, seed=0, d=64, dv=64, scale=0.125, balanced=False, gmax=128, grid=None):
    """one key set (self-attention, attention_small, the bidirectional attention_enc, text-only cross attention)"""
    pool = balanced_ids(d) if balanced else torch.arange(n_codes(d))
    assert Lk <= len(pool), "more real keys than codes"
    src, kind = key_layout(Lk, Lk_pad, seed, gmax)
    off = (torch.arange(B)[:, None] * H + torch.arange(H)[None, :]) * 37 + 11 * seed            # the code of key j differs per batch and head
    ids = pool[(src[None, None, :] + off[:, :, None]) % len(pool)]
    A = amplitude(d, scale)
    pi = pi_rows(B, H, Lq, Lk, seed)
    q = (A * code(torch.gather(ids, 2, pi), d)).permute(0, 2, 1, 3).contiguous().to(dtype)
    ks = KeySet(_keys_from_ids(ids, d, dtype), values(kind, B, H, dv, dtype, seed, grid), Lk, kind)
    return Problem(q, [ks], scale, dtype, A, what=f"B={B} H={H} Lq={Lq} Lk={Lk}|{Lk_pad} d={d} dv={dv}")


def causal_set(B, H, L, d, dtype, seed=0, scale=None):
    """attention_enc_causal: key j carries a code of its own, except j % 4 == 2, which repeats the code of key j - 2.  Row i with
    i % 4 == 1 takes key i - 1 as its needle -- the repeat, key i + 1, is in its future; every other row strides over the keys <= i (and
    gets the mean of a pair where it sees both).  Pair members hold quarters of [-4, 4]."""
    scale = d ** -0.5 if scale is None else scale
    j = torch.arange(L)
    src = torch.where(j % 4 == 2, j - 2, j)
    kind = torch.where(j % 2 == 0, torch.full_like(j, 2), torch.zeros_like(j))
    off = (torch.arange(B)[:, None] * H + torch.arange(H)[None, :]) * 37 + 11 * seed
    ids = (src[None, None, :] + off[:, :, None]) % n_codes(d)
    ok = [p for p in _ODD if math.gcd(p, L) == 1]
    pi = torch.empty(B, H, L, dtype=torch.long)
    for b in range(B):
        for h in range(H):
            t = b * H + h + seed
            stride = (j * ok[t % len(ok)] + 17 * t + 5) % (j + 1)
            pi[b, h] = torch.where(j % 4 == 1, j - 1, stride)
    A = amplitude(d, scale)
    q = (A * code(torch.gather(ids, 2, pi), d)).permute(0, 2, 1, 3).contiguous().to(dtype)
    ks = KeySet(_keys_from_ids(ids, d, dtype), values(kind, B, H, d, dtype, seed), L, kind)
    return Problem(q, [ks], scale, dtype, A, causal=True, what=f"causal B={B} H={H} L={L} d={d}")


def two_sets(B, H, Lq, nt, nip, dtype, seed=0, scale2=0.5, n_img=0, masks=None, weights=None, scale=0.125):
    """d = 64.  First parts: the 62 signed non-constant rows of H_32, n2 = min(nip, 62) of them in use.  Key j2 of a second set carries
    first part (j2 + shift) mod n2 alone (70 keys: eight first parts twice, a group of 2); key j of the first set carries first part
    j mod n2 and as second part the non-constant row 1 + (j // n2) mod 31, negated from j // n2 = 31 on -- all balanced codes, distinct
    while nt <= 62 n2 (n2 = the second set's distinct first parts).  Both sets have groups of <= 4 (key_layout) and poisoned pads.
    n_img = 0: out = O1 + scale2 O2.  n_img > 0 (regions): out = O1 + sum_i scale2 weights[i] masks[i, q] O2_i, the images' V of
    s {1, 2} in groups of <= 2, the text's s k / 2."""
    d = 64
    fp = torch.cat([torch.arange(1, 32), 1024 + torch.arange(1, 32)])           # first part u: row 1 + u % 31, negated for u >= 31
    bh = torch.arange(B)[:, None] * H + torch.arange(H)[None, :]
    lp2 = pad64(nip)
    if nip <= 62:                               # groups of <= 4 by key_layout; first parts = the dense rank of a key's source
        src2, kind2 = key_layout(nip, lp2, seed + 1, gmax=2 if n_img else 4)
        uniq = torch.unique(src2[:nip])
        rank2, n2 = torch.searchsorted(uniq, src2), len(uniq)
    else:                                       # more keys than first parts: key j2 and j2 + 62 are a group of 2
        n2 = 62
        rank2, kind2 = torch.arange(lp2) % n2, torch.zeros(lp2, dtype=torch.long)
        kind2[:nip] = torch.where((torch.arange(nip) % n2) < nip - n2, 2, 0)
        rank2[nip:], kind2[nip:] = torch.randint(0, n2, (lp2 - nip,), generator=_gen(5000 + seed)), -1
        rank2[nip] = (nip - 1) % n2
    assert nt <= 62 * n2
    src1, kind1 = key_layout(nt, pad64(nt), seed, gmax=4)
    m = src1 // n2
    ids1 = fp[(src1[None, None, :] + bh[:, :, None] * 5 + seed) % n2] + ((1 + m % 31) * 32 + ((m // 31) % 2) * 2048)[None, None, :]
    A = amplitude(d, scale)
    pi = pi_rows(B, H, Lq, nt, seed)
    q = (A * code(torch.gather(ids1, 2, pi), d)).permute(0, 2, 1, 3).contiguous().to(dtype)
    half = (2, 8)
    sets = [KeySet(_keys_from_ids(ids1, d, dtype), values(kind1, B, H, 64, dtype, seed, half), nt, kind1)]
    for i in range(max(n_img, 1)):
        ids2 = fp[(rank2[None, None, :] + bh[:, :, None] * 5 + seed + 3 * i) % n2]
        w, roww = scale2, None
        if n_img:
            w = scale2 * (1.0 if weights is None else float(weights[i]))
            roww = masks[i].double()
        sets.append(KeySet(_keys_from_ids(ids2, d, dtype, first_part_only=True),
                           values(kind2, B, H, 64, dtype, seed + 50 + i, (1, 2) if n_img else half), nip, kind2, w, roww))
    return Problem(q, sets, scale, dtype, A, what=f"B={B} H={H} Lq={Lq} nt={nt} nip={nip} n_img={n_img}")


def region_masks(n_img, Lq, seed=0):
    """fp32 [n_img, Lq] of {0, 1, 0.5}; rows i % 5 == 3 are 0 in every image (the text-only rows)"""
    m = torch.tensor([0.0, 1.0, 0.5])[torch.randint(0, 3, (n_img, Lq), generator=_gen(4000 + seed))]
    m[:, torch.arange(Lq) % 5 == 3] = 0.0
    return m


def region_weights(n_img):
    """fp32 [n_img]: 1, 0.5, 1, ..."""
    return torch.tensor([(1.0, 0.5)[i % 2] for i in range(n_img)])


# ------------------------------------------------------------------------------------------------ the statement and the premise
def _row_scores(p, s, b, h):
    """float64 raw scores [Lq, Lp] of (b, h) against ALL keys of the set, pads included, and the mask of the keys the row may see"""
    S = p.q[b, :, h].double() @ s.k[b, :, h].double().t()
    seen = torch.arange(s.Lp, device=S.device)[None, :] < s.Lk
    if p.causal:
        seen = seen & (torch.arange(s.Lp, device=S.device)[None, :] <= torch.arange(S.shape[0], device=S.device)[:, None])
    return S, seen.expand_as(S)


def solve(p):
    """-> dict: want float64 [B, Lq, H, dv] (per set the mean of V over the seen keys whose score is the row maximum, summed with the sets'
    weights), and what the premise is about: the largest off-needle mass, whether all scores are integers below 2^24, all needle counts
    powers of two, every set's own selection a value of T"""
    if p._sol is not None:
        return p._sol
    B, Lq, H, _ = p.q.shape
    dv = p.sets[0].v.shape[-1]
    want = torch.zeros(B, Lq, H, dv, dtype=F64, device=p.q.device)
    mass, top, ints, pow2, in_t = 0.0, 0.0, True, True, True
    absum = torch.zeros_like(want)
    for s in p.sets:
        for b in range(B):
            for h in range(H):
                S, seen = _row_scores(p, s, b, h)
                ints = ints and bool((S == S.round()).all())
                top = max(top, float(S.abs().max()))
                Sm = torch.where(seen, S, torch.full_like(S, -float("inf")))
                smax = Sm.max(-1, keepdim=True).values
                E = torch.exp((Sm - smax) * p.scale)
                hit = Sm == smax
                cnt = hit.sum(-1)
                pow2 = pow2 and bool(((cnt & (cnt - 1)) == 0).all()) and int(cnt.min()) >= 1
                mass = max(mass, float(((E * ~hit).sum(-1) / E.sum(-1)).max()))
                sel = (hit.double() @ s.v[b, :, h].double()) / cnt[:, None].double()
                in_t = in_t and bool((sel.to(p.dtype).double() == sel).all())
                if s.roww is not None:
                    sel = sel * s.roww[:Lq, None]
                want[b, :, h] += s.w * sel
                absum[b, :, h] += (s.w * sel).abs()
    p._sol = dict(want=want, mass=mass, top=top, ints=ints, pow2=pow2, in_t=in_t, uncancelled=bool(((want.abs() == absum) & (want != 0)).all()))
    return p._sol


def expected(p):
    """the statement, rounded once to T"""
    return solve(p)["want"].to(p.dtype)


def assert_premise(p):
    """what makes equality the right comparison, asserted on the operands a case launches"""
    s = solve(p)
    assert s["ints"] and s["top"] < 2.0 ** 24, f"{p.what}: raw scores are not integers below 2^24 (largest {s['top']})"
    assert s["mass"] <= MASS, f"{p.what}: off-needle softmax mass {s['mass']:.3e} above 2^-24"
    assert s["pow2"], f"{p.what}: a row's needle count is not a power of two"
    assert s["in_t"], f"{p.what}: a group mean is not a value of {p.dtype}"
    assert s["uncancelled"], f"{p.what}: a value of the statement is 0 or a sum of terms that cancel: no relative margin"
    assert bool((s["want"].to(p.dtype).double() == s["want"]).all()), f"{p.what}: the sum over the key sets is not a value of {p.dtype}"
    for t in [p.q] + [x for ks in p.sets for x in (ks.k, ks.v)]:
        assert t.dtype == p.dtype and bool(torch.isfinite(t).all())


def describe_row(p, b, i, h):
    """class and needle keys of one row, for a failure message"""
    out = []
    for n, s in enumerate(p.sets):
        S, seen = _row_scores(p, s, b, h)
        row = S[i]
        top = row[seen[i]].max()
        keys = [int(j) for j in ((row == top) & seen[i]).nonzero().flatten()[:8]]
        hidden = int(((row == top) & ~seen[i]).sum())
        g = int(((row == top) & seen[i]).sum())
        cls = "single needle" if g == 1 else f"equal group of {g}"
        out.append(f"set {n}: {cls}, needle key(s) {keys}" + (f", {hidden} unseen key(s) carry the same code" if hidden else ""))
    return "; ".join(out)


def assert_selected(out, p, what):
    """out [B, Lq, H, dv] (or anything that views to it) == expected(p); the message names the first differing (batch, head, row), its
    class, its needle keys, got and expected"""
    want = expected(p)
    out = out.reshape(want.shape)
    assert out.dtype == want.dtype
    if torch.equal(out, want):
        return
    bad = ~(out.double() == want.double())
    rows = bad.any(-1)
    b, i, h = (int(x) for x in rows.nonzero()[0])
    e = int(bad[b, i, h].nonzero()[0])
    raise AssertionError(f"{what} [{p.what}]: {int(rows.sum())} of {rows.numel()} (batch, row, head) differ; first (batch {b}, head {h}, row {i}) -- "
                         f"{describe_row(p, b, i, h)} -- dim {e}: got {float(out[b, i, h, e])!r}, expected {float(want[b, i, h, e])!r}")
