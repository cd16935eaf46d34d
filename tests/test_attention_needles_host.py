"""CPU: the premises of tests/attention_needles.py for every shape tests/test_gpu_exact_attention.py launches, and seeded faults -- a plain
torch attention (float64 softmax over the problem's own operands, one rounding to T) that is wrong in one of the ways a key loop, a
ring, a tail or a merge goes wrong -- each of which the equality check must refuse."""
import pytest
import torch

import attention_needles as an

DTYPES = [torch.bfloat16, torch.float16]
BF = torch.bfloat16


# ------------------------------------------------------------------------------------------------ the codes
@pytest.mark.parametrize("d,n,A,scale", [(64, 32, 8, 0.125), (40, 16, 16, 0.125), (36, 16, 16, 0.125), (128, 64, 4, 0.125), (80, 32, 16, 80 ** -0.5)])
def test_codes_are_distinct_and_32_nats_apart(d, n, A, scale):
    assert an.part(d) == n and an.amplitude(d, scale) == A and an.n_codes(d) == 4 * n * n
    c = an.code(torch.arange(an.n_codes(d)), d)
    assert set(c.unique().tolist()) <= {-1.0, 0.0, 1.0} and bool((c[:, 2 * n:] == 0).all())
    g = c @ c.t()
    assert bool((g.diagonal() == 2 * n).all())
    off = g - torch.diag(g.diagonal())
    assert float(off.max()) == n, "two different codes agree in at most one part"
    assert A * n * scale >= an.GAP_NATS and A * 2 * n < 2 ** 24
    for dt in DTYPES:                                       # queries and keys are values of T
        assert torch.equal((A * c).to(dt).double(), A * c)
    bal = an.code(an.balanced_ids(d), d)[:, :2 * n]
    assert bool((bal.mean(-1) == 0).all()) and bool(((bal * bal).mean(-1) == 1).all())


def test_pi_covers_every_key_and_differs_per_head():
    for Lk in (1, 63, 64, 77, 100, 130, 988, 1024, 4031):
        pi = an.pi_rows(2, 3, an.pad64(Lk), Lk, seed=1)
        for b in range(2):
            for h in range(3):
                assert len(pi[b, h].unique()) == Lk
        if Lk > 1:
            assert not torch.equal(pi[0, 0], pi[0, 1]) and not torch.equal(pi[0, 0], pi[1, 0])
            assert int((pi[0, 0, 1:] - pi[0, 0, :-1]).abs().min()) >= 3, "consecutive rows select keys apart"


def test_group_layouts_straddle_groups_tiles_quarters_and_halves():
    src, kind = an.key_layout(1024, 1024, seed=16)
    sizes = set(kind[kind > 0].tolist())
    assert sizes == set(an.GROUP_SIZES)
    spans = set()
    for j0 in src[kind > 0].unique().tolist():
        m = (src == j0).nonzero().flatten()
        assert len(m) == int(kind[j0]) and int(m[0]) == j0
        spans.add(int(m[1] - m[0]))
    assert {1, 16, 32, 64, 256, 512} <= spans
    assert int((kind > 0).sum()) <= 512
    src, kind = an.key_layout(988, 1024, seed=3)
    assert int(src[988]) == int(src[987]) and bool((kind[988:] == -1).all()) and bool((src[988:] < 988).all())


# ------------------------------------------------------------------------------------------------ the premises of every GPU case
def _all_problems(dtype):
    for B, H, Lq in an.SELF_SHAPES:
        yield an.single_set(B, H, Lq, Lq, Lq, dtype, seed=Lq // 64)
    for B, H, Lk, Lp in an.SELF_MASKED:
        yield an.single_set(B, H, Lp, Lk, Lp, dtype, seed=Lk)
    for B, H, Lq, nt, nip in an.SELF_K2:
        yield an.two_sets(B, H, Lq, nt, nip, dtype, seed=nip)
    for B, H, Lq, nt, nip, ln in an.CROSS:
        yield an.two_sets(B, H, Lq, nt, nip, dtype, seed=nt + nip) if nip else an.single_set(B, H, Lq, nt, an.pad64(nt), dtype, seed=nt, balanced=True, gmax=4)
    for B, H, Lq, nt, T, N in an.REGIONS:
        for w in (None, an.region_weights(N)):
            yield an.two_sets(B, H, Lq, nt, T, dtype, seed=T + N, scale2=1.0, n_img=N, masks=an.region_masks(N, Lq, seed=N), weights=w)
    for B, H, Lq, Lk, dq, dv, which in an.SMALL:
        yield an.single_set(B, H, Lq, Lk, Lk, dtype, seed=Lk + dq, d=dq, dv=dv, scale=0.125)
    for B, H, L_, d in an.ENC:
        yield an.single_set(B, H, L_, L_, L_, dtype, seed=L_, d=d, dv=d, scale=d ** -0.5)
        yield an.causal_set(B, H, L_, d, dtype, seed=L_)


@pytest.mark.parametrize("dtype", DTYPES)
def test_premises_hold_for_every_gpu_shape(dtype):
    n = 0
    for p in _all_problems(dtype):
        an.assert_premise(p)
        assert an.solve(p)["mass"] <= 2.0 ** -36, "the construction's own margin: 2^12 below the bound"
        n += 1
    assert n == len(an.SELF_SHAPES) + len(an.SELF_MASKED) + len(an.SELF_K2) + len(an.CROSS) + 2 * len(an.REGIONS) + len(an.SMALL) + 2 * len(an.ENC)


def test_small_cases_take_the_kernel_they_name():
    for B, H, Lq, Lk, dq, dv, which in an.SMALL:
        fits = an.small_lds_bytes(Lk, dq, dv) <= 150 * 1024
        assert fits == (which != "big") and (dq % 8 == 0) == (which != "dq36")


def test_every_class_is_in_the_launches():
    p = an.single_set(1, 2, 1024, 1024, 1024, BF, seed=16)
    S, seen = an._row_scores(p, p.sets[0], 0, 0)
    cnt = (S == S.max(-1, keepdim=True).values).sum(-1)
    assert set(cnt.tolist()) == {1, 2, 4, 64, 128}
    p = an.causal_set(1, 1, 77, 64, BF)
    S, seen = an._row_scores(p, p.sets[0], 0, 0)
    top = S.max(-1, keepdim=True).values
    future = ((S == top) & ~seen).sum(-1)
    assert int((future > 0).sum()) >= 77 // 4 - 1, "rows with their needle's code in the future"
    assert int(future[61]) == 1 and int(future[62]) == 0, "row 61's repeat is key 63 (its diagonal tile)"


# ------------------------------------------------------------------------------------------------ seeded faults
def attend(p, see=None, weigh=None, vals=None, roww=None):
    """plain attention on the problem's operands: float64 softmax(scale q k^T) over the seen keys, P V / l per key set, the weighted sum,
    ONE rounding to T.  The hooks seed a fault: see(n, b, h, seen) -> seen, weigh(n, b, h, P) -> (P of the numerator, P of l),
    vals(n, b, h, v) -> v, roww(n, w) -> w"""
    B, Lq, H, _ = p.q.shape
    out = torch.zeros(B, Lq, H, p.sets[0].v.shape[-1], dtype=torch.float64)
    for n, s in enumerate(p.sets):
        for b in range(B):
            for h in range(H):
                S, seen = an._row_scores(p, s, b, h)
                if see:
                    seen = see(n, b, h, seen)
                P = torch.softmax(torch.where(seen, S * p.scale, torch.full_like(S, -float("inf"))), -1)
                Pn, Pl = weigh(n, b, h, P) if weigh else (P, P)
                v = s.v[b, :, h].double()
                if vals:
                    v = vals(n, b, h, v)
                o = (Pn @ v) / Pl.sum(-1, keepdim=True)
                w = s.roww
                if roww:
                    w = roww(n, w)
                out[b, :, h] += s.w * (o if w is None else o * w[:Lq, None])
    return out.to(p.dtype)


def refused(p, y, names):
    """the equality check refuses y and its message names the row"""
    with pytest.raises(AssertionError) as e:
        an.assert_selected(y, p, "seeded fault")
    for name in names:
        assert name in str(e.value), str(e.value)


@pytest.fixture(scope="module", params=DTYPES, ids=["bf16", "fp16"])
def probs(request):
    dt = request.param
    N, Lq = 3, 100
    ps = dict(self=an.single_set(1, 2, 256, 256, 256, dt, seed=4), masked=an.single_set(1, 2, 128, 100, 128, dt, seed=100),
              causal=an.causal_set(1, 2, 77, 64, dt, seed=77), k2=an.two_sets(1, 2, 128, 77, 16, dt, seed=16),
              regions=an.two_sets(1, 2, Lq, 77, 16, dt, seed=19, scale2=1.0, n_img=N, masks=an.region_masks(N, Lq, seed=N), weights=an.region_weights(N)))
    for p in ps.values():
        an.assert_premise(p)
    return ps


def test_plain_attention_gives_the_statement(probs):
    """the float64 softmax rounds to the selection for every kind of problem: nothing but a fault fails the check below"""
    for p in probs.values():
        an.assert_selected(attend(p), p, "no fault")


def test_last_key_of_a_tile_dropped_for_16_rows(probs):
    p = probs["self"]
    S, _ = an._row_scores(p, p.sets[0], 0, 0)
    i = int((S[:, 63] == S.max(-1).values).nonzero()[0])
    r0 = i // 16 * 16

    def weigh(n, b, h, P):
        if (b, h) == (0, 0):
            P = P.clone()
            P[r0:r0 + 16, 63] = 0
        return P, P
    refused(p, attend(p, weigh=weigh), ["head 0", f"row {i}", "63"])


@pytest.mark.parametrize("in_l", [True, False])
def test_one_key_counted_twice(probs, in_l):
    """in the numerator and in l: single needles do not see it, the equal groups do; in the numerator alone: every row of that key does"""
    p = probs["self"]
    j = int((p.sets[0].kind == 2).nonzero()[1])

    def weigh(n, b, h, P):
        Pn = P.clone()
        Pn[:, j] *= 2
        return Pn, (Pn if in_l else P)
    refused(p, attend(p, weigh=weigh), ["equal group of 2", str(j)])


def test_two_4_key_groups_of_the_vt_permutation_swapped(probs):
    p = probs["self"]

    def vals(n, b, h, v):
        if h == 1:
            v = v.clone()
            v[68:72], v[72:76] = v[72:76].clone(), v[68:72].clone()
        return v
    refused(p, attend(p, vals=vals), ["head 1"])


def test_one_pad_key_unmasked(probs):
    p = probs["masked"]

    def see(n, b, h, seen):
        seen = seen.clone()
        seen[:, 100] = True
        return seen
    refused(p, attend(p, see=see), ["99", "unseen key(s) carry the same code"])
    p = probs["k2"]                                         # ... of the second key set

    def see2(n, b, h, seen):
        seen = seen.clone()
        if n == 1:
            seen[:, 16] = True
        return seen
    refused(p, attend(p, see=see2), ["set 1"])


def test_heads_swapped(probs):
    for name in ("self", "k2", "causal"):
        p = probs[name]
        refused(p, attend(p).flip(2), ["head 0"])


def test_a_future_key_visible_in_the_causal_form(probs):
    p = probs["causal"]

    def see(n, b, h, seen):
        seen = seen.clone()
        seen[61, 62] = seen[61, 63] = True                  # the diagonal tile's mask off by two for ONE row
        return seen
    refused(p, attend(p, see=see), ["row 61", "unseen key(s) carry the same code"])


def test_one_region_mask_ignored(probs):
    p = probs["regions"]
    refused(p, attend(p, roww=lambda n, w: torch.ones_like(w) if n == 2 else w), ["set 2"])
    refused(p, attend(p, roww=lambda n, w: None if w is None else w.flip(0)), ["batch 0"])
