"""GPU: every row of the op table (imagharmony_amd.lib.OPS) launches the same thing eagerly and from a plan.  Per plan kind the smallest
launch the kind accepts runs once through its eager entry point and once recorded, then ``run()``, on identical operands; the outputs
are compared bit for bit.  A row that names the wrong entry point or the wrong argument struct fails here."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BOTH = (torch.bfloat16, torch.float16)


def _rnd(*shape, dtype=torch.float32, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (scale * torch.randn(*shape, generator=g)).to(dtype).to(DEV)


def _zeros(*shape, dtype):
    return torch.zeros(*shape, dtype=dtype, device=DEV)


def _qkv(dt):
    """one 64-query, 64-key, one-head problem: q / x, k [keys, 64], vt [64, keys], wq"""
    return _rnd(64, 64, dtype=dt, seed=1), _rnd(64, 64, dtype=dt, seed=2), _rnd(64, 64, dtype=dt, seed=3), _rnd(64, 64, dtype=dt, seed=4, scale=0.125)


def _gemm(ctx, dt):
    return ctx.gemm(_rnd(64, 64, dtype=dt, seed=1), _rnd(64, 64, dtype=dt, seed=2), cfg=(64, 64, 1))


def _gemm_dual(ctx, dt):
    return ctx.gemm_dual(dict(x=_rnd(64, 64, dtype=dt, seed=1), w=_rnd(64, 64, dtype=dt, seed=2)),
                         dict(x=_rnd(64, 64, dtype=dt, seed=3), w=_rnd(64, 64, dtype=dt, seed=4)))


def _attn(ctx, dt):
    q, k, vt, _ = _qkv(dt)
    return ctx.attention(q, k, vt, _zeros(64, 64, dtype=dt), 1, 1, 64, 64, 64, 64, 64, 64, 64, 0.125)


def _xattn(ctx, dt):
    x, k, vt, wq = _qkv(dt)
    return ctx.cross_attention(x, wq, k, vt, _zeros(64, 64, dtype=dt), 1, 1, 64, 64, 64, 64, 64, 0.125)


def _xattn_regions(ctx, dt):
    x, k, vt, wq = _qkv(dt)
    k2, vt2 = _rnd(64, 64, dtype=dt, seed=5), _rnd(64, 64, dtype=dt, seed=6)
    mask = (_rnd(1, 64, seed=7) > 0).float()
    return ctx.cross_attention_regions(x, wq, k, vt, _zeros(64, 64, dtype=dt), 1, 1, 64, 64, 64, 64, 64, 0.125, k2, vt2, 64, 64, 64, 64, 1, mask)


def _attn_small(ctx, dt):
    q, k, v, _ = _qkv(dt)
    return ctx.attention_small(q, k, v, 1, 1, 64, 64, 64, 64, 0.125)


def _attn_enc(causal):
    def case(ctx, dt):
        q, k, v, _ = _qkv(dt)
        return ctx.attention_enc(q, k, v, 1, 1, 64, 64, causal=causal)
    return case


def _groupnorm(ctx, dt):
    return ctx.groupnorm(_rnd(1, 64, 32, dtype=dt, seed=1), _rnd(32, dtype=dt, seed=2), _rnd(32, dtype=dt, seed=3), 8, 1e-5, True)       # GN_ALL


def _layernorm(ctx, dt):
    return ctx.layernorm(_rnd(64, 64, dtype=dt, seed=1), _rnd(64, dtype=dt, seed=2), _rnd(64, dtype=dt, seed=3), 1e-5)


def _ew_add(ctx, dt):
    from imagharmony_amd import lib as L
    return ctx.ew(L.EW_ADD, _zeros(64, dtype=dt), a=_rnd(64, dtype=dt, seed=1), b=_rnd(64, dtype=dt, seed=2), n=64)


def _step_seeded(ctx, dt):
    """S = 1, HW = 64, CFG on, history on; the step counter points at row 1 of the six-column table"""
    from imagharmony_amd import lib as L
    lat, hist = _rnd(1, 4, 64, seed=1), _rnd(1, 4, 64, seed=2)
    tab = _rnd(4, 6, seed=3)
    tab[1] = torch.tensor([0.9, -0.3, 0.45, 0.7, 1.6, -1.2])
    step = torch.full((1,), 1, dtype=torch.int32, device=DEV)
    seeds = torch.tensor([[42, 7, 0, 0]], dtype=torch.int32, device=DEV)
    ctx.ew(L.EW_CFG_MSTEP, lat, a=_rnd(2, 64, 4, dtype=dt, seed=4), tab=tab, step=step, hist=hist, seeds=seeds, i=(1, 64, 0, 1, 0, 0), f=(0.0, 0.0, 4.0, 0.0))
    return lat, hist


def _randn_seeded(ctx, dt):
    return ctx.randn_seeded(torch.tensor([[42, 7, 0, 0]], dtype=torch.int32, device=DEV), 64, row=3)


def _clip_preprocess(ctx, dt):
    return ctx.clip_preprocess(_rnd(1, 3, 16, 20, seed=1).clamp(-1, 1), _zeros(1, 3 * 14 * 14, dtype=dt), 14, 14, (0.48, 0.46, 0.41), (0.27, 0.26, 0.28))


def _control_add(ctx, dt):
    return ctx.control_add(_rnd(1, 8, 8, 32, dtype=dt, seed=1), _rnd(1, 8, 8, 32, dtype=dt, seed=2), scale=0.5)


def _cases():
    """plan kind -> (the call, the compute dtypes the kind has)"""
    from imagharmony_amd import lib as L
    return {L.OP_GEMM: (_gemm, BOTH), L.OP_GEMM_DUAL: (_gemm_dual, BOTH), L.OP_ATTN: (_attn, BOTH), L.OP_XATTN: (_xattn, BOTH),
            L.OP_XATTN_REGIONS: (_xattn_regions, BOTH), L.OP_ATTN_SMALL: (_attn_small, BOTH), L.OP_ATTN_ENC: (_attn_enc(False), BOTH),
            L.OP_ATTN_ENC_CAUSAL: (_attn_enc(True), BOTH), L.OP_GROUPNORM: (_groupnorm, BOTH), L.OP_LAYERNORM: (_layernorm, BOTH),
            L.OP_EW: (_ew_add, BOTH), L.OP_STEP_SEEDED: (_step_seeded, BOTH),
            L.OP_RANDN_SEEDED: (_randn_seeded, BOTH[:1]),                 # fp32 normals whatever the context computes in
            L.OP_CLIP_PREPROCESS: (_clip_preprocess, BOTH + (torch.float32,)),     # the dtype is that of its output rows
            L.OP_CONTROL_ADD: (_control_add, BOTH)}


def _bits(t):
    return t.contiguous().view(-1).view(torch.uint8)


def test_the_cases_are_the_op_table():
    from imagharmony_amd import lib as L
    assert sorted(_cases()) == sorted(L.OPS)


@pytest.mark.parametrize("kind", [*range(12), 13, 15, 17])
def test_eager_and_recorded_launch_agree_bit_for_bit(kind):
    from imagharmony_amd.ctx import Ctx
    call, dtypes = _cases()[kind]
    for dt in dtypes:
        cdt = dt if dt in BOTH else torch.bfloat16
        eager = call(Ctx(DEV, cdt), dt)
        rec = Ctx(DEV, cdt, record=True)
        planned = call(rec, dt)
        assert [t[1] for t in rec.tags] == [kind if kind != 6 else 0] and [o[0] for o in rec._ops] == [kind], f"kind {kind}: one launch of that kind"
        assert rec.lib.imh_plan_get_kind(rec.plan, 0) == kind
        rec.run()
        torch.cuda.synchronize()
        eager, planned = (o if isinstance(o, tuple) else (o,) for o in (eager, planned))
        assert len(eager) == len(planned) > 0
        for e, p in zip(eager, planned):
            assert e.shape == p.shape and e.dtype == p.dtype and _bits(e).any(), f"kind {kind} {dt}: an output of zero bits"
            assert torch.equal(_bits(e), _bits(p)), f"kind {kind} {dt}: eager and recorded outputs differ"
