"""CPU: the seeded step noise (include/imh.h "seeded step noise") -- no GPU.

1. Philox4x32-10 known answers, from the numpy restatement (imagharmony_amd/noise.py) and from the library's host entry;
2. the host entry (csrc/imh_philox.h compiled for the host) against the restatement: words bit-equal, normals within 1e-5;
3. the restatement's own statistics at 2^20 normals;
4. the ABI stayed what it was and the new entries are bound in header order; bad arguments are status codes;
5. the host logic of the engine, PNS and the pipelines around seeds."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from test_multistep_host import _cpu_engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Random123's published vectors for philox4x32-10 (kat_vectors): counter, key, words
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
# the ceiling of the GPU fill test (tests/test_gpu_seeded_noise.py): 29 fp32 ulps at |z| = 5.77
CEILING = 1e-5


def _host_fill(seed_rows, HW, row, raw, stream=0, quad0=0, step=None):
    from imagharmony_amd import lib
    l = lib.load()
    rows = np.ascontiguousarray(seed_rows, dtype=np.uint32)
    y = np.zeros((rows.shape[0], 4, HW), dtype=np.uint32 if raw else np.float32)
    a = lib.RandnArgs()
    a.y, a.seeds, a.S, a.HW, a.row, a.stream, a.raw, a.quad0 = y.ctypes.data, rows.ctypes.data, rows.shape[0], HW, row, stream, int(raw), quad0
    if step is not None:
        step = np.array([step], dtype=np.int32)
        a.step = step.ctypes.data
    assert l.imh_randn_seeded_host(C.byref(a)) == 0, l.imh_last_error()
    return y


# ------------------------------------------------------------------------------------ 1. known answers
@pytest.mark.parametrize("ctr,key,want", KAT, ids=["zeros", "ones", "pi"])
def test_philox_known_answers(ctr, key, want):
    from imagharmony_amd import noise
    got = [int(w) for w in noise.philox4x32_10(ctr, key)]
    assert got == list(want), [hex(w) for w in got]
    # the host entry: counter = (quad, row, stream, lane), key = (k0, k1); one quad starting at quad0 = counter word 0
    y = _host_fill([[key[0], key[1], ctr[3], 0]], 1, ctr[1], True, stream=ctr[2], quad0=ctr[0])
    assert [int(w) for w in y.reshape(-1)] == list(want), [hex(int(w)) for w in y.reshape(-1)]
    # ... and with the row read through *step (an int32 whose bits are the counter word)
    y = _host_fill([[key[0], key[1], ctr[3], 0]], 1, 12345, True, stream=ctr[2], quad0=ctr[0], step=np.uint32(ctr[1]).astype(np.int32))
    assert [int(w) for w in y.reshape(-1)] == list(want)


def test_uniform_mapping_is_exact_and_open():
    """u = ((w >> 9) + 0.5) * 2^-23 is representable in fp32 at both ends and never 0 or 1 (an 8-bit shift would round to 1.0)"""
    for w, want in ((0, 2.0 ** -24), (0xffffffff, 1 - 2.0 ** -24)):
        u = np.float32((np.float32(w >> 9) + np.float32(0.5)) * np.float32(2.0 ** -23))
        assert float(u) == want and 0.0 < float(u) < 1.0
    assert float(np.float32(((0xffffffff >> 8) + 0.5) * 2.0 ** -24)) == 1.0
    from imagharmony_amd import noise
    z = noise.normals_from_words(np.array([[0, 0, 0xffffffff, 0xffffffff]], dtype=np.uint32))
    assert np.isfinite(z).all() and np.abs(z).max() <= 5.77


# ------------------------------------------------------------------------------------ 2. host entry == restatement
SEEDS = [0, 42, 2 ** 63 + 5, 2 ** 64 - 1]


@pytest.mark.parametrize("row", [0, 29])
@pytest.mark.parametrize("lane", [0, 3])
def test_host_entry_matches_the_restatement(row, lane):
    """HW = 35: 4 * 35 = 140 elements per sample, the quads straddle the channel boundaries.  Words bit-equal; normals within the GPU
    test's ceiling (the host computes them in float64 and rounds once, as the restatement does: the difference is in fact 0 or 1 ulp)"""
    from imagharmony_amd import noise
    HW = 35
    rows = noise.seed_rows(SEEDS, [lane] * len(SEEDS))
    assert rows.dtype == np.uint32 and rows.shape == (4, 4)
    assert rows[2].tolist() == [5, 0x80000000, lane, 0] and rows[3].tolist() == [0xffffffff, 0xffffffff, lane, 0]
    want_w = noise.seeded_words(SEEDS, row, (4, HW), [lane] * len(SEEDS))
    assert np.array_equal(_host_fill(rows, HW, row, True), want_w)
    want_z = noise.seeded_randn(SEEDS, row, (4, HW), [lane] * len(SEEDS))
    got = _host_fill(rows, HW, row, False)
    err = float(np.abs(got.astype(np.float64) - want_z.astype(np.float64)).max())
    print(f"host normals vs float64 restatement, row {row} lane {lane}: max |dz| = {err:.3e}")
    assert want_z.dtype == np.float32 and err <= CEILING
    # element e takes z_(e & 3) of quad e >> 2: the (4, 5, 7) view of the same sample is the same numbers
    assert np.array_equal(noise.seeded_randn(SEEDS, row, (4, 5, 7), [lane] * len(SEEDS)).reshape(4, 4, HW), want_z)
    # nothing but (seed, lane, row, stream, element) enters: a sample alone equals the sample in the batch; row, lane, stream matter
    assert np.array_equal(noise.seeded_words([42], row, (4, HW), [lane])[0], want_w[1])
    assert not np.array_equal(noise.seeded_words([42], row + 1, (4, HW), [lane])[0], want_w[1])
    assert not np.array_equal(noise.seeded_words([42], row, (4, HW), [lane + 1])[0], want_w[1])
    assert not np.array_equal(noise.seeded_words([42], row, (4, HW), [lane], stream=1)[0], want_w[1])


# ------------------------------------------------------------------------------------ 3. statistics
N_STAT = (4, 512, 512)          # 2^20 normals
# 5 sigma of each statistic at N = 2^20: mean 1/sqrt(N) = 9.8e-4, variance sqrt(2/N) = 1.4e-3, fourth moment sqrt(96/N) = 9.6e-3 -> 4.9e-3,
# 6.9e-3, 4.8e-2 (held tighter, at 0.025); the mean product of two independent rows has sigma 1/sqrt(N)
MEAN_TOL, VAR_TOL, M4_TOL, PROD_TOL = 5e-3, 7e-3, 0.025, 5e-3


def moments_ok(z):
    z = np.asarray(z, dtype=np.float64).ravel()
    m, v, m4 = z.mean(), z.var(), (z ** 4).mean()
    return (abs(m) <= MEAN_TOL and abs(v - 1) <= VAR_TOL and abs(m4 - 3) <= M4_TOL and np.abs(z).max() <= 5.77), (m, v - 1, m4)


@pytest.mark.parametrize("seed,row", [(42, 0), (42, 29), (2 ** 63 + 5, 7)])
def test_restatement_statistics(seed, row):
    from imagharmony_amd import noise
    ok, (m, dv, m4) = moments_ok(noise.seeded_randn([seed], row, N_STAT))
    print(f"seed {seed} row {row}: mean {m:.2e}, var - 1 {dv:.2e}, E z^4 {m4:.4f}")
    assert ok, (m, dv, m4)


def test_rows_and_seeds_are_uncorrelated():
    from imagharmony_amd import noise
    a = noise.seeded_randn([42], 0, N_STAT).astype(np.float64).ravel()
    b = noise.seeded_randn([42], 1, N_STAT).astype(np.float64).ravel()
    c = noise.seeded_randn([43], 0, N_STAT).astype(np.float64).ravel()
    p_rows, p_seeds = float((a * b).mean()), float((a * c).mean())
    print(f"mean product: rows 0 / 1 of seed 42 {p_rows:.2e}, seeds 42 / 43 at row 0 {p_seeds:.2e}")
    assert abs(p_rows) <= PROD_TOL and abs(p_seeds) <= PROD_TOL


# ------------------------------------------------------------------------------------ 4. ABI
def _struct_names(hdr, cname):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        parts = decl.replace("*", " ").split(",")
        names.append(parts[0].split()[-1])
        names.extend(p.strip() for p in parts[1:])
    return names


def test_abi_is_additive():
    from imagharmony_amd import lib
    hdr = open(os.path.join(ROOT, "include", "imh.h")).read()
    l = lib.load()
    assert l.imh_abi_version() == lib.ABI_VERSION == 13 and re.search(r"#define IMH_ABI_VERSION 13\b", hdr)
    body = re.search(r"enum imh_ew_op \{(.*?)\n\};", hdr, re.S).group(1)
    names = re.findall(r"^\s*(IMH_EW_[A-Z0-9_]+)", re.sub(r"/\*.*?\*/", "", body, flags=re.S), re.M)
    assert names == ["IMH_EW_TIMESTEP", "IMH_EW_SILU", "IMH_EW_CONCAT", "IMH_EW_CONV_IN", "IMH_EW_CFG_STEP", "IMH_EW_CAST_F32", "IMH_EW_ADD",
                     "IMH_EW_STEP_SET", "IMH_EW_CFG_RESCALE", "IMH_EW_SOFTMAX", "IMH_EW_ROW_STATS", "IMH_EW_STEP_ROW", "IMH_EW_GATHER_ROWS",
                     "IMH_EW_CFG_MSTEP"]
    assert _struct_names(hdr, "imh_ew_args") == [f[0] for f in lib.EwArgs._fields_] == [
        "a", "b", "y", "w", "bias", "tab", "step", "n", "i0", "i1", "i2", "i3", "i4", "i5", "f0", "f1", "f2", "f3", "dtype", "x2", "noise", "mask",
        "blend_tab"]
    kinds = dict((k, int(v)) for k, v in re.findall(r"(IMH_OP_[A-Z_]+) = (\d+)", re.search(r"enum imh_op_kind \{(.*?)\};", hdr, re.S).group(1)))
    assert kinds["IMH_OP_ATTN_ENC_CAUSAL"] == 9 and kinds["IMH_OP_STEP_SEEDED"] == 10 == lib.OP_STEP_SEEDED
    assert kinds["IMH_OP_RANDN_SEEDED"] == 11 == lib.OP_RANDN_SEEDED and len(kinds) == 12
    assert _struct_names(hdr, "imh_seeded_args") == [f[0] for f in lib.SeededArgs._fields_]
    assert _struct_names(hdr, "imh_randn_args") == [f[0] for f in lib.RandnArgs._fields_]
    assert lib.SeededArgs._fields_[0][1] is lib.EwArgs
    # every new entry says what memory it touches
    for entry in ("imh_step_seeded", "imh_randn_seeded"):
        before = hdr[:hdr.index(f"int {entry}(")]
        assert "Memory:" in before[-2500:], entry


def test_bad_arguments_are_status_codes():
    from imagharmony_amd import lib
    l = lib.load()
    a = lib.SeededArgs()
    a.ew.y = a.ew.a = a.ew.tab = a.ew.step = 64
    a.ew.i0, a.ew.i1 = 1, 64
    assert l.imh_step_seeded(C.byref(a), None) == -1 and b"imh_step_seeded" in l.imh_last_error() and b"seeds" in l.imh_last_error()
    a.seeds, a.ew.bias = 64, 64
    assert l.imh_step_seeded(C.byref(a), None) == -1 and b"imh_step_seeded" in l.imh_last_error() and b"bias" in l.imh_last_error()
    assert l.imh_step_seeded(None, None) == -1
    r = lib.RandnArgs()
    r.y = 64
    r.S, r.HW = 1, 4
    for fn, args in ((l.imh_randn_seeded, (C.byref(r), None)), (l.imh_randn_seeded_host, (C.byref(r),))):
        assert fn(*args) == -1 and b"imh_randn_seeded" in l.imh_last_error() and b"seeds" in l.imh_last_error()
    r.seeds, r.HW = 64, 0
    assert l.imh_randn_seeded_host(C.byref(r)) == -2 and b"imh_randn_seeded_host" in l.imh_last_error()
    p = l.imh_plan_create()
    assert l.imh_plan_add(p, lib.OP_STEP_SEEDED, C.byref(a), 0, 3) == 0 and l.imh_plan_get_kind(p, 0) == 10
    assert l.imh_plan_add(p, lib.OP_RANDN_SEEDED, C.byref(r), 0, 4) == 1 and l.imh_plan_get_kind(p, 1) == 11
    assert l.imh_plan_add(p, 12, C.byref(r), 0, 0) == -1
    l.imh_plan_destroy(p)
    import imagharmony_amd
    assert imagharmony_amd.seeded_randn.__module__ == imagharmony_amd.seed_rows.__module__ == "imagharmony_amd.noise"


# ------------------------------------------------------------------------------------ 5. host logic
def test_seed_range_errors():
    from imagharmony_amd import noise
    for bad in (-1, 2 ** 64, 1.5, "7", None, True):
        with pytest.raises(ValueError):
            noise.seed_rows([bad])
    with pytest.raises(ValueError):
        noise.seed_rows([1, 2], [0])
    with pytest.raises(ValueError):
        noise.seeded_randn([1], 0, (3, 5))          # 15 elements: not whole quads
    assert noise.seed_rows([2 ** 64 - 1, 0]).tolist() == [[0xffffffff, 0xffffffff, 0, 0], [0, 0, 0, 0]]
    assert noise.seed_rows([7, 7], [0, 1])[:, 2].tolist() == [0, 1]


def test_plan_key_and_state_of_a_seeded_schedule():
    from imagharmony_amd import schedulers as hs
    e = _cpu_engine(S=2, H=5, W=7)
    ea = hs.EulerAncestralDiscreteScheduler()
    e.set_schedule(ea, 6)
    k_bank = e._sched_key
    assert e.stochastic and not e.seeded and e.st.seed_rows is None and tuple(e.st.noise_bank.shape) == (6, 2, 4, 5, 7)
    e.set_schedule(ea, 6, seeded_noise=True)
    k_seed = e._sched_key
    assert k_seed != k_bank and k_seed[:-1] == k_bank[:-1]
    assert k_seed.seeded and not k_bank.seeded and k_seed == k_bank._replace(seeded=True)
    assert e.stochastic and e.seeded and e.st.noise_bank is None
    assert e.st.seed_rows.dtype == torch.int32 and tuple(e.st.seed_rows.shape) == (2, 4)
    assert tuple(e.st.coef6_tab.shape) == (6, 6)
    # the SDE multistep sampler keeps its history slot next to the seed rows
    e.set_schedule(hs.DPMSolverMultistepScheduler(algorithm_type="sde-dpmsolver++"), 6, seeded_noise=True)
    assert e.seeded and e.st.hist is not None and e.st.noise_bank is None and e.st.seed_rows is not None
    # a deterministic sampler ignores the flag: today's key, today's state
    e.set_schedule(hs.DPMSolverMultistepScheduler(), 6)
    k_det = e._sched_key
    e.set_schedule(hs.DPMSolverMultistepScheduler(), 6, seeded_noise=True)
    assert e._sched_key == k_det and not e.seeded and e.st.seed_rows is None
    e.set_schedule(hs.DDIMScheduler(), 6, seeded_noise=True)
    assert not e.seeded and not e.general and e.st.seed_rows is None


def test_step_seeds_are_required_where_seeded_and_refused_elsewhere():
    from imagharmony_amd import lib as L
    from imagharmony_amd import noise
    from imagharmony_amd import schedulers as hs
    e = _cpu_engine(S=2, H=5, W=7)
    e.set_schedule(hs.DPMSolverMultistepScheduler(algorithm_type="sde-dpmsolver++"), 6, t_start=2, seeded_noise=True)
    e.st.hist.fill_(float("nan"))
    e._start_general_step(step_seeds=[42, 2 ** 63 + 5], step_lanes=[0, 3])
    assert np.array_equal(e.st.seed_rows.numpy().view(np.uint32), noise.seed_rows([42, 2 ** 63 + 5], [0, 3])) and (e.st.hist == 0).all()
    e._start_general_step(step_seeds=[7, 7])
    assert e.st.seed_rows.numpy().view(np.uint32).tolist() == [[7, 0, 0, 0], [7, 0, 0, 0]]
    with pytest.raises(L.ImhError, match="step_seeds"):
        e._start_general_step()
    with pytest.raises(L.ImhError, match="generator"):
        e._start_general_step(generator=torch.Generator().manual_seed(1), step_seeds=[1, 2])
    with pytest.raises(L.ImhError, match="step_noise"):
        e._start_general_step(step_noise=torch.zeros(4, 2, 4, 5, 7), step_seeds=[1, 2])
    with pytest.raises(L.ImhError, match="2 samples"):
        e._start_general_step(step_seeds=[1])
    for bad in ([1, -1], [2 ** 64, 0], [0.5, 1]):
        with pytest.raises(ValueError):
            e._start_general_step(step_seeds=bad)
    # a bank schedule, a deterministic general schedule and a two-term schedule refuse seeds
    e.set_schedule(hs.EulerAncestralDiscreteScheduler(), 6)
    with pytest.raises(L.ImhError, match="seeded schedule"):
        e._start_general_step(step_seeds=[1, 2])
    e.set_schedule(hs.DPMSolverMultistepScheduler(), 6, seeded_noise=True)
    with pytest.raises(L.ImhError, match="seeded schedule"):
        e._start_general_step(step_seeds=[1, 2])

    class _Noop:
        def replay(self):
            pass

        def ew(self, *a, **k):
            pass
    e.set_schedule(hs.DDIMScheduler(), 6)
    e.plan, e.eager, e.cfg_role, e.do_cfg = _Noop(), _Noop(), None, True
    e.st.latents = torch.zeros(2, 4, 5, 7)
    e.init_noise_sigma = 1.0
    with pytest.raises(L.ImhError, match="seeded schedule"):
        e.denoise(torch.zeros(2, 4, 5, 7), step_seeds=[1, 2])
    e.denoise(torch.zeros(2, 4, 5, 7))


def test_cfg_split_runs_a_stochastic_scheduler_only_with_a_seeded_schedule_and_seeds():
    from imagharmony_amd import schedulers as hs
    e = _cpu_engine(S=2, H=5, W=7)
    e.cfg_role, e.do_cfg = 0, True
    lat = torch.zeros(2, 4, 5, 7)

    class Reached(Exception):
        pass

    def record():
        raise Reached()
    e._record = record
    ea = hs.EulerAncestralDiscreteScheduler()
    e.set_schedule(ea, 6)
    for kw in ({}, dict(step_seeds=[1, 2])):                      # a bank schedule: refused with or without seeds
        with pytest.raises(NotImplementedError, match="stochastic"):
            e.denoise_cfg_split(lat, None, **kw)
    e.set_schedule(ea, 6, seeded_noise=True)
    with pytest.raises(NotImplementedError, match="stochastic"):   # seeded, but no seeds
        e.denoise_cfg_split(lat, None)
    with pytest.raises(Reached):                                   # seeded and seeds: past the check, on to recording
        e.denoise_cfg_split(lat, None, step_seeds=[1, 2])


@pytest.mark.parametrize("batch", [1, 2])
def test_run_pns_hands_each_group_its_seeds(batch):
    from imagharmony_amd import pns
    seeds = [3, 9, 27]
    calls = []

    def rec(name):
        def fn(noise, **kw):
            calls.append((name, noise.shape[0], kw))
            return noise.clone()
        return fn
    scorer = lambda lat: lat.flatten(1).mean(1)
    r = pns.run_pns(rec("pre"), seeds, (1, 4, 8, 8), scorer=scorer, final_fn=rec("fin"), batch=batch, pass_seeds=True)
    groups = [seeds[i:i + batch] for i in range(0, len(seeds), batch)]
    assert calls[:-1] == [("pre", len(g), {"seeds": g}) for g in groups]
    assert calls[-1] == ("fin", 1, {"seeds": [r["best_seed"]]})
    calls.clear()
    r2 = pns.run_pns(rec("pre"), seeds, (1, 4, 8, 8), scorer=scorer, final_fn=rec("fin"), batch=batch)
    assert all(kw == {} for _, _, kw in calls) and len(calls) == len(groups) + 1 and r2["best_seed"] == r["best_seed"]


def test_two_stage_fns_pass_seeds_only_under_a_seeded_schedule():
    from imagharmony_amd import pns

    class Eng:
        def __init__(self, stochastic):
            self.stochastic, self.seeded, self.log = stochastic, False, []

        def set_schedule(self, sch, steps, **kw):
            self.seeded = bool(kw.get("seeded_noise")) and self.stochastic
            self.log.append(("sched", steps, kw))

        def denoise(self, noise, **kw):
            self.log.append(("denoise", kw))
            return noise
    z = torch.zeros(2, 4, 8, 8)
    e = Eng(True)
    pre, fin = pns.two_stage_fns(e, None, 2, 3, step_noise="seed", t_start=0)
    pre(z, seeds=[5, 6]); fin(z[:1], seeds=[6])
    assert e.log == [("sched", 2, dict(seeded_noise=True, t_start=0)), ("denoise", dict(step_seeds=[5, 6])),
                     ("sched", 3, dict(seeded_noise=True, t_start=0)), ("denoise", dict(step_seeds=[6]))]
    with pytest.raises(ValueError, match="pass_seeds"):
        pre(z)
    e = Eng(False)                                   # a deterministic sampler: the flag is ignored, no seeds are handed on
    pre, fin = pns.two_stage_fns(e, None, 2, 3, step_noise="seed")
    pre(z, seeds=[5, 6])
    assert e.log[-1] == ("denoise", {})
    e = Eng(True)                                    # the default: today's calls, keyword for keyword
    pre, fin = pns.two_stage_fns(e, None, 2, 3)
    pre(z); fin(z)
    assert e.log == [("sched", 2, {}), ("denoise", {}), ("sched", 3, {}), ("denoise", {})]
    with pytest.raises(ValueError):
        pns.two_stage_fns(e, None, step_noise="device")


def test_pipelines_derive_the_seed_table_from_their_generators():
    from imagharmony_amd import noise
    from imagharmony_amd.pipeline import (StableDiffusionXLCustomPipeline, StableDiffusionXLImg2ImgCustomPipeline,
                                          StableDiffusionXLInpaintCustomPipeline)
    for cls in (StableDiffusionXLCustomPipeline, StableDiffusionXLImg2ImgCustomPipeline, StableDiffusionXLInpaintCustomPipeline):
        tab = cls.step_seed_table
        assert tab("generator", None, 3) is None and tab("generator", torch.Generator().manual_seed(1), 3) is None
        seeds, lanes = tab("seeded", torch.Generator().manual_seed(2 ** 63 + 5), 3)
        assert seeds == [2 ** 63 + 5] * 3 and lanes == [0, 1, 2]
        assert noise.seed_rows(seeds, lanes).tolist() == [[5, 0x80000000, s, 0] for s in range(3)]
        seeds, lanes = tab("seeded", [torch.Generator().manual_seed(10 + s) for s in range(3)], 3)
        assert seeds == [10, 11, 12] and lanes == [0, 0, 0]
        with pytest.raises(ValueError, match="generator"):
            tab("seeded", None, 3)
        with pytest.raises(ValueError, match="2 generators"):
            tab("seeded", [torch.Generator(), torch.Generator()], 3)
        with pytest.raises(ValueError, match="step_noise"):
            tab("device", None, 3)

    class _E:
        seeded = True
    kw = StableDiffusionXLCustomPipeline._noise_kw(_E, ([4, 4], [0, 1]), "g")
    assert kw == dict(step_seeds=[4, 4], step_lanes=[0, 1])
    _E.seeded = False                                # a deterministic scheduler under step_noise="seeded": nothing to seed
    assert StableDiffusionXLCustomPipeline._noise_kw(_E, ([4, 4], [0, 1]), "g") == dict(generator="g")
    assert StableDiffusionXLCustomPipeline._noise_kw(_E, None, "g") == dict(generator="g")
