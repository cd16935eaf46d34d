"""CPU (no GPU): what a real DenoiseEngine records and caches on a tiny UNet under dry recording contexts -- the forward part of every
plan as a launch count and a hash, its step tail op for op with every pointer resolved to the name of the engine buffer behind it, the
plan keys, the plan cache's hits, evictions and drops, and what fork() shares -- against the trace recorded before the engine kept one
record per plan and one step-tail emitter (tools/engine_trace.py states the cases; tests/golden/engine_trace.json is its output at that
commit)."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("engine_trace", os.path.join(ROOT, "tools", "engine_trace.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TOOL = _tool()
with open(os.path.join(ROOT, "tests", "golden", "engine_trace.json")) as f:
    GOLDEN = json.load(f)


def test_the_case_list_is_the_recorded_one():
    names = sorted(TOOL.cases())
    assert names == sorted(GOLDEN)
    assert [len([n for n in names if n.startswith(k)]) for k in ("plan/", "sequence/")] == [18, 2]
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "engine_trace.json")) <= \
        os.path.getsize(os.path.join(ROOT, "tests", "golden", "frontend_trace.json"))


@pytest.mark.parametrize("name", sorted(n for n in GOLDEN if n.startswith("plan/")))
def test_recorded_plan_matches_the_recorded_one(name):
    got = json.loads(json.dumps(TOOL.cases()[name]()))             # tuples -> lists, as the file holds them
    want = GOLDEN[name]
    assert got["key"] == want["key"] and got["state"] == want["state"]
    assert got["forward"] == want["forward"]
    for part in ("tail", "plan_tail"):
        assert (part in got) == (part in want)
        for i, (g, w) in enumerate(zip(got.get(part, ()), want.get(part, ()))):
            assert g == w, f"{name}: {part} op {i} differs: {g['descr']} against the recorded {w['descr']}"
        assert len(got.get(part, ())) == len(want.get(part, ()))
    assert got == want


def test_plan_cache_events_match_the_recorded_ones():
    got = json.loads(json.dumps(TOOL.cases()["sequence/plan_cache"]()))
    want = GOLDEN["sequence/plan_cache"]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"event {i} differs: {g[0]}"
    assert len(got) == len(want)


def test_fork_shares_what_the_recorded_fork_shared():
    got = json.loads(json.dumps(TOOL.cases()["sequence/fork"]()))
    want = GOLDEN["sequence/fork"]
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k] == want[k], k


def test_a_second_conditioning_before_any_schedule_carries_what_there_is():
    """a StepState has no coef_tab until set_schedule gives it one: the carry-over of set_conditioning and fork() take it as None"""
    def run():
        eng = TOOL.engine()
        first = eng.st
        TOOL.condition(eng)
        assert eng.st is not first and eng.st.coef_tab is None and eng.st.t_table is None and eng.plan is None
        assert eng.fork().st.coef_tab is None
        eng.set_schedule(TOOL.hs.DDIMScheduler(), 4)
        tab = eng.st.coef_tab
        TOOL.condition(eng)
        assert eng.st.coef_tab is tab and eng.st.temb_table is None and eng._sched_key is not None
    TOOL.dry(run)()


with open(os.path.join(ROOT, "tests", "golden", "engine_args.json")) as f:
    ARGS = json.load(f)


def test_the_argument_digests_cover_every_plan_case():
    assert sorted(ARGS) == sorted(n for n in GOLDEN if n.startswith("plan/")) == sorted(TOOL.PLAN_CASES)


@pytest.mark.parametrize("name", sorted(ARGS))
def test_recorded_plan_arguments_match_the_recorded_ones(name):
    """per plan of the case (the tail plan of a split engine second): every field of every launch's argument struct, pointers as
    (allocation, byte offset), prefetch fields included (tools/forward_trace.py args_digest), against the digest taken before Ctx got
    one recorder and shared argument packers; the rest of the case is what it is without the digest"""
    got = json.loads(json.dumps(TOOL.cases()[name](args=True)))
    assert got.pop("args") == ARGS[name]
    assert got == GOLDEN[name]
