"""CPU (no GPU): what the full-width SDXL UNet and ControlNet forwards record under dry contexts -- per case the launch count, a hash of
the (tag, kind, descr, shape, epilogue) list and a second one that also covers which buffer every launch reads and writes; per model a
hash of the parameter names, of the processor names and of the cross-attention order -- against the trace recorded before unet.py and
controlnet.py got one encoder base class and one GroupNorm front end (tools/forward_trace.py states the cases;
tests/golden/forward_trace.json is its output at that commit)."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("forward_trace", os.path.join(ROOT, "tools", "forward_trace.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TOOL = _tool()
with open(os.path.join(ROOT, "tests", "golden", "forward_trace.json")) as f:
    GOLDEN = json.load(f)


def test_the_case_list_is_the_recorded_one():
    names = sorted(TOOL.cases())
    assert names == sorted(GOLDEN)
    assert [len([n for n in names if n.startswith(k)]) for k in ("unet/", "unet/ab/", "unet9/", "controlnet/", "adapter/", "model/")] == \
        [13 + 8, 8, 1, 2, 2, 3]
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "forward_trace.json")) <= \
        os.path.getsize(os.path.join(ROOT, "tests", "golden", "frontend_trace.json"))


def test_the_recorded_launch_counts_are_the_known_ones():
    """the figures the forward had when the golden was taken, conditioning included"""
    assert [GOLDEN[k]["launches"] for k in ("unet/1x128x128", "unet9/1x128x128", "controlnet/1x128x128", "adapter/1x128x128")] == \
        [745, 745, 1117, 749]


@pytest.mark.parametrize("name", sorted(n for n in GOLDEN if not n.startswith("model/")))
def test_recorded_forward_matches_the_recorded_one(name):
    got = TOOL.cases()[name]()
    want = GOLDEN[name]
    if got != want:
        diff = {d: (got["descr"].get(d, 0), want["descr"].get(d, 0)) for d in sorted(set(got["descr"]) | set(want["descr"]))
                if got["descr"].get(d, 0) != want["descr"].get(d, 0)}
        print(f"{name}: {got['launches']} launches against the recorded {want['launches']}; descr: (now, recorded) {diff}")
    assert got["launches"] == want["launches"] and got["descr"] == want["descr"]
    assert got["sha1"] == want["sha1"], "the same launches by name, but an order, tag, shape or epilogue differs"
    assert got["sha1_alias"] == want["sha1_alias"], "the same launch list, but a launch reads or writes another buffer"
    assert got == want


@pytest.mark.parametrize("name", sorted(n for n in GOLDEN if n.startswith("model/")))
def test_parameter_and_processor_names_match_the_recorded_ones(name):
    got = TOOL.cases()[name]()
    for k in ("state_dict", "attn_processors", "attn2_modules"):
        assert got[k] == GOLDEN[name][k], k
    assert got == GOLDEN[name]


# ------------------------------------------------------------------------------------------------------------------ the exact arguments
with open(os.path.join(ROOT, "tests", "golden", "forward_args.json")) as f:
    ARGS = json.load(f)


def test_the_argument_digests_cover_every_forward_and_45_direct_calls():
    names = sorted(TOOL.args_cases())
    assert names == sorted(ARGS)
    assert sorted(n for n in names if not n.startswith("direct/")) == sorted(n for n in GOLDEN if not n.startswith("model/"))
    assert len([n for n in names if n.startswith("direct/")]) == len(TOOL.DIRECT) == 45
    assert ARGS["unet/1x128x128"][0] == 745


@pytest.mark.parametrize("name", sorted(ARGS))
def test_recorded_arguments_match_the_recorded_ones(name):
    """every field of every launch's argument struct, pointers as (allocation, byte offset), prefetch fields included
    (tools/forward_trace.py args_digest), against the digest taken before Ctx got one recorder and shared argument packers"""
    got = TOOL.args_cases()[name]()
    assert got[0] == ARGS[name][0], "another launch count"
    assert got == ARGS[name], "the same launch count, but a scalar argument, a byte offset or a prefetch field differs"
