"""CPU (no GPU, no library): the host front end's call trace -- every engine, scheduler and VAE-encoder call of the four pipelines'
``__call__`` and of ``IPAdapterXL.generate_pns``, in order, with the bits of every tensor handed over -- against the trace recorded
before the pipelines shared one call skeleton and PNS the pipelines' edit preparation (tools/frontend_trace.py states the cases and
the fakes; tests/golden/frontend_trace.json is its output at that commit)."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("frontend_trace", os.path.join(ROOT, "tools", "frontend_trace.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TOOL = _tool()
with open(os.path.join(ROOT, "tests", "golden", "frontend_trace.json")) as f:
    GOLDEN = json.load(f)


def test_the_grid_is_the_recorded_one():
    names = sorted(TOOL.cases())
    assert names == sorted(GOLDEN)
    assert [len([n for n in names if n.startswith(k)]) for k in ("pipe/", "pns/", "cross/")] == [20, 6, 3]


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_call_trace_matches_the_recorded_one(name):
    got = json.loads(json.dumps(TOOL.cases()[name]()))             # tuples -> lists, as the file holds them
    want = GOLDEN[name]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{name}: call {i} differs: {g[0]} against the recorded {w[0]}"
    assert len(got) == len(want), f"{name}: {len(got)} calls against the recorded {len(want)}"
