"""bench.py: a plain run times the headline and prints it with its configuration; --full adds the measurements that take
runs of their own (rooflines, clocks under load, extras, CPU baseline)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_full_is_off_by_default(monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1"])
    assert bench.parse().full is False
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1", "--full"])
    assert bench.parse().full is True


def _bench_line(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "1",
           "--res", "512", "--denoise-steps", "2", *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_line_is_the_headline_and_full_adds_the_rest():
    plain = _bench_line()
    assert plain["full"] is False
    assert plain["metric"] == "512^2 SDXL images/sec (2 DDIM steps, PNS N seeds)"
    assert plain["unit"] == "images/sec" and plain["higher_is_better"] is True and plain["dtype"] == "bf16"
    assert plain["value"] > 0 and abs(plain["value"] * plain["ms_per_step"] - 1e3) < 1e-6      # one GPU: images/sec = 1000 / ms per step
    assert plain["config"]["outputs_finite"] is True
    assert not any(k.startswith("roofline") or k == "cpu_baseline" for k in plain)
    assert "clocks_under_load" not in plain["config"]
    assert len(plain["config"]["conditioning_prepare_ms"]["later_calls"]) == 0

    full = _bench_line("--full", "--no-cpu-baseline", "--in-flight", "1", "--stacked", "1")
    assert full["full"] is True and full["config"]["outputs_finite"] is True
    assert full["roofline"]["launches_per_step"] > 0 and full["roofline_attention"]["launches_per_step"] > 0
    assert "clocks_under_load" in full["config"]
    assert len(full["config"]["conditioning_prepare_ms"]["later_calls"]) == 2
