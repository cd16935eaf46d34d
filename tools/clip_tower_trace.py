"""CPU only: writes ``tests/golden/clip_tower_trace.json`` -- per dry recording of the CLIP towers that tests/test_derived_host.py lists,
what its ``_describe`` returns: ``ctx.tags``, the buffer aliasing, and the digest of the exact launch arguments.

    python tools/clip_tower_trace.py [out.json]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_derived_host as T                                                  # noqa: E402


def trace():
    return {name: T._describe(record()["ctx"]) for name, record in T._RECORDINGS.items()}


if __name__ == "__main__":
    text = "{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, sort_keys=True)}" for k, v in sorted(trace().items())) + "\n}\n"
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
