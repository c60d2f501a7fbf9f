"""Records tests/golden/scene_tables.json: for every scene and setter step of tests/scene_tables_cases.py, what a host-only scene answers
(info().device_bytes; byte count and SHA-256 of every AKR_ARRAY_* array) and, with --device on a machine with a GPU, info().device_bytes of
the same scenes created on a context (the "device" key; without --device a recorded "device" key is kept as it is).
Recorded once, at the commit before a scene's device tables were written as one list; tests/test_scene_tables.py and
tests/test_gpu_scene_tables.py hold every later commit to it. python tests/golden/make_scene_tables_golden.py [--device]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from akari_render_amd import capi  # noqa: E402
from tests import scene_tables_cases as T  # noqa: E402

if __name__ == "__main__":
    out = os.path.join(ROOT, "tests", "golden", "scene_tables.json")
    gold = json.load(open(out)) if os.path.exists(out) else {}
    if "--device" in sys.argv:
        ctx, device = capi.Context(0), {}
        T.walk(ctx, lambda key, sc, state, tree: device.__setitem__(key, int(sc.info().device_bytes)))
        gold["device"] = device
    else:
        host = {}
        T.walk(None, lambda key, sc, state, tree: host.__setitem__(key, T.record(sc)))
        gold["host"] = host
    with open(out, "w") as f:
        json.dump(gold, f, indent=1, sort_keys=True)
        f.write("\n")
    print({k: len(v) for k, v in gold.items()}, "->", out)
