"""The megakernel's pair loop visits the same nodes and tests the same triangles as the commit before the loop's text was shared.

With wavefront=0 a wave's lanes are fixed by the pixel order, so when a wave leaves its intersection phase, which lanes it carries and when a
kept scene's exact tests are taken are all deterministic: n_node_visits and n_tri_tests of a session are reproducible and were recorded from
the parent of the commit that introduced trace_pair / InstGate / carry_save (tests/golden/pair_loop_visits.json; its "recorded_with" field
holds the command). The wavefront schedule's trace counters depend on the order in which waves claim the queue: not pinned."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from akari_render_amd import capi, procedural  # noqa: E402
from oracle import scene_json  # noqa: E402
from tests.helpers import make_config, textured_room  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "pair_loop_visits.json")
COUNTERS = ("n_node_visits", "n_tri_tests")
# scene -> options: the flattened arm with stragglers, the flattened arm without (textured kernels), the kept arm and its gate
CASES = {"cbox_bvh": dict(force_bvh=1), "textured_room_bvh": dict(force_bvh=1), "forest_kept": dict(instancing=1)}


def _scene_data(name):
    if name == "cbox_bvh":
        sd = scene_json.load_scene(os.path.join(ROOT, "scenes", "cbox", "scene.json"), 64, 64)
    elif name == "textured_room_bvh":
        sd = textured_room(64, 64, alpha_cutout=True)
    else:
        sd = procedural.instanced_forest(40, 3000, width=64, height=64)
    sd.ggx_table = np.fromfile(os.path.join(ROOT, "tests", "golden", "ggx_dielectric_s.f32"), dtype=np.float32)
    return sd


def measure(ctx, name):
    """64 x 64, 16 spp in 2 passes: 64 waves with mixed path lengths, so phases end with lanes left and traversals are carried."""
    cfg = make_config(spp=16, spp_per_pass=8, max_depth=8)
    with capi.options(wavefront=0, **CASES[name]):
        scene = capi.Scene(ctx, _scene_data(name))
        assert scene.info().uses_bvh == (2 if name == "forest_kept" else 1)
        st = capi.pt_render(ctx, scene, cfg, capi.Film(ctx, 64, 64))
    return {k: int(st[k]) for k in COUNTERS + ("n_closest", "n_shadow")}


@pytest.mark.parametrize("name", sorted(CASES))
def test_megakernel_visit_counters_are_the_parents(ctx, name):
    want = json.load(open(GOLDEN))["scenes"][name]
    got = measure(ctx, name)
    print(name, got)
    assert want, "nothing pinned"
    for k, v in want.items():
        assert got[k] == v, (name, k, got[k], v)


if __name__ == "__main__":  # --record OUT.json: two runs; a counter that differs between them is left out
    ctx = capi.Context(0)
    runs = [{n: measure(ctx, n) for n in sorted(CASES)} for _ in range(2)]
    out = {"recorded_with": "AKR_HIP_LIB=<libakari_hip.so built from the parent commit> python tests/test_gpu_pair_loop_visits.py --record OUT.json, MI355X",
           "scenes": {n: {k: v for k, v in runs[0][n].items() if runs[1][n][k] == v} for n in sorted(CASES)}}
    print(json.dumps(runs))
    json.dump(out, open(sys.argv[sys.argv.index("--record") + 1], "w"), indent=1)
