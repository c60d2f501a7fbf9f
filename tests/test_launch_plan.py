"""Which kernel a pt session launches and how its LDS is laid out, held to the decisions recorded before that logic was gathered into
PtVariant / pt_lds_layout (csrc/kernels.h): every row of tests/launch_plan_matrix.py against tests/golden/pt_launch_plan.json -- the ten
variant flags, the parameter-block fields that follow from them, the staged tables, every LDS offset, the launch's size, and the text
that instantiates a per-scene kernel (a digest: the text is part of the kernel cache's key). No GPU."""
import json
import os

import pytest

from akari_render_amd import abi, capi
from tests import launch_plan_matrix as M
from tests.helpers import make_config

MF_EVAL_METAL, MF_TEXTURED = 1 << 3, 1 << 8  # csrc/device/dbsdf.h


@pytest.fixture(scope="module")
def golden(root):
    return json.load(open(os.path.join(root, "tests", "golden", "pt_launch_plan.json")))


@pytest.fixture(scope="module")
def rows(hip_lib):
    return M.rows()


def test_every_row_is_reproduced(rows, golden):
    assert sorted(rows) == sorted(golden["rows"]) and len(rows) >= 300
    names = list(abi.PtLaunchPlan.VARIANT) + list(M.FIELDS) + [f"stage_bytes[{i}]" for i in range(13)] + ["wrapper"]
    bad = []
    for key, plan in rows.items():
        want = golden["plans"][golden["rows"][key]]
        bad += [f"{key}: {n} = {a}, recorded {b}" for n, a, b in zip(names, plan, want) if a != b]
    assert not bad, f"{len(bad)} fields differ:\n" + "\n".join(bad[:40])


def test_the_matrix_reaches_every_decision(rows):
    """the recorded rows do cover what they are there for: every variant flag both ways, staging granted and refused, DEFER and SIMPLE on,
    a node tile, blue-noise columns, per-scene kernels at both budgets"""
    v = {n: {r[i] for r in rows.values()} for i, n in enumerate(abi.PtLaunchPlan.VARIANT)}
    assert all(s == {0, 1} for s in v.values()), v
    col = {n: 10 + i for i, n in enumerate(M.FIELDS)}
    assert any(r[col["bvh_tile_nodes"]] for r in rows.values()) and any(r[col["bn_offset"]] for r in rows.values())
    assert {r[col["stage_total"]] != 0 for k, r in rows.items() if k.startswith("tex_tree")} == {True, False}
    assert all(r[col["stage_total"]] == 0 for k, r in rows.items() if k.startswith("tex_tree_unstaged"))
    assert {r[col["specialised"]] for r in rows.values()} == {0, 1}
    assert {r[col["defer_flags"]] for r in rows.values()} >= {MF_EVAL_METAL, MF_TEXTURED, MF_EVAL_METAL | MF_TEXTURED}


def test_wrapper_text_of_a_per_scene_kernel(hip_lib):
    """the text itself, for one request of each shape: flattened, kept, with an environment, with a lens"""
    def text(sd, opts, **kw):
        with capi.options(**opts):
            s = capi.Scene(None, sd)
        return s.launch_plan(make_config(spp=4, sampler_type=abi.SAMPLER_PMJ02BN), spec_waves=3, **kw)["wrapper"]
    head = ('// per-scene instantiation of k_pt_pass (host/specialise.cpp)\n#define AKR_SPEC_GRAPHS 1\n#include "device/pt_pass.h"\n'
            'extern "C" __global__ __launch_bounds__(256, 3) void akr_pt_pass_spec(const akr::PtParams p) {\n    akr::pt_pass_body<')
    sd = M.textured_room(32, 32, n_floor=8)
    assert text(sd, M.FLAT, defer_metal=1) == head + "true, false, true, true, true, true, akr::kSpecAbsent, false>(p);\n}\n"
    sd.environment = M.ENV
    assert text(sd, M.FLAT, defer_metal=1) == head + "true, false, true, true, true, false, akr::kSpecAbsent, false, true>(p);\n}\n"
    sd.lens = M.LENS
    assert text(sd, M.FLAT) == head + "true, false, true, true, true, false, akr::kSpecAbsent, false, true, true>(p);\n}\n"
    sd.environment = None
    assert text(sd, M.FLAT) == head + "true, false, true, true, true, false, akr::kSpecAbsent, false, false, true>(p);\n}\n"
    kept = M.instanced_scene(n_inst=2, n=4, width=32, height=32, textured=True)
    assert text(kept, dict(force_bvh=0, instancing=1), defer_metal=1) == head + "true, false, true, true, false, false, akr::kSpecAbsent, true>(p);\n}\n"
