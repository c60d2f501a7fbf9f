"""What a scene says it holds, held to the answers recorded before its device tables were written as one list (csrc/host/api_scene.cpp):
info().device_bytes of a host-only scene and every AKR_ARRAY_* array (byte count, SHA-256), for every scene and setter step of
tests/scene_tables_cases.py against tests/golden/scene_tables.json. No GPU."""
import json
import os

import pytest

from tests import scene_tables_cases as T


@pytest.fixture(scope="module")
def golden(root):
    return json.load(open(os.path.join(root, "tests", "golden", "scene_tables.json")))["host"]


@pytest.fixture(scope="module")
def records(hip_lib):
    out = {}
    T.walk(None, lambda key, sc, state, tree: out.__setitem__(key, T.record(sc)))
    return out


def test_every_record_is_reproduced(records, golden):
    assert sorted(records) == sorted(golden) and len(records) == len(T.SCENES) + sum(len(s[1]) for s in T.SEQUENCES.values())
    bad = []
    for key, rec in records.items():
        want = golden[key]
        if rec["device_bytes"] != want["device_bytes"]:
            bad.append(f"{key}: device_bytes = {rec['device_bytes']}, recorded {want['device_bytes']}")
        bad += [f"{key}: array {i} = {a}, recorded {b}" for i, (a, b) in enumerate(zip(rec["arrays"], want["arrays"])) if a != b]
        assert len(rec["arrays"]) == len(want["arrays"]) == T.N_ARRAYS
    assert not bad, f"{len(bad)} answers differ:\n" + "\n".join(bad[:40])


@pytest.mark.parametrize("which", [-1, -2, T.N_ARRAYS, 1 << 20])
def test_an_id_that_is_none_is_refused(hip_lib, which):
    """-1 among them: what the rows of tables without an id carry; akr_scene_get_array shows no table that has none"""
    import ctypes as C

    from akari_render_amd import capi
    sc = T.make_scene(None, "tex")
    p, n = C.c_void_p(), C.c_uint64()
    assert capi.lib().akr_scene_get_array(sc.h, which, C.byref(p), C.byref(n)) == capi.ERR_INVALID_ARGUMENT
    assert "unknown array id" in capi.last_error()


def test_the_cases_reach_every_kind_of_table(records):
    """the recorded scenes do cover what they are there for: every array non-empty somewhere, and each group of tables present and absent"""
    sizes = {key: [a[0] for a in rec["arrays"]] for key, rec in records.items()}
    assert all(any(s[i] for s in sizes.values()) for i in range(T.N_ARRAYS))
    from akari_render_amd import capi
    for i in (capi.ARRAY_BVH_NODES, capi.ARRAY_TEX_NODES, capi.ARRAY_MESH_TRIS, capi.ARRAY_ENV_TEXELS, capi.ARRAY_PUNCTUAL_LIGHTS, capi.ARRAY_LIGHT_TREE):
        assert {bool(s[i]) for s in sizes.values()} == {True, False}, i
    assert sizes["cbox_env_1x1"][capi.ARRAY_ENV_TEXELS] == 16 and sizes["cbox_env_13x7"][capi.ARRAY_ENV_TEXELS] == 13 * 7 * 16
    assert sizes["cbox_point_tree"][capi.ARRAY_LIGHT_TREE] == 0  # (one local light: no tree)


def test_a_setter_sequence_ends_where_a_fresh_scene_is(records):
    """the environment removed, the lights cleared, the tree switched off: the tables of the scene that never had them"""
    assert records["env_set_remove/set"] == records["cbox_env_13x7"] and records["env_set_remove/removed"] == records["cbox"]
    assert records["lights_add_clear/added"] == records["cbox_three_lights"] and records["lights_add_clear/cleared"] == records["cbox"]
    assert records["light_tree_on_off/on"] == records["cbox_three_lights_tree"] and records["light_tree_on_off/off"] == records["cbox_three_lights"]
