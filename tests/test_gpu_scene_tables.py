"""The scenes and setter sequences of tests/scene_tables_cases.py created on a context: info().device_bytes against the values recorded on
an MI355X before a scene's device tables were written as one list (tests/golden/scene_tables.json, key "device"); after every step of a
setter sequence one sample per pixel against the oracle (a pointer of DScene left at a released table shows there); and one session under a
non-default colour pipeline on the textured scene and on the scene with lights (the colour sets' copies of the tables)."""
import json
import os

import pytest

from akari_render_amd import abi, capi
from oracle import pyoracle
from tests import scene_tables_cases as T
from tests.helpers import make_config
from tests.test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(root):
    return json.load(open(os.path.join(root, "tests", "golden", "scene_tables.json")))["device"]


def parity(ctx, sc, sd, tree, cfg):
    film = capi.Film(ctx, T.W, T.H)
    gst = capi.pt_render(ctx, sc, cfg, film)
    o, ost = pyoracle.OracleScene(sd, light_tree=tree).render(cfg)
    assert_parity(film.read(), o, T.W, T.H, gst, ost)


@pytest.mark.parametrize("name", list(T.SCENES))
def test_device_bytes_of_a_scene(ctx, golden, name):
    assert T.make_scene(ctx, name).info().device_bytes == golden[name]


@pytest.mark.parametrize("name", list(T.SEQUENCES))
def test_setter_sequence(ctx, golden, name):
    start, steps = T.SEQUENCES[name]
    sc = T.make_scene(ctx, start)
    cfg = make_config(spp=1, spp_per_pass=1, max_depth=5, rr_depth=2)
    for step, change, state, tree in steps:
        change(sc)
        assert sc.info().device_bytes == golden[f"{name}/{step}"], step
        parity(ctx, sc, state(), tree, cfg)


@pytest.mark.parametrize("name", ["tex", "cbox_three_lights"])
def test_session_under_another_colour_pipeline(ctx, name):
    build, _, tree = T.SCENES[name]
    parity(ctx, T.make_scene(ctx, name), build(), tree, make_config(spp=1, spp_per_pass=1, max_depth=5, rr_depth=2, color=abi.COLOR_REPR_ACESCG))
