"""The CPU oracle's light tree (oracle/or_lighttree.h) as a third restatement: its node words, its light list with the tree's one
entry and its walk against the numpy model (tests/light_tree_model.py) AND the library's host build, bit for bit, over the seven scenes of
tests/test_light_tree.py; mode off, or fewer than two local lights, as the oracle that never heard of the mode; and one oracle film whose every
value is exact, which ties the oracle's render loop to its sampler. No GPU is needed: the library's side is capi.Scene(None, ...)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from akari_render_amd import abi, capi
from oracle import pyoracle
from tests import light_tree_model as lt
from tests.helpers import make_config, n_bit_diff
from tests.test_environment import quad_scene
from tests.test_light_tree import HOOK_SCENES, assert_rows_equal, edge_rows, local_lights, make_scene, model_of, threshold_rows
from tests.test_oracle_punct import assert_tables_equal
from tests.test_punctual import light_table, point, spot, sun, two_emitter_scene
from tests.test_soft_lights import random_rows9

F = np.float32


def hook_scene(name):
    """the library's host scene of HOOK_SCENES[name] as tests/test_light_tree.py makes it, its description, and the oracle's scene told of the mode"""
    n, arrangement, mixed = HOOK_SCENES[name]
    lights = local_lights(n, 7 + n, arrangement)
    if mixed:
        lights = [sun()] + lights
    sc, sd = make_scene(lights, mixed=mixed)
    return n, mixed, sc, sd, pyoracle.OracleScene(sd, light_tree=True)


# ---------------------------------------------------------------------------------------------------------------- build, light list, walk
@pytest.mark.parametrize("name", sorted(HOOK_SCENES))
def test_nodes_and_light_list_equal_library_and_model(hip_lib, name):
    n, mixed, sc, sd, osc = hook_scene(name)
    records, weights, words, entries = model_of(sc, sd)
    assert osc.light_tree() == sc.light_tree() == (1, 2 * n - 1)
    nodes = osc.light_tree_nodes()
    assert nodes.shape == (2 * n - 1, 8)
    assert np.array_equal(nodes, sc.array(capi.ARRAY_LIGHT_TREE, np.uint32).reshape(-1, 8))
    assert np.array_equal(nodes, words)
    # instances, weights, selection pdfs, the alias entries, the records (ALL of them, in the order given) and the descriptions
    rows = assert_tables_equal(sc, osc)
    assert [r[0] for r in rows].count(capi.LIGHT_TREE_INSTANCE) == 1 and len(rows) == len(entries) == (5 if mixed else 1)
    tree = [e[0] for e in entries].index("tree")
    assert rows[tree][0] == capi.LIGHT_TREE_INSTANCE == lt.TREE_INST
    assert F(osc.light_info(tree)[1]).view(np.uint32) == lt.tree_power(records, weights).view(np.uint32)
    assert len(osc.punctual_records(0)) == len(records) == n + int(mixed)


@pytest.mark.parametrize("name", sorted(HOOK_SCENES))
def test_walk_equals_model_and_hook(hip_lib, name):
    n, mixed, sc, sd, osc = hook_scene(name)
    records, weights, words, entries = model_of(sc, sd)
    rows = np.concatenate([random_rows9(4096, 3 + n), edge_rows(words, records, n)])
    if not mixed:
        rows = np.concatenate([rows, threshold_rows(sc, records, words, entries, rows[:48])])
    got = osc.light_tree_sample_many(rows)
    want, _ = lt.light_sample_rows(light_table(sc), entries, records, words, rows)
    assert_rows_equal(got, want)
    assert_rows_equal(got, sc.host_light_tree_sample(rows))
    out, light, record = got
    at_tree = light == [e[0] for e in entries].index("tree")
    assert at_tree.sum() > 1000 and len(set(record[at_tree])) >= min(n, 2) and np.all(record[~at_tree] == lt.NO_RECORD)
    # the call that knows no tree samples nothing at the tree's entry, as the library's does, and answers the other entries as before
    soft, soft_light = osc.punct_sample_many(rows)
    lib_soft = sc.host_light_sample_soft(rows)
    assert np.array_equal(soft_light, lib_soft[1]) and np.array_equal(soft.view(np.uint32), lib_soft[0].view(np.uint32))
    assert np.array_equal(soft[~at_tree].view(np.uint32), out[~at_tree].view(np.uint32))


def test_setting_the_lights_while_the_mode_is_on_rebuilds_the_tree(hip_lib):
    lights = [sun()] + local_lights(5, 3) + [sun(direction=(0.0, 0.3, -1.0))]
    sd = two_emitter_scene()
    sd.environment = abi.EnvironmentData(color=(0.5, 0.6, 0.7))
    osc = pyoracle.OracleScene(sd, light_tree=True)
    assert osc.light_tree() == (1, 0) and osc.num_lights() == 3
    osc.set_punctual_lights(lights)
    sc, sd1 = make_scene(lights, mixed=True)
    assert osc.light_tree() == sc.light_tree() == (1, 9)
    assert_tables_equal(sc, osc)
    assert np.array_equal(osc.light_tree_nodes(), sc.array(capi.ARRAY_LIGHT_TREE, np.uint32).reshape(-1, 8))
    # suns given before and after the local lights: their record indices (0 and 6) are not their ranks (2 and 3)
    rows = random_rows9(2048, 19)
    assert_rows_equal(osc.light_tree_sample_many(rows), sc.host_light_tree_sample(rows))
    more = lights + local_lights(1, 99)
    osc.set_punctual_lights(more)
    sc.add_punctual_light(more[-1])
    assert osc.light_tree() == sc.light_tree() == (1, 11)
    assert_tables_equal(sc, osc)
    assert_rows_equal(osc.light_tree_sample_many(rows), sc.host_light_tree_sample(rows))
    osc.set_environment(None)  # the other setter that rebuilds the list keeps the tree
    sc.set_environment()
    assert osc.light_tree() == (1, 11)
    assert_tables_equal(sc, osc)
    osc.set_light_tree(False)
    sc.set_light_tree(False)
    assert osc.light_tree() == sc.light_tree() == (0, 0) and osc.light_tree_nodes().shape == (0, 8)
    assert_tables_equal(sc, osc)
    osc.set_punctual_lights(None)
    osc.set_light_tree(True)
    assert osc.light_tree() == (1, 0) and osc.num_lights() == 2


# ---------------------------------------------------------------------------------------------------------------- mode off is off
def _render(sd, cfg, **kw):
    w, h = sd.camera.width, sd.camera.height
    states = pyoracle.init_pcg32_states(w * h, cfg.sampler_seed)
    film, st = pyoracle.OracleScene(sd, **kw).render(cfg, states=states)
    return film, st, states


def assert_same_oracle(sd, cfg, told, plain):
    """`told` was told of the mode, `plain` never was: the same light list, rows and films"""
    assert told.num_lights() == plain.num_lights() and told.light_tree()[1] == 0 and told.light_tree_nodes().size == 0
    assert [told.light_info(i) for i in range(told.num_lights())] == [plain.light_info(i) for i in range(plain.num_lights())]
    (te, tp), (pe, pp) = told.light_table(), plain.light_table()
    assert np.array_equal(te, pe) and np.array_equal(tp.view(np.uint32), pp.view(np.uint32))
    rows = random_rows9(2048, 9)
    for color in (0, abi.COLOR_REPR_ACESCG | abi.COLOR_RGB_ACESCG):
        a, b = told.punct_sample_many(rows, color), plain.punct_sample_many(rows, color)
        assert np.array_equal(a[1], b[1]) and n_bit_diff(a[0], b[0]) == 0
        t = told.light_tree_sample_many(rows, color)  # without a tree: the same answer, and no record
        assert np.array_equal(t[1], b[1]) and n_bit_diff(t[0], b[0]) == 0 and np.all(t[2] == lt.NO_RECORD)
    w, h = sd.camera.width, sd.camera.height
    films = []
    for osc in (told, plain):
        states = pyoracle.init_pcg32_states(w * h, cfg.sampler_seed)
        film, st = osc.render(cfg, states=states)
        films.append((film, st, states))
    assert n_bit_diff(films[0][0], films[1][0]) == 0 and films[0][1] == films[1][1] and np.array_equal(films[0][2], films[1][2])
    assert films[1][1]["n_shadow"] > 0


def test_mode_off_or_one_local_light_is_the_oracle_that_never_heard_of_it():
    cfg = make_config(spp=4, max_depth=4, sampler_seed=3)
    many = [sun()] + local_lights(5, 3) + [sun(direction=(0.0, 0.3, -1.0))]
    for lights, mode in ((many, False), ([sun(), local_lights(1, 3)[0]], True), ([sun(), sun(direction=(0.0, 0.3, -1.0))], True)):
        sd = two_emitter_scene()
        sd.environment, sd.lights = abi.EnvironmentData(color=(0.5, 0.6, 0.7)), lights
        told = pyoracle.OracleScene(sd, light_tree=mode)
        if not mode:  # on and off again
            told.set_light_tree(True)
            assert told.light_tree() == (1, 9) and told.num_lights() == 6
            told.set_light_tree(False)
        assert told.light_tree()[0] == int(mode)
        assert_same_oracle(sd, cfg, told, pyoracle.OracleScene(sd))
    # with a tree the film is another one
    sd = two_emitter_scene()
    sd.environment, sd.lights = abi.EnvironmentData(color=(0.5, 0.6, 0.7)), many
    assert n_bit_diff(_render(sd, cfg, light_tree=True)[0], _render(sd, cfg)[0]) > 0


def test_gpt_and_mcmc_refuse_a_scene_with_a_tree():
    sd = quad_scene(emissive=True)
    sd.lights = local_lights(4, 1)
    osc = pyoracle.OracleScene(sd, light_tree=True)
    assert osc.light_tree() == (1, 7)
    g = abi.GptConfig.default()
    g.spp = 1
    film, aux = np.zeros(7 * 1024, F), np.zeros(3 * 1024 + 6 * 33 * 33, F)
    fp = C.POINTER(C.c_float)
    assert pyoracle.lib().or_gpt_render(osc.h, C.byref(g), film.ctypes.data_as(fp), aux.ctypes.data_as(fp), 1) == -5
    m = abi.McmcConfig.default()
    res, chains = np.zeros(4, np.float64), np.zeros(max(int(m.n_chains), 1), abi.MARKOV_STATE_DTYPE)
    assert pyoracle.lib().or_mcmc_render(osc.h, C.byref(m), film.ctypes.data_as(fp), res.ctypes.data_as(C.POINTER(C.c_double)),
                                         chains.ctypes.data_as(C.POINTER(C.c_uint32)), 1) == -5


# ---------------------------------------------------------------------------------------------------------------- one exact-valued film
def oracle_points(osc, w, h):
    """the float32 point the oracle shades for every pixel's centre ray: its own camera ray, intersection and surface interaction; every ray must hit"""
    px = np.stack(np.meshgrid(np.arange(w), np.arange(h)), -1).reshape(-1, 2).astype(np.uint32)
    half = np.full((w * h, 2), 0.5, F)
    rays = osc.lens_ray_many(px, half, half, abi.FILTER_BOX, 0.0)
    pts = np.zeros((w * h, 3), F)
    for k, r in enumerate(rays):
        hit, inst, prim, bary = osc.intersect(r[0:3], r[3:6])
        assert hit
        pts[k] = osc.surface_interaction(inst, prim, float(bary[0]), float(bary[1]))[0:3]
    return pts


def test_exact_film_of_four_lights_at_one_point(hip_lib):
    """Four delta lights at one point over the quad, the tree the table's only entry, depth 1, one sample through every pixel's centre. A pixel's sample is
    (li f) (1 / pdf) in f32 (MIS weight 1: the sample is a delta light's); alone in a scene light i has pdf 1, so its one-light film holds li f itself,
    and the tree's film must hold, per pixel, that value times the f32 reciprocal of the probability the model's walk gives light i at the oracle's own
    float32 point -- for exactly one i, the colours being distinct. Every light is reached."""
    from tests.test_gpu_punctual import RHO, centre_cfg
    w = h = 16
    where = (0.25, -0.5, 0.75)
    colours = [(2.0, 1.0, 1.5), (1.0, 2.0, 0.5), (0.5, 1.0, 3.0), (1.0, 1.0, 1.0)]
    lights = [point(position=where, color=c, strength=s) for c, s in zip(colours[:3], (1.0, 2.0, 0.75))]
    lights.append(spot(position=where, direction=(0.0, 0.0, -1.0), cone_angle=1.5, blend=0.0, color=colours[3], strength=3.0))
    sc, sd = make_scene(lights, width=w, height=h, albedo=RHO)
    cfg = centre_cfg(spp=1, sampler_seed=5)
    n = w * h
    film, st, _ = _render(sd, cfg, light_tree=True)
    assert st["n_shadow"] == st["n_shaded"] == n and np.all(film[6 * n:7 * n] == 1)
    records, weights, words, entries = model_of(sc, sd)
    assert [e[0] for e in entries] == ["tree"] and np.array_equal(pyoracle.OracleScene(sd, light_tree=True).light_tree_nodes(), words)
    p, _ = lt.record_pdfs(words, records, oracle_points(pyoracle.OracleScene(sd), w, h))
    assert np.all(np.abs(p.astype(np.float64).sum(axis=1) - 1.0) < 1e-5) and p.shape == (n, 4)
    got = film[:3 * n].reshape(n, 3)
    matches = np.zeros((n, 4), bool)
    for i, l in enumerate(lights):
        alone = _render(dataclasses.replace(sd, lights=[l]), cfg, light_tree=True)[0][:3 * n].reshape(n, 3)
        assert np.all(alone > 0)
        with np.errstate(all="ignore"):
            want = (alone * (F(1) / p[:, i]).astype(F)[:, None]).astype(F)
        matches[:, i] = (got.view(np.uint32) == want.view(np.uint32)).all(axis=1)
    assert np.all(matches.sum(axis=1) == 1), f"{int((matches.sum(axis=1) != 1).sum())} pixels are not exactly one light's f / p"
    assert matches.any(axis=0).all()
    # by power alone the same pixels are f / (the alias table's pdf): the tree's film is not mode 0's
    assert n_bit_diff(film, _render(sd, cfg)[0]) > 0
