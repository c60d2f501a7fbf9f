"""The conditions that keep tests/test_gpu_light_tree_parity.py from passing emptily, checked without a GPU: for every case of
tests/light_tree_parity_cases.py the library's host build must hold a tree of 2 L - 1 nodes and plan the kernel variant the case is there for, and the
oracle alone must show that the tree's film differs in at least a quarter of its floats both from the film of the same scene by power alone (mode 0)
and from the film without lights; that the light-table cases shade with and without shadow rays; that the far light of the clamp case sits at the
2^-16 clamp and a sample is clamped; that the filler suns leave the tree a quarter of the selection; and that the sweep names all 96 LTREE kernels."""
import numpy as np
import pytest

from akari_render_amd import abi, capi
from oracle import pyoracle
from tests import light_tree_parity_cases as T
from tests import punct_parity_cases as P
from tests.helpers import make_config, n_bit_diff


def _fraction(a, b):
    return n_bit_diff(a, b) / a.size


def host_scene(sd, opts):
    with capi.options(**opts):
        return capi.Scene(None, sd)


def tree_entry(sc):
    """(index, selection pdf) of the tree's entry of the light list"""
    at = [i for i in range(sc.info().n_lights) if sc.light(i)[0] == capi.LIGHT_TREE_INSTANCE]
    assert len(at) == 1
    return at[0], sc.light(at[0])[2]


@pytest.mark.parametrize("name", list(T.CASES))
def test_case_is_what_it_claims(hip_lib, name):
    case = T.CASES[name]
    sd, cfg = case.scene(), case.config()
    w, h = sd.camera.width, sd.camera.height
    assert max(w, h) <= 32 and cfg.spp <= 16 and case.opts["light_tree"] == 1
    L = T.n_local(sd)
    sc = host_scene(sd, case.opts)
    assert L >= 2 and sc.light_tree() == (1, 2 * L - 1) and len(sc.punctual_lights()) == len(sd.lights)
    v = P.host_plan(sd, cfg, case.opts)["variant"]
    assert case.want["punct"] == 1 and {k: v[k] for k in case.want} == case.want, (v, case.want)
    assert "ltree" not in v  # the plan does not report the tree: on the GPU the flag is kernel_flags & 256
    film, st, _ = T.tree_render(sd, cfg)
    assert np.all(np.isfinite(film))
    bare, bst, _ = P.oracle_render(sd, cfg, lights=False)
    if "dark_ok" in case.tags:  # use_nee = 0: no ray ever hits a punctual light, and nothing is what the case pins
        assert n_bit_diff(film, bare) == 0 and st == bst and st["n_shadow"] == 0
    else:
        by_power = P.oracle_render(sd, cfg)[0]
        assert _fraction(film, by_power) >= 0.25, f"the tree changes {_fraction(film, by_power):.3f} of the floats of the film by power alone"
        assert _fraction(film, bare) >= 0.25, f"the lights change {_fraction(film, bare):.3f} of the film's floats"
    if "interplay" in case.tags:
        assert 0 < st["n_shadow"] < st["n_shaded"], st
    if "filler" in case.tags:
        assert tree_entry(sc)[1] >= 0.25 and L >= 5 and sc.info().n_lights > 100, (tree_entry(sc), sc.info().n_lights)
    if "past_limit" in case.tags:
        assert L == P.exhaustive_limit() + 1 and sc.info().uses_bvh == 0 and sc.info().n_lights == 1
        with capi.options(**dict(case.opts, light_tree=0)):
            with pytest.raises(capi.AkariError) as e:
                capi.Scene(None, sd)
        assert e.value.code == capi.ERR_UNSUPPORTED and "LDS budget" in str(e.value)
    if "clamp" in case.tags:
        # the far light's walked probability, at points of the floor and whatever u: at most the clamp's 2^-16 times the entry's pdf
        far = [k for k, l in enumerate(sd.lights) if max(abs(c) for c in l.position) > 1e5]
        assert len(far) == 1
        m = 1 << 18
        rows = np.zeros((4 * m, 9), np.float32)
        rows[:, 0:3] = np.repeat(np.float32([[0.0, -1.0, 0.0], [2.0, -1.0, 1.5], [-1.5, -1.0, -2.0], [0.5, -1.0, 3.0]]), m, axis=0)
        rows[:, 4], rows[:, 6], rows[:, 7:9] = 1.0, np.tile((np.arange(m) + 0.5) / m, 4), 0.5
        out, light, record = pyoracle.OracleScene(sd, light_tree=True).light_tree_sample_many(rows)
        at = record == far[0]
        assert np.all(at.reshape(4, m).sum(axis=1) >= 2) and np.all(out[at, 6] == np.float32(2.0 ** -16) * np.float32(tree_entry(sc)[1])) and np.all(out[at, 11] == 1)
        assert np.all(out[at, 0:3].max(axis=1) / out[at, 6] > 5000.0)  # li / pdf: over the radiance clamp of 1000 wherever the BSDF's value times the cosine passes 0.2
        assert np.all(out[~at, 6] <= np.float32(1.0 - 2.0 ** -16) * np.float32(tree_entry(sc)[1]))  # (a near light: the clamp's other side, times its own level's share)
        # With debug_depth = 2 a sample is the clamped indirect sum of its depth-2 terms alone (base stays 0), so a clamped sample is exactly 1000 in
        # a film of its own; every term is >= 0, so the same path's whole indirect sum is clamped in the case's own render too.
        c2 = cfg.copy()
        c2.debug_depth, c2.spp, c2.spp_per_pass = 2, 1, 1
        states = P.initial_states(c2, w, h)
        clamped = 0
        for _ in range(cfg.spp):
            one, _, states = T.tree_render(sd, c2, states=states)
            clamped += int(np.count_nonzero(one[:3 * w * h] == np.float32(1000.0)))
        assert clamped >= 1


def test_the_sweep_names_all_96_ltree_kernels(hip_lib):
    seen = set()
    for name in T.SWEEP_CASES:
        w = T.CASES[name].want
        seen.add((w["env"], w["lens"], w["bvh"], w["stage"], w["fd"], w["tex"], w["pmj"]))
    assert len(T.SWEEP_CASES) == len(seen) == 96
    assert {s[2:4] for s in seen} == {(0, 1), (1, 1), (1, 0)}  # exhaustive + staged, BVH + staged, BVH unstaged
    for unit in ((0, 0), (1, 0), (0, 1), (1, 1)):
        assert any(T.CASES[n].cfg["sampler_type"] == abi.SAMPLER_SOBOL for n in T.SWEEP_CASES if (T.CASES[n].want["env"], T.CASES[n].want["lens"]) == unit)


def test_filler_counts_come_from_the_host(hip_lib):
    """the count of filler suns is found by bisection, not hard-coded: one sun fewer and the BVH kernels still stage their tables"""
    cfg = make_config(**T.SWEEP_CFG)
    for tex, env, lens in ((0, 0, 0), (1, 1, 1)):
        n = T.unstaged_suns(tex, env, lens)
        assert 100 < n < 1000
        assert P.host_plan(T._sweep_scene(tex, env, lens, "bvh_unstaged", n_suns=n), cfg, T.BVH_T)["variant"]["stage"] == 0
        assert P.host_plan(T._sweep_scene(tex, env, lens, "bvh_unstaged", n_suns=n - 1), cfg, T.BVH_T)["variant"]["stage"] == 1


def test_case_counts():
    assert (len(T.SWEEP_CASES), len(T.SHAPE_CASES), len(T.POSITION_CASES), len(T.INTERPLAY_CASES), len(T.MATERIAL_CASES), len(T.PIPELINE_CASES)) == (96, 15, 10, 16, 12, 12)
    assert len(T.CASES) == 161


@pytest.mark.parametrize("name", list(T.EXTRA))
def test_scenes_outside_the_table(hip_lib, name):
    """the scenes of the schedule and session tests: a tree exists, and it and the lights change a quarter of the film's floats"""
    scene, kw = T.EXTRA[name]
    sd, cfg = scene(), make_config(**kw)
    assert max(sd.camera.width, sd.camera.height) <= 32 and cfg.spp <= 16
    assert host_scene(sd, T.EXH_T).light_tree() == (1, 2 * T.n_local(sd) - 1)
    film, st, _ = T.tree_render(sd, cfg)
    assert _fraction(film, P.oracle_render(sd, cfg)[0]) >= 0.25 and _fraction(film, P.oracle_render(sd, cfg, lights=False)[0]) >= 0.25 and st["n_shadow"] > 0


def test_session_states_differ(hip_lib):
    """the states the session test walks through are different films: with the tree, by power, with a light more, with other lights"""
    import dataclasses
    sd, cfg = T.SESSION_SCENE(), make_config(**T.EXTRA["sessions"][1])
    films = [T.tree_render(sd, cfg)[0], P.oracle_render(sd, cfg)[0], T.tree_render(dataclasses.replace(sd, lights=T.COLOURED + [T.COLOURED_MORE]), cfg)[0],
             T.tree_render(dataclasses.replace(sd, lights=list(T.COLOURED_AFTER)), cfg)[0]]
    for i in range(4):
        for j in range(i):
            assert _fraction(films[i], films[j]) >= 0.25, (i, j)


def test_reader_scene(hip_lib, tmp_path):
    from oracle import scene_json
    from tests.test_gpu_light_tree_parity import READER_CFG, reader_scene_file
    path = reader_scene_file(tmp_path)
    sd = scene_json.load_scene(path, 32, 32)
    with capi.options(light_tree=1):
        lib_scene = capi.Scene(None, path, 32, 32)
    assert sd.lights == lib_scene.punctual_lights() and lib_scene.light_tree() == (1, 2 * T.n_local(sd) - 1) and T.n_local(sd) >= 4
    cfg = make_config(**READER_CFG)
    o = T.tree_render(sd, cfg)[0]
    assert _fraction(o, P.oracle_render(sd, cfg)[0]) >= 0.25 and _fraction(o, P.oracle_render(sd, cfg, lights=False)[0]) >= 0.25
