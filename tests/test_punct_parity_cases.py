"""The conditions that keep tests/test_gpu_punct_parity.py from passing emptily, checked without a GPU: for every case of
tests/punct_parity_cases.py the library's host plan must name the kernel variant the case is there for, and the oracle alone must show that
the case's lights (or its lens) change at least a quarter of the film's floats, that a spot's cone edge leaves at least 20 surface pixels on
either side at depth 1, that the light-table cases shade with and without shadow rays, and that the clamp case clamps a sample."""
import dataclasses

import numpy as np
import pytest

from akari_render_amd import abi, capi
from oracle import pyoracle
from tests import punct_parity_cases as P
from tests.helpers import make_config, n_bit_diff


def _fraction(a, b):
    return n_bit_diff(a, b) / a.size


@pytest.mark.parametrize("name", list(P.CASES))
def test_case_is_what_it_claims(hip_lib, name):
    case = P.CASES[name]
    sd, cfg = case.scene(), case.config()
    w, h = sd.camera.width, sd.camera.height
    assert max(w, h) <= (64 if "spot" in case.tags else 32) and cfg.spp <= 16
    v = P.host_plan(sd, cfg, case.opts)["variant"]
    assert {k: v[k] for k in case.want} == case.want, (v, case.want)
    film, st, _ = P.oracle_render(sd, cfg)
    assert np.all(np.isfinite(film))
    if case.want["punct"]:
        assert sd.lights
        bare, bst, _ = P.oracle_render(sd, cfg, lights=False)
        if "dark_ok" in case.tags:  # use_nee = 0: a punctual light gives nothing (no ray ever hits one), and nothing is what the case pins
            assert n_bit_diff(film, bare) == 0 and st == bst and st["n_shadow"] == 0
        else:
            assert _fraction(film, bare) >= 0.25, f"the lights change {_fraction(film, bare):.3f} of the film's floats"
    if "lens" in case.tags:
        assert sd.lens is not None
        pin, _, _ = P.oracle_render(sd, cfg, lens=False)
        assert _fraction(film, pin) >= 0.25, f"the lens changes {_fraction(film, pin):.3f} of the film's floats"
    if "interplay" in case.tags:
        assert 0 < st["n_shadow"] < st["n_shaded"], st
    if "spot" in case.tags:
        # the cone's direct light at depth 1: the spot alone, no bounce; among the pixels whose centre sees a surface (aov: a geometric normal)
        dark = [dataclasses.replace(m, emission_strength=0.0) for m in sd.materials]
        alone = dataclasses.replace(sd, lights=[l for l in sd.lights if l.type == abi.LIGHT_SPOT], environment=None, materials=dark)
        c1 = cfg.copy()
        c1.max_depth, c1.force_diffuse = 1, 1
        direct = P.oracle_render(alone, c1)[0][:3 * w * h].reshape(h, w, 3).max(axis=-1) > 0
        a = abi.AovConfig.default()
        a.spp, a.aov = 4, 1
        surface = np.abs(pyoracle.OracleScene(alone).aov_render(a)[0][:3 * w * h].reshape(h, w, 3)).max(axis=-1) > 0
        assert (direct & surface).sum() >= 20 and (~direct & surface).sum() >= 20, ((direct & surface).sum(), (~direct & surface).sum())
    if "tmax" in case.tags:
        # the light is below the floor and lights surfaces above it: at depth 1 with the light alone, at least 20 surface pixels are lit through the floor
        dark = [dataclasses.replace(m, emission_strength=0.0) for m in sd.materials]
        c1 = cfg.copy()
        c1.max_depth = 1
        through = P.oracle_render(dataclasses.replace(sd, materials=dark), c1)[0][:3 * w * h].reshape(h, w, 3).max(axis=-1) > 0
        assert all(l.position[1] < -1.0 for l in sd.lights) and 20 <= through.sum() <= w * h - 20, through.sum()
    if "clamp" in case.tags:
        # With debug_depth = 2 a sample is the clamped indirect sum of its depth-2 terms alone (base stays 0), so a clamped sample is exactly 1000 in
        # a film of its own; every term is >= 0, so the same path's whole indirect sum is clamped in the case's own render too.
        c2 = cfg.copy()
        c2.debug_depth, c2.spp, c2.spp_per_pass = 2, 1, 1
        states = P.initial_states(c2, w, h)
        clamped = 0
        for _ in range(cfg.spp):
            one, _, states = P.oracle_render(sd, c2, states=states)
            clamped += int(np.count_nonzero(one[:3 * w * h] == np.float32(1000.0)))
        assert clamped >= 1


def test_the_sweep_names_all_96_punct_kernels(hip_lib):
    seen = set()
    for name in P.SWEEP_CASES:
        w = P.CASES[name].want
        seen.add((w["env"], w["lens"], w["bvh"], w["stage"], w["fd"], w["tex"], w["pmj"]))
    assert len(P.SWEEP_CASES) == len(seen) == 96
    assert {s[2:4] for s in seen} == {(0, 1), (1, 1), (1, 0)}  # exhaustive + staged, BVH + staged, BVH unstaged
    for unit in ((0, 0), (1, 0), (0, 1), (1, 1)):
        assert any(P.CASES[n].cfg["sampler_type"] == abi.SAMPLER_SOBOL for n in P.SWEEP_CASES if (P.CASES[n].want["env"], P.CASES[n].want["lens"]) == unit)


def test_light_count_limits(hip_lib):
    """the two budgets, found on the host and not hard-coded: one light more changes the plan / is refused as DESIGN.md 4.14 says"""
    cfg = make_config(**P.COUNT_CFG)
    n = P.bvh_stage_limit()
    assert 100 < n < 1000
    assert P.host_plan(P.count_scene(n), cfg, P.BVH)["variant"]["stage"] == 1 and P.host_plan(P.count_scene(n + 1), cfg, P.BVH)["variant"]["stage"] == 0
    m = P.exhaustive_limit()
    assert n < m < 4096
    assert P.host_plan(P.count_scene(m), cfg, P.EXH)["variant"]["stage"] == 1
    with capi.options(**P.EXH):
        with pytest.raises(capi.AkariError) as e:
            capi.Scene(None, P.count_scene(m + 1))
    assert e.value.code == capi.ERR_UNSUPPORTED and "point light" in str(e.value) and "LDS budget" in str(e.value)
    powers = {capi.Scene(None, P.count_scene(65)).light(i)[1] for i in range(65)}
    assert len(powers) >= 7  # the alias table is not flat


@pytest.mark.parametrize("name", list(P.EXTRA))
def test_scenes_outside_the_table(hip_lib, name):
    """the scenes of the schedule, kept-scene, wavefront, aov and guide tests: their lights / their lens change a quarter of the film's floats"""
    scene, kw, what = P.EXTRA[name]
    sd, cfg = scene(), make_config(**kw)
    assert max(sd.camera.width, sd.camera.height) <= 32 and cfg.spp <= 16
    film, st, _ = P.oracle_render(sd, cfg)
    if "lights" in what:
        assert sd.lights and _fraction(film, P.oracle_render(sd, cfg, lights=False)[0]) >= 0.25 and st["n_shadow"] > 0
    if "lens" in what:
        assert sd.lens is not None and _fraction(film, P.oracle_render(sd, cfg, lens=False)[0]) >= 0.25


def test_aov_scene(hip_lib, aov=abi.AOV_ALBEDO):
    """the oracle's aov film of the lens scene differs from the pinhole's in a quarter of its floats, and does not see the punctual lights"""
    sd = P.AOV_LENS_SCENE()
    a = abi.AovConfig.default()
    a.spp, a.aov, a.remap, a.sampler_seed = 8, aov, 0, 2
    o = pyoracle.OracleScene(sd).aov_render(a)[0]
    assert _fraction(o, pyoracle.OracleScene(sd, lens=False).aov_render(a)[0]) >= 0.25
    assert n_bit_diff(o, pyoracle.OracleScene(sd, lights=False).aov_render(a)[0]) == 0


@pytest.mark.parametrize("soft", [True, False], ids=["soft", "soft_lights_0"])
def test_reader_scene(hip_lib, tmp_path, soft):
    from oracle import scene_json
    from tests.test_gpu_punct_parity import READER_CFG, reader_scene_file
    sd = scene_json.load_scene(reader_scene_file(tmp_path), 32, 32, lens=True, soft_lights=soft)
    cfg = make_config(**READER_CFG)
    o = P.oracle_render(sd, cfg)[0]
    assert _fraction(o, P.oracle_render(sd, cfg, lights=False)[0]) >= 0.25 and _fraction(o, P.oracle_render(sd, cfg, lens=False)[0]) >= 0.25
