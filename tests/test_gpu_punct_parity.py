"""Punctual lights, soft shadows and the thin lens on the GPU against the CPU oracle (oracle/or_punct.h, the oracle's camera; DESIGN.md 4.14,
4.15, 4.9), bit for bit: raw films, ray counters and final sampler states over materials x light kinds, light positions that stress the geometry,
the light table beside emitters and an environment, all 96 PUNCT kernels, light counts across the two LDS budgets, colour pipelines x samplers,
schedules, the lens alone through every kernel family that takes one, and one scene.json read by both readers. The cases are those of
tests/punct_parity_cases.py; tests/test_punct_parity_cases.py shows on the CPU that none of them can pass emptily. Every case asserts the kernel
it ran (kernel_flags, and the host plan's variant for what the flags do not say), is at most 64 x 64 and at most 16 spp."""
import dataclasses
import json

import numpy as np
import pytest

from akari_render_amd import abi, capi, distributed
from oracle import pyoracle, scene_json
from tests import adaptive_model as am
from tests import punct_parity_cases as P
from tests.helpers import make_config, n_bit_diff
from tests.test_gpu_parity import assert_parity
from tests.test_punctual import json_light, write_scene_with_lights

pytestmark = pytest.mark.gpu

COUNTERS = ("n_samples", "n_closest", "n_shadow", "n_shaded")


def gpu_render(ctx, sd, cfg, opts, scene=None, drive=None):
    """one session to its end under `opts` -> (film, counters, final sampler states, kernel info)"""
    w, h = sd.camera.width, sd.camera.height
    with capi.options(**opts):
        scene = scene if scene is not None else capi.Scene(ctx, sd)
        film = capi.Film(ctx, w, h)
        se = capi.PtSession(ctx, scene, cfg, film)
        if drive is not None:
            drive(se, film)
        else:
            se.passes(1000, blocking=True)
        states = se.sampler_states(w * h)
        info = se.kernel_info()
        st = se.end()
    return film.read(), st, states, info


def check(ctx, sd, cfg, opts, flags, want=None, **oracle_kw):
    """the session runs the kernel with `flags` (and the host plan, which the session follows, has `want`); film, counters and states are the oracle's"""
    if want is not None:
        v = P.host_plan(sd, cfg, opts)["variant"]
        assert {k: v[k] for k in want} == want, (v, want)
    g, gst, gstates, info = gpu_render(ctx, sd, cfg, opts)
    assert info["kernel_flags"] == flags and info["specialised"] == 0, (info, flags)
    o, ost, ostates = P.oracle_render(sd, cfg, **oracle_kw)
    assert_parity(g, o, sd.camera.width, sd.camera.height, gst, ost)
    assert np.array_equal(gstates, ostates), f"{np.count_nonzero(gstates != ostates)} sampler state words differ"
    return g, gst


def run_case(ctx, name):
    case = P.CASES[name]
    return check(ctx, case.scene(), case.config(), case.opts, case.flags(), case.want)


# ---------------------------------------------------------------------------------------------------------------- the case table
@pytest.mark.parametrize("name", P.MATERIAL_CASES)
def test_materials_and_light_kinds(ctx, name):
    run_case(ctx, name)


@pytest.mark.parametrize("name", P.POSITION_CASES)
def test_light_positions(ctx, name):
    g, st = run_case(ctx, name)
    if name.startswith("pos-below_floor"):  # shadow rays are traced from the floor's upper side towards a light it cannot see
        assert 0 < st["n_shadow"] <= st["n_shaded"]


@pytest.mark.parametrize("name", P.INTERPLAY_CASES)
def test_light_table_interplay(ctx, name):
    run_case(ctx, name)


@pytest.mark.parametrize("name", P.SWEEP_CASES)
def test_all_96_punct_kernels(ctx, name):
    run_case(ctx, name)


@pytest.mark.parametrize("name", P.COUNT_CASES)
def test_light_counts(ctx, name):
    run_case(ctx, name)


def test_one_light_past_the_exhaustive_budget_is_refused(ctx):
    """an exhaustive scene whose staged tables would pass the LDS budget with the lights' entries is refused; nothing is rendered"""
    sd = P.count_scene(P.exhaustive_limit() + 1)
    with capi.options(**P.EXH):
        with pytest.raises(capi.AkariError) as e:
            capi.Scene(ctx, sd)
        assert e.value.code == capi.ERR_UNSUPPORTED and "LDS budget" in str(e.value)
        scene = capi.Scene(ctx, P.count_scene(P.exhaustive_limit()))
        with pytest.raises(capi.AkariError) as e:
            scene.add_punctual_light(P.LIGHTS["sun"])
        assert e.value.code == capi.ERR_UNSUPPORTED and len(scene.punctual_lights()) == P.exhaustive_limit()


@pytest.mark.parametrize("name", P.PIPELINE_CASES)
def test_colour_pipelines_and_samplers(ctx, name):
    run_case(ctx, name)


@pytest.mark.parametrize("pipeline", ["repr_aces", "acescg"])
def test_lights_changed_mid_scene_under_a_pipeline(ctx, pipeline):
    """a session of a non-default pipeline gets records of its own; after the lights change the next one folds them again"""
    cfg = make_config(**dict(P.BASE, color=P.PIPELINES[pipeline], sampler_seed=3))
    sd = P.lit_scene("coated", P.COLOURED, emitters=1, floor="alpha")
    flags = P.F_STAGE | P.F_PUNCT
    with capi.options(**P.EXH):
        scene = capi.Scene(ctx, sd)
    first = gpu_render(ctx, sd, cfg, P.EXH, scene=scene)
    assert n_bit_diff(first[0], P.oracle_render(sd, cfg)[0]) == 0
    scene.clear_punctual_lights()
    for l in P.COLOURED_AFTER:
        scene.add_punctual_light(l)
    sd2 = dataclasses.replace(sd, lights=list(P.COLOURED_AFTER))
    g, gst, gstates, info = gpu_render(ctx, sd2, cfg, P.EXH, scene=scene)
    assert info["kernel_flags"] == flags
    o, ost, ostates = P.oracle_render(sd2, cfg)
    assert_parity(g, o, 32, 32, gst, ost)
    assert np.array_equal(gstates, ostates) and n_bit_diff(g, first[0]) > 0


# ---------------------------------------------------------------------------------------------------------------- schedules
def test_progressive_passes(ctx):
    """spp_per_pass splits: the film after every pass is the oracle's film of that many samples"""
    sd = P.SCHED_SCENE()
    cfg = make_config(spp=12, spp_per_pass=5, max_depth=5, rr_depth=2, sampler_seed=4)
    prefixes = []

    def drive(se, film):
        for done in (5, 10, 12):
            assert se.passes(1, blocking=True) == done
            prefixes.append(film.read())

    g, gst, gstates, info = gpu_render(ctx, sd, cfg, P.BVH, drive=drive)
    assert info["kernel_flags"] == P.F_BVH | P.F_STAGE | P.F_PUNCT
    film, states = None, P.initial_states(cfg, 32, 32)
    total = dict.fromkeys(COUNTERS, 0)
    for k, n in enumerate((5, 5, 2)):  # (the independent sampler: a later pass goes on where the stream stood)
        film, ost, states = P.oracle_render(sd, make_config(spp=n, spp_per_pass=n, max_depth=5, rr_depth=2, sampler_seed=4), film=film, states=states)
        assert n_bit_diff(prefixes[k], film) == 0, f"after pass {k + 1}: {n_bit_diff(prefixes[k], film)} floats differ"
        for c in COUNTERS:
            total[c] += ost[c]
    assert all(gst[c] == total[c] for c in COUNTERS) and np.array_equal(gstates, states)
    whole = P.oracle_render(sd, cfg)
    assert n_bit_diff(g, whole[0]) == 0 and np.array_equal(gstates, whole[2])


def test_two_tile_shards(ctx):
    sd = P.SCHED_SCENE()
    cfg = make_config(spp=8, spp_per_pass=4, max_depth=5, rr_depth=2, sampler_type=abi.SAMPLER_PMJ02BN, sampler_seed=6)
    whole, wst, _ = P.oracle_render(sd, cfg)
    acc, counts = np.zeros_like(whole), dict.fromkeys(COUNTERS, 0)
    for r in range(2):
        sc = distributed.shard_config(cfg, r, 2, 8, 8)
        g, gst, _, info = gpu_render(ctx, sd, sc, P.EXH)
        assert info["kernel_flags"] == P.F_PMJ | P.F_STAGE | P.F_PUNCT
        o, ost, _ = P.oracle_render(sd, sc)
        assert n_bit_diff(g, o) == 0 and all(gst[c] == ost[c] for c in COUNTERS), r  # the oracle's shard
        assert not np.any((acc != 0) & (g != 0))
        acc += g
        for c in COUNTERS:
            counts[c] += gst[c]
    assert n_bit_diff(acc, whole) == 0 and all(counts[c] == wst[c] for c in COUNTERS)


def test_sample_ranges_with_an_index_sampler(ctx):
    sd = P.SCHED_SCENE()
    cfg = make_config(spp=12, spp_per_pass=4, max_depth=5, rr_depth=2, sampler_type=abi.SAMPLER_SOBOL, sampler_seed=5)
    whole, wst, wstates = P.oracle_render(sd, cfg)
    with capi.options(**P.BVH):
        scene = capi.Scene(ctx, sd)
        film = capi.Film(ctx, 32, 32)
        counts = dict.fromkeys(COUNTERS, 0)
        for b, c in ((0, 5), (5, 4), (9, 3)):
            rc = cfg.copy()
            rc.sample_begin, rc.sample_count = b, c
            se = capi.PtSession(ctx, scene, rc, film)
            assert se.passes(1000, blocking=True) == c
            states, info = se.sampler_states(32 * 32), se.kernel_info()
            st = se.end()
            assert info["kernel_flags"] == P.F_BVH | P.F_PMJ | P.F_STAGE | P.F_PUNCT
            for k in COUNTERS:
                counts[k] += st[k]
    assert n_bit_diff(film.read(), whole) == 0 and np.array_equal(states, wstates) and all(counts[k] == wst[k] for k in COUNTERS)


def test_half_the_tiles_retired_after_the_first_pass(ctx):
    """akr_pt_set_active_tiles: the retired tiles keep the oracle's 4-sample film and states, the others get its 8-sample ones"""
    sd = P.SCHED_SCENE()
    n, keep = 32 * 32, [1, 2]  # of the 2 x 2 tiles of 16 x 16 pixels
    cfg = make_config(spp=8, spp_per_pass=4, max_depth=5, rr_depth=2, sampler_seed=8, tile_w=16, tile_h=16)

    def drive(se, film):
        assert se.passes(1, blocking=True) == 4
        se.set_active_tiles(keep)
        assert se.passes(1, blocking=True) == 8

    g, gst, gstates, info = gpu_render(ctx, sd, cfg, P.EXH, drive=drive)
    assert info["kernel_flags"] == P.F_STAGE | P.F_PUNCT
    half = make_config(spp=4, spp_per_pass=4, max_depth=5, rr_depth=2, sampler_seed=8, tile_w=16, tile_h=16)
    f4, st4, s4 = P.oracle_render(sd, half)
    f8, st8, s8 = P.oracle_render(sd, half, film=f4.copy(), states=s4.copy())
    m = am.tile_mask(32, 32, 16, 16, keep).reshape(-1)
    assert m.sum() == n // 2
    rgb = np.where(np.repeat(m, 3), f8[:3 * n], f4[:3 * n])
    assert n_bit_diff(g[:3 * n], rgb) == 0 and np.array_equal(g[6 * n:], np.where(m, f8[6 * n:], f4[6 * n:]))
    assert np.array_equal(gstates, np.where(np.repeat(m, 2), s8, s4))
    assert gst["n_samples"] == 4 * n + 4 * (n // 2)


# ---------------------------------------------------------------------------------------------------------------- the lens alone
@pytest.mark.parametrize("name", P.LENS_CASES)
def test_lens(ctx, name):
    run_case(ctx, name)


@pytest.mark.parametrize("wavefront", [0, 1], ids=["megakernel", "wavefront"])
def test_lens_kept_scene_kernels(ctx, wavefront):
    """k_pt_pass_inst / the wavefront kernels of a scene kept as meshes + instances, through a defocusing lens"""
    sd = P.kept_lens_scene()
    cfg = make_config(spp=8, spp_per_pass=4, max_depth=6, sampler_type=abi.SAMPLER_PMJ02BN, sampler_seed=7)
    opts = dict(force_bvh=1, instancing=1, wavefront=wavefront, specialise=0)
    with capi.options(**opts):
        assert capi.Scene(None, sd).info().uses_bvh == 2
    g, gst, gstates, info = gpu_render(ctx, sd, cfg, opts)
    assert info["kernel_flags"] & P.F_LENS and info["kernel_flags"] & P.F_PMJ and ("wavefront" in info["status"]) == bool(wavefront), info
    o, ost, ostates = P.oracle_render(sd, cfg)
    assert_parity(g, o, 32, 32, gst, ost)
    assert np.array_equal(gstates, ostates)


@pytest.mark.parametrize("sampler", list(P.SAMPLERS))
def test_lens_forced_wavefront(ctx, sampler):
    sd = P.WAVEFRONT_LENS_SCENE()
    cfg = make_config(spp=8, spp_per_pass=4, max_depth=9, rr_depth=8, sampler_type=P.SAMPLERS[sampler], sampler_seed=9)
    opts = dict(force_bvh=1, instancing=0, wavefront=1, specialise=0)
    g, gst, gstates, info = gpu_render(ctx, sd, cfg, opts)
    assert info["kernel_flags"] & P.F_LENS and "wavefront" in info["status"], info
    o, ost, ostates = P.oracle_render(sd, cfg)
    assert_parity(g, o, 32, 32, gst, ost)
    assert np.array_equal(gstates, ostates)


def _aov_cfg(cfg, aov):
    a = abi.AovConfig.default()
    a.spp, a.aov, a.remap = cfg.spp, aov, 0
    a.filter_type, a.filter_radius, a.sampler_type, a.sampler_seed, a.color = cfg.filter_type, cfg.filter_radius, cfg.sampler_type, cfg.sampler_seed, cfg.color
    return a


@pytest.mark.parametrize("route", ["exh", "bvh"])
def test_lens_aov(ctx, route, aov=abi.AOV_ALBEDO):
    """k_aov<LENS>: the oracle's aov renders through the lens as well (a denoiser's guides must see what the beauty pass sees)"""
    sd = P.AOV_LENS_SCENE()
    a = _aov_cfg(make_config(spp=8, sampler_seed=2), aov)
    with capi.options(**(P.BVH if route == "bvh" else P.EXH)):
        scene = capi.Scene(ctx, sd)
        film = capi.Film(ctx, 32, 32)
        capi.aov_render(ctx, scene, a, film)
    assert n_bit_diff(film.read(), pyoracle.OracleScene(sd).aov_render(a)[0]) == 0


@pytest.mark.parametrize("sampler", ["pmj02bn", "sobol"])
def test_lens_feature_guides_equal_the_oracles_aov(ctx, sampler):
    """with an index-based sampler the depth-0 guides of a FEAT session are the aov integrator's albedo and shading normal of the same
    samples -- here the oracle's, through the lens; the colour film stays the oracle's pt film"""
    sd = P.FEAT_LENS_SCENE()
    cfg = make_config(spp=8, spp_per_pass=4, max_depth=5, sampler_type=P.SAMPLERS[sampler], sampler_seed=5)
    with capi.options(**P.EXH):
        scene = capi.Scene(ctx, sd)
        film, albedo, normal = (capi.Film(ctx, 32, 32) for _ in range(3))
        se = capi.PtSession(ctx, scene, cfg, film, albedo, normal)
        se.passes(1000, blocking=True)
        info = se.kernel_info()
        gst = se.end()
    assert info["kernel_flags"] & P.F_FEAT and info["kernel_flags"] & P.F_LENS
    pyoracle.set_pmj_tables(*capi.host_pmj02bn_tables())
    osc = pyoracle.OracleScene(sd)
    assert n_bit_diff(albedo.read(), osc.aov_render(_aov_cfg(cfg, abi.AOV_ALBEDO))[0]) == 0
    assert n_bit_diff(normal.read(), osc.aov_render(_aov_cfg(cfg, abi.AOV_NS))[0]) == 0
    o, ost, _ = P.oracle_render(sd, cfg)
    assert_parity(film.read(), o, 32, 32, gst, ost)


# ---------------------------------------------------------------------------------------------------------------- readers
def reader_scene_file(tmp_path):
    """one scene.json with a light of each kind (soft and delta), the reference's empty entry and a lens"""
    lights = [abi.PunctualLightData(abi.LIGHT_POINT, position=(0.3, -0.2, 1.5), color=(3.0, 2.0, 1.0), strength=2.0, radius=0.25),
              abi.PunctualLightData(abi.LIGHT_SPOT, position=(0.25, 0.5, 2.0), direction=(0.1, -0.3, -1.0), cone_angle=0.375, blend=0.25, color=(1.0, 4.0, 2.0), strength=1.5),
              abi.PunctualLightData(abi.LIGHT_SUN, direction=(0.2, -0.1, -1.0), color=(1.0, 0.9, 0.8), strength=0.5, angle=0.5),
              abi.PunctualLightData(abi.LIGHT_SPOT, position=(-0.5, -0.5, 1.0), direction=(0.2, 0.2, -1.0), cone_angle=0.5, blend=0.5, color=(2.0, 1.0, 1.0), strength=1.0, radius=0.125)]
    entries = {}
    for k, l in enumerate(lights):
        e = json_light(l)
        if l.radius:
            e["data"]["radius"] = l.radius
        if l.angle:
            e["data"]["angle"] = l.angle
        entries["dcba"[k]] = e
    entries["reference_shaped"] = {"type": "point", "data": {}}
    path = write_scene_with_lights(tmp_path, entries)
    doc = json.load(open(path))
    doc["camera"]["data"]["focal_distance"], doc["camera"]["data"]["fstop"] = 3.0, 6.0
    open(path, "w").write(json.dumps(doc))
    return path


READER_CFG = dict(spp=8, spp_per_pass=8, max_depth=3, sampler_seed=2)


@pytest.mark.parametrize("soft", [1, 0], ids=["soft", "soft_lights_0"])
def test_scene_json_both_readers(ctx, tmp_path, soft):
    """the file read by akr_scene_load and by the Python reader, rendered by the library and by the oracle; under option soft_lights = 0 both read
    every light as a delta light"""
    path = reader_scene_file(tmp_path)
    cfg = make_config(**READER_CFG)
    with capi.options(lens=1, soft_lights=soft, **P.EXH):
        lib_scene = capi.Scene(ctx, path, 32, 32)
        film = capi.Film(ctx, 32, 32)
        se = capi.PtSession(ctx, lib_scene, cfg, film)
        se.passes(1000, blocking=True)
        info, gstates = se.kernel_info(), se.sampler_states(32 * 32)
        gst = se.end()
    assert info["kernel_flags"] == P.F_STAGE | P.F_LENS | P.F_PUNCT
    sd = scene_json.load_scene(path, 32, 32, lens=True, soft_lights=bool(soft))
    assert sd.lights == lib_scene.punctual_lights() and len(sd.lights) == 4 and sd.lens == lib_scene.lens()
    assert any(l.radius or l.angle for l in sd.lights) == bool(soft)
    o, ost, ostates = P.oracle_render(sd, cfg)
    assert_parity(film.read(), o, 32, 32, gst, ost)
    assert np.array_equal(gstates, ostates)
