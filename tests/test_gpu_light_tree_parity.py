"""Films of scenes with a light tree on the GPU against the CPU oracle (oracle/or_lighttree.h), bit for bit: raw films, ray counters
and final sampler states over all 96 LTREE kernels, tree shapes and counts, light positions that reach the walk's edges, the light table beside
emitters, suns and an environment, materials, colour pipelines x samplers, schedules, the mode and the lights changed between sessions of one scene,
and one scene.json read by both readers. This is the text films run -- the LTREE branch of sample_direct -- which the device probe does not. The
cases are those of tests/light_tree_parity_cases.py; tests/test_light_tree_parity_cases.py shows on the CPU that none of them can pass emptily.
Every case asserts the kernel it ran: its kernel_flags with bits 128 (PUNCT) and 256 (walks a light tree) set."""
import dataclasses

import numpy as np
import pytest

from akari_render_amd import abi, capi, distributed
from oracle import scene_json
from tests import adaptive_model as am
from tests import light_tree_parity_cases as T
from tests import punct_parity_cases as P
from tests.helpers import make_config, n_bit_diff
from tests.test_gpu_parity import assert_parity
from tests.test_gpu_punct_parity import COUNTERS, gpu_render
from tests.test_punctual import json_light, write_scene_with_lights

pytestmark = pytest.mark.gpu

TREE_BITS = P.F_PUNCT | T.F_LTREE


def check(ctx, sd, cfg, opts, flags, want=None, scene=None, light_tree=True):
    """the session runs the kernel with `flags` (and the host plan, which the session follows, has `want`); film, counters and states are the oracle's"""
    if want is not None:
        v = P.host_plan(sd, cfg, opts)["variant"]
        assert {k: v[k] for k in want} == want, (v, want)
    g, gst, gstates, info = gpu_render(ctx, sd, cfg, opts, scene=scene)
    assert info["kernel_flags"] == flags and info["specialised"] == 0, (info, flags)
    o, ost, ostates = P.oracle_render(sd, cfg, light_tree=light_tree)
    assert_parity(g, o, sd.camera.width, sd.camera.height, gst, ost)
    assert np.array_equal(gstates, ostates), f"{np.count_nonzero(gstates != ostates)} sampler state words differ"
    return g, gst


def run_case(ctx, name):
    case = T.CASES[name]
    assert T.flags(case) & TREE_BITS == TREE_BITS
    return check(ctx, case.scene(), case.config(), case.opts, T.flags(case), case.want)


# ---------------------------------------------------------------------------------------------------------------- the case table
@pytest.mark.parametrize("name", T.SWEEP_CASES)
def test_all_96_ltree_kernels(ctx, name):
    run_case(ctx, name)


@pytest.mark.parametrize("name", T.SHAPE_CASES)
def test_tree_shapes_and_counts(ctx, name):
    run_case(ctx, name)


@pytest.mark.parametrize("name", T.POSITION_CASES)
def test_light_positions(ctx, name):
    run_case(ctx, name)


@pytest.mark.parametrize("name", T.INTERPLAY_CASES)
def test_light_table_interplay(ctx, name):
    run_case(ctx, name)


@pytest.mark.parametrize("name", T.MATERIAL_CASES)
def test_materials(ctx, name):
    run_case(ctx, name)


@pytest.mark.parametrize("name", T.PIPELINE_CASES)
def test_colour_pipelines_and_samplers(ctx, name):
    run_case(ctx, name)


# ---------------------------------------------------------------------------------------------------------------- schedules
def test_progressive_passes(ctx):
    """eight one-sample passes driven as 3 + 5: the film after the third is the oracle's three-sample film, the end is the one-shot render"""
    sd = T.SCHED_SCENE()
    kw = T.EXTRA["schedules-independent"][1]
    cfg = make_config(**kw)
    prefix = []

    def drive(se, film):
        assert se.passes(3, blocking=True) == 3
        prefix.append(film.read())
        assert se.passes(5, blocking=True) == 8

    g, gst, gstates, info = gpu_render(ctx, sd, cfg, T.BVH_T, drive=drive)
    assert info["kernel_flags"] == P.F_BVH | P.F_STAGE | TREE_BITS
    film, ost3, states = P.oracle_render(sd, make_config(**dict(kw, spp=3)), light_tree=True)
    assert n_bit_diff(prefix[0], film) == 0
    film, ost5, states = P.oracle_render(sd, make_config(**dict(kw, spp=5)), film=film, states=states, light_tree=True)
    assert n_bit_diff(g, film) == 0 and np.array_equal(gstates, states) and all(gst[c] == ost3[c] + ost5[c] for c in COUNTERS)
    whole = P.oracle_render(sd, cfg, light_tree=True)
    assert n_bit_diff(g, whole[0]) == 0 and np.array_equal(gstates, whole[2]) and all(gst[c] == whole[1][c] for c in COUNTERS)


def test_two_tile_shards(ctx):
    sd = T.SCHED_SCENE()
    cfg = make_config(**T.EXTRA["schedules-pmj02bn"][1])
    whole, wst, _ = P.oracle_render(sd, cfg, light_tree=True)
    acc, counts = np.zeros_like(whole), dict.fromkeys(COUNTERS, 0)
    for r in range(2):
        sc = distributed.shard_config(cfg, r, 2, 8, 8)
        g, gst, _, info = gpu_render(ctx, sd, sc, T.EXH_T)
        assert info["kernel_flags"] == P.F_PMJ | P.F_STAGE | TREE_BITS
        o, ost, _ = P.oracle_render(sd, sc, light_tree=True)
        assert n_bit_diff(g, o) == 0 and all(gst[c] == ost[c] for c in COUNTERS), r  # the oracle's shard
        assert not np.any((acc != 0) & (g != 0))
        acc += g
        for c in COUNTERS:
            counts[c] += gst[c]
    assert n_bit_diff(acc, whole) == 0 and all(counts[c] == wst[c] for c in COUNTERS)


def test_sample_ranges_with_an_index_sampler(ctx):
    sd = T.SCHED_SCENE()
    cfg = make_config(**T.EXTRA["schedules-sobol"][1])
    whole, wst, wstates = P.oracle_render(sd, cfg, light_tree=True)
    with capi.options(**T.BVH_T):
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
            assert info["kernel_flags"] == P.F_BVH | P.F_PMJ | P.F_STAGE | TREE_BITS
            for k in COUNTERS:
                counts[k] += st[k]
    assert n_bit_diff(film.read(), whole) == 0 and np.array_equal(states, wstates) and all(counts[k] == wst[k] for k in COUNTERS)


def test_half_the_tiles_retired_after_the_first_pass(ctx):
    """akr_pt_set_active_tiles with a tree: the retired tiles keep the oracle's 4-sample film and states, the others get its 8-sample ones"""
    sd = T.SCHED_SCENE()
    n, keep = 32 * 32, [1, 2]  # of the 2 x 2 tiles of 16 x 16 pixels
    kw = dict(spp_per_pass=4, max_depth=5, rr_depth=2, sampler_seed=8, tile_w=16, tile_h=16)
    cfg = make_config(spp=8, **kw)

    def drive(se, film):
        assert se.passes(1, blocking=True) == 4
        se.set_active_tiles(keep)
        assert se.passes(1, blocking=True) == 8

    g, gst, gstates, info = gpu_render(ctx, sd, cfg, T.EXH_T, drive=drive)
    assert info["kernel_flags"] == P.F_STAGE | TREE_BITS
    half = make_config(spp=4, **kw)
    f4, st4, s4 = P.oracle_render(sd, half, light_tree=True)
    f8, st8, s8 = P.oracle_render(sd, half, film=f4.copy(), states=s4.copy(), light_tree=True)
    m = am.tile_mask(32, 32, 16, 16, keep).reshape(-1)
    assert m.sum() == n // 2
    rgb = np.where(np.repeat(m, 3), f8[:3 * n], f4[:3 * n])
    assert n_bit_diff(g[:3 * n], rgb) == 0 and np.array_equal(g[6 * n:], np.where(m, f8[6 * n:], f4[6 * n:]))
    assert np.array_equal(gstates, np.where(np.repeat(m, 2), s8, s4))
    assert gst["n_samples"] == 4 * n + 4 * (n // 2)


# ---------------------------------------------------------------------------------------------------------------- one scene, many sessions
@pytest.mark.parametrize("pipeline", ["repr_aces", "acescg"])
def test_mode_and_lights_changed_between_sessions(ctx, pipeline):
    """One capi.Scene under a non-default pipeline (records and nodes of its own colour set, uploaded per session): the tree, the mode off, the mode on
    with a light more, the lights cleared and refilled. Every film, counter and state is that of a fresh OracleScene of that state."""
    cfg = make_config(**dict(T.EXTRA["sessions"][1], color=P.PIPELINES[pipeline]))
    sd = T.SESSION_SCENE()
    base = P.F_STAGE | P.F_PUNCT
    with capi.options(**T.EXH_T):
        scene = capi.Scene(ctx, sd)
    films = [check(ctx, sd, cfg, T.EXH_T, base | T.F_LTREE, scene=scene)[0]]
    scene.set_light_tree(False)
    films.append(check(ctx, sd, cfg, T.EXH_T, base, scene=scene, light_tree=False)[0])
    scene.set_light_tree(True)
    scene.add_punctual_light(T.COLOURED_MORE)
    sd2 = dataclasses.replace(sd, lights=T.COLOURED + [T.COLOURED_MORE])
    assert scene.light_tree() == (1, 2 * T.n_local(sd2) - 1)
    films.append(check(ctx, sd2, cfg, T.EXH_T, base | T.F_LTREE, scene=scene)[0])
    scene.clear_punctual_lights()
    for l in T.COLOURED_AFTER:
        scene.add_punctual_light(l)
    sd3 = dataclasses.replace(sd, lights=list(T.COLOURED_AFTER))
    assert scene.light_tree() == (1, 2 * T.n_local(sd3) - 1)
    films.append(check(ctx, sd3, cfg, T.EXH_T, base | T.F_LTREE, scene=scene)[0])
    assert all(n_bit_diff(films[i], films[j]) > 0 for i in range(4) for j in range(i))


# ---------------------------------------------------------------------------------------------------------------- readers
def reader_scene_file(tmp_path):
    """one scene.json with four local lights (soft and delta, a spot) and a sun between them"""
    lights = [abi.PunctualLightData(abi.LIGHT_POINT, position=(0.3, -0.2, 1.5), color=(3.0, 2.0, 1.0), strength=2.0, radius=0.25),
              abi.PunctualLightData(abi.LIGHT_SPOT, position=(0.25, 0.5, 2.0), direction=(0.1, -0.3, -1.0), cone_angle=0.375, blend=0.25, color=(1.0, 4.0, 2.0), strength=1.5),
              abi.PunctualLightData(abi.LIGHT_SUN, direction=(0.2, -0.1, -1.0), color=(1.0, 0.9, 0.8), strength=0.5, angle=0.5),
              abi.PunctualLightData(abi.LIGHT_POINT, position=(-0.5, -0.5, 1.0), color=(2.0, 1.0, 1.0), strength=1.0),
              abi.PunctualLightData(abi.LIGHT_POINT, position=(-0.25, 0.5, 0.5), color=(1.0, 1.0, 3.0), strength=0.5, radius=0.125)]
    entries = {}
    for k, l in enumerate(lights):
        e = json_light(l)
        if l.radius:
            e["data"]["radius"] = l.radius
        if l.angle:
            e["data"]["angle"] = l.angle
        entries["abcde"[k]] = e
    return write_scene_with_lights(tmp_path, entries)


READER_CFG = dict(spp=8, spp_per_pass=8, max_depth=3, sampler_seed=2)


def test_scene_json_both_readers(ctx, tmp_path):
    """the file read by akr_scene_load under option light_tree = 1 and by the Python reader, rendered by the library and by the oracle told of the mode"""
    path = reader_scene_file(tmp_path)
    cfg = make_config(**READER_CFG)
    with capi.options(**T.EXH_T):
        lib_scene = capi.Scene(ctx, path, 32, 32)
        film = capi.Film(ctx, 32, 32)
        se = capi.PtSession(ctx, lib_scene, cfg, film)
        se.passes(1000, blocking=True)
        info, gstates = se.kernel_info(), se.sampler_states(32 * 32)
        gst = se.end()
    assert info["kernel_flags"] == P.F_STAGE | TREE_BITS
    sd = scene_json.load_scene(path, 32, 32)
    assert sd.lights == lib_scene.punctual_lights() and len(sd.lights) == 5 and lib_scene.light_tree() == (1, 7)
    o, ost, ostates = P.oracle_render(sd, cfg, light_tree=True)
    assert_parity(film.read(), o, 32, 32, gst, ost)
    assert np.array_equal(gstates, ostates)
