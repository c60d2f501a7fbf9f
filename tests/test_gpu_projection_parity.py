"""The orthographic and the panorama camera on the GPU against the CPU oracle (oracle/akr_oracle.c or_camera_ray, a restatement of DESIGN.md 4.17
that shares no text with device/dpath.h), bit for bit: raw films, ray counters and final sampler states over projections x materials x routes x
lighting, every LENS unit of the pt kernels, axis-aligned rays along the walls and through the edges and vertices of a room on the film's lattice
(exhaustive, BVH, kept scenes, both schedules, carried traversal), the panorama's poles, seam and a 2^-6 window inside a closed room, schedules,
`aov` and the FEAT guides, and one scene.json per projection read by both readers. The cases are those of tests/projection_parity_cases.py;
tests/test_projection_parity_cases.py shows on the CPU that none of them can pass emptily. Every case asserts the kernel it ran, is at most
32 x 32 and at most 16 spp."""
import json

import numpy as np
import pytest

from akari_render_amd import abi, capi, distributed
from oracle import pyoracle, scene_json
from tests import adaptive_model as am
from tests import projection_parity_cases as J
from tests import punct_parity_cases as P
from tests.helpers import make_config, n_bit_diff
from tests.test_gpu_parity import assert_parity
from tests.test_gpu_punct_parity import COUNTERS, _aov_cfg, gpu_render, reader_scene_file

pytestmark = pytest.mark.gpu


def check(ctx, sd, cfg, opts, flags, want=None, wavefront=False, **oracle_kw):
    """test_gpu_punct_parity.check: the session runs the kernel with `flags` (and the host plan, which the session follows, has `want`); film,
    counters and states are the oracle's. A wavefront session must say so; its kernels stage nothing, so bit 2 is not compared there."""
    if want is not None:
        v = P.host_plan(sd, cfg, opts)["variant"]
        assert {k: v[k] for k in want} == want, (v, want)
    g, gst, gstates, info = gpu_render(ctx, sd, cfg, opts)
    mask = ~P.F_STAGE if wavefront else ~0
    assert info["kernel_flags"] & mask == flags & mask and info["kernel_flags"] & P.F_LENS and info["specialised"] == 0, (info, flags)
    assert ("wavefront" in info["status"]) == wavefront, info
    o, ost, ostates = P.oracle_render(sd, cfg, **oracle_kw)
    assert_parity(g, o, sd.camera.width, sd.camera.height, gst, ost)
    assert np.array_equal(gstates, ostates), f"{np.count_nonzero(gstates != ostates)} sampler state words differ"
    return g, gst


def run_case(ctx, name):
    case = J.CASES[name]
    kw = dict(light_tree=True) if "ltree" in case.tags else {}
    return check(ctx, case.scene(), case.config(), case.opts, J.flags(case), case.want, wavefront=bool(case.opts.get("wavefront")), **kw)


# ---------------------------------------------------------------------------------------------------------------- the case table
@pytest.mark.parametrize("name", J.MATERIAL_CASES)
def test_projections_materials_routes_lighting(ctx, name):
    run_case(ctx, name)


@pytest.mark.parametrize("name", [n for n in J.UNIT_CASES if "feat" not in J.CASES[n].tags])
def test_every_lens_unit(ctx, name):
    run_case(ctx, name)


@pytest.mark.parametrize("name", [n for n in J.UNIT_CASES if "feat" in J.CASES[n].tags])
def test_every_lens_unit_with_guides(ctx, name):
    """the FEAT units: a session that collects the guides; its colour film, counters and states are the oracle's pt render's (the guides themselves
    are held to the oracle's aov below)"""
    case = J.CASES[name]
    sd, cfg = case.scene(), case.config()
    w, h = sd.camera.width, sd.camera.height
    with capi.options(**case.opts):
        scene = capi.Scene(ctx, sd)
        v = scene.features_plan(cfg, feat=True)["variant"]
        assert v["feat"] == 1 and {k: v[k] for k in case.want} == case.want, (v, case.want)
        film, albedo, normal = (capi.Film(ctx, w, h) for _ in range(3))
        se = capi.PtSession(ctx, scene, cfg, film, albedo, normal)
        se.passes(1000, blocking=True)
        info, gstates = se.kernel_info(), se.sampler_states(w * h)
        gst = se.end()
    assert info["kernel_flags"] == J.flags(case) and info["kernel_flags"] & P.F_FEAT and info["kernel_flags"] & P.F_LENS, info
    o, ost, ostates = P.oracle_render(sd, cfg)
    assert_parity(film.read(), o, w, h, gst, ost)
    assert np.array_equal(gstates, ostates)


@pytest.mark.parametrize("name", J.ALIGNED_CASES)
def test_aligned_rays(ctx, name):
    """primary rays along exactly (0, 0, -1) or (-1, 0, 0): every plane row parallel to them gives a zero divisor in the pair walk, two of safe_inv's
    three reciprocals are +-1e20 and origins lie on slab planes in the tree, and with the box filter of radius 0 rays pass exactly through shared
    edges and vertices, where the winning triangle is the oracle's rule"""
    run_case(ctx, name)


@pytest.mark.parametrize("turned", [False, True], ids=["identity", "turned"])
def test_aligned_rays_cull_the_boxes_beside_them(ctx, turned):
    """What no film shows: fminf / fmaxf drop a NaN operand, so a slab test whose reciprocals were 1 / 0 would still find every hit -- it would only stop
    culling across the ray, and visit boxes the ray never enters. safe_inv's +-1e20 keeps the two axes across an aligned ray in the test; the primary
    rays' node visits then stay inside the bound geometry gives (projection_parity_cases.aligned_visit_bound: the nodes whose ancestors' boxes contain
    the ray's line), and the film is still the oracle's."""
    sd = J.aligned_room("diffuse", turned)
    cfg = make_config(spp=1, spp_per_pass=1, max_depth=0, sampler_seed=3, **J.BOX0)
    bound, n_nodes, n_rays = J.aligned_visit_bound(sd, P.BVH)
    g, gst, gstates, info = gpu_render(ctx, sd, cfg, P.BVH)
    assert info["kernel_flags"] & P.F_BVH and info["kernel_flags"] & P.F_LENS
    assert gst["n_samples"] == gst["n_closest"] == n_rays and gst["n_shadow"] == 0  # one closest-hit ray a pixel and nothing else
    assert n_rays <= gst["n_node_visits"] <= bound, (gst["n_node_visits"], bound, n_nodes)
    o, ost, ostates = P.oracle_render(sd, cfg)
    assert_parity(g, o, 32, 32, gst, ost)
    assert np.array_equal(gstates, ostates)


@pytest.mark.parametrize("name", J.PANORAMA_CASES)
def test_panorama_extremes(ctx, name):
    run_case(ctx, name)


# ---------------------------------------------------------------------------------------------------------------- schedules
def test_progressive_passes(ctx):
    """spp_per_pass splits: the film after every pass is the oracle's film of that many samples (orthographic)"""
    sd = J.SCHED["progressive"]()
    cfg = make_config(**J.EXTRA["schedules-progressive"][1])
    prefixes = []

    def drive(se, film):
        for done in (5, 10, 12):
            assert se.passes(1, blocking=True) == done
            prefixes.append(film.read())

    g, gst, gstates, info = gpu_render(ctx, sd, cfg, P.BVH, drive=drive)
    assert info["kernel_flags"] == P.F_BVH | P.F_STAGE | P.F_PUNCT | P.F_LENS
    film, states = None, P.initial_states(cfg, 32, 32)
    total = dict.fromkeys(COUNTERS, 0)
    for k, n in enumerate((5, 5, 2)):
        film, ost, states = P.oracle_render(sd, make_config(spp=n, spp_per_pass=n, max_depth=5, rr_depth=2, sampler_seed=4), film=film, states=states)
        assert n_bit_diff(prefixes[k], film) == 0, f"after pass {k + 1}: {n_bit_diff(prefixes[k], film)} floats differ"
        for c in COUNTERS:
            total[c] += ost[c]
    assert all(gst[c] == total[c] for c in COUNTERS) and np.array_equal(gstates, states)
    whole = P.oracle_render(sd, cfg)
    assert n_bit_diff(g, whole[0]) == 0 and np.array_equal(gstates, whole[2])


def test_two_tile_shards(ctx):
    """(panorama)"""
    sd = J.SCHED["shards"]()
    cfg = make_config(**J.EXTRA["schedules-shards"][1])
    whole, wst, _ = P.oracle_render(sd, cfg)
    acc, counts = np.zeros_like(whole), dict.fromkeys(COUNTERS, 0)
    for r in range(2):
        sc = distributed.shard_config(cfg, r, 2, 8, 8)
        g, gst, _, info = gpu_render(ctx, sd, sc, P.EXH)
        assert info["kernel_flags"] == P.F_PMJ | P.F_STAGE | P.F_PUNCT | P.F_LENS
        o, ost, _ = P.oracle_render(sd, sc)
        assert n_bit_diff(g, o) == 0 and all(gst[c] == ost[c] for c in COUNTERS), r  # the oracle's shard
        assert not np.any((acc != 0) & (g != 0))
        acc += g
        for c in COUNTERS:
            counts[c] += gst[c]
    assert n_bit_diff(acc, whole) == 0 and all(counts[c] == wst[c] for c in COUNTERS)


def test_sample_ranges_with_an_index_sampler(ctx):
    """(orthographic with a lens, Sobol')"""
    sd = J.SCHED["ranges"]()
    cfg = make_config(**J.EXTRA["schedules-ranges"][1])
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
            assert info["kernel_flags"] == P.F_BVH | P.F_PMJ | P.F_STAGE | P.F_PUNCT | P.F_LENS
            for k in COUNTERS:
                counts[k] += st[k]
    assert n_bit_diff(film.read(), whole) == 0 and np.array_equal(states, wstates) and all(counts[k] == wst[k] for k in COUNTERS)


def test_half_the_tiles_retired_after_the_first_pass(ctx):
    """akr_pt_set_active_tiles: the retired tiles keep the oracle's 4-sample film and states, the others get its 8-sample ones (a panorama's window)"""
    sd = J.SCHED["retired"]()
    n, keep = 32 * 32, [1, 2]  # of the 2 x 2 tiles of 16 x 16 pixels
    kw = J.EXTRA["schedules-retired"][1]
    cfg = make_config(**kw)

    def drive(se, film):
        assert se.passes(1, blocking=True) == 4
        se.set_active_tiles(keep)
        assert se.passes(1, blocking=True) == 8

    g, gst, gstates, info = gpu_render(ctx, sd, cfg, P.EXH, drive=drive)
    assert info["kernel_flags"] == P.F_STAGE | P.F_PUNCT | P.F_LENS
    half = make_config(**dict(kw, spp=4))
    f4, st4, s4 = P.oracle_render(sd, half)
    f8, st8, s8 = P.oracle_render(sd, half, film=f4.copy(), states=s4.copy())
    m = am.tile_mask(32, 32, 16, 16, keep).reshape(-1)
    assert m.sum() == n // 2
    rgb = np.where(np.repeat(m, 3), f8[:3 * n], f4[:3 * n])
    assert n_bit_diff(g[:3 * n], rgb) == 0 and np.array_equal(g[6 * n:], np.where(m, f8[6 * n:], f4[6 * n:]))
    assert np.array_equal(gstates, np.where(np.repeat(m, 2), s8, s4))
    assert gst["n_samples"] == 4 * n + 4 * (n // 2)


# ---------------------------------------------------------------------------------------------------------------- aov and the guides
@pytest.mark.parametrize("route", ["exh", "bvh"])
@pytest.mark.parametrize("which", list(J.AOV_SCENES))
def test_aov(ctx, which, route, aov=abi.AOV_ALBEDO):
    """k_aov<LENS> through either projection against the oracle's aov"""
    sd = J.AOV_SCENES[which]()
    a = _aov_cfg(make_config(spp=8, sampler_seed=2), aov)
    with capi.options(**(P.BVH if route == "bvh" else P.EXH)):
        scene = capi.Scene(ctx, sd)
        assert scene.projection() == sd.projection
        film = capi.Film(ctx, 32, 32)
        capi.aov_render(ctx, scene, a, film)
    assert n_bit_diff(film.read(), pyoracle.OracleScene(sd).aov_render(a)[0]) == 0


@pytest.mark.parametrize("which", list(J.FEAT_SCENES))
@pytest.mark.parametrize("sampler", ["pmj02bn", "sobol"])
def test_feature_guides_equal_the_oracles_aov(ctx, sampler, which):
    """with an index-based sampler the depth-0 guides of a FEAT session are the aov integrator's albedo and shading normal of the same
    samples -- here the oracle's, through the projection; the colour film stays the oracle's pt film"""
    sd = J.FEAT_SCENES[which]()
    cfg = make_config(spp=8, spp_per_pass=4, max_depth=5, sampler_type=P.SAMPLERS[sampler], sampler_seed=5)
    with capi.options(**P.EXH):
        scene = capi.Scene(ctx, sd)
        film, albedo, normal = (capi.Film(ctx, 32, 32) for _ in range(3))
        se = capi.PtSession(ctx, scene, cfg, film, albedo, normal)
        se.passes(1000, blocking=True)
        info, gstates = se.kernel_info(), se.sampler_states(32 * 32)
        gst = se.end()
    assert info["kernel_flags"] & P.F_FEAT and info["kernel_flags"] & P.F_LENS
    pyoracle.set_pmj_tables(*capi.host_pmj02bn_tables())
    osc = pyoracle.OracleScene(sd)
    assert n_bit_diff(albedo.read(), osc.aov_render(_aov_cfg(cfg, abi.AOV_ALBEDO))[0]) == 0
    assert n_bit_diff(normal.read(), osc.aov_render(_aov_cfg(cfg, abi.AOV_NS))[0]) == 0
    o, ost, ostates = P.oracle_render(sd, cfg)
    assert_parity(film.read(), o, 32, 32, gst, ost)
    assert np.array_equal(gstates, ostates)


# ---------------------------------------------------------------------------------------------------------------- readers
def projected_scene_file(tmp_path, camera_type):
    """tests/test_gpu_punct_parity.py's file (a light of each kind, a lens) with the camera entry rewritten: the orthographic camera keeps the lens,
    the panorama has none"""
    path = reader_scene_file(tmp_path)
    doc = json.load(open(path))
    cam = doc["camera"]
    cam["type"] = camera_type
    cam["data"].pop("fov")
    if camera_type == "orthographic":
        cam["data"]["ortho_scale"] = 2.5
        cam["data"]["focal_distance"], cam["data"]["fstop"] = 1.0, 2.0  # (radius 1/4, focused well in front of the quad: the quad is blurred)
    else:
        cam["data"].pop("focal_distance")
        cam["data"].pop("fstop")
        cam["data"].update(longitude_min=-1.0, longitude_max=0.75, latitude_min=-0.5)
    open(path, "w").write(json.dumps(doc))
    return path


READER_CFG = dict(spp=8, spp_per_pass=8, max_depth=3, sampler_seed=2)


@pytest.mark.parametrize("camera_type", ["orthographic", "panorama"])
def test_scene_json_both_readers(ctx, tmp_path, camera_type):
    """the file read by akr_scene_load and by the Python reader, rendered by the library and by the oracle"""
    path = projected_scene_file(tmp_path, camera_type)
    cfg = make_config(**READER_CFG)
    with capi.options(lens=1, **P.EXH):
        lib_scene = capi.Scene(ctx, path, 32, 32)
        film = capi.Film(ctx, 32, 32)
        se = capi.PtSession(ctx, lib_scene, cfg, film)
        se.passes(1000, blocking=True)
        info, gstates = se.kernel_info(), se.sampler_states(32 * 32)
        gst = se.end()
    assert info["kernel_flags"] == P.F_STAGE | P.F_LENS | P.F_PUNCT
    sd = scene_json.load_scene(path, 32, 32, lens=True)
    assert sd.projection == lib_scene.projection() and sd.projection.type == (J.ORTHO if camera_type == "orthographic" else J.PANORAMA)
    assert sd.lights == lib_scene.punctual_lights() and sd.lens == lib_scene.lens() and (sd.lens is not None) == (camera_type == "orthographic")
    o, ost, ostates = P.oracle_render(sd, cfg)
    assert_parity(film.read(), o, 32, 32, gst, ost)
    assert np.array_equal(gstates, ostates)
    assert n_bit_diff(o, P.oracle_render(sd, cfg, projection=False)[0]) / o.size >= 0.25
