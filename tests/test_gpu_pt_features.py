"""Guides collected inside the pt pass (the FEAT kernels) on the GPU: the colour film, sampler states and counters of a session
that collects guides are those of the session that does not; the guides are akr_aov_render's films bit for bit wherever pt draws what aov draws;
one set of guides under every route; weights and retired tiles; the refusals and fall-backs; akari-cli --denoise-features."""
import copy
import json
import os
import subprocess

import numpy as np
import pytest

from akari_render_amd import abi, capi, distributed
from oracle import pyoracle, scene_json
from tests.helpers import cbox_variant, grid_scene, instanced_scene, make_config, n_bit_diff, textured_room
from tests.test_environment import sample_image

pytestmark = pytest.mark.gpu
F = np.float32
FEAT_BIT = 64
SAMPLERS = {"independent": abi.SAMPLER_INDEPENDENT, "pmj02bn": abi.SAMPLER_PMJ02BN, "sobol": abi.SAMPLER_SOBOL}
EXH = dict(force_bvh=0, instancing=0, wavefront=0, specialise=0)
BVH = dict(force_bvh=1, instancing=0, wavefront=0, specialise=0)


def _run(ctx, scene, cfg, feat=True, drive=None):
    """one session to the end -> (colour, albedo, normal raw films or None, sampler states, kernel info, stats)"""
    w, h = scene.info().width, scene.info().height
    film = capi.Film(ctx, w, h)
    albedo, normal = (capi.Film(ctx, w, h), capi.Film(ctx, w, h)) if feat else (None, None)
    se = capi.PtSession(ctx, scene, cfg, film, albedo, normal)
    if drive:
        drive(se)
    else:
        se.passes(1000, blocking=True)
    states = se.sampler_states(w * h)
    info = se.kernel_info()
    stats = se.end()
    return film.read(), (albedo.read() if feat else None), (normal.read() if feat else None), states, info, stats


def _aov(ctx, scene, cfg, spp=None):
    """the two aov films of the same spp, sampler, seed, filter and colour pipeline -> (albedo, ns not remapped)"""
    w, h = scene.info().width, scene.info().height
    out = []
    for aov in (abi.AOV_ALBEDO, abi.AOV_NS):
        ac = abi.AovConfig.default()
        ac.spp, ac.aov, ac.remap = (spp or cfg.spp), aov, 0
        ac.filter_type, ac.filter_radius, ac.sampler_type, ac.sampler_seed, ac.color = cfg.filter_type, cfg.filter_radius, cfg.sampler_type, cfg.sampler_seed, cfg.color
        film = capi.Film(ctx, w, h)
        capi.aov_render(ctx, scene, ac, film)
        out.append(film.read())
    return out


def _env():
    img = sample_image(W=48, H=24, seed=4) * F(0.6)
    a = -0.4
    rot = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    return abi.EnvironmentData(image=img, strength=1.5, rotation=rot.astype(F), filter=abi.TEX_FILTER_LINEAR)


def _open_room(w, h):
    """the open heightfield (a tree, per-corner normals, two materials) in front of an environment: camera rays above the floor leave the scene"""
    sd = grid_scene(n=6, width=w, height=h, with_normals=True)
    sd.environment = _env()
    return sd


# ---------------------------------------------------------------------------------------------------------------- 1. colour untouched
def _route(name, cbox_path, w, h):
    """-> (scene data, options, config fields)"""
    cbox = lambda: scene_json.load_scene(cbox_path, w, h)
    if name == "cbox_force_diffuse":
        return cbox(), EXH, dict(force_diffuse=1)
    if name == "cbox_full":
        return cbox(), EXH, {}
    if name == "cbox_bvh":
        return cbox_variant(cbox(), "glass_coat"), BVH, {}
    if name == "textured_room":
        return textured_room(w, h), EXH, {}
    if name == "textured_room_bvh":
        return textured_room(w, h, n_floor=8), BVH, {}
    if name == "environment":
        sd = textured_room(w, h)
        sd.environment = _env()
        return sd, EXH, {}
    if name == "environment_misses":
        return _open_room(w, h), BVH, {}
    if name == "lens":
        sd = cbox()
        sd.lens = abi.LensData(0.2, 5.0)
        return sd, EXH, {}
    raise ValueError(name)


ROUTES = ["cbox_force_diffuse", "cbox_full", "cbox_bvh", "textured_room", "textured_room_bvh", "environment", "environment_misses", "lens"]


@pytest.mark.parametrize("sampler", list(SAMPLERS))
@pytest.mark.parametrize("route", ROUTES)
def test_colour_is_untouched(ctx, cbox_path, route, sampler):
    w = h = 48
    sd, opts, fields = _route(route, cbox_path, w, h)
    cfg = make_config(spp=8, spp_per_pass=4, max_depth=8, sampler_type=SAMPLERS[sampler], sampler_seed=3, **fields)
    with capi.options(**opts):
        scene = capi.Scene(ctx, sd)
        plain, _, _, p_states, p_info, p_stats = _run(ctx, scene, cfg, feat=False)
        film, albedo, normal, states, info, stats = _run(ctx, scene, cfg)
    assert p_info["kernel_flags"] & FEAT_BIT == 0 and info["kernel_flags"] & FEAT_BIT == FEAT_BIT
    assert (p_info["kernel_flags"] ^ info["kernel_flags"]) & ~(FEAT_BIT | 8) == 0  # the same kernel but for FEAT (and DEFER, which FEAT excludes)
    assert n_bit_diff(film, plain) == 0 and np.array_equal(states, p_states)
    for k in ("n_samples", "n_closest", "n_shadow", "n_shaded", "n_node_visits", "n_tri_tests"):
        assert stats[k] == p_stats[k], k
    assert np.any(albedo[:3 * w * h] != 0) and np.any(normal[:3 * w * h] != 0)
    if route == "cbox_full" and sampler == "independent":  # ... and both are the oracle's (tests/test_gpu_lens.py test_nothing_moves_without_a_lens)
        o_states = pyoracle.init_pcg32_states(w * h, cfg.sampler_seed)
        o_film, _ = pyoracle.OracleScene(sd).render(cfg, states=o_states)
        assert n_bit_diff(film, o_film) == 0 and np.array_equal(states, o_states)


# ---------------------------------------------------------------------------------------------------------------- 2. guides = aov, index-based samplers
def _guide_scene(name, cbox_path, w, h):
    cbox = lambda: scene_json.load_scene(cbox_path, w, h)
    if name == "cbox_glass_coat":  # transmission, coat, a metal
        return cbox_variant(cbox(), "glass_coat"), EXH, 0
    if name == "cbox_kinds":  # the glass, diffuse and emission materials, a constant normal input
        return cbox_variant(cbox(), "kinds"), EXH, 0
    if name == "cbox_kinds_bvh":
        return cbox_variant(cbox(), "kinds"), BVH, 0
    if name == "textured_room":
        return textured_room(w, h), EXH, 0
    if name == "textured_room_bvh":
        return textured_room(w, h, n_floor=8), BVH, 0
    if name == "grid_normals":
        return grid_scene(n=5, width=w, height=h, with_normals=True), EXH, 0
    if name == "grid_normals_bvh":
        return grid_scene(width=w, height=h, with_normals=True), BVH, 0
    if name == "environment_misses":
        return _open_room(w, h), BVH, 0
    if name == "lens":
        sd = cbox_variant(cbox(), "kinds")
        sd.lens = abi.LensData(0.2, 5.0)
        return sd, EXH, 0
    if name == "acescg":
        return textured_room(w, h), EXH, abi.COLOR_REPR_ACESCG | abi.COLOR_RGB_ACESCG
    raise ValueError(name)


GUIDE_SCENES = ["cbox_glass_coat", "cbox_kinds", "cbox_kinds_bvh", "textured_room", "textured_room_bvh", "grid_normals", "grid_normals_bvh", "environment_misses", "lens", "acescg"]


def _assert_guides(albedo, normal, film, a_aov, n_aov, n_pix):
    assert n_bit_diff(albedo, a_aov) == 0, f"albedo: {n_bit_diff(albedo, a_aov)} floats differ"
    assert n_bit_diff(normal, n_aov) == 0, f"normal: {n_bit_diff(normal, n_aov)} floats differ"
    assert np.array_equal(albedo[6 * n_pix:], film[6 * n_pix:]) and np.array_equal(normal[6 * n_pix:], film[6 * n_pix:])


@pytest.mark.parametrize("sampler", ["pmj02bn", "sobol"])
@pytest.mark.parametrize("name", GUIDE_SCENES)
def test_guides_equal_aov_index_based(ctx, cbox_path, name, sampler):
    w, h = 40, 32
    sd, opts, color = _guide_scene(name, cbox_path, w, h)
    cfg = make_config(spp=12, spp_per_pass=4, max_depth=6, sampler_type=SAMPLERS[sampler], sampler_seed=5, color=color)
    with capi.options(**opts):
        scene = capi.Scene(ctx, sd)
        film, albedo, normal, _, info, _ = _run(ctx, scene, cfg)
        a_aov, n_aov = _aov(ctx, scene, cfg)
    assert info["kernel_flags"] & FEAT_BIT
    _assert_guides(albedo, normal, film, a_aov, n_aov, w * h)
    if name == "environment_misses":  # some pixels do miss: their guides are (0, 0, 0) with the full weight
        miss = np.all(albedo[:3 * w * h].reshape(-1, 3) == 0, axis=1) & np.all(normal[:3 * w * h].reshape(-1, 3) == 0, axis=1)
        assert 0 < miss.sum() < w * h and np.all(albedo[6 * w * h:][miss] == 12)


@pytest.mark.parametrize("sampler", ["pmj02bn", "sobol"])
@pytest.mark.parametrize("name", ["cbox_kinds", "textured_room", "textured_room_bvh"])
def test_guides_equal_aov_partial_workgroup(ctx, cbox_path, name, sampler):
    """41 x 29: the last tiles are partial, lanes with in_frame == false"""
    w, h = 41, 29
    sd, opts, color = _guide_scene(name, cbox_path, w, h)
    cfg = make_config(spp=12, spp_per_pass=4, max_depth=6, sampler_type=SAMPLERS[sampler], sampler_seed=5, color=color)
    with capi.options(**opts):
        scene = capi.Scene(ctx, sd)
        film, albedo, normal, _, _, _ = _run(ctx, scene, cfg)
        a_aov, n_aov = _aov(ctx, scene, cfg)
    _assert_guides(albedo, normal, film, a_aov, n_aov, w * h)


# ---------------------------------------------------------------------------------------------------------------- 3. guides = aov, independent sampler
@pytest.mark.parametrize("name", ["cbox_kinds", "textured_room", "textured_room_bvh", "environment_misses", "lens"])
def test_guides_equal_aov_independent(ctx, cbox_path, name):
    """PCG32: a later sample starts where the earlier ones stopped, so pt draws what aov draws only with camera dimensions alone (max_depth = 0)
    and in one pass (spp_per_pass >= spp). max_depth = 0 still records the guides."""
    w, h = 40, 32
    sd, opts, color = _guide_scene(name, cbox_path, w, h)
    cfg = make_config(spp=12, spp_per_pass=16, max_depth=0, sampler_type=abi.SAMPLER_INDEPENDENT, sampler_seed=9, color=color)
    with capi.options(**opts):
        scene = capi.Scene(ctx, sd)
        film, albedo, normal, states, _, stats = _run(ctx, scene, cfg)
        a_aov, n_aov = _aov(ctx, scene, cfg)
    assert stats["n_shaded"] == 0
    _assert_guides(albedo, normal, film, a_aov, n_aov, w * h)
    # (the binding does not expose the sampler states an aov render leaves: films only)


def test_guides_ignore_what_the_path_does_with_the_vertex(ctx, cbox_path):
    """force_diffuse, indirect_only, debug_depth and max_depth change the colour film, not the guides (pmj02bn: dimensions by index)"""
    w, h = 40, 32
    sd = cbox_variant(scene_json.load_scene(cbox_path, w, h), "kinds")
    base = dict(spp=8, spp_per_pass=4, max_depth=6, sampler_type=abi.SAMPLER_PMJ02BN, sampler_seed=5)
    with capi.options(**EXH):
        scene = capi.Scene(ctx, sd)
        ref = _run(ctx, scene, make_config(**base))
        for fields in (dict(force_diffuse=1), dict(indirect_only=1), dict(debug_depth=2), dict(max_depth=0), dict(max_depth=1)):
            got = _run(ctx, scene, make_config(**{**base, **fields}))
            assert n_bit_diff(got[0], ref[0]) > 0, fields
            assert n_bit_diff(got[1], ref[1]) == 0 and n_bit_diff(got[2], ref[2]) == 0, fields


# ---------------------------------------------------------------------------------------------------------------- 4. one set of guides under every route
@pytest.mark.parametrize("name", ["cbox_glass_coat", "textured_room"])
def test_one_set_of_guides_under_every_route(ctx, cbox_path, name):
    w, h = 40, 32
    sd = cbox_variant(scene_json.load_scene(cbox_path, w, h), "glass_coat") if name == "cbox_glass_coat" else textured_room(w, h, n_floor=2)
    cfg = make_config(spp=12, spp_per_pass=4, max_depth=8, sampler_type=abi.SAMPLER_INDEPENDENT, sampler_seed=7)
    with capi.options(**EXH):
        scene = capi.Scene(ctx, sd)
        assert scene.info().uses_bvh == 0
        ref = _run(ctx, scene, cfg)

    def same(got, what):
        for k, plane in enumerate(("colour", "albedo", "normal")):
            assert n_bit_diff(got[k], ref[k]) == 0, f"{what}: {plane}: {n_bit_diff(got[k], ref[k])} floats differ"
        assert np.array_equal(got[3], ref[3]), what

    def three_calls(se):
        for _ in range(3):
            se.passes(1, blocking=True)

    with capi.options(**BVH):
        bvh = capi.Scene(ctx, sd)
        assert bvh.info().uses_bvh == 1
        same(_run(ctx, bvh, cfg), "force_bvh")
        with capi.options(max_fused_passes=1):
            same(_run(ctx, bvh, cfg), "max_fused_passes=1")
        same(_run(ctx, bvh, cfg, drive=three_calls), "three passes(1) calls")
        with capi.options(wavefront=-1, sched_trial=1):  # the timed schedule trial stays on the megakernel
            got = _run(ctx, bvh, cfg)
            same(got, "sched_trial")
            assert "wavefront" not in got[4]["status"] and "trial" not in got[4]["status"], got[4]["status"]
    with capi.options(**EXH):
        # two tile shards, summed on the host
        acc = [np.zeros(7 * w * h, F) for _ in range(3)]
        for r in range(2):
            films = [capi.Film(ctx, w, h) for _ in range(3)]
            capi.pt_render_features(ctx, scene, distributed.shard_config(cfg, r, 2, 8, 8), *films)
            for k in range(3):
                part = films[k].read()
                assert not np.any((acc[k] != 0) & (part != 0))
                acc[k] = acc[k] + part
        for k in range(3):
            assert n_bit_diff(acc[k], ref[k]) == 0, ("tile shards", k)
        # sample ranges, pmj02bn: sessions of consecutive ranges accumulating into the same three films (as tests/test_gpu_lens.py sums them)
        pcfg = dict(spp=12, spp_per_pass=4, max_depth=8, sampler_type=abi.SAMPLER_PMJ02BN, sampler_seed=7)
        whole = [capi.Film(ctx, w, h) for _ in range(3)]
        capi.pt_render_features(ctx, scene, make_config(**pcfg), *whole)
        films = [capi.Film(ctx, w, h) for _ in range(3)]
        for begin, count in ((0, 7), (7, 5)):
            capi.pt_render_features(ctx, scene, make_config(sample_begin=begin, sample_count=count, **pcfg), *films)
        for k in range(3):
            assert n_bit_diff(films[k].read(), whole[k].read()) == 0, ("sample ranges", k)


# ---------------------------------------------------------------------------------------------------------------- 5. weights and retirement
def test_weights_and_retired_tiles(ctx, cbox_path):
    w, h = 48, 32
    sd = textured_room(w, h)
    cfg = make_config(spp=12, spp_per_pass=4, max_depth=6, sampler_type=abi.SAMPLER_INDEPENDENT, sampler_seed=2, tile_w=16, tile_h=16)
    n = w * h
    with capi.options(**EXH):
        scene = capi.Scene(ctx, sd)
        films = [capi.Film(ctx, w, h) for _ in range(3)]
        se = capi.PtSession(ctx, scene, cfg, *films)
        se.passes(1, blocking=True)
        before = [f.read() for f in films]
        for k in range(3):
            assert np.all(before[k][6 * n:] == 4)
        active = [0, 2, 4]  # of the 3 x 2 tiles
        se.set_active_tiles(active)
        se.passes(2, blocking=True)
        after = [f.read() for f in films]
        se.end()
    tile_of = (np.arange(h)[:, None] // 16) * 3 + (np.arange(w)[None, :] // 16)
    is_active = np.isin(tile_of, active).reshape(-1)
    for k in range(3):
        wgt_b, wgt_a = before[k][6 * n:], after[k][6 * n:]
        assert np.all(wgt_a[is_active] == 12) and np.all(wgt_a[~is_active] == 4)
        assert np.array_equal(wgt_a, after[0][6 * n:])
        rgb_b, rgb_a = before[k][:3 * n].reshape(n, 3), after[k][:3 * n].reshape(n, 3)
        assert np.array_equal(rgb_b[~is_active].view(np.uint32), rgb_a[~is_active].view(np.uint32))
        assert np.any(rgb_b[is_active] != rgb_a[is_active])


# ---------------------------------------------------------------------------------------------------------------- 6. refusals and fall-backs
def _three_films(ctx, w, h, fill):
    films = [capi.Film(ctx, w, h) for _ in range(3)]
    for k, f in enumerate(films):
        f.write(np.full(7 * w * h, fill + k, F))
    return films


def _untouched(films, fill, w, h):
    return all(np.array_equal(f.read(), np.full(7 * w * h, fill + k, F)) for k, f in enumerate(films))


def test_refusals(ctx, cbox_path):
    w, h = 32, 32
    cfg = make_config(spp=4, spp_per_pass=4, max_depth=4)
    cbox_sd = scene_json.load_scene(cbox_path, w, h)
    cases = []
    with capi.options(force_bvh=1, instancing=1):
        cases.append((capi.Scene(ctx, instanced_scene(n_inst=4, n=2, width=w, height=h)), dict(instancing=1), "instances"))
    flat = capi.Scene(ctx, cbox_sd)
    cases.append((flat, dict(wavefront=1), "wavefront"))
    cases.append((flat, dict(arith=1), "arith"))
    for scene, opts, word in cases:
        films = _three_films(ctx, w, h, 3.0)
        with capi.options(**opts):
            with pytest.raises(capi.AkariError) as e:
                capi.PtSession(ctx, scene, cfg, *films)
            assert e.value.code == capi.ERR_UNSUPPORTED and word in str(e.value), str(e.value)
            with pytest.raises(capi.AkariError) as e:
                capi.pt_render_features(ctx, scene, cfg, *films)
            assert e.value.code == capi.ERR_UNSUPPORTED
        assert _untouched(films, 3.0, w, h), word
    # a host-only scene ("CPU context")
    films = _three_films(ctx, w, h, 5.0)
    with pytest.raises(capi.AkariError) as e:
        capi.PtSession(ctx, capi.Scene(None, cbox_sd), cfg, *films)
    assert e.value.code == capi.ERR_UNSUPPORTED and "host-only" in str(e.value)
    # one guide alone, a guide of the wrong size, the same film twice
    small = capi.Film(ctx, w, h // 2)
    for albedo, normal in ((films[1], None), (None, films[2]), (films[1], small), (small, films[2]), (films[1], films[1]), (films[0], films[2])):
        with pytest.raises(capi.AkariError) as e:
            capi.PtSession(ctx, flat, cfg, films[0], albedo, normal)
        assert e.value.code == capi.ERR_INVALID_ARGUMENT, (albedo, normal)
    assert _untouched(films, 5.0, w, h)


def test_fall_backs(ctx):
    w, h = 40, 32
    sd = textured_room(w, h, n_floor=8)
    cfg = make_config(spp=8, spp_per_pass=4, max_depth=6, sampler_seed=4)
    with capi.options(**BVH):
        scene = capi.Scene(ctx, sd)
        ref = _run(ctx, scene, cfg)
    with capi.options(force_bvh=1, instancing=0, wavefront=0, specialise=1):
        got = _run(ctx, capi.Scene(ctx, sd), cfg)
        assert got[4]["specialised"] == 0 and got[4]["status"] != "ok" and got[4]["kernel_flags"] & FEAT_BIT, got[4]
        plain = _run(ctx, capi.Scene(ctx, sd), cfg, feat=False)
        assert plain[4]["specialised"] == 1  # (the option does take where no guides are collected)
    for k in range(4):
        assert np.array_equal(got[k], ref[k]), k
    with capi.options(force_bvh=1, instancing=0, wavefront=-1, sched_trial=1, specialise=0):
        got = _run(ctx, capi.Scene(ctx, sd), cfg)
        assert "wavefront" not in got[4]["status"] and got[4]["kernel_flags"] & FEAT_BIT
    for k in range(4):
        assert np.array_equal(got[k], ref[k]), k


# ---------------------------------------------------------------------------------------------------------------- 7. driver
METHOD = {"method": {"type": "pt", "spp": 8, "spp_per_pass": 4, "max_depth": 12, "rr_depth": 5}, "sampler": {"type": "independent", "seed": 3},
          "film": {"filter": {"type": "gaussian", "radius": 1.5}}}


def _read_exr(path):
    return capi.host_decode_exr(open(path, "rb").read())[..., :3]


def _cli(root, tmp_path, scene_file, extra, env=None):
    from akari_render_amd import build
    cli = build.build_cli()
    method = copy.deepcopy(METHOD)
    method["film"]["out"] = str(tmp_path / "out" / "img.exr")
    (tmp_path / "m.json").write_text(json.dumps(method))
    res = subprocess.run([cli, "-s", scene_file, "-m", str(tmp_path / "m.json"), "--resolution", "32x32", "-v"] + extra, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, text=True, cwd=tmp_path, env=dict(os.environ, **(env or {})))
    assert res.returncode == 0, res.stdout[-2000:]
    return res.stdout


def test_cli_denoise_features(ctx, root, cbox_path, tmp_path):
    w = h = 32
    scene = capi.Scene(ctx, cbox_path, w, h)
    cfg = make_config(spp=8, spp_per_pass=4, max_depth=12, sampler_seed=3)
    color, albedo, normal = (capi.Film(ctx, w, h) for _ in range(3))
    capi.pt_render_features(ctx, scene, cfg, color, albedo, normal)
    noisy = color.resolve()
    # the half film of --denoise-variance: the colour film after the first of the two passes
    half, c2, a2, n2 = (capi.Film(ctx, w, h) for _ in range(4))
    se = capi.PtSession(ctx, scene, cfg, c2, a2, n2)
    se.passes(1, blocking=True)
    half.write(c2.read())
    se.passes(1, blocking=True)
    se.end()
    capi.denoise_variance(ctx, c2, half, a2, n2, c2)
    with_variance = c2.resolve()
    capi.denoise(ctx, color, albedo, normal, color)
    manual = color.resolve()
    for extra, want in ((["--denoise-features"], manual), (["--denoise-features", "--denoise", "4"], manual), (["--denoise-features", "--denoise-variance"], with_variance)):
        out = _cli(root, tmp_path, cbox_path, extra)
        assert "guides collected by the task's own" in out, out[-1500:]
        written = _read_exr(tmp_path / "out" / "img.denoised.exr")
        assert np.array_equal(written.view(np.uint32), want.view(np.uint32)), extra
        assert np.array_equal(_read_exr(tmp_path / "out" / "img.exr").view(np.uint32), noisy.view(np.uint32)), extra
        os.remove(tmp_path / "out" / "img.denoised.exr")
    # a session that refuses guides (the relaxed tier): the run succeeds through the aov route, at 16 spp or --denoise's
    for extra, spp in ((["--denoise-features"], 16), (["--denoise-features", "--denoise", "4"], 4)):
        out = _cli(root, tmp_path, cbox_path, extra, env={"AKR_ARITH": "1"})
        assert f"aov passes of {spp} spp" in out and f"feature passes of {spp} spp" in out, out[-1500:]
        assert os.path.getsize(tmp_path / "out" / "img.denoised.exr") > w * h * 12
        os.remove(tmp_path / "out" / "img.denoised.exr")
