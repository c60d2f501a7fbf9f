"""Adaptive sampling on the GPU: akr_film_tile_error against the host build of the same text and the numpy restatement;
akr_pt_set_active_tiles against the CPU oracle's films and sampler states, per sampler, kernel and schedule; akr_pt_adaptive_render against
the restatement run on the oracle's prefix films -- all bit for bit; the `adaptive` option through akr_render_task."""
import functools
import json

import numpy as np
import pytest

from akari_render_amd import abi, capi
from oracle import scene_json
from tests import adaptive_model as am
from tests.helpers import make_config

pytestmark = pytest.mark.gpu
f32 = np.float32


def film_with(ctx, w, h, data):
    f = capi.Film(ctx, w, h)
    f.write(data)
    return f


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=f32).view(np.uint32), np.asarray(b, dtype=f32).view(np.uint32))


# ---------------------------------------------------------------------------------------------- the error estimate
@pytest.mark.parametrize("shape", am.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}-tiles{s[2]}x{s[3]}")
def test_device_tile_error_equals_host_equals_restatement(ctx, shape):
    w, h, tw, th = shape
    film, half = am.random_films(w, h, tw, th)
    tiles = am.all_tiles(w, h, tw, th)
    got = capi.film_tile_error(ctx, film_with(ctx, w, h, film), film_with(ctx, w, h, half), tw, th, tiles)
    ref = am.reference_errors(w, h, tw, th)
    assert same_bits(got, ref), f"{np.count_nonzero(got.view(np.uint32) != ref.view(np.uint32))} of {ref.size} tile errors differ from the restatement: {got} {ref}"
    assert same_bits(got, capi.host_tile_error(w, h, film, half, tw, th, tiles))
    assert np.isinf(got[tiles.tolist().index(1)])


def test_tile_error_refusals(ctx):
    a, b, c = capi.Film(ctx, 24, 16), capi.Film(ctx, 24, 16), capi.Film(ctx, 16, 24)
    for args, what in (((a, a, 8, 8, [0]), "itself"), ((a, c, 8, 8, [0]), "size"), ((a, b, 12, 8, [0]), "multiples of 8"), ((a, b, 128, 64, [0]), "4096"),
                       ((a, b, 8, 8, [6]), "out of range")):
        with pytest.raises(capi.AkariError) as e:
            capi.film_tile_error(ctx, *args)
        assert e.value.code == capi.ERR_INVALID_ARGUMENT and what in str(e.value)
    other = capi.Context(0)
    foreign = capi.Film(other, 24, 16)
    with pytest.raises(capi.AkariError) as e:
        capi.film_tile_error(ctx, a, foreign, 8, 8, [0])
    assert e.value.code == capi.ERR_INVALID_ARGUMENT and "context" in str(e.value)
    foreign.close()
    other.close()


# ---------------------------------------------------------------------------------------------- active tiles
W = H = 64
SUBSET = [9, 2, 15, 4, 7]  # of the 4 x 4 tiles of 16 x 16 pixels: arbitrary, unsorted


@functools.lru_cache(maxsize=None)
def oracle_steps(root, sampler, bvh):
    """The oracle's films and sampler states of cbox 64 x 64 after 2, 4, 6 and 8 samples of an 8-spp render at spp_per_pass 2."""
    return am.oracle_prefix_films(root, W, H, 8, 2, 1, seed=3, sampler=sampler, chunk=2, want_states=True, bvh=bvh)


def mixed(root, sampler, bvh, spp_on, spp_off):
    """(film rgb + weight planes, states): the oracle's spp_on-sample result on SUBSET's pixels and its spp_off-sample result elsewhere."""
    films, states = oracle_steps(root, sampler, bvh)
    m = am.tile_mask(W, H, 16, 16, SUBSET).reshape(-1)
    n = W * H
    on, off = films[spp_on // 2 - 1], films[spp_off // 2 - 1]
    rgb = np.where(np.repeat(m, 3), on[:3 * n], off[:3 * n])
    wt = np.where(m, on[6 * n:], off[6 * n:])
    st = np.where(np.repeat(m, 2), states[spp_on // 2 - 1], states[spp_off // 2 - 1])
    return rgb, wt, st


def begin(ctx, cbox_path, sampler, bvh, wavefront=0):
    sd = scene_json.load_scene(cbox_path, W, H)
    with capi.options(force_bvh=1 if bvh else 0, wavefront=wavefront):
        scene = capi.Scene(ctx, sd)
        film = capi.Film(ctx, W, H)
        cfg = make_config(spp=8, spp_per_pass=2, sampler_type=sampler, sampler_seed=3, tile_w=16, tile_h=16)
        se = capi.PtSession(ctx, scene, cfg, film)
    info = se.kernel_info()
    assert bool(info["kernel_flags"] & 1) == bvh and ("wavefront" in info["status"]) == bool(wavefront)
    return scene, film, se


def check_film(film, se, expect):
    rgb, wt, st = expect
    n = W * H
    got = film.read()
    assert np.array_equal(got[:3 * n].view(np.uint32), rgb.view(np.uint32)), f"{np.count_nonzero(got[:3 * n].view(np.uint32) != rgb.view(np.uint32))} rgb floats differ"
    assert np.array_equal(got[6 * n:], wt)
    assert np.array_equal(se.sampler_states(n), st)


@pytest.mark.parametrize("schedule", ["exhaustive", "bvh", "wavefront"])
@pytest.mark.parametrize("sampler", [abi.SAMPLER_INDEPENDENT, abi.SAMPLER_PMJ02BN, abi.SAMPLER_SOBOL], ids=["independent", "pmj02bn", "sobol"])
def test_a_subset_of_tiles_goes_on_where_every_pixel_stood(ctx, root, cbox_path, oracle_lib, sampler, schedule):
    bvh = schedule != "exhaustive"
    scene, film, se = begin(ctx, cbox_path, sampler, bvh, 1 if schedule == "wavefront" else 0)
    assert se.passes(2, blocking=True) == 4
    se.set_active_tiles(SUBSET)
    assert se.passes(2, blocking=True) == 8
    check_film(film, se, mixed(root, sampler, bvh, 8, 4))
    st = se.end()
    assert st["n_samples"] == 4 * W * H + 4 * len(SUBSET) * 256


@pytest.mark.parametrize("schedule", ["exhaustive", "wavefront"])
def test_widening_back_and_an_empty_list(ctx, root, cbox_path, oracle_lib, schedule):
    bvh = schedule == "wavefront"
    scene, film, se = begin(ctx, cbox_path, abi.SAMPLER_INDEPENDENT, bvh, 1 if bvh else 0)
    assert se.passes(1, blocking=True) == 2
    se.set_active_tiles([])  # nothing runs, the pass is counted
    assert se.passes(1, blocking=True) == 4
    se.set_active_tiles(None)
    assert se.passes(1, blocking=True) == 6
    se.set_active_tiles(SUBSET)
    se.set_active_tiles(None)
    se.set_active_tiles(SUBSET)
    assert se.passes(1, blocking=True) == 8
    check_film(film, se, mixed(root, abi.SAMPLER_INDEPENDENT, bvh, 6, 4))  # every pixel sat out one pass, the others two
    assert se.end()["n_samples"] == 4 * W * H + 2 * len(SUBSET) * 256


def test_active_tile_refusals(ctx, cbox_path):
    scene, film, se = begin(ctx, cbox_path, abi.SAMPLER_INDEPENDENT, False)
    for tiles, what in (([3, 5, 3], "duplicate"), ([16], "out of range"), ([0, 0xFFFFFFFF], "out of range")):
        with pytest.raises(capi.AkariError) as e:
            se.set_active_tiles(tiles)
        assert e.value.code == capi.ERR_INVALID_ARGUMENT and what in str(e.value)
    se.end()
    cfg = make_config(spp=8, spp_per_pass=2, sampler_seed=3, tile_w=16, tile_h=16, shard_rank=1, shard_count=2)
    shard = capi.PtSession(ctx, scene, cfg, film)
    from akari_render_amd import distributed
    owned = distributed.owned_pixel_mask(W, H, 1, 2, 16, 16)[::16, ::16].reshape(-1)
    mine, not_mine = int(np.nonzero(owned)[0][0]), int(np.nonzero(~owned)[0][0])
    shard.set_active_tiles([mine])
    with pytest.raises(capi.AkariError) as e:
        shard.set_active_tiles([mine, not_mine])
    assert e.value.code == capi.ERR_INVALID_ARGUMENT and "not owned" in str(e.value)
    shard.end()


# ---------------------------------------------------------------------------------------------- the adaptive render
def adaptive_both(ctx, root, cbox_path, threshold, min_spp=8):
    c = am.CBOX
    scene = capi.Scene(ctx, scene_json.load_scene(cbox_path, c["w"], c["h"]))
    film, half = capi.Film(ctx, c["w"], c["h"]), film_with(ctx, c["w"], c["h"], np.full(7 * c["w"] * c["h"], 3.5, dtype=f32))  # (whatever the half held is cleared)
    cfg = make_config(spp=c["spp"], spp_per_pass=c["spp_per_pass"], sampler_seed=c["seed"], tile_w=c["tw"], tile_h=c["th"])
    acfg = abi.AdaptiveConfig.default()
    acfg.threshold, acfg.min_spp, acfg.round_passes = threshold, min_spp, c["round_passes"]
    stats, tile_spp = capi.pt_adaptive_render(ctx, scene, cfg, film, acfg, half)
    model = am.adaptive(am.cbox_prefix(root), c["w"], c["h"], c["tw"], c["th"], c["spp"], c["spp_per_pass"], c["round_passes"], threshold, min_spp)
    return scene, film, half, stats, tile_spp, model


def check_adaptive(film, half, stats, tile_spp, model):
    m_film, m_half, m_spp, m_drawn, m_rounds, _ = model
    n = am.CBOX["w"] * am.CBOX["h"]
    assert np.array_equal(tile_spp, m_spp)
    got, got_half = film.read(), half.read()
    for name, g, m in (("film", got, m_film), ("half", got_half, m_half)):
        assert np.array_equal(g[:3 * n].view(np.uint32), m[:3 * n].view(np.uint32)), f"{name}: {np.count_nonzero(g[:3 * n].view(np.uint32) != m[:3 * n].view(np.uint32))} rgb floats differ"
        assert np.array_equal(g[6 * n:].view(np.uint32), m[6 * n:].view(np.uint32)) and not g[3 * n:6 * n].any()
    assert stats["samples_drawn"] == m_drawn == stats["pt"]["n_samples"] and stats["rounds"] == m_rounds
    assert stats["samples_uniform"] == n * am.CBOX["spp"] and stats["tiles_retired"] == int(np.count_nonzero(m_spp < am.CBOX["spp"]))


def test_adaptive_render_equals_the_restatement_on_oracle_prefix_films(ctx, root, cbox_path, oracle_lib):
    scene, film, half, stats, tile_spp, model = adaptive_both(ctx, root, cbox_path, 0.125)
    assert 1 < len(set(tile_spp.reshape(-1).tolist()))  # some tiles retired, at different times, others ran to spp
    check_adaptive(film, half, stats, tile_spp, model)
    # the half is what akr_denoise_variance takes
    out = capi.Film(ctx, 64, 64)
    capi.denoise_variance(ctx, film, half, None, None, out)
    assert np.isfinite(out.resolve()).all()


def test_adaptive_render_threshold_extremes(ctx, root, cbox_path, oracle_lib):
    scene, film, half, stats, tile_spp, model = adaptive_both(ctx, root, cbox_path, float("inf"), 16)
    check_adaptive(film, half, stats, tile_spp, model)
    assert np.all(tile_spp == 16) and stats["samples_drawn"] == 16 * 4096 and stats["tiles_retired"] == 64
    scene, film, half, stats, tile_spp, model = adaptive_both(ctx, root, cbox_path, 0.0)
    check_adaptive(film, half, stats, tile_spp, model)
    assert np.all(tile_spp == 32) and stats["tiles_retired"] == 0
    uniform = capi.Film(ctx, 64, 64)
    capi.pt_render(ctx, scene, make_config(spp=32, spp_per_pass=2, sampler_seed=3, tile_w=8, tile_h=8), uniform)
    assert np.array_equal(film.read().view(np.uint32), uniform.read().view(np.uint32))


def test_adaptive_render_refusals(ctx, cbox_path):
    scene = capi.Scene(ctx, scene_json.load_scene(cbox_path, 64, 64))
    film = capi.Film(ctx, 64, 64)
    acfg = abi.AdaptiveConfig.default()
    for cfg, a, what in ((make_config(spp=4, spp_per_pass=4), dict(), "two rounds"), (make_config(spp=16, spp_per_pass=4, tile_w=128, tile_h=64), dict(), "4096"),
                         (make_config(spp=16, spp_per_pass=4), dict(round_passes=0), "round_passes"), (make_config(spp=16, spp_per_pass=4), dict(threshold=float("nan")), "threshold"),
                         (make_config(spp=16, spp_per_pass=4, sampler_type=abi.SAMPLER_SOBOL, sample_begin=4, sample_count=8), dict(), "sample range")):
        ac = abi.AdaptiveConfig.default()
        for k, v in a.items():
            setattr(ac, k, v)
        with pytest.raises(capi.AkariError) as e:
            capi.pt_adaptive_render(ctx, scene, cfg, film, ac)
        assert e.value.code == capi.ERR_INVALID_ARGUMENT and what in str(e.value)
    with pytest.raises(capi.AkariError) as e:
        capi.pt_adaptive_render(ctx, scene, make_config(spp=16, spp_per_pass=4), film, acfg, film)
    assert e.value.code == capi.ERR_INVALID_ARGUMENT and "itself" in str(e.value)


# ---------------------------------------------------------------------------------------------- the driver
def method(out):
    return json.dumps({"method": {"type": "pt", "spp": 32, "spp_per_pass": 4, "max_depth": 12, "rr_depth": 5}, "sampler": {"type": "independent", "seed": 3},
                       "film": {"filter": {"type": "gaussian", "radius": 1.5}, "out": str(out)}})


def test_render_task_with_and_without_the_adaptive_option(ctx, cbox_path, tmp_path):
    scene = capi.Scene(ctx, cbox_path, 64, 64)
    capi.render_task(ctx, scene, method(tmp_path / "plain.exr"))
    with capi.options(adaptive=0, adaptive_min_spp=8):
        capi.render_task(ctx, scene, method(tmp_path / "off.exr"))
    assert open(tmp_path / "plain.exr", "rb").read() == open(tmp_path / "off.exr", "rb").read()
    with capi.options(adaptive=256, adaptive_min_spp=8):
        st = capi.render_task(ctx, scene, method(tmp_path / "on.exr"))
        with pytest.raises(capi.AkariError) as e:
            capi.render_task(ctx, scene, method(tmp_path / "no.exr"), save_intermediate=True, name=str(tmp_path / "x"))
        assert e.value.code == capi.ERR_UNSUPPORTED
    # the manual composition: the default configuration with the option's threshold and min_spp
    film = capi.Film(ctx, 64, 64)
    acfg = abi.AdaptiveConfig.default()
    acfg.threshold, acfg.min_spp = 256 / 1024.0, 8
    stats, _ = capi.pt_adaptive_render(ctx, scene, make_config(spp=32, spp_per_pass=4, sampler_seed=3), film, acfg)
    capi.image_write(tmp_path / "manual.exr", film.resolve())
    assert open(tmp_path / "on.exr", "rb").read() == open(tmp_path / "manual.exr", "rb").read()
    assert st["n_samples"] == stats["samples_drawn"] < stats["samples_uniform"]
    assert open(tmp_path / "on.exr", "rb").read() != open(tmp_path / "plain.exr", "rb").read()
