"""The timed test hooks (akr_probe_denoise_times, akr_probe_denoise_variance_times, akr_probe_display_times, akr_probe_adapt_times): the stage
times are finite, not negative and laid out as documented, and a timed call writes the film the untimed call writes, bit for bit. No
thresholds: what a stage costs is tools/*_bench.py's business."""
import ctypes as C

import numpy as np
import pytest

from akari_render_amd import abi, capi
from tests import adaptive_model as am
from tests import denoise_variance_model as dvm
from tests import display_model as dpm

pytestmark = pytest.mark.gpu
f32 = np.float32
W, H = 33, 17
KERNELS = [0, 1]
ITERATIONS = 3  # fewer than the 8 level slots of times11: the unused ones have to read 0


def film_with(ctx, w, h, data, splat_scale=1.0):
    f = capi.Film(ctx, w, h)
    f.write(data)
    f.splat_scale = splat_scale
    return f


def check_times(values, total):
    values = np.asarray(values, dtype=np.float64)
    assert np.all(np.isfinite(values)) and np.all(values >= 0), values
    assert np.all(total >= values), (total, values)


def denoise_films(ctx):
    color, half, albedo, normal = dvm.case_inputs(W, H, "random", "equal")
    return [film_with(ctx, W, H, f) for f in (color, half, albedo, normal)]


@pytest.mark.parametrize("kernel", KERNELS, ids=["gather", "tiled"])
@pytest.mark.parametrize("variance", [False, True], ids=["plain", "variance"])
def test_denoise_times(ctx, variance, kernel):
    cfg = dvm.config(iterations=ITERATIONS)
    color, half, albedo, normal = denoise_films(ctx)
    guides = (color, half, albedo, normal) if variance else (color, albedo, normal)
    timed, untimed = capi.Film(ctx, W, H), capi.Film(ctx, W, H)
    t = (capi.denoise_variance_times if variance else capi.denoise_times)(ctx, *guides, timed, kernel, cfg)
    assert len(t["levels"]) == ITERATIONS
    check_times([t["prepare"], *t["levels"], t["finish"], t["total"]], t["total"])
    with capi.options(denoise_kernel=kernel):
        (capi.denoise_variance if variance else capi.denoise)(ctx, *guides, untimed, cfg)
    assert np.array_equal(timed.read().view(np.uint32), untimed.read().view(np.uint32))
    # the layout of times11: prepare, levels [8], finish, total; the slots of levels that did not run are exactly 0
    raw = np.full(11, np.nan, dtype=f32)
    hook = capi.lib().akr_probe_denoise_variance_times if variance else capi.lib().akr_probe_denoise_times
    capi.check(hook(ctx.h, C.byref(cfg), *(f.h for f in guides), timed.h, kernel, capi._fp(raw)))
    check_times(raw, raw[10])
    assert np.all(raw[1 + ITERATIONS:9].view(np.uint32) == 0)
    assert np.array_equal(timed.read().view(np.uint32), untimed.read().view(np.uint32))


@pytest.mark.parametrize("kernel", KERNELS, ids=["gather", "lds"])
def test_display_times(ctx, kernel):
    cfg = dpm.config(curve=abi.DISPLAY_ACES, auto_exposure=1, bloom_strength=0.5, bloom_levels=5)
    film = film_with(ctx, W, H, dpm.case_film(W, H, "random"), dpm.SPLAT_SCALE["random"])
    timed, untimed = capi.Film(ctx, W, H), capi.Film(ctx, W, H)
    t = capi.display_times(ctx, film, timed, kernel, cfg)
    assert len(t) == 8
    check_times(list(t.values()), t["total"])
    with capi.options(display_kernel=kernel):
        capi.display_transform(ctx, film, untimed, cfg)
    assert np.array_equal(timed.read().view(np.uint32), untimed.read().view(np.uint32))


def test_adapt_times(ctx):
    w, h, tw, th = am.SHAPES[0]
    film, half = am.random_films(w, h, tw, th)
    t = capi.adapt_times(ctx, film_with(ctx, w, h, film), film_with(ctx, w, h, half), tw, th, am.all_tiles(w, h, tw, th))
    assert len(t) == 3
    values = np.asarray(list(t.values()), dtype=np.float64)
    assert np.all(np.isfinite(values)) and np.all(values >= 0), values
