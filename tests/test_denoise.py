"""akr_denoise without a GPU: the host build of csrc/device/ddenoise.h (akr_host_denoise) against the numpy restatement of
the definition bit for bit, properties that restate nothing, the quality bar on oracle films, the configuration and its refusals."""
import ctypes as C

import numpy as np
import pytest

from akari_render_amd import abi, capi
from oracle import pyoracle
from tests import denoise_model as dm
from tests.probe_matrix import same_bits_or_both_nan

f32 = np.float32
CASES = dm.cases()


def host(w, h, color, albedo, normal, cfg, scales=(1.0, 1.0, 1.0)):
    return capi.host_denoise(w, h, color, albedo, normal, cfg, scales)


@pytest.mark.parametrize("shape", dm.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_host_equals_the_restatement(hip_lib, oracle_lib, case, shape):
    name, kind, use_a, use_n, cfg, scales = case
    w, h = shape
    color, albedo, normal = dm.case_inputs(w, h, kind)
    got = host(w, h, color, albedo if use_a else None, normal if use_n else None, cfg, scales)
    ref = dm.case_reference(w, h, name)
    same = same_bits_or_both_nan(got, ref)
    assert same.all(), f"{name} {w}x{h}: {np.count_nonzero(~same)} of {same.size} floats differ"
    assert np.isfinite(ref).all()  # (no case above feeds a non-finite value: the NaN route has a test of its own)


@pytest.mark.parametrize("name", dm.LARGE_CASES)
def test_host_equals_the_restatement_on_the_large_frame(hip_lib, oracle_lib, name):
    """dm.LARGE_SHAPE, all guides, demodulation, five iterations: the reference tests/test_gpu_frame_thresholds.py holds the device to, held to
    the host build first."""
    _, kind, use_a, use_n, cfg, scales = next(c for c in CASES if c[0] == name)
    assert use_a and use_n and cfg.demodulate == 1 and cfg.iterations == 5
    w, h = dm.LARGE_SHAPE
    color, albedo, normal = dm.case_inputs(w, h, kind)
    got = host(w, h, color, albedo, normal, cfg, scales)
    ref = dm.case_reference(w, h, name)
    same = same_bits_or_both_nan(got, ref)
    assert same.all(), f"{name} {w}x{h}: {np.count_nonzero(~same)} of {same.size} floats differ"
    assert np.isfinite(ref).all()


@pytest.mark.parametrize("demodulate", [0, 1])
@pytest.mark.parametrize("shape", [(5, 5), (33, 17), (70, 45)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_constant_image_stays_itself(hip_lib, shape, demodulate):
    """Every tap carries the centre's value, so y = (sum w x) / (sum w) is x up to rounding: within 4 ulp per level of itself, with and
    without demodulation (whose division and product have to fit into the same bound)."""
    w, h = shape
    for value in (f32(0.37), f32(1.0), f32(513.25), f32(3e-6)):
        rgb = np.ones((h, w, 3), dtype=f32) * np.array([value, value * f32(0.5), value * f32(3.0)], dtype=f32)
        guide = np.ones((h, w, 3), dtype=f32) * np.array([0.3, 0.6, 0.9], dtype=f32)
        for iterations in (1, 5):
            out = host(w, h, dm.film_of(rgb), dm.film_of(guide), dm.film_of(guide), dm.config(iterations=iterations, demodulate=demodulate))
            ulps = np.abs(out.view(np.int32).astype(np.int64) - rgb.view(np.int32).astype(np.int64)).max()
            print(f"{w}x{h} value {value} iterations {iterations} demodulate {demodulate}: {ulps} ulp")
            assert ulps <= 4 * iterations


def test_an_edge_in_the_normals_separates_the_two_sides(hip_lib):
    """Normals (0, 0, 1) | (1, 0, 0) under sigma_normal = 1/8: e >= 2 * 64 = 128 for every tap across, beyond exp_f's lower cut-off (103.28),
    so such a tap weighs exactly 0 and a side's output is a function of its own side alone."""
    w, h = 37, 21
    rng = np.random.default_rng(5)
    left = np.arange(w) < 17
    color = rng.random((h, w, 3)).astype(f32)
    normal = np.where(left[None, :, None], np.array([0, 0, 1], dtype=f32), np.array([1, 0, 0], dtype=f32)) * np.ones((h, w, 3), dtype=f32)
    albedo = np.full((h, w, 3), 0.5, dtype=f32)
    cfg = dm.config(sigma_normal=0.125)
    base = host(w, h, dm.film_of(color), dm.film_of(albedo), dm.film_of(normal), cfg)
    other = color.copy()
    other[:, ~left] = (rng.random((h, w - 17, 3)) * 50).astype(f32)
    out = host(w, h, dm.film_of(other), dm.film_of(albedo), dm.film_of(normal), cfg)
    assert np.array_equal(out[:, left].view(np.uint32), base[:, left].view(np.uint32))
    assert not np.array_equal(out[:, ~left].view(np.uint32), base[:, ~left].view(np.uint32))
    other = color.copy()
    other[:, left] = f32(9.0)
    out = host(w, h, dm.film_of(other), dm.film_of(albedo), dm.film_of(normal), cfg)
    assert np.array_equal(out[:, ~left].view(np.uint32), base[:, ~left].view(np.uint32))


def test_one_nan_pixel_stays_one_nan_pixel(hip_lib):
    dm.check_nan_pixel(lambda c, a, n: host(41, 23, c, a, n, dm.config()))


def test_no_iterations_and_no_demodulation_is_the_resolve(hip_lib, oracle_lib):
    w, h = 33, 17
    color, albedo, normal = dm.random_films(w, h, seed=1, weights=True, splat=True)
    out = host(w, h, color, albedo, normal, dm.config(iterations=0, demodulate=0), (0.375, 1.0, 1.0))
    assert np.array_equal(out.view(np.uint32), pyoracle.resolve(color, w, h, 0.375).view(np.uint32))


def test_an_albedo_below_the_floor_makes_no_inf(hip_lib):
    w, h = 16, 9
    rng = np.random.default_rng(2)
    color = (rng.random((h, w, 3)) * 1e3).astype(f32)
    albedo = rng.choice(np.array([0.0, 1e-30, 1e-42, 9.99e-4, -0.5, 0.5], dtype=f32), size=(h, w, 3)).astype(f32)
    for iterations in (0, 1, 5):
        out = host(w, h, dm.film_of(color), dm.film_of(albedo), None, dm.config(iterations=iterations))
        assert np.isfinite(out).all() and out.max() <= 1.001e3


def test_denoising_the_oracle_film_reduces_its_error(hip_lib, root):
    """The bar is the factor 1: relMSE against the oracle's 2048-spp image of the denoised 16-spp film is lower than that of the film."""
    noisy, albedo, ns, ref = dm.golden_cbox(root)
    out = host(64, 64, noisy, albedo, ns, abi.DenoiseConfig.default())
    before, after = dm.rel_mse(dm.resolve_np(noisy, 64, 64), ref), dm.rel_mse(out, ref)
    print(f"relMSE noisy {before:.5f} denoised {after:.5f} ratio {after / before:.3f}")
    assert after < before


def test_config_default_size_and_refusals(hip_lib):
    c = abi.DenoiseConfig()
    assert hip_lib.akr_denoise_config_default(C.byref(c)) == 0
    assert bytes(c) == bytes(abi.DenoiseConfig.default())
    assert (c.iterations, c.demodulate) == (5, 1) and c.albedo_floor == f32(1e-3)
    assert C.sizeof(abi.DenoiseConfig) == 32 and hip_lib.akr_struct_size(17) == 32 and hip_lib.akr_struct_size(18) == 0
    assert hip_lib.akr_denoise_config_default(None) == capi.ERR_INVALID_ARGUMENT
    color, albedo, normal = dm.random_films(5, 5)
    for bad in (dict(iterations=9), dict(sigma_color=-1.0), dict(sigma_normal=float("nan")), dict(sigma_albedo=float("inf")), dict(sigma_color=-0.5),
                dict(sigma_normal=1e-30), dict(sigma_albedo=1e-20), dict(sigma_color=1e-19), dict(sigma_color=1e-18, iterations=8),
                dict(albedo_floor=0.0), dict(albedo_floor=-1e-3), dict(albedo_floor=float("nan"))):
        with pytest.raises(capi.AkariError) as e:
            host(5, 5, color, albedo, normal, dm.config(**bad))
        assert e.value.code == capi.ERR_INVALID_ARGUMENT and "akr_denoise" in str(e.value), bad
    host(5, 5, color, albedo, normal, dm.config(iterations=8, sigma_color=0.0, sigma_normal=0.0, sigma_albedo=0.0))  # the edges of the range pass
    assert np.isfinite(host(5, 5, color, albedo, normal, dm.config(iterations=1, sigma_color=1e-18, sigma_normal=1e-18, sigma_albedo=1e-18))).all()
    assert hip_lib.akr_denoise(None, C.byref(c), None, None, None, None) == capi.ERR_INVALID_ARGUMENT


def test_the_options(hip_lib):
    assert capi.get_option("denoise") == 0 and capi.get_option("denoise_kernel") == -1
    with capi.options(denoise=16, denoise_kernel=1):
        assert capi.get_option("denoise") == 16 and capi.get_option("denoise_kernel") == 1
    for name, value in (("denoise", -1), ("denoise", 65537), ("denoise_kernel", 2), ("denoise_kernel", -2)):
        with pytest.raises(capi.AkariError):
            capi.set_option(name, value)
    assert capi.get_option("denoise") == 0 and capi.get_option("denoise_kernel") == -1
