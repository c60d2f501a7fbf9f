"""akr_denoise_variance without a GPU (DESIGN.md 4.10 "Variance guide"): the host build of csrc/device/ddenoise.h (akr_host_denoise_variance)
against the numpy restatement of the definition bit for bit, the two properties the mode exists for (a converged film is left alone; noise
decides how hard a pixel is filtered, not contrast), the quality bar on oracle films, the configuration and its refusals."""
import ctypes as C
import functools

import numpy as np
import pytest

from akari_render_amd import abi, capi
from oracle import pyoracle
from tests import denoise_model as dm
from tests import denoise_variance_model as dvm
from tests.probe_matrix import same_bits_or_both_nan

f32 = np.float32
CASES = dvm.cases()


def host(w, h, color, half, albedo, normal, cfg, scales=(1.0, 1.0, 1.0)):
    return capi.host_denoise_variance(w, h, color, half, albedo, normal, cfg, scales)


@pytest.mark.parametrize("shape", dvm.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_host_equals_the_restatement(hip_lib, oracle_lib, case, shape):
    name, kind, halves, use_a, use_n, cfg = case
    w, h = shape
    color, half, albedo, normal = dvm.case_inputs(w, h, kind, halves)
    got = host(w, h, color, half, albedo if use_a else None, normal if use_n else None, cfg)
    ref = dvm.case_reference(w, h, name)
    same = same_bits_or_both_nan(got, ref)
    assert same.all(), f"{name} {w}x{h}: {np.count_nonzero(~same)} of {same.size} floats differ"
    assert np.isfinite(ref).all()  # (no case feeds a non-finite colour: the NaN route has a test of its own)


@pytest.mark.parametrize("name", dvm.LARGE_CASES)
def test_host_equals_the_restatement_on_the_large_frame(hip_lib, oracle_lib, name):
    """dvm.LARGE_SHAPE, all guides, demodulation, five iterations: the reference tests/test_gpu_frame_thresholds.py holds the device to, held
    to the host build first."""
    _, kind, halves, use_a, use_n, cfg = next(c for c in CASES if c[0] == name)
    assert use_a and use_n and cfg.demodulate == 1 and cfg.iterations == 5
    w, h = dvm.LARGE_SHAPE
    color, half, albedo, normal = dvm.case_inputs(w, h, kind, halves)
    got = host(w, h, color, half, albedo, normal, cfg)
    ref = dvm.case_reference(w, h, name)
    same = same_bits_or_both_nan(got, ref)
    assert same.all(), f"{name} {w}x{h}: {np.count_nonzero(~same)} of {same.size} floats differ"
    assert np.isfinite(ref).all()


def test_the_unequal_halves_case_has_pixels_without_an_estimate():
    """(what the case is for: wA = 0 at some pixels, wA != wB at the others)"""
    color, half, _, _ = dvm.case_inputs(33, 17, "intweights", "unequal")
    n = 33 * 17
    wa, wc = half[6 * n:], color[6 * n:]
    assert (wa == 0).any() and ((wa > 0) & (wc - wa != wa)).any()


@pytest.mark.parametrize("shape", [(33, 17), (70, 45)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_converged_film_is_not_blurred(hip_lib, shape):
    """H.rgb = C.rgb / 2, H.w = C.w / 2 (exact): the halves agree, r = 0 everywhere, so kcp = kv / 1e-10 = 1.5625e8 under the default
    sigma_variance of 8. Colours that differ by >= 1e-3 in a channel (here: >= 2e-3 in red) give every foreign tap e >= 1e-6 * 1.5625e8 = 156, beyond exp_f's cut-off
    (103.28): it weighs exactly 0, and y = (w x) / w is x up to the rounding of one product and one quotient -- within 1 ulp per level of
    resolve(C). akr_host_denoise, whose sigma_color cannot know that the film has converged, moves the same pixels by more than 1 %."""
    w, h = shape
    rng = np.random.default_rng(11 * w + h)
    # a random permutation of the multiples of 2e-3 in [0.25, 0.25 + 2e-3 N): any two pixels are >= 2e-3 apart in the red channel
    red = (f32(0.25) + f32(2e-3) * rng.permutation(w * h).astype(f32)).reshape(h, w)
    rgb = np.stack([red, rng.random((h, w)).astype(f32), rng.random((h, w)).astype(f32)], axis=-1).astype(f32)
    color = dm.film_of(rgb, np.full(w * h, 16, dtype=f32))
    half = (color * f32(0.5)).astype(f32)
    guide = dm.film_of(np.ones((h, w, 3), dtype=f32) * np.array([0.0, 0.0, 1.0], dtype=f32))
    resolved = dm.resolve_np(color, w, h)
    for iterations in (1, 5):
        out = host(w, h, color, half, None, guide, dvm.config(iterations=iterations))
        ulps = np.abs(out.view(np.int32).astype(np.int64) - resolved.view(np.int32).astype(np.int64)).max()
        print(f"{w}x{h} iterations {iterations}: {ulps} ulp")
        assert ulps <= iterations
    fixed = capi.host_denoise(w, h, color, None, guide, dm.config())
    moved = np.abs(fixed - resolved) / resolved
    print(f"{w}x{h} akr_host_denoise: median relative change {np.median(moved):.3f}")
    assert np.median(moved) > 0.01


# -------------------------------------------------------------------------------------------- noise decides, not contrast
PROPERTY_W, PROPERTY_H = 64, 64


def noise_property_films(seed=20):
    """The true image: rows 0 .. 31 a step 0.50 | 0.55 down the middle, rows 32 .. 63 a flat 0.5 -- grey, albedo 0.5 and normal (0, 0, 1)
    everywhere. Each half is the true image plus Gaussian noise per pixel and channel: sigma 0.005 in the upper region, 0.2 in the lower.
    -> (C, H, albedo, normal, true image)."""
    w, h = PROPERTY_W, PROPERTY_H
    rng = np.random.default_rng(seed)
    true = np.full((h, w, 3), 0.5)
    true[:h // 2, w // 2:] = 0.55
    sigma = np.where(np.arange(h) < h // 2, 0.005, 0.2)[:, None, None]
    a_half = (true + sigma * rng.normal(size=(h, w, 3))).astype(f32)
    b_half = (true + sigma * rng.normal(size=(h, w, 3))).astype(f32)
    half, rest = dm.film_of(a_half), dm.film_of(b_half)
    n = w * h
    color = np.concatenate([(half[:3 * n] + rest[:3 * n]).astype(f32), half[3 * n:6 * n], (half[6 * n:] + rest[6 * n:]).astype(f32)])
    albedo = dm.film_of(np.full((h, w, 3), 0.5, dtype=f32))
    normal = dm.film_of(np.ones((h, w, 3), dtype=f32) * np.array([0.0, 0.0, 1.0], dtype=f32))
    return color, half, albedo, normal, true.astype(f32)


def noise_property_numbers(out, color, true):
    """(the step's contrast after filtering as a fraction of 0.05, the lower region's RMS error after filtering over that of the input) -- both
    over the 16 rows of a region that lie farthest from the other one."""
    w, h = PROPERTY_W, PROPERTY_H
    top, bottom = slice(0, h // 4), slice(3 * h // 4, h)
    contrast = (float(np.mean(out[top, w // 2:], dtype=np.float64)) - float(np.mean(out[top, :w // 2], dtype=np.float64))) / 0.05
    noisy = dm.resolve_np(color, w, h)
    rms = lambda img: float(np.sqrt(np.mean((img[bottom].astype(np.float64) - true[bottom]) ** 2)))
    return contrast, rms(out) / rms(noisy)


# measured with the restatement (`python -m tests.test_denoise_variance`), seed 20, default configuration -- DESIGN.md 4.10 carries them
MEASURED_CONTRAST_LOST, MEASURED_ERROR_RATIO = 0.0020, 0.0221  # (contrast kept: 0.9980)


@functools.lru_cache(maxsize=None)
def _noise_property_of_the_host():
    color, half, albedo, normal, true = noise_property_films()
    out = host(PROPERTY_W, PROPERTY_H, color, half, albedo, normal, dvm.config())
    fixed = capi.host_denoise(PROPERTY_W, PROPERTY_H, color, albedo, normal, dm.config())
    got, old = noise_property_numbers(out, color, true), noise_property_numbers(fixed, color, true)
    print(f"variance guide: contrast kept {got[0]:.4f}, error ratio {got[1]:.4f}; fixed sigma_color: contrast kept {old[0]:.4f}, error ratio {old[1]:.4f}")
    return got


def test_noise_decides_the_noisy_region_is_filtered_hard(hip_lib):
    """A flat region under sigma 0.2 noise -- 40 % of its value, four times the step next door -- is filtered hard by the configuration that
    leaves the step alone, because the weight of a colour difference is set by the pixel's measured variance. Measured: RMS error after / before
    = 0.0221 (akr_denoise with its fixed sigmas: 0.0321). The assertion takes half the measured margin to 1: ratio <= (0.0221 + 1) / 2. The input
    is seeded; the margin absorbs nothing else."""
    _, ratio = _noise_property_of_the_host()
    assert ratio <= 0.5 * (MEASURED_ERROR_RATIO + 1.0)


def test_noise_decides_the_step_keeps_its_contrast(hip_lib):
    """The 10 % step under sigma 0.005 noise survives. Measured: the filter loses the fraction 0.0020 of the step's contrast, i.e. keeps 0.9980
    (akr_denoise with its fixed sigmas keeps 0.5671). The assertion takes half the measured margin between what is kept and nothing kept:
    contrast kept >= (1 + measured fraction) / 2 with the measured fraction the one lost, = 0.5010 (half of the kept 0.9980 would be 0.4990; the
    form with the lost fraction is the stricter of the two). Read with the kept fraction the same formula gives 0.9990, above the measurement
    it is derived from -- as for every kept fraction below 1 -- so that cannot be the margin meant. The input is seeded; the margin absorbs
    nothing else."""
    contrast, _ = _noise_property_of_the_host()
    assert contrast >= 0.5 * (1.0 + MEASURED_CONTRAST_LOST)


def test_one_nan_pixel_stays_one_nan_pixel(hip_lib):
    def run(c, a, n):
        half = (np.asarray(c, dtype=f32) * f32(0.5)).astype(f32)  # the halves of the colour film passed in (a NaN stays a NaN)
        k = 41 * 23
        rng = np.random.default_rng(9)
        half[:3 * k] = (half[:3 * k] * rng.uniform(0.8, 1.2, size=3 * k)).astype(f32)
        return host(41, 23, c, half, a, n, dvm.config())
    dm.check_nan_pixel(run)


def test_no_iterations_and_no_demodulation_is_the_resolve(hip_lib, oracle_lib):
    w, h = 33, 17
    color, albedo, normal = dm.random_films(w, h, seed=1, weights=True, splat=True)
    half = (color * f32(0.25)).astype(f32)
    out = host(w, h, color, half, albedo, normal, dvm.config(iterations=0, demodulate=0), (0.375, 1.0, 1.0))
    assert np.array_equal(out.view(np.uint32), pyoracle.resolve(color, w, h, 0.375).view(np.uint32))


def test_denoising_the_oracle_film_reduces_its_error(hip_lib, root):
    """The bar is the factor 1: relMSE against the oracle's 2048-spp image of the denoised 16-spp film is lower than that of the film."""
    _, albedo, ns, ref = dm.golden_cbox(root)
    half, full = dvm.golden_halves(root)
    n = 64 * 64
    assert np.all(half[6 * n:] == 8) and np.all(full[6 * n:] == 16)
    out = host(64, 64, full, half, albedo, ns, abi.DenoiseConfig.default())
    before, after = dm.rel_mse(dm.resolve_np(full, 64, 64), ref), dm.rel_mse(out, ref)
    print(f"relMSE noisy {before:.5f} denoised {after:.5f} ratio {after / before:.3f}")
    assert after < before


def test_config_default_size_and_refusals(hip_lib):
    c = abi.DenoiseConfig()
    assert hip_lib.akr_denoise_config_default(C.byref(c)) == 0
    assert bytes(c) == bytes(abi.DenoiseConfig.default())
    assert c.sigma_variance == f32(dvm.SIGMA_VARIANCE) and c._pad == 0
    assert C.sizeof(abi.DenoiseConfig) == 32 and hip_lib.akr_struct_size(17) == 32 and hip_lib.akr_struct_size(18) == 0
    color, albedo, normal = dm.random_films(5, 5)
    half = (color * f32(0.5)).astype(f32)
    for bad in (dict(iterations=9), dict(sigma_color=-1.0), dict(sigma_normal=float("nan")), dict(sigma_albedo=float("inf")), dict(sigma_normal=1e-30),
                dict(albedo_floor=0.0), dict(albedo_floor=float("nan")),  # akr_denoise's
                dict(sigma_variance=0.0), dict(sigma_variance=-1.0), dict(sigma_variance=float("nan")), dict(sigma_variance=float("inf")),
                dict(sigma_variance=1e-30), dict(sigma_variance=1e-15)):  # 1 / sigma^2 = inf; 1e30 / 1e-10 = inf
        with pytest.raises(capi.AkariError) as e:
            host(5, 5, color, half, albedo, normal, dvm.config(**bad))
        assert e.value.code == capi.ERR_INVALID_ARGUMENT and "akr_denoise" in str(e.value), bad
    # the edges of the range pass: kv / 1e-10 finite (sigma_variance 1e-14: kv = 1e28), kv = 0 (sigma_variance^2 = inf)
    assert np.isfinite(host(5, 5, color, half, albedo, normal, dvm.config(sigma_variance=1e-14))).all()
    assert np.isfinite(host(5, 5, color, half, albedo, normal, dvm.config(sigma_variance=3e38))).all()
    ok = abi.DenoiseConfig.default()
    assert hip_lib.akr_denoise_variance(None, C.byref(ok), None, None, None, None, None) == capi.ERR_INVALID_ARGUMENT
    out = np.zeros(75, dtype=f32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    assert hip_lib.akr_host_denoise_variance(C.byref(ok), 5, 5, fp(color), 1.0, None, fp(albedo), 1.0, fp(normal), 1.0, fp(out)) == capi.ERR_INVALID_ARGUMENT  # half is NULL


def test_akr_denoise_ignores_sigma_variance(hip_lib):
    """Arbitrary bytes in the field that used to be padding: the bits akr_host_denoise returns with the field zero."""
    w, h = 33, 17
    color, albedo, normal = dm.random_films(w, h)
    base = capi.host_denoise(w, h, color, albedo, normal, dm.config())
    for bits in (0xFFFFFFFF, 0x7FC00000, 0x80000000, 0x12345678):
        cfg = dm.config()
        cfg.sigma_variance = float(np.array([bits], dtype=np.uint32).view(f32)[0])
        assert np.array_equal(capi.host_denoise(w, h, color, albedo, normal, cfg).view(np.uint32), base.view(np.uint32))


def test_the_option(hip_lib):
    assert capi.get_option("denoise_variance") == 0
    with capi.options(denoise=16, denoise_variance=1):
        assert capi.get_option("denoise_variance") == 1
    for value in (-1, 2):
        with pytest.raises(capi.AkariError):
            capi.set_option("denoise_variance", value)
    assert capi.get_option("denoise_variance") == 0


if __name__ == "__main__":  # the two numbers of the noise property, measured with the restatement
    color, half, albedo, normal, true = noise_property_films()
    out = dvm.denoise_variance_np(PROPERTY_W, PROPERTY_H, color, half, albedo, normal, dvm.config())
    print("variance guide: contrast kept %.4f, error ratio %.4f" % noise_property_numbers(out, color, true))
    out = dm.denoise_np(PROPERTY_W, PROPERTY_H, color, albedo, normal, dm.config())
    print("fixed sigma_color: contrast kept %.4f, error ratio %.4f" % noise_property_numbers(out, color, true))
