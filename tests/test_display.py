"""akr_display_transform without a GPU: the host build of csrc/device/ddisplay.h (akr_host_display_transform,
akr_host_luminance_histogram) and akr_display_exposure against the numpy restatement of the definition bit for bit, properties that restate
nothing, the configuration, its refusals and the options."""
import ctypes as C

import numpy as np
import pytest

from akari_render_amd import abi, capi
from tests import display_model as dm
from tests.denoise_model import film_of
from tests.probe_matrix import same_bits_or_both_nan

f32 = np.float32
CASES = dm.cases()


@pytest.mark.parametrize("shape", dm.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_host_equals_the_restatement(hip_lib, oracle_lib, case, shape):
    name, cfg = case
    w, h = shape
    for kind in dm.KINDS:
        got, k = capi.host_display_transform(w, h, dm.case_film(w, h, kind), cfg, dm.SPLAT_SCALE[kind])
        ref, k_ref = dm.case_reference(w, h, kind, name)
        assert f32(k).view(np.uint32) == f32(k_ref).view(np.uint32), f"{name} {w}x{h} {kind}: exposure {k} against {k_ref}"
        same = same_bits_or_both_nan(got, ref)
        assert same.all(), f"{name} {w}x{h} {kind}: {np.count_nonzero(~same)} of {same.size} floats differ"
        assert np.isfinite(ref).all() and ref.min() >= 0 and ref.max() <= 1  # (the transform is total: whatever the film holds)


@pytest.mark.parametrize("kind", dm.KINDS)
@pytest.mark.parametrize("shape", dm.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_histogram_is_the_bincount_of_the_restated_bins(hip_lib, oracle_lib, shape, kind):
    w, h = shape
    counts, skipped = capi.host_luminance_histogram(w, h, dm.case_film(w, h, kind), dm.SPLAT_SCALE[kind])
    ref_counts, ref_skipped = dm.case_histogram(w, h, kind)
    assert np.array_equal(counts, ref_counts) and skipped == ref_skipped
    assert int(counts.sum()) + skipped == w * h


def test_host_equals_the_restatement_on_the_large_frame(hip_lib, oracle_lib):
    """dm.LARGE_SHAPE under dm.LARGE_CASE (Hable, auto-exposure, bloom of five levels): the reference tests/test_gpu_frame_thresholds.py holds
    the device to, held to the host build first."""
    w, h = dm.LARGE_SHAPE
    cfg = next(c for n, c in CASES if n == dm.LARGE_CASE)
    assert (cfg.curve, cfg.auto_exposure, cfg.bloom_levels) == (abi.DISPLAY_HABLE, 1, 5) and cfg.bloom_strength > 0
    got, k = capi.host_display_transform(w, h, dm.case_film(w, h, "random"), cfg, dm.SPLAT_SCALE["random"])
    ref, k_ref = dm.case_reference(w, h, "random", dm.LARGE_CASE)
    assert f32(k).view(np.uint32) == f32(k_ref).view(np.uint32), f"exposure {k} against {k_ref}"
    same = same_bits_or_both_nan(got, ref)
    assert same.all(), f"{np.count_nonzero(~same)} of {same.size} floats differ"
    assert np.isfinite(ref).all() and ref.min() >= 0 and ref.max() <= 1


@pytest.mark.parametrize("kind", dm.KINDS)
def test_host_histogram_on_the_large_frame(hip_lib, oracle_lib, kind):
    w, h = dm.LARGE_SHAPE
    counts, skipped = capi.host_luminance_histogram(w, h, dm.case_film(w, h, kind), dm.SPLAT_SCALE[kind])
    ref_counts, ref_skipped = dm.case_histogram(w, h, kind)
    assert np.array_equal(counts, ref_counts) and skipped == ref_skipped
    assert int(counts.sum()) + skipped == w * h


def test_exposure_on_hand_made_counts(hip_lib, oracle_lib):
    def both(cfg, counts):
        k, ref = capi.display_exposure(cfg, counts), dm.exposure(cfg, counts)
        assert f32(k).view(np.uint32) == f32(ref).view(np.uint32), (k, ref)
        return k

    one = np.zeros(256, dtype=np.uint32)
    one[160] = 1000  # all in one bin: avg = 160.5 / 8 - 20 = 0.0625 whatever the trimming, k = key 2^-0.0625
    for low, high in ((0, 0), (50, 20), (999, 0), (0, 999), (500, 499)):
        k = both(dm.config(low_permille=low, high_permille=high), one)
        assert abs(k / (0.18 * 2.0 ** -0.0625) - 1) < 1e-6
    assert abs(both(dm.config(exposure_ev=2.0, key=0.36), one) / (4 * 0.36 * 2.0 ** -0.0625) - 1) < 1e-6
    # trimming that splits a bin: 10 + 10 samples, 25 % off the bottom takes 5 of bin 100, 10 % off the top 2 of bin 200:
    # m = (5 * 100.5 + 8 * 200.5) / 13
    two = np.zeros(256, dtype=np.uint32)
    two[100], two[200] = 10, 10
    k = both(dm.config(low_permille=250, high_permille=100), two)
    assert abs(k / (0.18 * 2.0 ** -((5 * 100.5 + 8 * 200.5) / 13 / 8 - 20)) - 1) < 1e-5
    # uint64 arithmetic: 2^32 - 1 samples per bin in four bins
    big = np.zeros(256, dtype=np.uint32)
    big[[3, 90, 91, 250]] = 0xFFFFFFFF
    both(dm.config(low_permille=333, high_permille=333), big)
    # everything skipped (an empty histogram) -> the manual k
    for ev in (0.0, 1.5, -3.0):
        cfg = dm.config(exposure_ev=ev, auto_exposure=1)
        assert f32(both(cfg, np.zeros(256, dtype=np.uint32))).view(np.uint32) == dm.manual_exposure(cfg).view(np.uint32)
    assert both(dm.config(), np.zeros(256, dtype=np.uint32)) == 1.0  # (exp_f(0) is 1)
    # a film below 2^-20 everywhere, through the whole transform
    dark = film_of(np.full((5, 7, 3), 1e-9, dtype=f32))
    _, k = capi.host_display_transform(7, 5, dark, dm.config(auto_exposure=1, exposure_ev=1.0))
    assert k == 2.0


@pytest.mark.parametrize("cv", dm.CURVES, ids=[abi.DISPLAY_CURVE_NAMES[c] for c in dm.CURVES])
def test_curves_start_at_zero_rise_and_stay_in_range(hip_lib, cv):
    """10^4 points of [0, 100] through the host build: a 100 x 100 film, manual exposure 0 EV (k = 1), no bloom."""
    x = np.linspace(0.0, 100.0, 10000).astype(f32)
    for white in (0.0, 2.0, 30.0):
        out, k = capi.host_display_transform(100, 100, film_of(np.repeat(x[:, None], 3, axis=1).reshape(100, 100, 3)), dm.config(curve=cv, white=white))
        y = out.reshape(-1, 3)
        assert k == 1.0 and np.array_equal(y[:, 0], y[:, 1]) and np.array_equal(y[:, 0], y[:, 2])
        y = y[:, 0]
        assert y[0] == 0.0 and np.all(np.diff(y) >= 0) and y.min() >= 0.0 and y.max() <= 1.0
        assert same_bits_or_both_nan(y, dm.curve(x, dm.config(curve=cv, white=white))).all()


@pytest.mark.parametrize("levels", [1, 2, 3, 5, 6, 7, 8])
@pytest.mark.parametrize("shape", dm.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_constant_image_is_a_fixed_point_of_the_pyramid(hip_lib, shape, levels):
    """Every weight set sums to 1 in dyadic constants: a constant 0.5 image under threshold 0 feeds 0.5 into every level, every U_l is
    0.5 (levels - l + 1) exactly, and the linear curve shows 0.5 + strength 0.5 wherever that is <= 1."""
    w, h = shape
    film = film_of(np.full((h, w, 3), 0.5, dtype=f32))
    for strength in (0.25, 0.5, 1.0):
        out, _ = capi.host_display_transform(w, h, film, dm.config(curve=abi.DISPLAY_LINEAR, bloom_strength=strength, bloom_threshold=0.0, bloom_levels=levels))
        assert np.all(out == f32(0.5 + strength * 0.5))


def test_strength_zero_is_bloom_off(hip_lib):
    w, h = 41, 23
    for kind in dm.KINDS:
        film = dm.case_film(w, h, kind)
        for cv in dm.CURVES:
            off, _ = capi.host_display_transform(w, h, film, dm.config(curve=cv, auto_exposure=1))
            for levels, threshold in ((1, 0.0), (8, 1.0), (0, 1.0), (99, 0.5)):  # (the levels are not read, not even checked, without a strength)
                zero, _ = capi.host_display_transform(w, h, film, dm.config(curve=cv, auto_exposure=1, bloom_strength=0.0, bloom_levels=levels, bloom_threshold=threshold))
                assert np.array_equal(zero.view(np.uint32), off.view(np.uint32))


def test_bloom_spreads_a_highlight_and_nothing_else(hip_lib):
    """One pixel of 50 on a field of 0.25 under threshold 1: the field feeds nothing (its bright pass is exactly 0), so the bloom term is the
    highlight's alone -- positive around it, and the image without the highlight is untouched by the bloom."""
    w, h = 33, 21
    rgb = np.full((h, w, 3), 0.25, dtype=f32)
    flat_on, _ = capi.host_display_transform(w, h, film_of(rgb), dm.config(curve=abi.DISPLAY_LINEAR, bloom_strength=1.0, bloom_levels=4))
    assert np.all(flat_on == f32(0.25))
    rgb[10, 16] = 50.0
    on, _ = capi.host_display_transform(w, h, film_of(rgb), dm.config(curve=abi.DISPLAY_LINEAR, bloom_strength=1.0, bloom_levels=4))
    assert on[10, 15, 0] > 0.25 and on[8, 16, 0] > 0.25 and np.all(on >= f32(0.25))


def test_config_default_size_and_refusals(hip_lib):
    c = abi.DisplayConfig()
    assert hip_lib.akr_display_config_default(C.byref(c)) == 0
    assert bytes(c) == bytes(abi.DisplayConfig.default())
    assert (c.curve, c.auto_exposure, c.low_permille, c.high_permille, c.bloom_levels) == (abi.DISPLAY_ACES, 0, 50, 20, 5)
    assert (c.exposure_ev, c.key, c.white, c.bloom_strength, c.bloom_threshold) == (0.0, f32(0.18), 0.0, 0.0, 1.0)
    hip_lib.akr_struct_size.restype = C.c_uint32
    assert C.sizeof(abi.DisplayConfig) == 48 and hip_lib.akr_struct_size(22) == C.sizeof(abi.DisplayConfig)
    for unknown in (18, 21, 23, 99):
        assert hip_lib.akr_struct_size(unknown) == 0
    assert hip_lib.akr_display_config_default(None) == capi.ERR_INVALID_ARGUMENT
    film = dm.case_film(7, 5, "random")
    nan, inf = float("nan"), float("inf")
    for bad in (dict(curve=0), dict(curve=5), dict(bloom_strength=0.5, bloom_levels=0), dict(bloom_strength=0.5, bloom_levels=9),
                dict(bloom_strength=-0.5), dict(bloom_strength=nan), dict(bloom_strength=inf), dict(bloom_threshold=-1.0), dict(bloom_threshold=nan),
                dict(bloom_threshold=inf), dict(exposure_ev=nan), dict(exposure_ev=inf), dict(exposure_ev=-inf), dict(key=0.0), dict(key=-0.18), dict(key=nan),
                dict(key=inf), dict(white=-1.0), dict(white=nan), dict(white=inf), dict(low_permille=500, high_permille=500),
                dict(low_permille=1000, high_permille=0), dict(low_permille=0xFFFFFFFF, high_permille=2), dict(exposure_ev=101.0),
                dict(curve=abi.DISPLAY_REINHARD, white=1e-30)):
        with pytest.raises(capi.AkariError) as e:
            capi.host_display_transform(7, 5, film, dm.config(**bad))
        assert e.value.code == capi.ERR_INVALID_ARGUMENT and "akr_display" in str(e.value), bad
        if "exposure_ev" not in bad or bad["exposure_ev"] != 101.0:
            if bad != dict(curve=abi.DISPLAY_REINHARD, white=1e-30):
                with pytest.raises(capi.AkariError) as e:
                    capi.display_exposure(dm.config(**bad), np.zeros(256, dtype=np.uint32))
                assert e.value.code == capi.ERR_INVALID_ARGUMENT, bad
    # the edges of the ranges pass
    capi.host_display_transform(7, 5, film, dm.config(bloom_strength=0.5, bloom_levels=8, bloom_threshold=0.0, low_permille=999, high_permille=0, exposure_ev=-100.0))
    capi.host_display_transform(7, 5, film, dm.config(bloom_strength=64.0, bloom_levels=1, exposure_ev=99.0, low_permille=0, high_permille=999))
    assert hip_lib.akr_display_transform(None, C.byref(c), None, None, None) == capi.ERR_INVALID_ARGUMENT
    assert hip_lib.akr_film_luminance_histogram(None, None, None, None) == capi.ERR_INVALID_ARGUMENT
    assert hip_lib.akr_display_exposure(None, None, None) == capi.ERR_INVALID_ARGUMENT


def test_the_options(hip_lib):
    names = ("display", "display_auto_exposure", "display_exposure", "display_bloom", "display_kernel")
    defaults = (0, 0, 0, 0, -1)
    assert tuple(capi.get_option(n) for n in names) == defaults
    with capi.options(display=3, display_bloom=256, display_auto_exposure=1, display_exposure=-2048, display_kernel=1):
        assert tuple(capi.get_option(n) for n in names) == (3, 1, -2048, 256, 1)
    for name, value in (("display", -1), ("display", 5), ("display_auto_exposure", 2), ("display_exposure", 65537), ("display_exposure", -65537),
                        ("display_bloom", -1), ("display_bloom", 65537), ("display_kernel", 2), ("display_kernel", -2)):
        with pytest.raises(capi.AkariError):
            capi.set_option(name, value)
    assert tuple(capi.get_option(n) for n in names) == defaults
