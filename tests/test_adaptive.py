"""Adaptive sampling without a GPU: the host build of csrc/device/dadapt.h (akr_host_tile_error, akr_host_half_bracket)
against the numpy restatement, bit for bit; the restatement of the whole adaptive render on the CPU oracle's prefix films of scenes/cbox;
the new symbols and struct ids."""
import ctypes as C

import numpy as np
import pytest

from akari_render_amd import abi, capi
from tests import adaptive_model as am

f32 = np.float32


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=f32).view(np.uint32), np.asarray(b, dtype=f32).view(np.uint32))


@pytest.mark.parametrize("shape", am.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}-tiles{s[2]}x{s[3]}")
def test_host_tile_error_equals_the_restatement(hip_lib, shape):
    w, h, tw, th = shape
    film, half = am.random_films(w, h, tw, th)
    tiles = am.all_tiles(w, h, tw, th)
    ref = am.reference_errors(w, h, tw, th)
    got = capi.host_tile_error(w, h, film, half, tw, th, tiles)
    assert same_bits(got, ref), f"{np.count_nonzero(got.view(np.uint32) != ref.view(np.uint32))} of {ref.size} tile errors differ"
    # the cases the definition names are in the films: a tile without any estimate is +inf, every other tile finite and positive
    by_tile = dict(zip(tiles.tolist(), ref.tolist()))
    assert by_tile[1] == np.inf
    assert all(np.isfinite(e) and e > 0 for t, e in by_tile.items() if t != 1)
    e, has = am.pixel_error(w, h, film, half)
    n = w * h
    wa, wc = half[6 * n:].reshape(h, w), film[6 * n:].reshape(h, w)
    assert (wa == 0).any() and (wc - wa == 0).any() and np.isnan(half[:3 * n]).any()
    assert not has[wa == 0].any() and not has[wc - wa == 0].any() and not has[np.isnan(half[:3 * n].reshape(h, w, 3)).any(axis=2)].any()
    assert np.all(e[~has].view(np.uint32) == 0)  # +0.0f, not -0 and not NaN


def test_equal_halves_of_equal_colour_have_no_error_and_f_is_one_half(hip_lib):
    w, h, tw, th = 16, 8, 8, 8
    n = w * h
    rgb = np.random.default_rng(4).uniform(0.1, 1.0, size=(n, 3)).astype(f32)
    half = np.concatenate([(rgb * f32(4)).reshape(-1), np.zeros(3 * n, f32), np.full(n, 4, f32)])
    film = np.concatenate([(rgb * f32(8)).reshape(-1), np.zeros(3 * n, f32), np.full(n, 8, f32)])
    assert np.all(capi.host_tile_error(w, h, film, half, tw, th, [0, 1]) == 0)
    # the B half black: d = sum of cA, f = 1/2, l = half of that sum
    film2 = np.concatenate([half[:3 * n], np.zeros(3 * n, f32), np.full(n, 8, f32)])
    ca = rgb
    d = (ca[:, 0] + ca[:, 1]) + ca[:, 2]
    m = film2[:3 * n].reshape(n, 3) / f32(8)
    e = (d * f32(0.5)) / np.sqrt(((m[:, 0] + m[:, 1]) + m[:, 2]) + f32(0.01))
    ee, has = am.pixel_error(w, h, film2, half)
    assert has.all() and same_bits(ee.reshape(-1), e)


@pytest.mark.parametrize("shape", am.SHAPES[:3], ids=lambda s: f"{s[0]}x{s[1]}-tiles{s[2]}x{s[3]}")
def test_open_and_close_equal_the_restatement(hip_lib, shape):
    w, h, tw, th = shape
    n = w * h
    before, half = am.random_films(w, h, tw, th)
    rng = np.random.default_rng(8)
    after = np.array(before, copy=True)
    after[:3 * n] = (after[:3 * n] + rng.uniform(0, 3, size=3 * n)).astype(f32)
    after[6 * n:] = after[6 * n:] + f32(2)
    tiles = am.all_tiles(w, h, tw, th)[::2]  # some tiles, not all: the others' pixels must stay as they are
    opened = capi.host_half_bracket(w, h, before, half, tw, th, tiles, False)
    ref_open = am.half_bracket(w, h, before, half, tw, th, tiles, False)
    assert np.array_equal(opened.view(np.uint32), ref_open.view(np.uint32))
    closed = capi.host_half_bracket(w, h, after, opened, tw, th, tiles, True)
    ref = am.half_bracket(w, h, after, ref_open, tw, th, tiles, True)
    assert np.array_equal(closed.view(np.uint32), ref.view(np.uint32))
    off = ~np.repeat(am.tile_mask(w, h, tw, th, tiles).reshape(-1), 3)
    assert np.array_equal(closed[:3 * n][off].view(np.uint32), half[:3 * n][off].view(np.uint32))
    assert np.array_equal(closed[3 * n:6 * n].view(np.uint32), half[3 * n:6 * n].view(np.uint32))  # the splat plane is not touched
    on = am.tile_mask(w, h, tw, th, tiles).reshape(-1)
    assert np.all(closed[6 * n:][on] == half[6 * n:][on] + f32(2))


def test_host_refusals(hip_lib):
    film, half = am.random_films(24, 16, 8, 8)
    for tw, th, what in ((12, 8, "multiples of 8"), (128, 64, "4096"), (72, 64, "4096")):
        with pytest.raises(capi.AkariError) as e:
            capi.host_tile_error(24, 16, film, half, tw, th, [0])
        assert e.value.code == capi.ERR_INVALID_ARGUMENT and what in str(e.value)
    with pytest.raises(capi.AkariError) as e:
        capi.host_tile_error(24, 16, film, half, 8, 8, [6])  # 3 x 2 tiles
    assert e.value.code == capi.ERR_INVALID_ARGUMENT and "out of range" in str(e.value)
    assert capi.host_tile_error(24, 16, film, half, 8, 8, []).size == 0


# ---------------------------------------------------------------------------------------------- the whole render, on oracle prefix films
def run_model(root, threshold, min_spp=8):
    c = am.CBOX
    return am.adaptive(am.cbox_prefix(root), c["w"], c["h"], c["tw"], c["th"], c["spp"], c["spp_per_pass"], c["round_passes"], threshold, min_spp)


def test_every_pixel_holds_the_prefix_film_of_its_tiles_round_count(root, oracle_lib, hip_lib):
    c = am.CBOX
    w, h, tw, th = c["w"], c["h"], c["tw"], c["th"]
    prefix = am.cbox_prefix(root)
    ends = am.round_ends(c["spp"], c["spp_per_pass"], c["round_passes"])
    assert len(prefix) == 8 and ends == [4, 8, 12, 16, 20, 24, 28, 32]
    film, half, tile_spp, drawn, rounds, checks = run_model(root, 0.125)
    n = w * h
    assert 1 < len(set(tile_spp.reshape(-1).tolist())), "the threshold of this test should retire some tiles and keep others"
    for spp in sorted(set(tile_spp.reshape(-1).tolist())):
        tiles = np.nonzero(tile_spp.reshape(-1) == spp)[0]
        m = am.tile_mask(w, h, tw, th, tiles).reshape(-1)
        p = prefix[ends.index(spp)]
        assert np.array_equal(film[:3 * n][np.repeat(m, 3)].view(np.uint32), p[:3 * n][np.repeat(m, 3)].view(np.uint32))
        assert np.array_equal(film[6 * n:][m], p[6 * n:][m]) and np.all(film[6 * n:][m] == spp)
    assert drawn == int(film[6 * n:].sum()) == int((tile_spp.astype(np.int64) * tw * th).sum())
    # the half holds the A-rounds' samples: of a tile's k rounds the ceil(k / 2) A-rounds, four samples each
    wa = half[6 * n:].reshape(h, w)
    per_pixel = np.repeat(np.repeat(tile_spp, th, axis=0), tw, axis=1).astype(f32)
    a_rounds = (per_pixel / 4 + 1) // 2
    assert np.array_equal(wa, a_rounds * 4)
    # the errors the model saw are the host hook's on the same films
    tiles, err = checks[0]
    assert len(checks) >= 1 and same_bits(err, capi.host_tile_error(w, h, prefix[1], am.half_bracket(w, h, prefix[0], np.zeros(7 * n, f32), tw, th, tiles, True), tw, th, tiles))


def test_an_infinite_threshold_retires_every_tile_at_min_spp(root, oracle_lib):
    c = am.CBOX
    for min_spp, expect in ((8, 8), (16, 16), (10, 16), (1, 8)):  # (checks come after B-rounds: at 8, 16, 24 samples)
        film, half, tile_spp, drawn, rounds, _ = run_model(root, np.inf, min_spp)
        assert np.all(tile_spp == expect) and drawn == expect * c["w"] * c["h"] and rounds == expect // 4
        assert np.array_equal(film.view(np.uint32)[:3 * 4096], am.cbox_prefix(root)[expect // 4 - 1].view(np.uint32)[:3 * 4096])


def test_a_threshold_no_tile_meets_reproduces_the_uniform_film(root, oracle_lib):
    c = am.CBOX
    n = c["w"] * c["h"]
    film, half, tile_spp, drawn, rounds, checks = run_model(root, 0.0)
    full = am.cbox_prefix(root)[-1]
    assert np.array_equal(film[:3 * n].view(np.uint32), full[:3 * n].view(np.uint32)) and np.array_equal(film[6 * n:], full[6 * n:])
    assert np.all(tile_spp == c["spp"]) and drawn == c["spp"] * n and rounds == 8 and len(checks) == 3
    assert np.all(half[6 * n:] == 16)


def test_the_default_threshold_beats_uniform_sampling_at_equal_cost(root, oracle_lib):
    """DESIGN.md 4.11's table (tools/adaptive_grid.py): at the default threshold the adaptive film's relMSE against the 2048-spp image is below
    that of the uniform film with the largest spp whose samples do not exceed the adaptive render's -- factor 1, no margin."""
    from tools import adaptive_grid as ag
    rows = ag.grid(root, [abi.AdaptiveConfig.default().threshold])
    (thr, rel, drawn, u_spp, u_rel), = rows
    print(f"threshold {thr}: relMSE {rel:.5f} with {drawn} samples; uniform {u_spp} spp: {u_rel:.5f}")
    assert rel < u_rel


# ---------------------------------------------------------------------------------------------- ABI
def test_new_symbols_and_struct_ids(hip_lib):
    for name in ("akr_pt_set_active_tiles", "akr_film_tile_error", "akr_adaptive_config_default", "akr_pt_adaptive_render"):
        assert hasattr(hip_lib, name) and name in capi.EXPORTS
    for name in ("akr_host_tile_error", "akr_host_half_bracket", "akr_probe_adapt_times"):
        assert hasattr(hip_lib, name) and name in capi.TEST_EXPORTS
    hip_lib.akr_struct_size.restype = C.c_uint32
    assert hip_lib.akr_struct_size(19) == C.sizeof(abi.AdaptiveConfig) == 16
    assert hip_lib.akr_struct_size(20) == C.sizeof(abi.AdaptiveStats) == 24 + C.sizeof(abi.PtStats)
    assert hip_lib.akr_struct_size(99) == 0 and hip_lib.akr_struct_size(21) == 0
    assert hip_lib.akr_struct_size(6) == 88 and hip_lib.akr_struct_size(17) == 32  # the earlier ids are what they were
    c = abi.AdaptiveConfig()
    assert hip_lib.akr_adaptive_config_default(C.byref(c)) == 0
    assert bytes(c) == bytes(abi.AdaptiveConfig.default()) and c.threshold == 0.0625 and c.min_spp == 16 and c.round_passes == 1
    assert hip_lib.akr_adaptive_config_default(None) == capi.ERR_INVALID_ARGUMENT
    for name, bad in (("adaptive", -1), ("adaptive_min_spp", 65537)):
        assert capi.get_option(name) == 0
        with pytest.raises(capi.AkariError):
            capi.set_option(name, bad)
    with capi.options(adaptive=64, adaptive_min_spp=8):
        assert capi.get_option("adaptive") == 64 and capi.get_option("adaptive_min_spp") == 8
