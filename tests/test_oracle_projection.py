"""The oracle's camera projections (oracle/akr_oracle.c or_camera_ray, or_scene_set_projection) without a GPU. The oracle's arms
are a restatement in C of the section's text, so they are held from two sides: the numpy restatement (tests/camera_model.py) and the library's
shared ray-generation text run on the host (akr_host_lens_ray) must both give the oracle's rays, bit for bit, on the rows of
tests/test_projection.py. Beside that: the setter's refusals tabled against the library's, the u_lens pair a projected camera draws and leaves
unused, the integrators that refuse a projection, the fold following the resolution, and oracle/scene_json.py against akr_scene_load."""
import numpy as np
import pytest

from akari_render_amd import abi, capi
from oracle import pyoracle, scene_json
from tests import test_projection as TP
from tests.helpers import make_config
from tests.punct_parity_cases import initial_states
from tests.test_environment import quad_scene
from tests.test_lens import _camera

F = np.float32


def set_oracle_case(osc, case):
    """tests/test_projection.set_case on the oracle's scene"""
    osc.set_lens(None)
    if case.startswith("ortho"):
        osc.set_projection("orthographic", ortho_scale=TP.ORTHO_SCALE)
        if case == "ortho_lens":
            osc.set_lens(*TP.LENS)
    elif case == "panorama":
        osc.set_projection("panorama")
    else:
        osc.set_projection("panorama", longitude_min=TP.WINDOW[0], longitude_max=TP.WINDOW[1], latitude_min=TP.WINDOW[2], latitude_max=TP.WINDOW[3])


# ---------------------------------------------------------------------------------------------------------------- 1. three implementations, one ray
@pytest.mark.parametrize("rotated", [False, True], ids=["identity", "rotated"])
@pytest.mark.parametrize("size", TP.FILMS, ids=["%dx%d" % s for s in TP.FILMS])
def test_three_way_ray_identity(hip_lib, size, rotated):
    w, h = size
    sd = _camera(w, h, rotated)
    scene, osc = capi.Scene(None, sd), pyoracle.OracleScene(sd)
    pixels, u_filter, u_lens = TP.rows_of(w, h, 100 + 7 * w + h + int(rotated))
    for case in TP.CASES:
        TP.set_case(scene, case)
        set_oracle_case(osc, case)
        assert osc.projection() == scene.projection() and osc.lens() == scene.lens()
        for ft, fr in TP.FILTERS:
            got = osc.lens_ray_many(pixels, u_filter, u_lens, ft, fr).view(np.uint32)
            model = TP.model_rays(case, scene, w, h, pixels, u_filter, u_lens, ft, fr).view(np.uint32)
            host = scene.host_lens_ray(pixels, u_filter, u_lens, ft, fr).view(np.uint32)
            for name, want in (("model", model), ("host", host)):
                bad = np.flatnonzero(np.any(got != want, axis=1))
                assert len(bad) == 0, (case, ft, name, len(bad), pixels[bad[:3]], u_filter[bad[:3]], got[bad[:3]].view(F), want[bad[:3]].view(F))


def test_perspective_rays_are_what_they_were(hip_lib):
    """a projection set and taken back leaves the oracle's perspective camera, with and without a lens, to the bits"""
    w, h = 40, 32
    pixels, u_filter, u_lens = TP.rows_of(w, h, 5)
    for rotated in (False, True):
        sd = _camera(w, h, rotated)
        plain, osc = pyoracle.OracleScene(sd), pyoracle.OracleScene(sd)
        for back in ("orthographic", "panorama"):
            osc.set_projection(back, **({"ortho_scale": 3.0} if back == "orthographic" else {}))
            assert np.any(osc.lens_ray_many(pixels, u_filter, u_lens) != plain.lens_ray_many(pixels, u_filter, u_lens))
            osc.set_projection(None)
            assert osc.projection() == abi.ProjectionData()
            for lens in (None, (0.05, 3.0)):
                plain.set_lens(*(lens or (None,)))
                osc.set_lens(*(lens or (None,)))
                for ft, fr in TP.FILTERS:
                    a, b = plain.lens_ray_many(pixels, u_filter, u_lens, ft, fr), osc.lens_ray_many(pixels, u_filter, u_lens, ft, fr)
                    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (back, lens, ft)
            plain.set_lens(None)
            osc.set_lens(None)


def test_the_fold_follows_the_resolution(hip_lib):
    """or_scene_set_resolution redoes the orthographic matrix and the panorama's inv_w, inv_h: the rays are those of a scene made at that size"""
    for case in TP.CASES:
        osc = pyoracle.OracleScene(_camera(40, 32, True))
        set_oracle_case(osc, case)
        for w, h in ((7, 3), (3, 7)):
            fresh = pyoracle.OracleScene(_camera(w, h, True))
            set_oracle_case(fresh, case)
            osc.set_resolution(w, h)
            pixels, u_filter, u_lens = TP.rows_of(w, h, 3)
            assert np.array_equal(osc.lens_ray_many(pixels, u_filter, u_lens).view(np.uint32), fresh.lens_ray_many(pixels, u_filter, u_lens).view(np.uint32)), (case, w, h)


# ---------------------------------------------------------------------------------------------------------------- 2. refusals
def _bad_descriptions():
    up, hup = float(np.nextafter(F(np.pi), F(4))), float(np.nextafter(F(np.pi / 2), F(2)))
    return [dict(type=3), dict(type=0xffffffff),
            dict(type=1, ortho_scale=0.0), dict(type=1, ortho_scale=-1.0), dict(type=1, ortho_scale=np.nan), dict(type=1, ortho_scale=np.inf), dict(type=1, ortho_scale=-np.inf),
            dict(type=2, longitude_min=-up), dict(type=2, longitude_max=up), dict(type=2, longitude_min=1.0, longitude_max=1.0),
            dict(type=2, longitude_min=1.0, longitude_max=0.5), dict(type=2, longitude_min=np.nan), dict(type=2, longitude_max=np.inf),
            dict(type=2, latitude_min=-hup), dict(type=2, latitude_max=hup), dict(type=2, latitude_min=0.25, latitude_max=0.25),
            dict(type=2, latitude_min=0.5, latitude_max=-0.5), dict(type=2, latitude_max=np.nan), dict(type=2, latitude_min=-np.inf)]


def _good_descriptions():
    pi, hpi = float(F(np.pi)), float(F(np.pi / 2))
    return [dict(type=0), dict(type=0, ortho_scale=np.nan, longitude_min=9.0), dict(type=1, ortho_scale=2.5), dict(type=1, ortho_scale=1e-30, latitude_max=np.nan),
            dict(type=2), dict(type=2, ortho_scale=-1.0), dict(type=2, longitude_min=-pi, longitude_max=pi, latitude_min=-hpi, latitude_max=hpi),
            dict(type=2, longitude_min=0.5, longitude_max=float(F(0.5) + F(2.0 ** -6))), dict(type=2, latitude_min=-0.375, latitude_max=1.25)]


def _try(setter, *a):
    try:
        setter(*a)
        return True
    except (ValueError, capi.AkariError) as e:
        assert isinstance(e, ValueError) or e.code == capi.ERR_INVALID_ARGUMENT
        return False


def test_setter_refusals_are_the_librarys(hip_lib):
    sd = quad_scene()
    scene, osc = capi.Scene(None, sd), pyoracle.OracleScene(sd)
    scene.set_projection("orthographic", ortho_scale=1.5)
    osc.set_projection("orthographic", ortho_scale=1.5)
    for kw in _bad_descriptions():
        d = abi.ProjectionData(**kw)
        assert _try(scene.set_projection, d) is False and _try(osc.set_projection, d) is False, kw
        assert osc.projection() == scene.projection() == abi.ProjectionData(type=abi.PROJECTION_ORTHOGRAPHIC, ortho_scale=1.5), kw  # nothing changed
    for kw in _good_descriptions():  # ... and what the type does not read is neither checked nor kept
        d = abi.ProjectionData(**kw)
        assert _try(scene.set_projection, d) is True and _try(osc.set_projection, d) is True, kw
        assert osc.projection() == scene.projection(), kw
    # a panorama has no lens, whichever is set second; the state stays what it was
    for s in (scene, osc):
        s.set_projection("panorama")
        assert _try(s.set_lens, 0.1, 2.0) is False
        assert s.lens() is None and s.projection() == abi.ProjectionData(type=abi.PROJECTION_PANORAMA)
        s.set_lens(0.0, 0.0)  # (no lens is no lens)
        s.set_projection("orthographic", ortho_scale=1.5)
        s.set_lens(0.1, 2.0)
        assert _try(s.set_projection, "panorama") is False
        assert s.lens() == abi.LensData(float(F(0.1)), 2.0) and s.projection() == abi.ProjectionData(type=abi.PROJECTION_ORTHOGRAPHIC, ortho_scale=1.5)
        s.set_projection(None)
        assert s.projection() == abi.ProjectionData() and s.lens() == abi.LensData(float(F(0.1)), 2.0)
    bad = quad_scene()
    bad.projection, bad.lens = abi.ProjectionData(type=abi.PROJECTION_PANORAMA), abi.LensData(0.1, 2.0)
    with pytest.raises(ValueError):
        pyoracle.OracleScene(bad)
    assert pyoracle.OracleScene(bad, projection=False).projection() == abi.ProjectionData()
    assert pyoracle.OracleScene(bad, lens=False).projection() == bad.projection


def test_gpt_and_mcmc_refuse_a_projected_scene(hip_lib):
    osc = pyoracle.OracleScene(quad_scene(width=8, height=8))
    g, m = abi.GptConfig.default(), abi.McmcConfig.default()
    g.spp, m.spp, m.n_chains, m.n_bootstrap = 1, 1, 4, 16
    for kw in (dict(projection="orthographic", ortho_scale=2.0), dict(projection="panorama")):
        osc.set_projection(**kw)
        with pytest.raises(AssertionError, match="-5"):
            osc.gpt_render(g, n_threads=1)
        with pytest.raises(AssertionError, match="-5"):
            osc.mcmc_render(m, n_threads=1)
    osc.set_projection(None)
    osc.gpt_render(g, n_threads=1)  # perspective again: accepted


# ---------------------------------------------------------------------------------------------------------------- 3. the u_lens pair, drawn and unused
_M64, _MULT = (1 << 64) - 1, 6364136223846793005


def _advance(state, inc, delta):
    """Pcg32::advance as the reference has it (sampler/mod.rs; oracle/or_rng.h pcg_advance, which tests/test_oracle_kat.py pins)"""
    cur_mult, cur_plus, acc_mult, acc_plus, delta = _MULT, inc, 1, 0, delta & _M64
    while delta > 0:
        if delta & 1:
            acc_mult = (acc_mult * cur_mult) & _M64
            acc_plus = (acc_plus + cur_mult + cur_plus) & _M64
        cur_plus = ((cur_mult + 1) * cur_plus) & _M64
        cur_mult = (cur_mult * cur_mult) & _M64
        delta >>= 1
    return (acc_mult * state + acc_plus) & _M64


def _states_after(initial, spp, dims):
    """The independent sampler's states after one pass of `spp` samples that each draw `dims` numbers: start() advances by 16384, a number is
    one step of the generator, the sampler's Drop advances by minus the pass's dimensions (sampler/mod.rs:161-217)."""
    out = initial.copy()
    for i in range(len(initial) // 2):
        s, inc = int(initial[2 * i]), int(initial[2 * i + 1])
        for _ in range(spp):
            s = _advance(s, inc, 16384)
            for _ in range(dims):
                s = (s * _MULT + inc) & _M64
        out[2 * i] = _advance(s, inc, -(spp * dims))
    return out


@pytest.mark.parametrize("rotated", [False, True], ids=["identity", "rotated"])
def test_a_projected_camera_draws_u_lens_and_leaves_it_unused(hip_lib, rotated):
    """DESIGN.md 4.17 "Sampler dimensions" on the independent sampler at max_depth = 0, where a sample draws what its camera ray draws and
    nothing else: the perspective camera's final states are those of k numbers a sample (k found, the same for every pixel), a projected
    camera's with R == 0 those of k + 2, and the same states the projection leaves with a lens set, which uses the pair."""
    w, h, spp = 8, 6, 3
    sd = _camera(w, h, rotated)
    cfg = make_config(spp=spp, spp_per_pass=spp, max_depth=0, sampler_seed=11)
    first = initial_states(cfg, w, h)

    def final(projection=None, lens=None, **kw):
        osc = pyoracle.OracleScene(sd)
        if projection is not None:
            osc.set_projection(projection, **kw)
        if lens is not None:
            osc.set_lens(*lens)
        states = first.copy()
        film, _ = osc.render(cfg, n_threads=1, states=states)
        return states, film

    persp, _ = final()
    k = [d for d in range(0, 16) if np.array_equal(_states_after(first, spp, d), persp)]
    assert k == [2], k  # u_filter alone
    persp_lens, _ = final(lens=(0.125, 1.75))
    assert np.array_equal(persp_lens, _states_after(first, spp, 4))
    want = _states_after(first, spp, 4)
    assert not np.array_equal(want, persp)
    for kw in (dict(projection="orthographic", ortho_scale=2.5), dict(projection="panorama"), dict(projection="panorama", longitude_min=-2.25, longitude_max=0.5)):
        assert np.array_equal(final(**kw)[0], want), kw
    ortho, ortho_film = final(projection="orthographic", ortho_scale=2.5)
    with_lens, _ = final(projection="orthographic", ortho_scale=2.5, lens=(0.125, 1.75))
    assert np.array_equal(ortho, with_lens)
    # unused: the film of R == 0 is the film whose u_lens never mattered -- a lens of a radius too small to move an origin gives its bits
    tiny, tiny_film = final(projection="orthographic", ortho_scale=2.5, lens=(1e-30, 1.75))
    assert np.array_equal(tiny, ortho) and np.array_equal(tiny_film, ortho_film)


# ---------------------------------------------------------------------------------------------------------------- 4. one file, both readers
def test_both_readers_fill_the_same_projection(hip_lib, cbox_path, tmp_path):
    for name, camera_type, data, want in (
            ("ortho", "orthographic", dict(ortho_scale=0.75), abi.ProjectionData(type=abi.PROJECTION_ORTHOGRAPHIC, ortho_scale=0.75)),
            ("pano", "panorama", {}, abi.ProjectionData(type=abi.PROJECTION_PANORAMA)),
            ("win", "panorama", dict(longitude_min=-1.0, longitude_max=0.5, latitude_max=0.25), abi.ProjectionData(abi.PROJECTION_PANORAMA, 1.0, -1.0, 0.5, -float(F(np.pi / 2)), 0.25)),
            ("tenth", "orthographic", dict(ortho_scale=0.1, fov=50.0), abi.ProjectionData(type=abi.PROJECTION_ORTHOGRAPHIC, ortho_scale=float(F(0.1))))):
        path = TP._with_camera(cbox_path, tmp_path, name, camera_type, **data)
        lib_scene, sd = capi.Scene(None, path), scene_json.load_scene(path)
        assert sd.projection == lib_scene.projection() == want, name
        assert pyoracle.OracleScene(sd).projection() == want
        # the rest of the camera is the perspective file's: the size, c2w, and the field of view a switch back would render with
        there = lib_scene.to_scene_data().camera
        assert (sd.camera.width, sd.camera.height) == (there.width, there.height) and F(sd.camera.fov) == F(there.fov), name
        assert np.array_equal(np.asarray(sd.camera.c2w, F).view(np.uint32), lib_scene.array(capi.ARRAY_C2W, F).view(np.uint32))
    plain = scene_json.load_scene(cbox_path)
    assert plain.projection is None and capi.Scene(None, cbox_path).projection() == abi.ProjectionData()
    for name, camera_type, data in (("nokey", "orthographic", {}), ("neg", "orthographic", {"ortho_scale": -1.0}), ("badwin", "panorama", {"longitude_min": 2.0, "longitude_max": 1.0}),
                                    ("fisheye", "fisheye", {})):
        path = TP._with_camera(cbox_path, tmp_path, name, camera_type, **data)
        with pytest.raises(capi.AkariError):
            capi.Scene(None, path)
        with pytest.raises(ValueError):
            scene_json.load_scene(path)
