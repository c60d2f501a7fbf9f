"""Camera projections without a GPU: the orthographic and the panorama ray restated in numpy f32 (tests/camera_model.py)
against the shared ray-generation text run on the host (akr_host_lens_ray), their geometric properties in float64, the untouched perspective
route, the setter / getter / scene.json reader and their refusals, and the conservativeness of the acceleration structure's boxes for rays
that start on the rim of an orthographic film (following tests/test_lens.py)."""
import ctypes as C
import json
import os
import shutil

import numpy as np
import pytest

from akari_render_amd import abi, capi
from tests import bvh_model as bm
from tests import camera_model as cm
from tests.helpers import grid_scene, instanced_scene, make_config
from tests.test_environment import quad_scene
from tests.test_lens import _camera, _camera_inside, _rim_targets, restated_lens, restated_pinhole

F = np.float32
N_ROWS = 4096
FILMS = [(1, 1), (7, 3), (3, 7), (40, 32)]
FILTERS = [(abi.FILTER_BOX, 0.5), (abi.FILTER_GAUSSIAN, 1.5)]
WINDOW = (-2.25, 0.5, -0.375, 1.25)  # a longitude / latitude window, not centred
CASES = ["ortho", "ortho_lens", "panorama", "panorama_window"]
ORTHO_SCALE, LENS = 2.5, (0.125, 1.75)


def rows_of(w, h, seed):
    """N_ROWS random rows of (pixel, u_filter, u_lens) and the edge rows: u_filter components 0 and 1 - 2^-24, the first and last pixel of
    a row and of a column (the panorama's seam and poles), u_lens at the centre of the square."""
    rng = np.random.default_rng(seed)
    pixels = np.stack([rng.integers(0, w, N_ROWS), rng.integers(0, h, N_ROWS)], axis=1).astype(np.uint32)
    u_filter, u_lens = rng.random((N_ROWS, 2), dtype=F), rng.random((N_ROWS, 2), dtype=F)
    top = F(1.0) - F(2.0 ** -24)
    edge_px = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (0, h // 2), (w - 1, h // 2), (w // 2, 0), (w // 2, h - 1)]
    edge_uf = [(0.0, 0.0), (top, top), (0.0, top), (top, 0.0), (0.5, 0.5)]
    k = 0
    for p in edge_px:
        for u in edge_uf:
            pixels[k], u_filter[k] = p, u
            k += 1
    u_lens[k:k + 8] = [0.5, 0.5]
    u_lens[:4] = [0.5, 0.5]
    return pixels, u_filter, u_lens


def set_case(scene, case):
    """The projection (and lens) of a case on `scene`."""
    scene.set_lens(None)
    if case.startswith("ortho"):
        scene.set_projection("orthographic", ortho_scale=ORTHO_SCALE)
        if case == "ortho_lens":
            scene.set_lens(*LENS)
    elif case == "panorama":
        scene.set_projection("panorama")
    else:
        scene.set_projection("panorama", longitude_min=WINDOW[0], longitude_max=WINDOW[1], latitude_min=WINDOW[2], latitude_max=WINDOW[3])


def model_rays(case, scene, w, h, pixels, u_filter, u_lens, ft, fr):
    c2w = scene.array(capi.ARRAY_C2W, F)
    if case.startswith("ortho"):
        r2c = cm.ortho_r2c(w, h, ORTHO_SCALE)
        assert np.array_equal(scene.array(capi.ARRAY_R2C, F).view(np.uint32), r2c.view(np.uint32))  # AKR_ARRAY_R2C: the matrix in use
        R, Fd = LENS if case == "ortho_lens" else (0.0, 0.0)
        return cm.ortho_rays(r2c, c2w, pixels, u_filter, u_lens, ft, fr, R, Fd)
    return cm.panorama_rays(c2w, w, h, pixels, u_filter, ft, fr, WINDOW if case == "panorama_window" else ())


# ---------------------------------------------------------------------------------------------------------------- 1. the ray definition
@pytest.mark.parametrize("rotated", [False, True], ids=["identity", "rotated"])
@pytest.mark.parametrize("size", FILMS, ids=["%dx%d" % s for s in FILMS])
def test_ray_definition(hip_lib, size, rotated):
    w, h = size
    scene = capi.Scene(None, _camera(w, h, rotated))
    pixels, u_filter, u_lens = rows_of(w, h, 100 + 7 * w + h + int(rotated))
    for case in CASES:
        set_case(scene, case)
        for ft, fr in FILTERS:
            got = scene.host_lens_ray(pixels, u_filter, u_lens, ft, fr)
            want = model_rays(case, scene, w, h, pixels, u_filter, u_lens, ft, fr)
            assert np.all(np.isfinite(got)), (case, ft)
            bad = np.flatnonzero(np.any(got.view(np.uint32) != want.view(np.uint32), axis=1))
            assert len(bad) == 0, (case, ft, len(bad), pixels[bad[:3]], u_filter[bad[:3]], got[bad[:3]], want[bad[:3]])


# ---------------------------------------------------------------------------------------------------------------- 2. properties in float64
def _centres(w, h):
    ys, xs = np.mgrid[0:h, 0:w]
    pixels = np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.uint32)
    half = np.full((len(pixels), 2), 0.5, F)
    return pixels, half


def _ulp_of_one(x):
    """|x - 1| in ulp of 1.0f: FLT_EPSILON = 2^-23, the spacing of f32 at 1"""
    return np.abs(x.astype(np.float64) - 1.0) / 2.0 ** -23


@pytest.mark.parametrize("rotated", [False, True], ids=["identity", "rotated"])
@pytest.mark.parametrize("size", [(7, 3), (3, 7), (40, 32)], ids=["7x3", "3x7", "40x32"])
def test_properties(hip_lib, size, rotated):
    w, h = size
    scene = capi.Scene(None, _camera(w, h, rotated))
    pixels, half = _centres(w, h)
    m = scene.array(capi.ARRAY_C2W, F).astype(np.float64).reshape(4, 4).T
    X, Y, Z, T = m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3]
    # orthographic: one direction, c2w . (0, 0, -1); pixel-centre origins on a uniform grid that spans ortho_scale along the larger side
    scene.set_projection("orthographic", ortho_scale=ORTHO_SCALE)
    got = scene.host_lens_ray(pixels, half, half, abi.FILTER_BOX, 0.5).astype(np.float64)
    want_d = -(scene.array(capi.ARRAY_C2W, F).reshape(4, 4).T[:3, 2])
    if rotated:  # (the rows of section 4.9 step 4 applied to (0, 0, -1): c * 0 + c * 0 + c * -1)
        assert np.array_equal(got[:, 3:].astype(F), np.tile(want_d, (len(got), 1)))
    else:
        assert np.array_equal(got[:, 3:], np.tile([0.0, 0.0, -1.0], (len(got), 1)))
    rel = got[:, :3] - T[None, :]
    a, b, c = rel @ X, rel @ Y, rel @ Z
    pitch = ORTHO_SCALE / max(w, h)
    assert np.allclose(a, (pixels[:, 0] + 0.5 - w / 2) * pitch, rtol=1e-6, atol=1e-6 * ORTHO_SCALE)
    assert np.allclose(b, -(pixels[:, 1] + 0.5 - h / 2) * pitch, rtol=1e-6, atol=1e-6 * ORTHO_SCALE)
    assert np.abs(c).max() < 1e-6
    span = (a.max() - a.min() + pitch) if w >= h else (b.max() - b.min() + pitch)
    assert abs(span - ORTHO_SCALE) <= 1e-6 * ORTHO_SCALE
    # ... with a lens: |d| = 1 to 2 ulp, and every ray passes through its film point on the plane z = -F
    scene.set_lens(*LENS)
    rng = np.random.default_rng(w)
    u_lens = rng.random((len(pixels), 2), dtype=F)
    g = scene.host_lens_ray(pixels, half, u_lens, abi.FILTER_BOX, 0.5)
    assert _ulp_of_one(np.sqrt((g[:, 3:].astype(np.float64) ** 2).sum(1))).max() <= 2.0
    g = g.astype(np.float64)
    t = LENS[1] / -(g[:, 3:] @ Z)
    focus = g[:, :3] + g[:, 3:] * t[:, None]
    assert np.abs(focus - (got[:, :3] - LENS[1] * Z[None, :])).max() < 1e-5 * LENS[1]
    scene.set_lens(None)
    # panorama: the closed form's longitude and latitude, unit length, origin = the pinhole's, the film's centre along -z of c2w
    for window in ((-np.pi, np.pi, -np.pi / 2, np.pi / 2), WINDOW):
        if window is WINDOW:
            scene.set_projection("panorama", longitude_min=WINDOW[0], longitude_max=WINDOW[1], latitude_min=WINDOW[2], latitude_max=WINDOW[3])
        else:
            scene.set_projection("panorama")
        g = scene.host_lens_ray(pixels, half, half, abi.FILTER_BOX, 0.5)
        assert _ulp_of_one(np.sqrt((g[:, 3:].astype(np.float64) ** 2).sum(1))).max() <= 2.0
        g = g.astype(np.float64)
        assert np.abs(g[:, :3] - T[None, :]).max() <= 1e-6 * max(1.0, np.abs(T).max())
        lon, lat = cm.panorama_angles(w, h, pixels, window)
        dx, dy, dz = g[:, 3:] @ X, g[:, 3:] @ Y, g[:, 3:] @ Z
        got_lat = np.arctan2(dy, np.hypot(dx, dz))  # (well conditioned at the poles, where arcsin is not)
        assert np.abs(got_lat - lat).max() <= 1e-6
        away = np.cos(lat) > 1e-3  # (the longitude of a pole is not defined)
        dlon = np.angle(np.exp(1j * (np.arctan2(dx, -dz) - lon)))
        assert np.abs(dlon[away]).max() <= 1e-6
    # the film's centre (a film point, not a pixel centre, on an even film: pixel w / 2 with the box filter's u = 0 and radius 1)
    scene.set_projection("panorama")
    for proj in ("panorama", "orthographic"):
        scene.set_projection(proj, **({"ortho_scale": ORTHO_SCALE} if proj == "orthographic" else {}))
        px = np.array([[w // 2, h // 2]], np.uint32)
        u = np.array([[0.0 if w % 2 == 0 else 0.5, 0.0 if h % 2 == 0 else 0.5]], F)
        g = scene.host_lens_ray(px, u, u, abi.FILTER_BOX, 1.0).astype(np.float64)[0]
        assert np.abs(g[3:] + Z).max() <= 1e-6, proj
        if proj == "orthographic":
            assert np.abs(g[:3] - T).max() <= 1e-6 * max(1.0, np.abs(T).max())


# ---------------------------------------------------------------------------------------------------------------- 3. perspective is untouched
def test_perspective_is_untouched(hip_lib):
    w, h = 40, 32
    pixels, u_filter, u_lens = rows_of(w, h, 5)
    for rotated in (False, True):
        plain, scene = capi.Scene(None, _camera(w, h, rotated)), capi.Scene(None, _camera(w, h, rotated))
        cfg = make_config(spp=4)
        plan0 = plain.launch_plan(cfg)
        assert plan0["variant"]["lens"] == 0
        r2c, c2w = plain.array(capi.ARRAY_R2C, F), plain.array(capi.ARRAY_C2W, F)
        for how in ("default", "explicit", "None", "back"):
            if how == "explicit":
                scene.set_projection(abi.ProjectionData(type=abi.PROJECTION_PERSPECTIVE))
            elif how == "None":
                scene.set_projection(None)
            elif how == "back":
                scene.set_projection("orthographic", ortho_scale=3.0)
                fp = scene.features_plan(cfg, feat=False)
                assert fp["variant"]["lens"] == 1 and fp["kernel_compiled"] == 1
                assert scene.launch_plan(cfg)["variant"]["lens"] == 1
                scene.set_projection("panorama")
                fp = scene.features_plan(cfg, feat=False)
                assert fp["variant"]["lens"] == 1 and fp["kernel_compiled"] == 1
                scene.set_projection("perspective")
            assert scene.projection() == abi.ProjectionData()
            assert np.array_equal(scene.array(capi.ARRAY_R2C, F).view(np.uint32), r2c.view(np.uint32)), how
            for ft, fr in FILTERS:
                a, b = plain.host_lens_ray(pixels, u_filter, u_lens, ft, fr), scene.host_lens_ray(pixels, u_filter, u_lens, ft, fr)
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), how
            assert scene.launch_plan(cfg) == plan0, how
        # ... and both are the restated perspective camera, without and with a lens
        want = restated_pinhole(r2c, c2w, pixels, u_filter, 0.5)
        assert np.array_equal(scene.host_lens_ray(pixels, u_filter, u_lens, abi.FILTER_BOX, 0.5).view(np.uint32), want.view(np.uint32))
        scene.set_lens(0.05, 3.0)
        want = restated_lens(r2c, c2w, pixels, u_filter, u_lens, 0.5, 0.05, 3.0)
        assert np.array_equal(scene.host_lens_ray(pixels, u_filter, u_lens, abi.FILTER_BOX, 0.5).view(np.uint32), want.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------- 4. setter, getter, refusals
def _refused(scene, code, *a, **kw):
    before = (scene.projection(), scene.lens())
    with pytest.raises(capi.AkariError) as e:
        scene.set_projection(*a, **kw)
    assert e.value.code == code, (a, kw, str(e.value))
    assert (scene.projection(), scene.lens()) == before, (a, kw)  # a refused call changes nothing
    return str(e.value)


def test_setter_getter_and_refusals(hip_lib):
    pi, hpi = float(F(np.pi)), float(F(np.pi / 2))
    d = abi.ProjectionDesc()
    assert hip_lib.akr_projection_desc_default(C.byref(d)) == 0
    assert abi.ProjectionData.from_desc(d) == abi.ProjectionData() == abi.ProjectionData(abi.PROJECTION_PERSPECTIVE, 1.0, -pi, pi, -hpi, hpi)
    assert hip_lib.akr_projection_desc_default(None) == capi.ERR_INVALID_ARGUMENT
    hip_lib.akr_struct_size.restype = C.c_uint32
    assert hip_lib.akr_struct_size(26) == C.sizeof(abi.ProjectionDesc) == 24 and hip_lib.akr_struct_size(25) == 0 and hip_lib.akr_struct_size(27) == 0
    assert hip_lib.akr_struct_size(24) == 60 and hip_lib.akr_struct_size(16) == 8  # the earlier ids are what they were
    scene = capi.Scene(None, quad_scene())
    assert scene.projection() == abi.ProjectionData()
    scene.set_projection("orthographic", ortho_scale=2.5)
    assert scene.projection() == abi.ProjectionData(type=abi.PROJECTION_ORTHOGRAPHIC, ortho_scale=2.5)
    assert scene.to_scene_data().projection == scene.projection()
    assert capi.Scene(None, scene.to_scene_data()).projection() == scene.projection()
    want = abi.ProjectionData(abi.PROJECTION_PANORAMA, 1.0, float(F(-2.25)), 0.5, -0.375, 1.25)
    scene.set_projection(want)
    assert scene.projection() == want
    scene.set_projection("panorama", longitude_min=-pi, longitude_max=pi, latitude_min=-hpi, latitude_max=hpi)  # the bounds are inclusive
    assert scene.projection() == abi.ProjectionData(type=abi.PROJECTION_PANORAMA)
    up = float(np.nextafter(F(np.pi), F(4)))
    for bad in (dict(type=3), dict(type=0xffffffff),
                dict(type=1, ortho_scale=0.0), dict(type=1, ortho_scale=-1.0), dict(type=1, ortho_scale=np.nan), dict(type=1, ortho_scale=np.inf),
                dict(type=2, longitude_min=-up), dict(type=2, longitude_max=up), dict(type=2, longitude_min=1.0, longitude_max=1.0),
                dict(type=2, longitude_min=1.0, longitude_max=0.5), dict(type=2, longitude_min=np.nan), dict(type=2, longitude_max=np.inf),
                dict(type=2, latitude_min=-float(np.nextafter(F(np.pi / 2), F(2)))), dict(type=2, latitude_max=float(np.nextafter(F(np.pi / 2), F(2)))),
                dict(type=2, latitude_min=0.25, latitude_max=0.25), dict(type=2, latitude_min=0.5, latitude_max=-0.5), dict(type=2, latitude_max=np.nan),
                dict(type=2, latitude_min=-np.inf)):
        _refused(scene, capi.ERR_INVALID_ARGUMENT, abi.ProjectionData(**bad))
    scene.set_projection(None)  # NULL resets
    assert scene.projection() == abi.ProjectionData()
    # a panorama has no lens, whichever is set second; the state stays what it was
    scene.set_projection("panorama")
    with pytest.raises(capi.AkariError) as e:
        scene.set_lens(0.1, 2.0)
    assert e.value.code == capi.ERR_INVALID_ARGUMENT and "panorama" in str(e.value)
    assert scene.lens() is None and scene.projection() == abi.ProjectionData(type=abi.PROJECTION_PANORAMA)
    scene.set_lens(0.0, 0.0)  # (no lens is no lens)
    scene.set_projection("orthographic", ortho_scale=1.5)
    scene.set_lens(0.1, 2.0)
    assert "panorama" in _refused(scene, capi.ERR_INVALID_ARGUMENT, "panorama")
    assert scene.lens() == abi.LensData(float(F(0.1)), 2.0)
    sd = quad_scene()
    sd.projection, sd.lens = abi.ProjectionData(type=abi.PROJECTION_PANORAMA), abi.LensData(0.1, 2.0)
    with pytest.raises(capi.AkariError):
        capi.Scene(None, sd)


def test_reach_of_an_orthographic_film(hip_lib):
    """A tree's padding was sized for origins at the camera position: a film whose corners leave that magnitude is refused with the reach
    message; the same film is accepted on the exhaustive scene, whose pair walk checks every ray's origin itself."""
    sd = _camera_inside(grid_scene(n=12, seed=1), 0.3)
    with capi.options(force_bvh=1, instancing=0):
        tree = capi.Scene(None, sd)
    assert tree.info().uses_bvh == 1
    tree.set_projection("orthographic", ortho_scale=0.5)
    msg = _refused(tree, capi.ERR_INVALID_ARGUMENT, "orthographic", ortho_scale=4096.0)
    assert "padded" in msg and "ortho" in msg
    assert tree.projection().ortho_scale == 0.5
    small = quad_scene()
    exhaustive = capi.Scene(None, small)
    assert exhaustive.info().uses_bvh == 0
    exhaustive.set_projection("orthographic", ortho_scale=4096.0)
    assert exhaustive.projection().ortho_scale == 4096.0
    # the lens counts towards the reach of an orthographic film, and so does the film's shape
    scale = _largest_accepted(tree, lambda s: tree.set_projection("orthographic", ortho_scale=s))
    tree.set_projection("orthographic", ortho_scale=scale)
    with pytest.raises(capi.AkariError) as e:
        tree.set_lens(0.25 * scale, 2.0)
    assert e.value.code == capi.ERR_INVALID_ARGUMENT and "padded" in str(e.value)
    assert tree.lens() is None


def _largest_accepted(scene, setter, hi=4096.0):
    lo = 0.0
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        try:
            setter(mid)
            lo = mid
        except capi.AkariError as e:
            assert e.code == capi.ERR_INVALID_ARGUMENT and "padded" in str(e)
            hi = mid
    assert 0.0 < lo < 4096.0, lo
    return lo


# ---------------------------------------------------------------------------------------------------------------- 5. scene.json
def _with_camera(cbox_path, tmp_path, name, camera_type, **data):
    """scenes/cbox with another camera entry, in a directory of its own next to copies of the scene's buffers (the loader looks for them there)."""
    src = os.path.dirname(os.path.abspath(cbox_path))
    dst = tmp_path / name
    dst.mkdir()
    for f in os.listdir(src):
        if not f.endswith(".json") and os.path.isfile(os.path.join(src, f)):
            shutil.copy(os.path.join(src, f), dst / f)
    scene = json.load(open(cbox_path))
    cam = scene["camera"]
    cam["type"] = camera_type
    if camera_type != "perspective":
        cam["data"].pop("fov")
    cam["data"].update(data)
    path = dst / "scene.json"
    path.write_text(json.dumps(scene))
    return str(path)


def test_scene_json_reader(hip_lib, cbox_path, tmp_path):
    plain = capi.Scene(None, cbox_path)
    assert plain.projection() == abi.ProjectionData()
    same = capi.Scene(None, _with_camera(cbox_path, tmp_path, "persp", "perspective"))
    assert same.projection() == abi.ProjectionData()
    for which in (capi.ARRAY_R2C, capi.ARRAY_C2W, capi.ARRAY_WOOP, capi.ARRAY_SHADE):
        assert np.array_equal(same.array(which, np.uint32), plain.array(which, np.uint32))
    ortho = capi.Scene(None, _with_camera(cbox_path, tmp_path, "ortho", "orthographic", ortho_scale=0.75))
    assert ortho.projection() == abi.ProjectionData(type=abi.PROJECTION_ORTHOGRAPHIC, ortho_scale=0.75)
    info = ortho.info()
    assert (info.width, info.height) == (plain.info().width, plain.info().height)
    assert np.array_equal(ortho.array(capi.ARRAY_R2C, F).view(np.uint32), cm.ortho_r2c(info.width, info.height, 0.75).view(np.uint32))
    assert np.array_equal(ortho.array(capi.ARRAY_C2W, F), plain.array(capi.ARRAY_C2W, F))
    pano = capi.Scene(None, _with_camera(cbox_path, tmp_path, "pano", "panorama"))
    assert pano.projection() == abi.ProjectionData(type=abi.PROJECTION_PANORAMA)
    win = capi.Scene(None, _with_camera(cbox_path, tmp_path, "win", "panorama", longitude_min=-1.0, longitude_max=0.5, latitude_max=0.25))
    assert win.projection() == abi.ProjectionData(abi.PROJECTION_PANORAMA, 1.0, -1.0, 0.5, -float(F(np.pi / 2)), 0.25)
    for name, camera_type, data, code in (("nokey", "orthographic", {}, capi.ERR_PARSE), ("neg", "orthographic", {"ortho_scale": -1.0}, capi.ERR_PARSE),
                                          ("badwin", "panorama", {"longitude_min": 2.0, "longitude_max": 1.0}, capi.ERR_PARSE)):
        with pytest.raises(capi.AkariError) as e:
            capi.Scene(None, _with_camera(cbox_path, tmp_path, name, camera_type, **data))
        assert e.value.code == code, (name, str(e.value))
    with pytest.raises(capi.AkariError) as e:
        capi.Scene(None, _with_camera(cbox_path, tmp_path, "fisheye", "fisheye"))
    assert "unsupported camera type" in str(e.value)  # today's error


# ---------------------------------------------------------------------------------------------------------------- 6. conservative boxes
def _film_rim_rays(c2w, half_x, half_y):
    """A stand-in for bvh_model.adversarial_rays with its signature: the same rim targets, but every ray starts on a corner or an edge
    midpoint of the orthographic film, T + a c2w[0:3] + b c2w[4:7] -- the origins farthest from the camera position such a camera has."""
    c2w = np.asarray(c2w, dtype=np.float64)
    spots = np.array([(a, b) for a in (-1.0, 0.0, 1.0) for b in (-1.0, 0.0, 1.0) if (a, b) != (0.0, 0.0)])

    def rays(A, B, Cv, n, rng, reach, extent):
        q = _rim_targets(A, B, Cv, n, rng, reach)
        if q is None:
            return None, None
        ab = spots[rng.integers(0, len(spots), size=n)]
        o = (c2w[12:15][None, :] + half_x * ab[:, :1] * c2w[0:3][None, :] + half_y * ab[:, 1:] * c2w[4:7][None, :]).astype(F)
        d = q - o.astype(np.float64)
        return o, (d / np.linalg.norm(d, axis=1)[:, None]).astype(F)
    return rays


def _half_extents(scale, w, h):
    return (0.5 * scale, 0.5 * scale * h / w) if w > h else (0.5 * scale * w / h, 0.5 * scale)


@pytest.mark.parametrize("seed", [1, 2])
def test_boxes_are_conservative_for_film_rim_origins(hip_lib, monkeypatch, seed):
    """The trees are those of the perspective compile; akr_scene_set_projection accepts an orthographic film only while its origins stay inside
    the coordinate magnitude the padding was derived from. At the LARGEST scale it accepts: rays from the film's corners and edge midpoints
    aimed at triangle rims -- every pair the triangle test accepts passes every box on the way to the triangle's leaf."""
    sd = _camera_inside(grid_scene(n=12, seed=seed), 0.3 * seed)
    with capi.options(force_bvh=1, instancing=0):
        plain, scene = capi.Scene(None, sd), capi.Scene(None, sd)
    assert scene.info().uses_bvh == 1
    scale = _largest_accepted(scene, lambda s: scene.set_projection("orthographic", ortho_scale=s))
    with pytest.raises(capi.AkariError):
        scene.set_projection("orthographic", ortho_scale=scale * 1.01 + 1e-3)
    scene.set_projection("orthographic", ortho_scale=scale)
    for which, dt in ((capi.ARRAY_BVH_NODES, np.uint32), (capi.ARRAY_WOOP, F)):  # the projection changes no tree
        assert np.array_equal(scene.array(which, dt).view(np.uint32), plain.array(which, dt).view(np.uint32))
    info = scene.info()
    monkeypatch.setattr(bm, "adversarial_rays", _film_rim_rays(scene.array(capi.ARRAY_C2W, F), *_half_extents(scale, info.width, info.height)))
    accepted, culled, worst = bm.check_flattened(scene, 96, np.random.default_rng(seed))
    assert accepted > 2000, accepted
    assert culled == 0, (culled, accepted, worst[:5])


def test_kept_boxes_are_conservative_for_film_rim_origins(hip_lib, monkeypatch):
    sd = _camera_inside(instanced_scene(width=16, height=16, n_inst=4, n=3), 0.5)
    with capi.options(force_bvh=1, instancing=1):
        kept, plain = capi.Scene(None, sd), capi.Scene(None, sd)
    with capi.options(force_bvh=1, instancing=0):
        flat = capi.Scene(None, sd)
    assert kept.info().uses_bvh == 2
    scale = _largest_accepted(kept, lambda s: kept.set_projection("orthographic", ortho_scale=s))
    kept.set_projection("orthographic", ortho_scale=scale)
    for which, dt in ((capi.ARRAY_BVH_NODES, np.uint32), (capi.ARRAY_MESH_TRIS, F), (capi.ARRAY_INST_LEAVES, F)):
        assert np.array_equal(kept.array(which, dt).view(np.uint32), plain.array(which, dt).view(np.uint32))
    monkeypatch.setattr(bm, "adversarial_rays", _film_rim_rays(kept.array(capi.ARRAY_C2W, F), *_half_extents(scale, 16, 16)))
    accepted, culled, worst = bm.check_kept(kept, flat, 96, np.random.default_rng(3))
    assert accepted > 2000, accepted
    assert culled == 0, (culled, accepted, worst[:5])
