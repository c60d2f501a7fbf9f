"""The thin lens without a GPU: the ray definition restated in numpy f32 against the shared ray-generation text run on
the host (akr_host_lens_ray), the setter / getter / scene.json reader, and the conservativeness of the acceleration structure's boxes for
rays that start on the rim of the lens (following tests/bvh_model.py)."""
import ctypes as C
import os

import numpy as np
import pytest

from akari_render_amd import abi, capi
from oracle import pyoracle
from tests import bvh_model as bm
from tests.helpers import grid_scene, instanced_scene
from tests.test_environment import quad_scene

F = np.float32


# ---------------------------------------------------------------------------------------------------------------- the definition, restated
def _sincos(theta):
    """The project's sincos_f, through the oracle's known-answer entry (tests/test_math pins the two to each other)."""
    L = pyoracle.lib()
    s, c = np.zeros(len(theta), F), np.zeros(len(theta), F)
    a, b = C.c_float(), C.c_float()
    for i, t in enumerate(theta):
        L.or_kat_sincos(C.c_float(float(t)), C.byref(a), C.byref(b))
        s[i], c[i] = a.value, b.value
    return s, c


def _normalize(v):
    ln = np.sqrt(((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]).astype(F) + v[:, 2] * v[:, 2]).astype(F)).astype(F)
    inv = (F(1.0) / ln).astype(F)
    return (v * inv[:, None]).astype(F)


def _concentric_disk(u):
    s = (F(2.0) * u - F(1.0)).astype(F)
    sx, sy = s[:, 0], s[:, 1]
    big_x = np.abs(sx) > np.abs(sy)
    with np.errstate(all="ignore"):
        r = np.where(big_x, sx, sy).astype(F)
        th_x = (F(np.pi / 4) * (sy / sx).astype(F)).astype(F)
        th_y = (F(np.pi / 2) - (F(np.pi / 4) * (sx / sy).astype(F)).astype(F)).astype(F)
    theta = np.where(big_x, th_x, th_y).astype(F)
    zero = (sx == 0) & (sy == 0)
    theta = np.where(zero, F(0), theta).astype(F)
    sn, cs = _sincos(theta)
    ab = np.stack([(r * cs).astype(F), (r * sn).astype(F)], axis=1)
    ab[zero] = 0
    return ab


def _pinhole_dc(r2c, pixels, u_filter, filter_radius):
    """dc = normalize(r2c . (p_film, 0, 1) / w), box filter: p_film = pixel + 0.5 + (u - 0.5) * radius."""
    m = r2c.astype(F)
    off = ((u_filter - F(0.5)) * F(filter_radius)).astype(F)
    pf = ((pixels.astype(F) + F(0.5)).astype(F) + off).astype(F)
    x, y = pf[:, 0], pf[:, 1]

    def row(k):
        return ((((m[k] * x).astype(F) + (m[4 + k] * y).astype(F)).astype(F) + m[8 + k] * F(0.0)).astype(F) + m[12 + k] * F(1.0)).astype(F)

    q = np.stack([row(0), row(1), row(2)], axis=1)
    inv = (F(1.0) / row(3)).astype(F)
    return _normalize((q * inv[:, None]).astype(F))


def _rot(c, v):
    return np.stack([(((c[k] * v[:, 0]).astype(F) + (c[4 + k] * v[:, 1]).astype(F)).astype(F) + (c[8 + k] * v[:, 2]).astype(F)).astype(F) for k in range(3)], axis=1)


def _is_identity(c2w):
    return bool(np.all(np.abs(c2w - np.eye(4, dtype=F).reshape(16)) <= F(1e-4)))


def restated_pinhole(r2c, c2w, pixels, u_filter, filter_radius):
    d = _pinhole_dc(r2c, pixels, u_filter, filter_radius)
    o = np.zeros_like(d)
    if not _is_identity(c2w):
        c = c2w.astype(F)
        o[:] = (c[12:15] * (F(1.0) / c[15]).astype(F)).astype(F)
        d = _rot(c, d)
    return np.concatenate([o, d], axis=1)


def restated_lens(r2c, c2w, pixels, u_filter, u_lens, filter_radius, R, Fd):
    """DESIGN.md 4.9, line by line."""
    dc = _pinhole_dc(r2c, pixels, u_filter, filter_radius)
    ab = _concentric_disk(u_lens)
    l = np.stack([(F(R) * ab[:, 0]).astype(F), (F(R) * ab[:, 1]).astype(F), np.zeros(len(ab), F)], axis=1)
    ft = (F(Fd) / (-dc[:, 2])).astype(F)
    p_focus = (dc * ft[:, None]).astype(F)
    d = _normalize((p_focus - l).astype(F))
    o = l
    if not _is_identity(c2w):
        c = c2w.astype(F)

        def row(k):
            return ((((c[k] * l[:, 0]).astype(F) + (c[4 + k] * l[:, 1]).astype(F)).astype(F) + (c[8 + k] * l[:, 2]).astype(F)).astype(F) + c[12 + k] * F(1.0)).astype(F)

        inv = (F(1.0) / row(3)).astype(F)
        o = (np.stack([row(0), row(1), row(2)], axis=1) * inv[:, None]).astype(F)
        d = _rot(c, d)
    return np.concatenate([o, d], axis=1)


def _camera(width, height, rotated):
    sd = quad_scene(width=width, height=height, cam_z=3.0, fov=0.7)
    if rotated:
        a, b = 0.4, -0.25
        ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
        m = np.eye(4)
        m[:3, :3] = ry @ rx
        m[:3, 3] = [0.3, -0.2, 3.0]
        sd.camera.c2w = m.astype(F).T.reshape(16).copy()
    else:
        sd.camera.c2w = np.eye(4, dtype=F).reshape(16).copy()
    return sd


def _oracle_camera(sd):
    o = pyoracle.OracleScene(sd)
    r2c, c2w, ident = np.zeros(16, F), np.zeros(16, F), C.c_int32()
    pyoracle.lib().or_scene_camera(o.h, r2c.ctypes.data_as(C.POINTER(C.c_float)), c2w.ctypes.data_as(C.POINTER(C.c_float)), C.byref(ident))
    return r2c, c2w, bool(ident.value)


@pytest.mark.parametrize("rotated", [False, True], ids=["identity", "rotated"])
@pytest.mark.parametrize("size", [(48, 32), (24, 40)], ids=["landscape", "portrait"])
def test_ray_definition(hip_lib, size, rotated):
    w, h = size
    sd = _camera(w, h, rotated)
    r2c, c2w, ident = _oracle_camera(sd)
    assert ident == (not rotated) == _is_identity(c2w)
    scene = capi.Scene(None, sd)
    assert np.array_equal(scene.array(capi.ARRAY_R2C, F), r2c) and np.array_equal(scene.array(capi.ARRAY_C2W, F), c2w)
    rng = np.random.default_rng(11 + w + int(rotated))
    n = 3000
    pixels = np.stack([rng.integers(0, w, n), rng.integers(0, h, n)], axis=1).astype(np.uint32)
    u_filter, u_lens = rng.random((n, 2), dtype=F), rng.random((n, 2), dtype=F)
    # corners of the mapping: the centre (0, 0), both diagonals (|sx| == |sy|), the axes, the largest u
    u_lens[:8] = [[0.5, 0.5], [0.25, 0.25], [0.75, 0.25], [0.5, 0.1], [0.1, 0.5], [0.0, 0.0], [np.nextafter(F(1), F(0))] * 2, [0.5, 0.9]]
    radius = 0.8
    # no lens: the pinhole function is today's camera (the oracle's matrices, camera/mod.rs:70-103)
    assert scene.lens() is None
    got = scene.host_lens_ray(pixels, u_filter, u_lens, abi.FILTER_BOX, radius)
    want = restated_pinhole(r2c, c2w, pixels, u_filter, radius)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    for R, Fd in ((0.05, 3.0), (0.7, 1.25), (1e-3, 40.0)):
        scene.set_lens(R, Fd)
        got = scene.host_lens_ray(pixels, u_filter, u_lens, abi.FILTER_BOX, radius)
        want = restated_lens(r2c, c2w, pixels, u_filter, u_lens, radius, R, Fd)
        bad = np.flatnonzero(np.any(got.view(np.uint32) != want.view(np.uint32), axis=1))
        assert len(bad) == 0, (R, Fd, len(bad), got[bad[:3]], want[bad[:3]])
        assert not np.array_equal(got[:, :3], restated_pinhole(r2c, c2w, pixels, u_filter, radius)[:, :3])  # the origins do move
        # ... and every ray passes through the pinhole ray's point on the plane of focus (to rounding): what "focused at Fd" means
        pin = restated_pinhole(r2c, c2w, pixels, u_filter, radius).astype(np.float64)
        axis = -(c2w.reshape(4, 4).T[:3, 2]).astype(np.float64)
        t_pin = Fd / (pin[:, 3:] @ axis)
        focus = pin[:, :3] + pin[:, 3:] * t_pin[:, None]
        g = got.astype(np.float64)
        t = ((focus - g[:, :3]) * g[:, 3:]).sum(1)
        assert np.abs(g[:, :3] + g[:, 3:] * t[:, None] - focus).max() < 1e-5 * Fd
    scene.set_lens(0.0, 0.0)  # radius 0 is no lens
    assert scene.lens() is None
    got = scene.host_lens_ray(pixels, u_filter, u_lens, abi.FILTER_BOX, radius)
    assert np.array_equal(got.view(np.uint32), restated_pinhole(r2c, c2w, pixels, u_filter, radius).view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------- setter, getter, reader
def test_setter_getter_and_refusals(hip_lib):
    scene = capi.Scene(None, quad_scene())
    assert scene.lens() is None
    scene.set_lens(0.25, 3.5)
    assert scene.lens() == abi.LensData(0.25, 3.5)
    assert scene.to_scene_data().lens == abi.LensData(0.25, 3.5)
    for bad in ((-0.1, 1.0), (0.1, -1.0), (np.nan, 1.0), (0.1, np.inf), (np.inf, 1.0), (0.1, 0.0), (0.1, np.nan)):
        with pytest.raises(capi.AkariError) as e:
            scene.set_lens(*bad)
        assert e.value.code == capi.ERR_INVALID_ARGUMENT, bad
        assert scene.lens() == abi.LensData(0.25, 3.5), bad  # a refused call changes nothing
    scene.set_lens(None)
    assert scene.lens() is None
    scene.set_lens(0.0, 0.0)
    assert scene.lens() is None
    # a scene description that carries a lens: capi.Scene sets it
    sd = quad_scene()
    sd.lens = abi.LensData(0.125, 2.0)
    assert capi.Scene(None, sd).lens() == abi.LensData(0.125, 2.0)
    assert hip_lib.akr_struct_size(16) == C.sizeof(abi.LensDesc) == 8


def test_scene_json_reader(hip_lib, cbox_path):
    assert capi.get_option("lens") == 0  # the default: every file renders as the reference renders it
    assert capi.Scene(None, cbox_path).lens() is None
    with capi.options(lens=1):
        lens = capi.Scene(None, cbox_path).lens()
    assert lens is not None
    assert F(lens.radius) == F(10.0) / (F(2.0) * F(2.8)) and F(lens.focal_distance) == F(10.0)
    assert abs(lens.radius - 10.0 / 5.6) < 1e-6
    assert capi.Scene(None, cbox_path).lens() is None
    with pytest.raises(capi.AkariError):
        capi.set_option("lens", 2)


# ---------------------------------------------------------------------------------------------------------------- BVH padding
def _rim_targets(A, B, Cv, n, rng, reach):
    """Points within a few round-off widths of the edges and corners of triangle ABC (as tests/bvh_model.py adversarial_rays aims)."""
    e1, e2 = B - A, Cv - A
    nl = np.linalg.norm(np.cross(e1, e2))
    if not nl > 0:
        return None
    rim = 2.0 ** -24 * reach * max(np.linalg.norm(e1), np.linalg.norm(e2)) / nl
    w = 10.0 ** rng.uniform(-1.5, 2.0, size=n) * rim * rng.choice([-1.0, 1.0], size=n)
    s = rng.random(n)
    which = rng.integers(0, 3, size=n)
    u = np.where(which == 0, w, s)
    v = np.where(which == 0, s, np.where(which == 1, w, 1.0 - s + w))
    corner = rng.random(n) < 0.25
    u = np.where(corner, rng.choice([0.0, 1.0], size=n) + w, u)
    v = np.where(corner, np.where(u > 0.5, 0.0, rng.choice([0.0, 1.0], size=n)) + w * rng.choice([-1.0, 1.0], size=n), v)
    return A[None, :] + u[:, None] * e1[None, :] + v[:, None] * e2[None, :]


def _lens_rim_rays(c2w, R):
    """A stand-in for bvh_model.adversarial_rays with its signature: the same rim targets, but every ray starts on the RIM of the lens,
    T + R (cos phi c2w[0:3] + sin phi c2w[4:7]) -- the origins farthest from the camera position a lens ray can have."""
    c2w = np.asarray(c2w, dtype=np.float64)

    def rays(A, B, Cv, n, rng, reach, extent):
        q = _rim_targets(A, B, Cv, n, rng, reach)
        if q is None:
            return None, None
        phi = rng.uniform(0, 2 * np.pi, size=n)
        o = (c2w[12:15][None, :] + R * (np.cos(phi)[:, None] * c2w[0:3][None, :] + np.sin(phi)[:, None] * c2w[4:7][None, :])).astype(F)
        d = q - o.astype(np.float64)
        return o, (d / np.linalg.norm(d, axis=1)[:, None]).astype(F)
    return rays


def _largest_accepted_radius(scene, focal):
    lo, hi = 0.0, 64.0
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        try:
            scene.set_lens(mid, focal)
            lo = mid
        except capi.AkariError as e:
            assert e.code == capi.ERR_INVALID_ARGUMENT and "padded" in str(e)
            hi = mid
    scene.set_lens(lo, focal)
    return lo


def _camera_inside(sd, turn):
    """The scene with a turned camera at the middle of its box: the lens has room up to the box's largest coordinates."""
    with capi.options(force_bvh=1, instancing=0):
        first = capi.Scene(None, sd)
    w0 = bm._world_vertices(first.array(capi.ARRAY_SHADE, F).reshape(-1, 32), first.array(capi.ARRAY_INSTANCES, F).reshape(-1, 32)).reshape(-1, 3)
    m = np.eye(4)
    a, b = turn, -0.2
    m[:3, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]) @ np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    m[:3, 3] = 0.5 * (w0.min(0) + w0.max(0))
    sd.camera.c2w = m.astype(F).T.reshape(16).copy()
    return sd


@pytest.mark.parametrize("seed", [1, 2])
def test_boxes_are_conservative_for_lens_rim_origins(hip_lib, monkeypatch, seed):
    """The trees are those of the lens-less compile; akr_scene_set_lens accepts a lens only while the origins on its disk stay inside the
    coordinate magnitude the padding was derived from. At the LARGEST radius it accepts: rays from the rim of the lens aimed at triangle
    rims -- every pair the triangle test accepts passes every box on the way to the triangle's leaf (tests/bvh_model.py check_flattened)."""
    sd = _camera_inside(grid_scene(n=12, seed=seed), 0.3 * seed)
    with capi.options(force_bvh=1, instancing=0):
        plain = capi.Scene(None, sd)
        scene = capi.Scene(None, sd)
    assert scene.info().uses_bvh == 1
    R = _largest_accepted_radius(scene, 2.0)
    assert 0.0 < R < 64.0, R
    with pytest.raises(capi.AkariError):
        scene.set_lens(R * 1.01 + 1e-3, 2.0)
    scene.set_lens(R, 2.0)
    for which, dt in ((capi.ARRAY_BVH_NODES, np.uint32), (capi.ARRAY_WOOP, F)):  # the lens changes no tree
        assert np.array_equal(scene.array(which, dt).view(np.uint32), plain.array(which, dt).view(np.uint32))
    monkeypatch.setattr(bm, "adversarial_rays", _lens_rim_rays(scene.array(capi.ARRAY_C2W, F), R))
    accepted, culled, worst = bm.check_flattened(scene, 96, np.random.default_rng(seed))
    assert accepted > 2000, accepted
    assert culled == 0, (culled, accepted, worst[:5])


def test_kept_boxes_are_conservative_for_lens_rim_origins(hip_lib, monkeypatch):
    """The same on a scene kept as meshes + instances, whose per-mesh paddings come from the per-axis magnitudes: the top-level
    boxes on the world ray and the mesh's boxes on the ray taken through the instance's inverse (tests/bvh_model.py check_kept), 0 culled."""
    sd = instanced_scene(width=16, height=16, n_inst=4, n=3)
    with capi.options(force_bvh=1, instancing=1):
        outside = capi.Scene(None, sd)  # the helper's own camera stands outside the box, tilted: no radius is accepted
        with pytest.raises(capi.AkariError) as e:
            outside.set_lens(0.5, 2.0)
        assert e.value.code == capi.ERR_INVALID_ARGUMENT and "padded" in str(e.value)
    sd = _camera_inside(sd, 0.5)
    with capi.options(force_bvh=1, instancing=1):
        kept = capi.Scene(None, sd)
        plain = capi.Scene(None, sd)
    with capi.options(force_bvh=1, instancing=0):
        flat = capi.Scene(None, sd)
    assert kept.info().uses_bvh == 2
    R = _largest_accepted_radius(kept, 2.0)
    assert R > 0.0
    for which, dt in ((capi.ARRAY_BVH_NODES, np.uint32), (capi.ARRAY_MESH_TRIS, F), (capi.ARRAY_INST_LEAVES, F)):
        assert np.array_equal(kept.array(which, dt).view(np.uint32), plain.array(which, dt).view(np.uint32))
    monkeypatch.setattr(bm, "adversarial_rays", _lens_rim_rays(kept.array(capi.ARRAY_C2W, F), R))
    accepted, culled, worst = bm.check_kept(kept, flat, 96, np.random.default_rng(3))
    assert accepted > 2000, accepted
    assert culled == 0, (culled, accepted, worst[:5])
