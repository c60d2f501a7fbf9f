"""Soft shadows on the GPU (csrc/device/dpunct.h, the PUNCT kernels): the device probe against the numpy restatement bit for bit, lights of
size 0 against the films the delta lights gave before they could have a size, penumbrae of each kind against a float64 quadrature over the disk / the
cap with the blocker's straight edges found analytically, the small-radius limit, a soft spot whose cone edge crosses the floor, tile shards and
akari-cli."""
import dataclasses
import hashlib
import json
import math
import os
import subprocess

import numpy as np
import pytest

from akari_render_amd import abi, capi
from tests import soft_light_model as sm
from tests.helpers import make_config, n_bit_diff
from tests.test_environment import quad_scene
from tests.test_gpu_punctual import CLOSED, PUNCT_BIT, RHO, centre_cfg, closed_form, pixel_points, render
from tests.test_punctual import assert_rows_equal, json_light, light_table, point, scene_with, spot, sun, write_scene_with_lights
from tests.test_punctual import as_dict as delta_dict
from tests.test_soft_lights import KINDS, edge_rows9, model_records, random_rows9, sizes, soft, soft_json_light

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "soft_lights_delta_films.json")


# ---------------------------------------------------------------------------------------------------------------- 1. probe
@pytest.mark.parametrize("which", [0, 1, 2, 3], ids=["small", "large", "tiny", "huge"])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_probe_equals_the_model_bit_for_bit(ctx, kind, which):
    base = KINDS[kind]
    light = soft(base, (sizes(base) + sizes(base, edge=True))[which])
    sc = scene_with([light], ctx)
    rows = np.concatenate([random_rows9(4096, 21 + which), edge_rows9(light)])
    got = sc.probe_light_sample_soft(rows)
    assert_rows_equal(got, sm.light_sample_rows(light_table(sc), model_records(sc), rows))
    assert_rows_equal(got, sc.host_light_sample_soft(rows))


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_probe_of_size_zero_is_the_old_probe(ctx, kind):
    sc = scene_with([KINDS[kind]], ctx)
    rows = np.concatenate([random_rows9(4096, 31), edge_rows9(KINDS[kind])])
    assert_rows_equal(sc.probe_light_sample_soft(rows), sc.probe_light_sample(rows[:, :7]))


# ---------------------------------------------------------------------------------------------------------------- 2. size 0 is the delta light
def blocker_scene(lights, xa=0.0, xb=0.3, hb=0.5, blocker=True):
    """quad_scene's floor (z = 0, albedo RHO) and over it a black strip xa <= x <= xb, |y| <= 3 at z = hb: two straight edges along y"""
    sd = quad_scene(albedo=RHO)
    if blocker:
        bv = np.array([[xa, -3.0, hb], [xb, -3.0, hb], [xb, 3.0, hb], [xa, 3.0, hb]], np.float32)
        sd.meshes.append(abi.MeshData(vertices=bv, indices=np.array([[0, 1, 2], [0, 2, 3]], np.uint32)))
        sd.materials.append(abi.MaterialData(kind=abi.MAT_DIFFUSE, base_color=(0.0, 0.0, 0.0)))
        sd.instances.append(abi.InstanceData(1, [1], np.eye(4, dtype=np.float32).reshape(16).copy()))
    sd.lights = list(lights)
    return sd


DELTA_CFG = dict(spp=16, max_depth=4, sampler_seed=5)


def delta_film_hashes(ctx):
    """sha256 of the raw film of the blocker scene lit by each delta light of test_gpu_punctual's CLOSED, exhaustive and through the tree. Uses nothing a
    library without soft lights lacks: tests/golden/soft_lights_delta_films.json holds what the library answered before lights could have a size."""
    out = {}
    for kind in ("point", "spot_blend", "spot_step", "sun"):
        for force_bvh in (0, 1):
            with capi.options(force_bvh=force_bvh):
                sc = capi.Scene(ctx, blocker_scene([CLOSED[kind]]))
            film = capi.Film(ctx, 32, 32)
            capi.pt_render(ctx, sc, make_config(**DELTA_CFG), film)
            out[f"{kind}/{'bvh' if force_bvh else 'exhaustive'}"] = hashlib.sha256(film.read().tobytes()).hexdigest()
    return out


def test_size_zero_films_are_the_films_of_the_unextended_lights(ctx):
    want = json.load(open(GOLDEN))["films"]
    got = delta_film_hashes(ctx)
    assert sorted(got) == sorted(want) and len(got) == 8
    assert got == want, [k for k in got if got[k] != want[k]]


@pytest.mark.parametrize("force_bvh", [0, 1], ids=["exhaustive", "bvh"])
def test_explicit_zero_and_ignored_sizes_change_no_film(ctx, force_bvh):
    """radius = 0 / angle = 0 given explicitly, and the size the kind does not read, against the light built without naming either"""
    films = []
    for variant in (lambda l: l, lambda l: dataclasses.replace(l, radius=0.0, angle=0.0),
                    lambda l: dataclasses.replace(l, **({"radius": 0.5} if l.type == abi.LIGHT_SUN else {"angle": 0.5}))):
        with capi.options(force_bvh=force_bvh):
            sc = capi.Scene(ctx, blocker_scene([variant(CLOSED[k]) for k in ("point", "spot_blend", "sun")]))
        film = capi.Film(ctx, 32, 32)
        capi.pt_render(ctx, sc, make_config(**DELTA_CFG), film)
        films.append(film.read())
    assert films[0].any() and n_bit_diff(films[0], films[1]) == 0 and n_bit_diff(films[0], films[2]) == 0


@pytest.mark.parametrize("sampler", [abi.SAMPLER_INDEPENDENT, abi.SAMPLER_PMJ02BN, abi.SAMPLER_SOBOL], ids=["independent", "pmj02bn", "sobol"])
def test_a_soft_light_takes_no_sampler_dimension(ctx, sampler):
    """one soft and one delta light against the two delta lights: other radiance, the same sampler states and counters"""
    out = []
    for radius in (0.0, 0.3):
        sc = capi.Scene(ctx, blocker_scene([dataclasses.replace(CLOSED["point"], radius=radius), CLOSED["sun"]], blocker=False))
        film = capi.Film(ctx, 32, 32)
        se = capi.PtSession(ctx, sc, make_config(sampler_type=sampler, **DELTA_CFG), film)
        se.passes(1, blocking=True)
        assert se.kernel_info()["kernel_flags"] & PUNCT_BIT
        states = se.sampler_states(32 * 32)
        st = se.end()
        out.append((film.read(), states, {k: v for k, v in st.items() if k.startswith("n_")}))
    assert np.array_equal(out[0][1], out[1][1]) and out[0][2] == out[1][2] and out[0][2]["n_samples"] == 32 * 32 * 16
    assert n_bit_diff(out[0][0], out[1][0]) > 0


# ---------------------------------------------------------------------------------------------------------------- 3. penumbrae
# The reference. A sample's value at the floor point P (normal +z, albedo RHO, depth 1, the only light, so pdf = 1 and no MIS weight) is
#   X = RHO / pi * max(wi.z, 0) * li(y) * V(P, y),
# y uniform over the disk (the concentric warp preserves area) or wi uniform over the cap. The pixel's mean is E[X] and its variance (E[X^2] - E[X]^2) / n
# for the n independent samples of the independent sampler. Both moments come from a float64 quadrature in which the blocker's two straight edges are not
# sampled but solved for: a segment from P to y passes the plane z = hb at x = P.x + hb (y.x - P.x) / (y.z - P.z), and x - x_e has the sign of
#   G_e(y) = hb (y.x - P.x) - (x_e - P.x) y.z            (y.z > 0, P.z = 0),
# which is linear in y: on a chord of the disk it has one root, on a ring of the cap G_e = R cos(phi - phi0) + gamma has two. Each chord / ring is cut at
# those roots and every piece, on which V is constant and X smooth, gets Gauss-Legendre nodes of its own; V is evaluated at the nodes, strictly inside.
GL_X, GL_W = np.polynomial.legendre.leggauss(12)


def pieces_nodes(ends):
    """ends (..., K + 1) sorted -> nodes (..., K, 12) and weights (..., K, 12) of Gauss-Legendre on each of the K intervals"""
    lo, hi = ends[..., :-1, None], ends[..., 1:, None]
    return lo + (hi - lo) * (GL_X + 1) / 2, (hi - lo) / 2 * GL_W


def moments(wt, h, V):
    """E[X], E[X^2] and the visible fraction: exactly 0 where no node of a piece of positive length sees the light, exactly 1 where every one does"""
    live = wt > 1e-15 * wt.max()
    frac = np.sum(wt * V, axis=(1, 2, 3))
    frac = np.where(np.all((V == 1) | ~live, axis=(1, 2, 3)), 1.0, np.where(np.all((V == 0) | ~live, axis=(1, 2, 3)), 0.0, np.clip(frac, 1e-12, 1 - 1e-12)))
    return np.sum(wt * h * V, axis=(1, 2, 3)), np.sum(wt * h * h * V, axis=(1, 2, 3)), frac


def spot_f64(rec, ct):
    inv, co = float(rec["inv_span"]), float(rec["cos_o"])
    if inv == 0.0:
        return (ct > co).astype(np.float64)
    s = np.clip((ct - co) * inv, 0.0, 1.0)
    return s * s * (3 - 2 * s)


def disk_reference(light, P, edges=None, hb=0.5, outer=96):
    """first and second moment of X / colour and the visible fraction of the disk at the floor points P (m, 3), float64; edges = (xa, xb) of the strip"""
    rec = sm.fold(dict(delta_dict(light), radius=light.radius, angle=0.0))
    q, r = rec["q"].astype(np.float64), float(rec["radius"])
    nd = (P - q) / np.linalg.norm(P - q, axis=1, keepdims=True)
    e1 = np.cross(nd, [0.0, 1.0, 0.0])
    e1 /= np.linalg.norm(e1, axis=1, keepdims=True)
    e2 = np.cross(nd, e1)
    gx, gw = np.polynomial.legendre.leggauss(outer)
    phi = gx * (math.pi / 2)
    b, A, wb = np.sin(phi), np.cos(phi), gw * (math.pi / 2) * np.cos(phi)  # b = sin(phi): the chord's half-length A = cos(phi) is smooth in phi
    m = P.shape[0]
    ends = [np.broadcast_to(-A, (m, outer)), np.broadcast_to(A, (m, outer))]
    coef = []
    for xe in edges or ():
        c = np.stack([np.full(m, hb), np.zeros(m), -(xe - P[:, 0])], axis=1)
        g0 = c @ q - hb * P[:, 0]
        alpha, beta = r * np.sum(c * e1, axis=1), r * np.sum(c * e2, axis=1)
        assert np.all(np.abs(alpha) > 1e-9)
        root = -(g0[:, None] + beta[:, None] * b[None, :]) / alpha[:, None]
        ends.append(np.clip(root, -A, A))
        coef.append(c)
    ends = np.sort(np.stack(ends, axis=-1), axis=-1)
    a, wa = pieces_nodes(ends)  # (m, outer, K, 12)
    y = q + r * (a[..., None] * e1[:, None, None, None, :] + b[None, :, None, None, None] * e2[:, None, None, None, :])
    w = y - P[:, None, None, None, :]
    dist2 = np.sum(w * w, axis=-1)
    wi = w / np.sqrt(dist2)[..., None]
    cosl = -np.sum(wi * nd[:, None, None, None, :], axis=-1)
    h = RHO / math.pi * np.maximum(wi[..., 2], 0.0) * cosl / dist2
    if light.type == abi.LIGHT_SPOT:
        h = h * spot_f64(rec, -(wi @ rec["a"].astype(np.float64)))
    V = np.ones_like(h)
    if edges:
        G = [coef[k][:, 0, None, None, None] * (y[..., 0] - P[:, 0, None, None, None]) + coef[k][:, 2, None, None, None] * y[..., 2] for k in range(2)]
        yc = P[:, 1, None, None, None] + hb / y[..., 2] * (y[..., 1] - P[:, 1, None, None, None])
        assert np.all(np.abs(yc) < 3.0)  # the strip's ends are out of reach: only its two long edges matter
        V = 1.0 - ((G[0] >= 0) & (G[1] <= 0))
    wt = wa * wb[None, :, None, None] / math.pi
    return moments(wt, h, V)


def cap_reference(light, P, edges=None, hb=0.5, outer=96):
    """the same for a sun of angle light.angle: wi uniform over the cap, li = colour * k"""
    rec = sm.fold(dict(delta_dict(light), radius=0.0, angle=light.angle))
    n = -rec["a"].astype(np.float64)
    n /= np.linalg.norm(n)
    t = np.cross(n, [0.0, 1.0, 0.0])
    t /= np.linalg.norm(t)
    s = np.cross(n, t)
    cm = math.cos(0.5 * float(np.float32(light.angle)))
    gx, gw = np.polynomial.legendre.leggauss(outer)
    ct = 1 - (gx + 1) / 2 * (1 - cm)
    st, wo = np.sqrt(1 - ct * ct), gw / 2
    m = P.shape[0]
    ends = [np.zeros((m, outer)), np.full((m, outer), 2 * math.pi)]
    coef = []
    for xe in edges or ():
        c = np.stack([np.full(m, hb), np.zeros(m), -(xe - P[:, 0])], axis=1)
        R = st[None, :] * np.hypot(c @ t, c @ s)[:, None]
        gamma = ct[None, :] * (c @ n)[:, None]
        phi0 = np.arctan2(c @ s, c @ t)[:, None]
        with np.errstate(invalid="ignore", divide="ignore"):
            d = np.arccos(np.clip(-gamma / R, -1.0, 1.0))
        has = np.abs(gamma) < R
        for sign in (1.0, -1.0):
            ends.append(np.where(has, np.mod(phi0 + sign * d, 2 * math.pi), 0.0))
        coef.append(c)
    ends = np.sort(np.stack(ends, axis=-1), axis=-1)
    ph, wp = pieces_nodes(ends)  # (m, outer, K, 12)
    wi = (st[None, :, None, None, None] * (np.cos(ph)[..., None] * t + np.sin(ph)[..., None] * s) + ct[None, :, None, None, None] * n)
    h = RHO / math.pi * np.maximum(wi[..., 2], 0.0) * float(rec["k"]) + 0 * ph
    V = np.ones_like(h)
    if edges:
        G = [coef[k][:, 0, None, None, None] * wi[..., 0] + coef[k][:, 2, None, None, None] * wi[..., 2] for k in range(2)]
        assert np.all(np.abs(P[:, 1, None, None, None] + hb * wi[..., 1] / wi[..., 2]) < 3.0) and np.all(wi[..., 2] > 0)
        V = 1.0 - ((G[0] >= 0) & (G[1] <= 0))
    wt = wp * wo[None, :, None, None] / (2 * math.pi)
    return moments(wt, h, V)


def reference(light, P, edges=None):
    P = np.array(P, np.float64)
    P[:, 2] = 0.0  # (the floor; the camera text leaves a rounding of it)
    return (cap_reference if light.type == abi.LIGHT_SUN else disk_reference)(light, P, edges)


def colour(light):
    return np.asarray(light.color, np.float32).astype(np.float64) * float(np.float32(light.strength))


N_SPP = 256
FLOAT_SLOP = 1e-5  # the relative error of the float32 chain li * f * cos / pdf itself: the rtol test_gpu_punctual's closed forms hold every pixel to


def check_against_quadrature(img, light, P, m1, m2, what):
    """every value within 5 standard errors (+ the float32 chain's own error) of the quadrature's mean; returns the worst excess for the log"""
    c = colour(light)
    mean, var = m1[..., None] * c, np.maximum(m2 - m1 * m1, 0.0)[..., None] * c * c
    se = np.sqrt(var / N_SPP)
    err = np.abs(img.astype(np.float64) - mean)
    allowed = 5 * se + FLOAT_SLOP * mean
    z = err[se > 0] / se[se > 0]
    print(f"{what}: worst |mean - reference| / standard error = {z.max():.2f}, median {np.median(z):.2f} over {z.size} values; median relative standard error {np.median(se[mean > 0] / mean[mean > 0]):.3g}")
    assert np.all(err <= allowed), f"{what}: {int(np.sum(err > allowed))} values beyond 5 standard errors, worst {float(np.max(err / np.maximum(allowed, 1e-300))):.2f} x the allowance"


def penumbra_light(kind):
    """the three lights of the penumbra tests; the strip XA <= x <= XB at z = HB is placed so that the camera sees an umbra and one whole penumbra of each"""
    return {"point": soft(point(position=(-0.6, 0.0, 2.0), color=(1.0, 0.8, 0.6), strength=5.0), 0.4),
            "spot": soft(spot(position=(-0.6, 0.0, 2.0), direction=(1.0, 0.0, -2.0), cone_angle=0.7, blend=0.5, color=(1.0, 0.8, 0.6), strength=5.0), 0.4),
            "sun": soft(sun(direction=(0.8, 0.0, -1.0), color=(1.0, 0.8, 0.6), strength=2.0), 0.3)}[kind]


PENUMBRA_KINDS = ("point", "spot", "sun")
XA, XB, HB = 0.0, 0.3, 0.5


def soft_cfg(seed=11, **kw):
    return centre_cfg(spp=N_SPP, sampler_type=abi.SAMPLER_INDEPENDENT, sampler_seed=seed, **kw)


@pytest.mark.parametrize("kind", PENUMBRA_KINDS)
def test_penumbra(ctx, kind):
    light = penumbra_light(kind)
    open_scene, blocked = capi.Scene(ctx, blocker_scene([light], blocker=False)), capi.Scene(ctx, blocker_scene([light], XA, XB, HB))
    a, b = render(ctx, open_scene, soft_cfg()), render(ctx, blocked, soft_cfg())
    x = pixel_points(open_scene)
    at_hb = pixel_points(open_scene, HB)[..., 0]
    sees_blocker = (at_hb >= XA - 1e-4) & (at_hb <= XB + 1e-4)  # every camera ray goes through its pixel's centre: the pixels whose ray meets the strip
    assert 0 < sees_blocker.mean() < 0.25
    keep = ~sees_blocker
    P = x[keep]
    m1, m2, frac = reference(light, P, (XA, XB))
    img = b[keep]
    umbra, full = frac == 0, frac == 1
    partial = ~umbra & ~full
    cols = np.zeros((32, 32), bool)
    cols[keep] = partial
    n_cols = int(cols.any(axis=0).sum())
    print(f"penumbra of the {kind}: {int(umbra.sum())} pixels in the umbra, {int(partial.sum())} in the penumbra over {n_cols} columns, {int(full.sum())} fully lit, {int(sees_blocker.sum())} left out")
    assert umbra.sum() >= 16 and full.sum() > 300 and n_cols >= 3
    assert np.all(img[umbra] == 0), "light where the whole disk is hidden"
    assert n_bit_diff(a[keep][full], img[full]) == 0, "a pixel that sees the whole disk differs from the unblocked render"
    check_against_quadrature(img, light, P, m1, m2, f"penumbra of the {kind}")
    # the unblocked render against the unblocked quadrature, every pixel
    u1, u2, _ = reference(light, x.reshape(-1, 3))
    check_against_quadrature(a.reshape(-1, 3), light, x.reshape(-1, 3), u1, u2, f"unblocked {kind}")
    # and the penumbra is one: between the hard shadow's two values
    mid = img[partial][:, 0] / a[keep][partial][:, 0]
    assert 0.2 < np.mean((mid > 0.05) & (mid < 0.95))


def test_reference_quadrature_converges():
    """the reference itself (no GPU work): a rule of four times as many chords / rings moves no pixel's mean by more than a fiftieth of ONE standard error
    of the N_SPP samples, and no second moment by more than 1e-3 of itself; it finds the same umbra and the same fully lit points"""
    pts = np.stack(np.meshgrid(np.linspace(-0.9, 0.9, 32), np.linspace(-0.9, 0.9, 5), [0.0]), -1).reshape(-1, 3)
    for light in map(penumbra_light, PENUMBRA_KINDS):
        fn, outer = (cap_reference, 96) if light.type == abi.LIGHT_SUN else (disk_reference, 96)
        used, fine = fn(light, pts, (XA, XB), HB), fn(light, pts, (XA, XB), HB, outer=4 * outer)
        se = np.sqrt(np.maximum(fine[1] - fine[0] ** 2, 0.0) / N_SPP)
        assert np.all(np.abs(used[0] - fine[0]) <= 0.02 * se) and np.all(np.abs(used[1] - fine[1]) <= 1e-3 * fine[1])
        assert np.array_equal(used[2] == 0, fine[2] == 0) and np.array_equal(used[2] == 1, fine[2] == 1)
        assert (used[2] == 0).sum() >= 5 and (used[2] == 1).sum() >= 50 and ((used[2] > 0) & (used[2] < 1)).sum() >= 15


# ---------------------------------------------------------------------------------------------------------------- 4. the small-radius limit
def test_small_radius_tends_to_the_delta_light(ctx):
    """An unblocked point light of radius 1e-3 two units over the floor against the delta light's closed form rho / pi cos I / d^2.

    The bound. With y = q + r (a e1 + b e2) on the disk that faces P and d = |q - P|: |y - P|^2 = d^2 + r^2 s^2 (s^2 = a^2 + b^2 <= 1), cosl = d / |y - P|,
    wi.z = y.z / |y - P|, so X = rho / pi I y.z d / (d^2 + r^2 s^2)^2. y.z = q.z + r (a e1.z + b e2.z); its second term is odd in (a, b), the rest even, so it
    integrates to nothing over the disk: E[X] = L0 E[(1 + (r s / d)^2)^-2] with L0 the closed form, and 1 - 2 (r / d)^2 <= E[X] / L0 <= 1. d >= 2 here."""
    r = 1e-3
    light = soft(point(position=(0.0, 0.0, 2.0), color=(1.0, 0.8, 0.6), strength=5.0), r)
    sc = capi.Scene(ctx, blocker_scene([light], blocker=False))
    img = render(ctx, sc, soft_cfg(seed=12)).astype(np.float64)
    x = pixel_points(sc)
    L0 = closed_form(dataclasses.replace(light, radius=0.0), x)
    m1, m2, _ = disk_reference(light, x.reshape(-1, 3))
    se = np.sqrt(np.maximum(m2 - m1 * m1, 0.0) / N_SPP).reshape(32, 32, 1) * colour(light)
    d = np.linalg.norm(x - np.asarray(light.position), axis=-1)
    assert d.min() >= 2.0
    allowed = 2 * (r / d[..., None]) ** 2 * L0 + 5 * se + FLOAT_SLOP * L0
    err = np.abs(img - L0)
    print(f"small radius: worst |render - closed form| / closed form = {float(np.max(err / L0)):.3g}; the allowance there is at least {float(np.min(allowed / L0)):.3g}")
    assert np.all(err <= allowed)
    assert float(np.max(allowed / L0)) < 1e-3  # the allowance is no loophole: a light ten times the size would not pass as a point


# ---------------------------------------------------------------------------------------------------------------- 5. a soft spot's cone edge
def test_soft_spot_whose_cone_edge_crosses_the_floor(ctx):
    """test_gpu_punctual's tilted blended spot with a radius: the falloff is taken at the sampled direction, so the edge is blurred by the disk. The
    falloff's float32 argument (ct - cos_o) inv_span carries at most eight roundings of values <= 1 (the reciprocal of the distance and its three products,
    three products and two sums of the dot, the difference), 2^-25 each, and smoothstep's slope is at most 1.5 inv_span: the falloff differs from float64's
    by less than df = 1.5 inv_span 8 2^-25 absolute, and the allowance gets df times the mean the same light would give without a falloff."""
    light = soft(CLOSED["spot_blend"], 0.1)
    sc = capi.Scene(ctx, blocker_scene([light], blocker=False))
    img = render(ctx, sc, soft_cfg(seed=13))
    x = pixel_points(sc).reshape(-1, 3)
    m1, m2, _ = disk_reference(light, x)
    no_falloff = disk_reference(dataclasses.replace(light, type=abi.LIGHT_POINT), x)[0]
    rec = sm.fold(dict(delta_dict(light), radius=light.radius, angle=0.0))
    df = 1.5 * float(rec["inv_span"]) * 8 * 2.0 ** -25
    c = colour(light)
    mean, se = m1[:, None] * c, np.sqrt(np.maximum(m2 - m1 * m1, 0.0) / N_SPP)[:, None] * c
    err = np.abs(img.reshape(-1, 3).astype(np.float64) - mean)
    allowed = 5 * se + FLOAT_SLOP * mean + df * no_falloff[:, None] * c
    inside, outside = m1 > 0.5 * no_falloff, m1 == 0
    print(f"soft spot: {int(inside.sum())} pixels mostly inside the cone, {int(outside.sum())} wholly outside, {int((~inside & ~outside).sum())} across the edge; "
          f"worst excess {float(np.max(err / allowed)):.2f} x the allowance")
    assert inside.sum() > 20 and outside.sum() > 20 and (~inside & ~outside).sum() > 20
    assert np.all(err <= allowed)
    # with the falloff at the light's centre instead, the pixels across the edge would differ: what the delta light's falloff gives there
    hard = closed_form(dataclasses.replace(light, radius=0.0), x)
    assert np.sum(np.abs(hard - mean) > allowed + 5 * se) > 10


# ---------------------------------------------------------------------------------------------------------------- 6. shards, 7. akari-cli
def test_sharded_render_assembles_to_the_unsharded_film(ctx):
    sd = blocker_scene([penumbra_light("spot"), penumbra_light("sun")], XA, XB, HB)
    sd.camera.height = 64
    sc = capi.Scene(ctx, sd)
    base = dict(spp=8, max_depth=3, sampler_seed=9, tile_w=16, tile_h=16)
    whole = capi.Film(ctx, 32, 64)
    capi.pt_render(ctx, sc, make_config(**base), whole)
    parts = np.zeros_like(whole.read())
    for rank in range(2):
        f = capi.Film(ctx, 32, 64)
        se = capi.PtSession(ctx, sc, make_config(shard_rank=rank, shard_count=2, **base), f)
        se.passes(1, blocking=True)
        assert se.kernel_info()["kernel_flags"] & PUNCT_BIT
        se.end()
        part = f.read()
        assert np.count_nonzero(part) > 0 and np.count_nonzero(parts[part != 0]) == 0
        parts += part
    assert n_bit_diff(parts, whole.read()) == 0


def test_cli(ctx, tmp_path):
    from akari_render_amd import build
    cli = build.build_cli()
    lights = [soft(point(position=(0.3, -0.2, 1.5)), 0.25), soft(sun(direction=(0.3, -0.2, -1.0), strength=0.5), 0.25)]
    method = {"method": {"type": "pt", "spp": 4, "spp_per_pass": 4, "max_depth": 2}, "sampler": {"type": "independent", "seed": 1}, "film": {"out": str(tmp_path / "out.exr")}}
    mpath = tmp_path / "pt.json"
    mpath.write_text(json.dumps(method))

    def cli_bytes(spath, *flags):
        res = subprocess.run([cli, "-s", spath, "-m", str(mpath), *flags], cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stderr
        return open(tmp_path / "out.exr", "rb").read()

    def api_bytes(spath, name):
        film = capi.Film(ctx, 16, 16)
        cfg, _ = capi.config_from_json(json.dumps(method))
        capi.pt_render(ctx, capi.Scene(ctx, spath), cfg, film)
        capi.image_write(str(tmp_path / name), film.resolve().reshape(16, 16, 3))
        return open(tmp_path / name, "rb").read()

    hard_path = write_scene_with_lights(tmp_path, {"a": json_light(lights[0]), "c": json_light(lights[1])})
    hard = cli_bytes(hard_path)
    assert hard == api_bytes(hard_path, "api_hard.exr")
    soft_path = write_scene_with_lights(tmp_path, {"a": soft_json_light(lights[0]), "c": soft_json_light(lights[1])})  # (the same file name, written again)
    lit = cli_bytes(soft_path)
    assert lit == api_bytes(soft_path, "api_soft.exr") and lit != hard
    assert capi.host_decode_exr(lit)[8, 8, :3].min() > 0
    assert cli_bytes(soft_path, "--no-soft-lights") == hard
