"""Point, spot and sun lights on the GPU (csrc/device/dpunct.h, the PUNCT kernels): the device probe against the numpy
restatement bit for bit, films against closed forms (a diffuse quad lit by one light of each kind, a hard shadow, two lights chosen at random,
an emitter and an environment beside a light), scenes without such lights unchanged, the refusals and fall-backs, and akari-cli."""
import json
import math
import subprocess

import numpy as np
import pytest

from akari_render_amd import abi, capi
from tests import punctual_model as pm
from tests.helpers import make_config, n_bit_diff, resolve_np, textured_room
from tests.test_environment import quad_scene
from tests.test_punctual import (KINDS, assert_rows_equal, edge_rows, json_light, light_table, model_records, point, random_rows, scene_with, spot, sun,
                                 write_scene_with_lights)

pytestmark = pytest.mark.gpu

RHO = 0.6
PUNCT_BIT, SPEC = 128, "specialised"


def render(ctx, scene, cfg):
    w, h = scene.info().width, scene.info().height
    film = capi.Film(ctx, w, h)
    capi.pt_render(ctx, scene, cfg, film)
    return resolve_np(film.read(), w, h)


def centre_cfg(spp=16, **kw):
    """depth 1, a box filter of radius 0: every camera ray goes through its pixel centre ((u - 0.5) * 0)"""
    kw.setdefault("max_depth", 1)
    return make_config(spp=spp, filter_type=abi.FILTER_BOX, filter_radius=0.0, **kw)


def pixel_points(scene, plane_z=0.0):
    """world point where the centre ray of every pixel meets the plane z = plane_z, (h, w, 3) float64 (the host's own camera text)"""
    w, h = scene.info().width, scene.info().height
    px = np.stack(np.meshgrid(np.arange(w), np.arange(h)), -1).reshape(-1, 2).astype(np.uint32)
    half = np.full((w * h, 2), 0.5, np.float32)
    r = scene.host_lens_ray(px, half, half, abi.FILTER_BOX, 0.0).astype(np.float64)
    t = (plane_z - r[:, 2]) / r[:, 5]
    return (r[:, 0:3] + t[:, None] * r[:, 3:6]).reshape(h, w, 3)


def device_points(ctx, scene):
    """The float32 surface point the kernels shade for every pixel's centre ray, (h, w, 3): the host's camera text (held to the device's elsewhere), the
    intersector the scene's kernels use, surface_interaction -- through the device probes. Every ray must hit."""
    w, h = scene.info().width, scene.info().height
    px = np.stack(np.meshgrid(np.arange(w), np.arange(h)), -1).reshape(-1, 2).astype(np.uint32)
    half = np.full((w * h, 2), 0.5, np.float32)
    r = scene.host_lens_ray(px, half, half, abi.FILTER_BOX, 0.0)
    if scene.info().uses_bvh:
        hit, bary = capi.probe_intersect(ctx, scene, np.c_[r, np.zeros(w * h, np.float32), np.full(w * h, 1e20, np.float32)])
        assert np.all(hit[:, 0] == 1)
        inst_prim = hit[:, 1:3]
    else:  # the pair walk, as k_pt_pass calls it (no shadow ray); one instance: prim = gid
        rays = np.zeros((w * h, 16), np.float32)
        rays[:, 0:6], rays[:, 6], rays[:, 14] = r, 1e20, -1.0
        out, tuv = capi.probe_intersect_pair(ctx, scene, rays, np.full((w * h, 3), 0xFFFFFFFF, np.uint32))
        assert np.all(out[:, 0] == 1)
        inst_prim, bary = np.c_[np.zeros(w * h, np.uint32), out[:, 1]], tuv[:, 1:3]
    return capi.probe_surface_interaction(ctx, scene, inst_prim, bary)[:, 0:3].reshape(h, w, 3).copy()


def record(light):
    return pm.fold(dict(type=light.type, position=light.position, direction=light.direction, color=light.color, strength=light.strength,
                        cone_angle=light.cone_angle, blend=light.blend))


def closed_form(light, x, p32=None):
    """Radiance leaving the quad (normal +z, albedo RHO) at points x, float64, (.., 3). A spot's falloff f is evaluated in float64 from the float32 cone cosine
    the model computes at the float32 points p32 (tests 1 holds the device's to it bit for bit) and the record's float32 cos_o, inv_span; without p32
    (points that are not the kernels' own) from the float64 cosine."""
    c = np.asarray(light.color, np.float32).astype(np.float64) * float(np.float32(light.strength))
    if light.type == abi.LIGHT_SUN:
        a = np.asarray(light.direction, np.float32).astype(np.float64)
        a /= np.linalg.norm(a)
        return RHO / math.pi * max(-a[2], 0.0) * c * np.ones(x.shape[:-1] + (1,))
    d = np.asarray(light.position, np.float32).astype(np.float64) - x
    r2 = np.sum(d * d, axis=-1)
    cos = np.maximum(d[..., 2], 0.0) / np.sqrt(r2)
    base = (RHO / math.pi * cos / r2)[..., None] * c
    if light.type == abi.LIGHT_POINT:
        return base
    return base * spot_falloff(light, x, p32)[..., None]


def spot_cosine(light, x, p32=None):
    rec = record(light)
    if p32 is not None:
        return pm.cone_cosine(rec, p32.reshape(-1, 3)).reshape(p32.shape[:-1]).astype(np.float64)
    d = rec["q"].astype(np.float64) - x
    return -np.sum(d / np.linalg.norm(d, axis=-1, keepdims=True) * rec["a"].astype(np.float64), axis=-1)


def spot_falloff(light, x, p32=None):
    rec = record(light)
    ct, co, inv = spot_cosine(light, x, p32), float(rec["cos_o"]), float(rec["inv_span"])
    if inv == 0.0:
        return (ct > co).astype(np.float64)
    s = np.clip((ct - co) * inv, 0.0, 1.0)
    return s * s * (3 - 2 * s)


# ---------------------------------------------------------------------------------------------------------------- 1. probe
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_probe_equals_the_model_bit_for_bit(ctx, kind):
    lights = KINDS[kind]
    sc = scene_with(lights, ctx)
    rows = np.concatenate([random_rows(4096, 11), edge_rows(lights[0])])
    got = sc.probe_light_sample(rows)
    assert_rows_equal(got, pm.light_sample_rows(light_table(sc), model_records(sc), rows))
    assert_rows_equal(got, sc.host_light_sample(rows))


def test_probe_over_a_mixed_light_list(ctx):
    sd = quad_scene(emissive=True)
    sd.lights = [point(), spot(), sun()]
    sd.environment = abi.EnvironmentData(color=(0.5, 0.6, 0.7))
    sc = capi.Scene(ctx, sd)
    rows = random_rows(4096, 5)
    assert_rows_equal(sc.probe_light_sample(rows), pm.light_sample_rows(light_table(sc), model_records(sc), rows))


# ---------------------------------------------------------------------------------------------------------------- 2. closed forms
CLOSED = {
    "point": point(position=(0.3, -0.2, 1.5)),
    # tilted: the cone's edge crosses the quad
    "spot_step": spot(position=(-0.4, 0.1, 1.2), direction=(0.5, -0.1, -1.0), cone_angle=0.45, blend=0.0),
    "spot_blend": spot(position=(-0.4, 0.1, 1.2), direction=(0.5, -0.1, -1.0), cone_angle=0.45, blend=0.4),
    "sun": sun(direction=(0.3, -0.2, -1.0)),
}
EPS = 2.0 ** -24


def check_closed_form(img, light, p32, edge_clear=0.0):
    """Every pixel within rtol 1e-5 of the float64 closed form at the kernels' own surface points (test_exact_furnace's bound for the same f cos / pdf chain),
    a spot's falloff taken from the model's float32 cone cosine; exactly 0 wherever that falloff is 0. edge_clear: the scene is also required to keep every
    pixel's cosine that far from cos_o."""
    want = closed_form(light, p32.astype(np.float64), p32)
    if light.type == abi.LIGHT_SPOT:
        f = spot_falloff(light, None, p32)
        assert (f == 0).sum() > 20 and (f > 0).sum() > 20, "the cone's edge does not cross the quad"
        assert np.all(img[f == 0] == 0), "light outside the outer cone"
        assert np.all(np.abs(spot_cosine(light, None, p32) - float(record(light)["cos_o"])) > edge_clear)
    err = np.abs(img.astype(np.float64) - want)
    lit = want > 0
    print(f"closed form, type {light.type}: worst relative error = {float(np.max(err[lit] / want[lit])):.3g}")
    assert np.all(err <= 1e-5 * want)
    assert float(want.max()) > 0.01


@pytest.mark.parametrize("force_bvh", [0, 1], ids=["exhaustive", "bvh"])
@pytest.mark.parametrize("kind", sorted(CLOSED))
def test_closed_form(ctx, kind, force_bvh):
    with capi.options(force_bvh=force_bvh):
        sc = scene_with([CLOSED[kind]], ctx, albedo=RHO)
        assert sc.info().uses_bvh == force_bvh
        check_closed_form(render(ctx, sc, centre_cfg()), CLOSED[kind], device_points(ctx, sc))


@pytest.mark.parametrize("kind", ["point", "spot_step", "sun"])
def test_closed_form_through_a_lens(ctx, kind):
    """A lens focused on the quad: the diffuse closed form does not depend on where the ray comes from (the LENS unit). The rays of a pixel meet at its
    centre's point on the quad up to the float32 rounding of each ray, a few ulp of the coordinates: a value the 1e-5 of the chain covers for a point
    light and a sun, and for the spot with the hard edge as long as no pixel sits on the edge -- which the scene is required to satisfy (64 ulp of 1 in
    the cosine). A blended spot's falloff near its outer edge is as ill-conditioned in the point as one likes: it is tested without the lens."""
    sd = quad_scene(albedo=RHO)
    sd.lights, sd.lens = [CLOSED[kind]], abi.LensData(0.05, 3.0)
    sc = capi.Scene(ctx, sd)
    film = capi.Film(ctx, 32, 32)
    se = capi.PtSession(ctx, sc, centre_cfg(), film)
    se.passes(1, blocking=True)
    assert se.kernel_info()["kernel_flags"] & (PUNCT_BIT | 32) == PUNCT_BIT | 32
    se.end()
    pinhole = scene_with([CLOSED[kind]], ctx, albedo=RHO)  # the same pixel centres, found without the lens: the plane of focus is the quad
    check_closed_form(resolve_np(film.read(), 32, 32), CLOSED[kind], device_points(ctx, pinhole), edge_clear=64 * EPS)


COLOR_PIPELINES = {"repr_aces": abi.COLOR_REPR_ACESCG, "rgb_aces": abi.COLOR_RGB_ACESCG, "both_aces": abi.COLOR_REPR_ACESCG | abi.COLOR_RGB_ACESCG}
# srgb_to_aces_with_cat_mat / aces_to_srgb_with_cat_mat of the reference's color.rs, the constants of csrc/device/dbsdf.h cs_convert
TO_ACES = np.array([[0.612494199, 0.338737252, 0.048855526], [0.070594252, 0.917671484, 0.011704306], [0.020727335, 0.106882232, 0.872338062]])
TO_SRGB = np.array([[1.707062673, -0.619959540, -0.087259850], [-0.130976829, 1.139032275, -0.007956297], [-0.024510601, -0.124810932, 1.149395971]])


@pytest.mark.parametrize("pipeline", sorted(COLOR_PIPELINES))
def test_closed_form_under_a_colour_pipeline(ctx, pipeline):
    """A session of a non-default colour pipeline gets records of its own (the colour set's): the light's colour goes sRGB -> rgb_colorspace -> the space
    the path shades in, as the quad's albedo does, the product is taken there, the film converts back. After the lights change, the next session of
    the pipeline folds them again."""
    bits = COLOR_PIPELINES[pipeline]
    rgb_aces, repr_aces = bool(bits & abi.COLOR_RGB_ACESCG), bool(bits & abi.COLOR_REPR_ACESCG)

    def to_repr(v):
        v = TO_ACES @ v if rgb_aces else v
        return v if rgb_aces == repr_aces else (TO_ACES @ v if repr_aces else TO_SRGB @ v)

    lights = [point(position=(0.3, -0.2, 1.5), color=(3.0, 0.5, 1.0), strength=2.0), point(position=(-0.5, 0.4, 1.0), color=(0.2, 1.0, 4.0), strength=1.0)]
    tint = (0.8, 0.3, 0.1)  # a coloured albedo: the product albedo x light depends on the space it is taken in (a grey one hardly does)
    sd = quad_scene()
    sd.materials[0].base_color, sd.lights = tint, lights[:1]
    sc = capi.Scene(ctx, sd)
    x = device_points(ctx, sc).astype(np.float64)
    albedo = to_repr(np.asarray(tint, np.float32).astype(np.float64))

    def expected(ls):
        total = np.zeros(x.shape)
        for l in ls:
            d = np.asarray(l.position, np.float32).astype(np.float64) - x
            r2 = np.sum(d * d, axis=-1)
            c = to_repr(np.asarray(l.color, np.float32).astype(np.float64) * float(np.float32(l.strength)))
            total += (d[..., 2] / np.sqrt(r2) / r2 / math.pi)[..., None] * (albedo * c)
        return total @ TO_SRGB.T if repr_aces else total

    got = render(ctx, sc, centre_cfg(color=bits)).astype(np.float64)
    want = expected(lights[:1])
    print(f"colour pipeline {pipeline}: worst relative error = {np.max(np.abs(got - want) / want):.3g}")
    assert np.all(np.abs(got - want) <= 1e-5 * want)
    if repr_aces:  # the product is taken in another space: the default pipeline's film differs (rgb_aces alone goes there and back)
        assert not np.allclose(got, render(ctx, sc, centre_cfg()), rtol=1e-3)
    # the lights change: the next session of the pipeline renders the new one
    sc.clear_punctual_lights()
    sc.add_punctual_light(lights[1])
    got = render(ctx, sc, centre_cfg(color=bits)).astype(np.float64)
    want = expected(lights[1:])
    assert np.all(np.abs(got - want) <= 1e-5 * want)


# ---------------------------------------------------------------------------------------------------------------- 3. hard shadow
def test_hard_shadow(ctx):
    light = point(position=(0.0, 0.0, 2.0), color=(1, 1, 1), strength=5.0)
    sd = quad_scene(albedo=RHO)
    open_scene = capi.Scene(ctx, abi.SceneData(sd.meshes, sd.instances, sd.materials, sd.camera, lights=[light]))
    # a blocker at z = 1.5 covering |x|, |y| <= 0.15: from the light at z = 2 its umbra on the floor is |x|, |y| <= 0.6. The camera at z = 3 sees the blocker
    # in front of the floor's |x|, |y| <= 0.3: those pixels are left out (by where their ray meets the plane z = 1.5), the ring between the two is umbra
    bv = np.array([[-0.15, -0.15, 1.5], [0.15, -0.15, 1.5], [0.15, 0.15, 1.5], [-0.15, 0.15, 1.5]], np.float32)
    sd.meshes.append(abi.MeshData(vertices=bv, indices=np.array([[0, 1, 2], [0, 2, 3]], np.uint32)))
    sd.materials.append(abi.MaterialData(kind=abi.MAT_DIFFUSE, base_color=(0.0, 0.0, 0.0)))
    sd.instances.append(abi.InstanceData(1, [1], np.eye(4, dtype=np.float32).reshape(16).copy()))
    sd.lights = [light]
    blocked = capi.Scene(ctx, sd)
    a, b = render(ctx, open_scene, centre_cfg()), render(ctx, blocked, centre_cfg())
    x = pixel_points(open_scene)
    px = 2 * 3.0 * math.tan(0.3) / 32  # a pixel's footprint on the floor
    sees_blocker = np.all(np.abs(pixel_points(open_scene, 1.5)[..., :2]) <= 0.15 + px, axis=-1)
    cheb = np.max(np.abs(x[..., :2]), axis=-1)
    umbra, lit = (cheb < 0.6 - px) & ~sees_blocker, cheb > 0.6 + px
    assert umbra.sum() >= 8 and lit.sum() > 300
    assert np.all(b[umbra] == 0)
    assert n_bit_diff(a[lit], b[lit]) == 0
    assert np.all(a[lit] > 0)


# ---------------------------------------------------------------------------------------------------------------- 4. selection
def test_selection_between_two_lights(ctx):
    l1, l2 = point(position=(-0.5, 0.0, 1.0), color=(1, 1, 1), strength=1.0), point(position=(0.6, 0.2, 1.5), color=(1, 1, 1), strength=3.0)
    sc = scene_with([l1, l2], ctx, width=16, height=16, albedo=RHO)
    p1, p2 = float(np.float32(sc.light(0)[2])), float(np.float32(sc.light(1)[2]))
    assert abs(p1 - 0.25) < 1e-6 and abs(p2 - 0.75) < 1e-6
    x = pixel_points(sc)
    L1, L2 = closed_form(l1, x)[..., 0], closed_form(l2, x)[..., 0]
    one = render(ctx, sc, centre_cfg(spp=1, sampler_seed=3))[..., 0].astype(np.float64)
    is1, is2 = np.isclose(one, L1 / p1, rtol=1e-5, atol=0), np.isclose(one, L2 / p2, rtol=1e-5, atol=0)
    assert np.all(is1 | is2) and is1.sum() > 20 and is2.sum() > 100  # every sample is L1 / p1 or L2 / p2
    n = 256
    mean = render(ctx, sc, centre_cfg(spp=n, sampler_seed=7))[..., 0].astype(np.float64)
    var = (L1 ** 2 / p1 + L2 ** 2 / p2 - (L1 + L2) ** 2) / n
    z = (mean - (L1 + L2)) / np.sqrt(var)
    print(f"selection: max |z| = {np.abs(z).max():.2f}, pooled mean of z = {z.mean():.3f} (allowed {5 / math.sqrt(z.size):.3f})")
    assert np.all(np.abs(z) < 6)
    assert abs(z.mean()) < 5 / math.sqrt(z.size)


# ---------------------------------------------------------------------------------------------------------------- 5. emitter + environment + light
def test_linearity_beside_an_emitter_and_an_environment(ctx):
    """{emitter, constant environment, point light} = {emitter, environment} + the point light's closed form, at depth 1 (the ENV unit): 24 x 24, sobol,
    1024 spp, within 5 standard errors per pixel and channel, estimated from 16 seeds of the light-free render.

    The standard error is the lit render's, derived from the light-free render's. Per sample the light-free estimator is X (mean mu, variance n V, V the
    variance of a render of n samples: the 16-seed estimate). The lit render chooses the light with probability p and then returns L / p, else it
    returns X / (1 - p): the others keep a (1 - p) share of the samples. So E[Y] = mu + L and E[Y^2] = E[X^2] / (1 - p) + L^2 / p, which gives
        Var(lit render) = V / (1 - p) + (mu sqrt(p / (1 - p)) - L sqrt((1 - p) / p))^2 / n.
    The comparison is with the 16-seed mean, whose variance V / 16 is added. p is the light's selection pdf as the scene reports it. (The term of X that
    comes from the BSDF-sampled ray is not thinned by the selection; treating it as if it were only adds to the allowance's V / (1 - p).)"""
    light = point(position=(0.3, -0.2, 0.25), color=(3.0, 2.0, 1.0), strength=0.12)  # low over the floor: power, and with it p, does not depend on the distance

    def scene(with_light):
        sd = quad_scene(width=24, height=24, albedo=RHO, emissive=True)
        # quad_scene's emitter (0.4 x 0.4, facing -z) hangs behind the quad: mirrored to z = +0.5, over (0.3, 0.3)
        sd.meshes[1].vertices = (np.asarray(sd.meshes[1].vertices) * np.float32([1, 1, -1]) + np.float32([0.3, 0.3, 0.0])).astype(np.float32)
        sd.environment = abi.EnvironmentData(color=(0.3, 0.4, 0.5))
        sd.lights = [light] if with_light else []
        return capi.Scene(ctx, sd)

    def cfg(seed):
        return make_config(spp=1024, max_depth=1, filter_type=abi.FILTER_BOX, filter_radius=0.0, sampler_type=abi.SAMPLER_SOBOL, sampler_seed=seed)

    n = 1024
    bare, lit = scene(False), scene(True)
    p = float(np.float32(lit.light(1)[2]))
    assert lit.light(1)[0] == capi.PUNCTUAL_LIGHT_INSTANCE and 0.15 < p < 0.4  # a real share of the samples
    seeds = np.stack([render(ctx, bare, cfg(100 + s)).astype(np.float64) for s in range(16)])
    mu, V = seeds.mean(axis=0), seeds.var(axis=0, ddof=1)
    at_emitter = pixel_points(bare, 0.5)
    floor = (np.abs(at_emitter[..., 0] - 0.3) > 0.3) | (np.abs(at_emitter[..., 1] - 0.3) > 0.3)  # pixels that see the floor, not the emitter's back, one pixel and more away
    got = render(ctx, lit, cfg(116)).astype(np.float64)
    L = closed_form(light, pixel_points(bare))
    se = np.sqrt(V / (1 - p) + (mu * math.sqrt(p / (1 - p)) - L * math.sqrt((1 - p) / p)) ** 2 / n + V / 16)
    excess = np.abs(got - (mu + L))[floor] / se[floor]
    print(f"linearity: light's selection probability {p:.3f}; worst |difference| / standard error = {excess.max():.2f}, median {np.median(excess):.2f} over {int(floor.sum())} pixels x 3; "
          f"values where the light alone is > 10 standard errors: {int(np.sum(L[floor] > 10 * se[floor]))}")
    assert floor.sum() > 350 and np.all(se[floor] > 0)
    assert np.all(excess <= 5.0)
    assert np.sum(L[floor] > 10 * se[floor]) > 150  # the light is far above the allowance: leaving it out would fail


# ---------------------------------------------------------------------------------------------------------------- 6. nothing else moved
def test_strength_zero_lights_change_nothing(ctx):
    sd = quad_scene(albedo=RHO, emissive=True)
    sd.meshes[1].vertices = (np.asarray(sd.meshes[1].vertices) * np.float32([1, 1, -1])).astype(np.float32)
    cfg = make_config(spp=16, max_depth=4, sampler_seed=5)
    out = []
    for lights in ([], [point(strength=0.0), spot(strength=0.0), sun(color=(0, 0, 0))]):
        sd.lights = lights
        sc = capi.Scene(ctx, sd)
        assert sc.punctual_lights() == []
        film = capi.Film(ctx, 32, 32)
        se = capi.PtSession(ctx, sc, cfg, film)
        se.passes(1, blocking=True)
        info = se.kernel_info()
        states = se.sampler_states(32 * 32)
        st = se.end()
        out.append((film.read(), states, {k: v for k, v in st.items() if k.startswith("n_")}, info["kernel_flags"]))
    assert out[0][3] & PUNCT_BIT == 0 and out[1][3] == out[0][3]
    assert n_bit_diff(out[0][0], out[1][0]) == 0 and np.array_equal(out[0][1], out[1][1]) and out[0][2] == out[1][2]


def test_sharded_render_assembles_to_the_unsharded_film(ctx):
    light = spot(position=(-0.4, 0.1, 1.2), direction=(0.5, -0.1, -1.0), cone_angle=0.45, blend=0.4)
    sc = scene_with([light], ctx, width=32, height=64, albedo=RHO)
    base = dict(spp=8, max_depth=3, sampler_seed=9, tile_w=16, tile_h=16)  # 2 x 4 tiles: in Morton order both ranks own four (kernels.h tile_owner)
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
        assert np.count_nonzero(part) > 0 and np.count_nonzero(parts[part != 0]) == 0  # the shards' pixels do not overlap
        parts += part
    assert n_bit_diff(parts, whole.read()) == 0


# ---------------------------------------------------------------------------------------------------------------- 7. refusals and fall-backs
def test_refusals_and_fallbacks(ctx):
    with capi.options(force_bvh=1):
        sc = scene_with([point()], ctx)
    film, albedo, normal = (capi.Film(ctx, 32, 32) for _ in range(3))
    cfg = centre_cfg(spp=4)

    def refused(fn):
        with pytest.raises(capi.AkariError) as e:
            fn()
        assert e.value.code == capi.ERR_UNSUPPORTED and "point light" in str(e.value), str(e.value)

    g = abi.GptConfig.default()
    g.spp, g.max_depth = 4, 4
    refused(lambda: capi.gpt_render(ctx, sc, g, film))
    m = abi.McmcConfig.default()
    m.spp, m.max_depth, m.n_chains, m.n_bootstrap = 2, 4, 256, 1024
    refused(lambda: capi.mcmc_render(ctx, sc, m, film))
    with capi.options(arith=1):
        refused(lambda: capi.pt_render(ctx, sc, cfg, film))
    with capi.options(wavefront=1):
        refused(lambda: capi.pt_render(ctx, sc, cfg, film))
    refused(lambda: capi.pt_render_features(ctx, sc, cfg, film, albedo, normal))
    with pytest.raises(capi.AkariError) as e:  # the setters, while a session holds the scene
        se = capi.PtSession(ctx, sc, cfg, film)
        try:
            sc.add_punctual_light(sun())
        finally:
            se.end()
    assert e.value.code == capi.ERR_INVALID_ARGUMENT and len(sc.punctual_lights()) == 1
    # the automatic choices land on the megakernel
    lit = render(ctx, sc, cfg)
    with capi.options(wavefront=-1, sched_trial=1, instancing=-1):
        f2 = capi.Film(ctx, 32, 32)
        se = capi.PtSession(ctx, sc, make_config(spp=16, spp_per_pass=2, max_depth=1, filter_type=abi.FILTER_BOX, filter_radius=0.0), f2)
        se.passes(8, blocking=True)
        info = se.kernel_info()
        se.end()
        assert "wavefront" not in info["status"] and info["kernel_flags"] & PUNCT_BIT
        assert np.allclose(resolve_np(f2.read(), 32, 32), lit, rtol=1e-6)
    # with use_nee = 0 a punctual light gives nothing
    assert not render(ctx, sc, centre_cfg(spp=4, use_nee=0)).any()
    # aov: the scene as if the light were not there
    a = abi.AovConfig.default()
    a.spp = 4
    fa, fb = capi.Film(ctx, 32, 32), capi.Film(ctx, 32, 32)
    capi.aov_render(ctx, sc, a, fa)
    with capi.options(force_bvh=1):
        capi.aov_render(ctx, scene_with([], ctx), a, fb)
    assert n_bit_diff(fa.read(), fb.read()) == 0
    # specialise: a scene with texture-fed materials and a light renders with the interpreter kernels
    sd = textured_room(width=32, height=32)
    sd.lights = [point(position=(0.0, 0.5, 0.0))]
    with capi.options(specialise=1):
        room = capi.Scene(ctx, sd)
        se = capi.PtSession(ctx, room, make_config(spp=2, max_depth=3), capi.Film(ctx, 32, 32))
        se.passes(1, blocking=True)
        info = se.kernel_info()
        se.end()
    assert info[SPEC] == 0 and info["kernel_flags"] & PUNCT_BIT and "punctual" in info["status"]


# ---------------------------------------------------------------------------------------------------------------- 8. akari-cli
def test_cli(ctx, tmp_path):
    from akari_render_amd import build
    cli = build.build_cli()
    lights = {"a": json_light(point(position=(0.3, -0.2, 1.5))), "b": json_light(spot(position=(-0.4, 0.1, 1.2), direction=(0.5, -0.1, -1.0), cone_angle=0.375, blend=0.5)),
              "c": json_light(sun(direction=(0.3, -0.2, -1.0), strength=0.5))}
    spath = write_scene_with_lights(tmp_path, lights)
    method = {"method": {"type": "pt", "spp": 4, "spp_per_pass": 4, "max_depth": 2}, "sampler": {"type": "independent", "seed": 1}, "film": {"out": str(tmp_path / "out.exr")}}
    mpath = tmp_path / "pt.json"
    mpath.write_text(json.dumps(method))

    def api_bytes(name, **opts):
        with capi.options(**opts):
            sc = capi.Scene(ctx, spath)
        film = capi.Film(ctx, 16, 16)
        cfg, _ = capi.config_from_json(json.dumps(method))
        capi.pt_render(ctx, sc, cfg, film)
        capi.image_write(str(tmp_path / name), film.resolve().reshape(16, 16, 3))
        return open(tmp_path / name, "rb").read()

    res = subprocess.run([cli, "-s", spath, "-m", str(mpath)], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    lit = open(tmp_path / "out.exr", "rb").read()
    assert lit == api_bytes("api_lit.exr")
    res = subprocess.run([cli, "-s", spath, "-m", str(mpath), "--no-punctual-lights"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    unlit = open(tmp_path / "out.exr", "rb").read()
    assert unlit == api_bytes("api_unlit.exr", punctual_lights=0) and unlit != lit
    assert not capi.host_decode_exr(unlit)[..., :3].any() and capi.host_decode_exr(lit)[8, 8, :3].min() > 0
