"""The CPU oracle's punctual lights (oracle/or_punct.h) and thin lens (4.9) as a third restatement: its light
sample, fold, light table and lens rays against the numpy models (tests/punctual_model.py, tests/soft_light_model.py, tests/test_lens.py)
AND the library's host hooks, bit for bit; the two scene.json readers; and oracle films whose values are exact. No GPU is needed: the
library's side is its host build (capi.Scene(None, ...))."""
import ctypes as C
import dataclasses
import json
import math

import numpy as np
import pytest

from akari_render_amd import abi, capi
from oracle import pyoracle, scene_json
from tests import soft_light_model as sm
from tests.helpers import make_config, n_bit_diff
from tests.test_environment import quad_scene
from tests.test_lens import _camera, restated_lens, restated_pinhole
from tests.test_punctual import KINDS, assert_rows_equal, edge_rows, json_light, light_table, point, random_rows, spot, sun, two_emitter_scene, write_scene_with_lights
from tests.test_soft_lights import KINDS as SOFT_KINDS
from tests.test_soft_lights import as_dict, edge_rows9, random_rows9, sizes, soft

F = np.float32
PIPELINES = {"srgb_srgb": 0, "acescg_repr": abi.COLOR_REPR_ACESCG, "acescg_rgb": abi.COLOR_RGB_ACESCG, "acescg": abi.COLOR_REPR_ACESCG | abi.COLOR_RGB_ACESCG}


def both(lights, sd=None):
    """the library's host scene and the oracle's of the same description"""
    sd = sd if sd is not None else quad_scene()
    sd.lights = list(lights)
    return capi.Scene(None, sd), pyoracle.OracleScene(sd)


def model_records(scene):
    lights = iter(scene.punctual_lights())
    return [sm.fold(as_dict(next(lights))) if scene.light(i)[0] == capi.PUNCTUAL_LIGHT_INSTANCE else None for i in range(scene.info().n_lights)]


def rows9_of(rows7):
    return np.ascontiguousarray(np.concatenate([rows7, np.full((rows7.shape[0], 2), 0.5, F)], axis=1))


def check_sample(lights, rows9, sd=None):
    """the oracle's known-answer call against the numpy model and against the library's host hook"""
    sc, osc = both(lights, sd)
    got = osc.punct_sample_many(rows9)
    assert_rows_equal(got, sm.light_sample_rows(light_table(sc), model_records(sc), rows9))
    assert_rows_equal(got, sc.host_light_sample_soft(rows9))
    return got


# ---------------------------------------------------------------------------------------------------------------- 1. light sampling
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_delta_sample_equals_model_and_hook(hip_lib, kind):
    lights = KINDS[kind]
    rows = np.concatenate([random_rows(4096, 11), edge_rows(lights[0])])
    out, _ = check_sample(lights, rows9_of(rows))
    assert np.all(out[:, 12] == 1) and np.all(out[:, 6] == 1)
    # the seven-column form: u_sample = (0.5, 0.5), and the old hook
    sc, osc = both(lights)
    assert_rows_equal(osc.punct_sample_many(rows), sc.host_light_sample(rows))
    # a delta light never looks at u_sample
    other = rows9_of(rows)
    other[:, 7:9] = np.random.default_rng(1).random((len(rows), 2))
    assert_rows_equal(osc.punct_sample_many(other), sc.host_light_sample(rows))


@pytest.mark.parametrize("which", [0, 1, 2, 3], ids=["small", "large", "tiny", "huge"])
@pytest.mark.parametrize("kind", sorted(SOFT_KINDS))
def test_soft_sample_equals_model_and_hook(hip_lib, kind, which):
    base = SOFT_KINDS[kind]
    light = soft(base, (sizes(base) + sizes(base, edge=True))[which])
    rows = np.concatenate([random_rows9(4096, 21 + which), edge_rows9(light)])
    out, _ = check_sample([light], rows)
    assert np.all(out[:, 12] == 1) and np.all(out[:, 6] == 1)
    if which < 2:  # (a disk of radius 1e3 seen from a unit away: nearly every direction misses a spot's cone)
        assert out[:4096, 11].mean() > (0.02 if light.type == abi.LIGHT_SPOT else 0.9)


def test_sample_over_a_mixed_light_list(hip_lib):
    """emitter, point, soft spot, soft sun, environment: whichever the alias table picks, or just its pdf"""
    sd = quad_scene(emissive=True)
    sd.environment = abi.EnvironmentData(color=(0.5, 0.6, 0.7))
    out, light = check_sample([point(), soft(spot(), 0.2), soft(sun(), 0.3)], random_rows9(4096, 5), sd)
    assert set(np.unique(light)) == set(range(5))
    assert np.all(out[np.isin(light, (0, 4))][:, 12] == 0) and not out[np.isin(light, (0, 4))][:, :6].any()


# ---------------------------------------------------------------------------------------------------------------- 2. fold and light table
def assert_tables_equal(sc, osc):
    n = sc.info().n_lights
    assert osc.num_lights() == n
    lib_rows = [sc.light(i) for i in range(n)]
    or_rows = [osc.light_info(i) for i in range(n)]
    for i, ((li, lp, lq), (oi, op, oq)) in enumerate(zip(lib_rows, or_rows)):
        assert li == oi or (li == capi.ENV_LIGHT_INSTANCE and oi == 0xFFFFFFFF), (i, li, oi)
        assert F(lp).tobytes() == F(op).tobytes() and F(lq).tobytes() == F(oq).tobytes(), (i, lp, op, lq, oq)
    j, t, pdf = light_table(sc)
    e, opdf = osc.light_table()
    assert np.array_equal(j, e["j"]) and np.array_equal(t.view(np.uint32), e["t"].view(np.uint32)) and np.array_equal(pdf.view(np.uint32), opdf.view(np.uint32))
    lib_rec = sc.array(capi.ARRAY_PUNCTUAL_LIGHTS, np.uint32).reshape(-1, 16)
    assert np.array_equal(lib_rec, osc.punctual_records(0))
    assert sc.punctual_lights() == osc.punctual_lights()  # the descriptions as held: what a kind does not read is stored as zero
    return lib_rows


ALL_LIGHTS = {**{k: v[0] for k, v in KINDS.items()}, **{"soft_" + k: soft(v, sizes(v)[0]) for k, v in SOFT_KINDS.items()},
              "ignored_sizes": dataclasses.replace(point(), angle=0.5), "sun_ignored_radius": dataclasses.replace(sun(), radius=0.5, position=(1.0, 2.0, 3.0)),
              "minus_zero_radius": dataclasses.replace(spot(), radius=-0.0)}


@pytest.mark.parametrize("kind", sorted(ALL_LIGHTS))
def test_fold_and_table_of_each_kind(hip_lib, kind):
    light = ALL_LIGHTS[kind]
    sc, osc = both([light])
    assert_tables_equal(sc, osc)
    want = sm.record_words(sm.fold(as_dict(sc.punctual_lights()[0])))
    assert np.array_equal(osc.punctual_records(0)[0], want)


@pytest.mark.parametrize("pipeline", sorted(PIPELINES))
def test_fold_under_each_colour_pipeline(hip_lib, pipeline):
    """c goes the way of an Emission material's constant colour: the oracle's record against the library's host evaluation of such a material
    whose colour is the light's f32 colour x strength; every other word is the default pipeline's"""
    bits = PIPELINES[pipeline]
    lights = [point(color=(3.0, 0.5, 1.0)), soft(spot(), 0.2), soft(sun(color=(0.2, 1.0, 4.0)), 0.3)]
    sd = quad_scene()
    for l in lights:
        c = (np.asarray(l.color, F) * F(l.strength)).astype(F)
        sd.materials.append(abi.MaterialData(kind=abi.MAT_EMISSION, emission_color=tuple(float(v) for v in c), emission_strength=1.0))
    sc, osc = both(lights, sd)
    rec, rec0 = osc.punctual_records(bits), osc.punctual_records(0)
    for k in range(3):
        want = capi.probe_material_inputs_host(sc, 1 + k, np.zeros((1, 2), F), bits)[0, 19:22]
        assert np.array_equal(rec[k, 8:11], want.view(np.uint32)), (k, rec[k, 8:11].view(F), want)
    mask = np.ones(16, bool)
    mask[8:11] = False
    assert np.array_equal(rec[:, mask], rec0[:, mask])
    assert (bits == 0) == np.array_equal(rec, rec0) or bits == abi.COLOR_RGB_ACESCG  # (rgb alone goes there and back: equal up to rounding)
    # the selection weights are the default pipeline's whatever the render's is: the known-answer call under the pipeline picks the same lights
    rows = random_rows9(1024, 3)
    o_def, l_def = osc.punct_sample_many(rows, 0)
    o_pip, l_pip = osc.punct_sample_many(rows, bits)
    assert np.array_equal(l_def, l_pip) and np.array_equal(o_def[:, 6], o_pip[:, 6])


def _emitters(n):
    if n == 0:
        return quad_scene()
    if n == 1:
        return quad_scene(emissive=True)
    return two_emitter_scene()


@pytest.mark.parametrize("env", [False, True], ids=["no_env", "env"])
@pytest.mark.parametrize("emitters", [0, 1, 2])
def test_light_list_order_and_alias_table(hip_lib, emitters, env):
    sd = _emitters(emitters)
    if env:
        sd.environment = abi.EnvironmentData(color=(0.5, 0.6, 0.7))
    lights = [point(), soft(spot(), 0.125), sun(), point(strength=0.0), spot(color=(0.0, 0.0, 0.0)), soft(sun(direction=(0, 1, -1)), 0.4)]
    sc, osc = both(lights, sd)
    rows = assert_tables_equal(sc, osc)
    inst = [r[0] for r in rows]
    assert len(inst) == emitters + 4 + int(env)  # the two that are "no light" are not there
    assert inst[emitters:emitters + 4] == [capi.PUNCTUAL_LIGHT_INSTANCE] * 4 and (not env or inst[-1] == capi.ENV_LIGHT_INSTANCE)
    # set in another order: environment after the lights, lights replaced, removed
    osc.set_environment(None)
    osc.set_punctual_lights(lights[:1])
    osc.set_environment(sd.environment)
    osc.set_punctual_lights(lights)
    assert_tables_equal(sc, osc)
    osc.set_punctual_lights(None)
    bare = capi.Scene(None, dataclasses.replace(sd, lights=[]))
    assert osc.num_lights() == bare.info().n_lights == emitters + int(env)
    for i in range(osc.num_lights()):
        assert F(osc.light_info(i)[2]).tobytes() == F(bare.light(i)[2]).tobytes()


def test_sun_only_scene(hip_lib):
    sc, osc = both([sun()])
    assert assert_tables_equal(sc, osc)[0][2] == 1.0


def test_refusals_are_the_librarys(hip_lib):
    osc = pyoracle.OracleScene(quad_scene())
    sc = capi.Scene(None, quad_scene())
    bad = [dict(type=7), dict(type=abi.LIGHT_SUN, direction=(0, 0, 0)), dict(type=abi.LIGHT_SPOT, direction=(0, float("nan"), 1), cone_angle=0.3),
           dict(type=abi.LIGHT_SPOT, direction=(0, 0, -1), cone_angle=0.0), dict(type=abi.LIGHT_SPOT, direction=(0, 0, -1), cone_angle=2.0),
           dict(type=abi.LIGHT_SPOT, direction=(0, 0, -1), cone_angle=0.3, blend=1.5), dict(type=abi.LIGHT_POINT, strength=-1.0),
           dict(type=abi.LIGHT_POINT, position=(float("inf"), 0, 0)), dict(type=abi.LIGHT_POINT, color=(1, -1, 1)), dict(type=abi.LIGHT_POINT, radius=-1.0),
           dict(type=abi.LIGHT_SUN, direction=(0, 0, -1), angle=float(F(math.pi))), dict(type=abi.LIGHT_SUN, direction=(0, 0, -1), angle=float("nan"))]
    good = [dict(type=abi.LIGHT_SPOT, direction=(0, 0, -1), cone_angle=float(F(math.pi / 2)), blend=1.0), dict(type=abi.LIGHT_SUN, direction=(0, 0, -1), radius=float("nan")),
            dict(type=abi.LIGHT_POINT, angle=-3.0), dict(type=abi.LIGHT_SUN, direction=(0, 0, -1), angle=float(np.nextafter(F(math.pi), F(0))))]
    for kw in bad:
        with pytest.raises(capi.AkariError):
            sc.add_punctual_light(**kw)
        with pytest.raises(ValueError):
            osc.set_punctual_lights([abi.PunctualLightData(**kw)])
    assert osc.num_lights() == 0
    for kw in good:
        sc.add_punctual_light(**kw)
    osc.set_punctual_lights([abi.PunctualLightData(**kw) for kw in good])
    assert_tables_equal(sc, osc)
    for lens in ((-0.1, 1.0), (0.1, -1.0), (np.nan, 1.0), (0.1, np.inf), (np.inf, 1.0), (0.1, 0.0), (0.1, np.nan)):
        with pytest.raises(ValueError):
            osc.set_lens(*lens)
    osc.set_lens(0.25, 3.5)
    assert osc.lens() == abi.LensData(0.25, 3.5)
    osc.set_lens(0.0, 3.5)
    assert osc.lens() is None


def test_description_layouts(hip_lib):
    """the oracle's two new descriptions against the public header's, field by field (tests/test_abi.py's way)"""
    L = pyoracle.lib()
    assert L.or_sizeof_punctual_light_desc() == C.sizeof(abi.PunctualLightDesc) == hip_lib.akr_struct_size(24) == 60
    assert L.or_sizeof_lens_desc() == C.sizeof(abi.LensDesc) == hip_lib.akr_struct_size(16) == 8
    want = {"type": 0, "position": 4, "direction": 16, "color": 28, "strength": 40, "cone_angle": 44, "blend": 48, "radius": 52, "angle": 56}
    assert {n: getattr(abi.PunctualLightDesc, n).offset for n, _ in abi.PunctualLightDesc._fields_} == want
    assert {n: getattr(abi.LensDesc, n).offset for n, _ in abi.LensDesc._fields_} == {"radius": 0, "focal_distance": 4}
    # ... and the oracle reads every field where the header puts it: a light whose every field is distinct comes back as given
    l = abi.PunctualLightData(abi.LIGHT_SPOT, (1.0, 2.0, 3.0), (4.0, 5.0, 6.0), (7.0, 8.0, 9.0), 10.0, 0.75, 0.5, 11.0, 0.0)
    osc = pyoracle.OracleScene(quad_scene())
    osc.set_punctual_lights([l])
    assert osc.punctual_lights() == [l]
    osc.set_lens(0.375, 2.5)
    assert osc.lens() == abi.LensData(0.375, 2.5)


# ---------------------------------------------------------------------------------------------------------------- 3. lens rays
U_LENS_EDGE = [[0.5, 0.5], [0.0, 0.0], [np.nextafter(F(1), F(0))] * 2, [0.25, 0.25], [0.75, 0.25], [0.25, 0.75], [0.75, 0.75], [0.5, 0.1], [0.1, 0.5],
               [0.5, 0.9], [0.0, np.nextafter(F(1), F(0))], [0.75 + 2.0 ** -23, 0.75], [0.75, 0.75 + 2.0 ** -23]]


@pytest.mark.parametrize("rotated", [False, True], ids=["identity", "rotated"])
def test_lens_rays_equal_definition_and_hook(hip_lib, rotated):
    w, h = 40, 24
    sd = _camera(w, h, rotated)
    scene, osc = capi.Scene(None, sd), pyoracle.OracleScene(sd)
    r2c, c2w, ident = np.zeros(16, F), np.zeros(16, F), C.c_int32()
    pyoracle.lib().or_scene_camera(osc.h, r2c.ctypes.data_as(C.POINTER(C.c_float)), c2w.ctypes.data_as(C.POINTER(C.c_float)), C.byref(ident))
    assert bool(ident.value) == (not rotated)
    rng = np.random.default_rng(17 + int(rotated))
    n = 3000
    pixels = np.stack([rng.integers(0, w, n), rng.integers(0, h, n)], axis=1).astype(np.uint32)
    u_filter, u_lens = rng.random((n, 2), dtype=F), rng.random((n, 2), dtype=F)
    u_lens[:len(U_LENS_EDGE)] = U_LENS_EDGE
    radius = 0.8
    for lens in (None, (0.05, 3.0), (0.7, 1.25), (1e-3, 40.0)):
        scene.set_lens(*lens) if lens else scene.set_lens(None)
        osc.set_lens(*lens) if lens else osc.set_lens(None)
        got = osc.lens_ray_many(pixels, u_filter, u_lens, abi.FILTER_BOX, radius)
        want = restated_lens(r2c, c2w, pixels, u_filter, u_lens, radius, *lens) if lens else restated_pinhole(r2c, c2w, pixels, u_filter, radius)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), lens
        assert np.array_equal(got.view(np.uint32), scene.host_lens_ray(pixels, u_filter, u_lens, abi.FILTER_BOX, radius).view(np.uint32)), lens
        g2 = osc.lens_ray_many(pixels, u_filter, u_lens, abi.FILTER_GAUSSIAN, 1.5)
        assert np.array_equal(g2.view(np.uint32), scene.host_lens_ray(pixels, u_filter, u_lens, abi.FILTER_GAUSSIAN, 1.5).view(np.uint32)), lens
    if not rotated:  # the c2w_identity shortcut: the origin is the lens point itself, the small translation is dropped
        sd.camera.c2w[12] = 5e-5
        osc2 = pyoracle.OracleScene(sd)
        osc2.set_lens(0.3, 2.0)
        sc2 = capi.Scene(None, sd)
        sc2.set_lens(0.3, 2.0)
        a, b = osc2.lens_ray_many(pixels, u_filter, u_lens, abi.FILTER_BOX, radius), sc2.host_lens_ray(pixels, u_filter, u_lens, abi.FILTER_BOX, radius)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.all(a[:, 2] == 0)


# ---------------------------------------------------------------------------------------------------------------- 4. readers
def test_scene_json_both_readers(hip_lib, tmp_path):
    lights = [point(), soft(spot(cone_angle=0.375, blend=0.25), 0.125), soft(sun(), 0.25), soft(point(position=(0.5, 0.5, 1.0)), 0.5), spot(cone_angle=0.25, blend=0.0), sun(direction=(0, 1, -1))]
    entries = {}
    for k, l in enumerate(lights):
        e = json_light(l)
        if l.radius:
            e["data"]["radius"] = l.radius
        if l.angle:
            e["data"]["angle"] = l.angle
        e["data"]["angle" if l.type != abi.LIGHT_SUN else "radius"] = 9.0  # the other kind's key is not read
        entries["zyxwvu"[k]] = e  # names in descending order: the readers must sort them
    entries["reference_shaped"] = {"type": "point", "data": {}}
    entries["defaults"] = {"type": "point", "data": {"position": [0, 0, 1]}}
    path = write_scene_with_lights(tmp_path, entries)
    doc = json.load(open(path))
    doc["camera"]["data"]["focal_distance"], doc["camera"]["data"]["fstop"] = 3.0, 2.8
    open(path, "w").write(json.dumps(doc))
    with capi.options(lens=1):
        lib_scene = capi.Scene(None, path)
    sd = scene_json.load_scene(path, lens=True)
    assert len(sd.lights) == 7 and sd.lights == lib_scene.punctual_lights()
    assert sd.lights[0].color == (1.0, 1.0, 1.0) and sd.lights[0].strength == 1.0
    assert sd.lens == lib_scene.lens() and F(sd.lens.radius) == F(3.0) / (F(2.0) * F(2.8))
    assert_tables_equal(lib_scene, pyoracle.OracleScene(sd))
    # the options' mirrors
    assert scene_json.load_scene(path).lens is None and capi.Scene(None, path).lens() is None
    with capi.options(soft_lights=0):
        assert scene_json.load_scene(path, soft_lights=False).lights == capi.Scene(None, path).punctual_lights()
    assert all(l.radius == 0 and l.angle == 0 for l in scene_json.load_scene(path, soft_lights=False).lights)
    assert scene_json.load_scene(path, punctual_lights=False).lights == []
    for bad in ({"type": "laser", "data": {"position": [0, 0, 1]}}, {"type": "point", "data": {"strength": 1.0}}, {"type": "spot", "data": {"position": [0, 0, 1], "direction": [0, 0, -1]}}):
        with pytest.raises(ValueError):
            scene_json.load_scene(write_scene_with_lights(tmp_path, {"the_lamp": bad}))


# ---------------------------------------------------------------------------------------------------------------- 5. exact-valued oracle films
def _render(sd, cfg, **kw):
    w, h = sd.camera.width, sd.camera.height
    if cfg.sampler_type == abi.SAMPLER_INDEPENDENT:
        states = pyoracle.init_pcg32_states(w * h, cfg.sampler_seed)
    else:
        pyoracle.set_pmj_tables(*capi.host_pmj02bn_tables())
        i = np.arange(w * h, dtype=np.uint64)
        states = np.zeros(2 * w * h, np.uint64)
        states[0::2], states[1::2] = 0xFFFFFFFF, (i % np.uint64(w)) | ((i // np.uint64(w)) << np.uint64(32))
    film, st = pyoracle.OracleScene(sd, **kw).render(cfg, states=states)
    return film, st, states


def test_zero_strength_lights_change_no_bit():
    sd = quad_scene(emissive=True)
    sd.environment = abi.EnvironmentData(color=(0.5, 0.6, 0.7))
    cfg = make_config(spp=4, max_depth=4, sampler_seed=3)
    a = _render(sd, cfg)
    sd.lights = [point(strength=0.0), spot(color=(0.0, 0.0, 0.0)), soft(sun(strength=0.0), 0.3)]
    b = _render(sd, cfg)
    assert n_bit_diff(a[0], b[0]) == 0 and a[1] == b[1] and np.array_equal(a[2], b[2])
    sd.lights = [point()]
    c = _render(sd, cfg)
    assert n_bit_diff(a[0], c[0]) > 0 and np.array_equal(a[2], c[2])  # a light does reach the film, and takes no sampler dimension


def test_hard_shadow_umbra_is_zero():
    """tests/test_gpu_punctual.py test_hard_shadow's scene: the ring of floor pixels in the blocker's umbra is exactly 0, the lit floor is the unblocked
    render's bit for bit and > 0"""
    from tests.test_gpu_punctual import RHO, centre_cfg, pixel_points
    light = point(position=(0.0, 0.0, 2.0), color=(1, 1, 1), strength=5.0)
    sd = quad_scene(albedo=RHO)
    sd.lights = [light]
    a = _render(sd, centre_cfg())[0]
    open_scene = capi.Scene(None, sd)
    bv = np.array([[-0.15, -0.15, 1.5], [0.15, -0.15, 1.5], [0.15, 0.15, 1.5], [-0.15, 0.15, 1.5]], np.float32)
    sd.meshes.append(abi.MeshData(vertices=bv, indices=np.array([[0, 1, 2], [0, 2, 3]], np.uint32)))
    sd.materials.append(abi.MaterialData(kind=abi.MAT_DIFFUSE, base_color=(0.0, 0.0, 0.0)))
    sd.instances.append(abi.InstanceData(1, [1], np.eye(4, dtype=np.float32).reshape(16).copy()))
    b = _render(sd, centre_cfg())[0]
    x = pixel_points(open_scene)
    px = 2 * 3.0 * math.tan(0.3) / 32
    sees_blocker = np.all(np.abs(pixel_points(open_scene, 1.5)[..., :2]) <= 0.15 + px, axis=-1)
    cheb = np.max(np.abs(x[..., :2]), axis=-1)
    umbra, lit = (cheb < 0.6 - px) & ~sees_blocker, cheb > 0.6 + px
    assert umbra.sum() >= 8 and lit.sum() > 300
    ia, ib = a[:3 * 1024].reshape(32, 32, 3), b[:3 * 1024].reshape(32, 32, 3)
    assert np.all(ib[umbra] == 0) and np.all(ia[lit] > 0) and n_bit_diff(ia[lit], ib[lit]) == 0


def test_no_nee_with_only_punctual_lights_is_black():
    sd = quad_scene()
    sd.lights = [point(), soft(spot(), 0.2), soft(sun(), 0.3)]
    film, st, _ = _render(sd, make_config(spp=4, max_depth=3, use_nee=0))
    assert not film[:6 * 1024].any() and st["n_shadow"] == 0 and st["n_shaded"] > 0
    lit, st2, _ = _render(sd, make_config(spp=4, max_depth=3))
    assert lit[:3 * 1024].any() and 0 < st2["n_shadow"] <= st2["n_shaded"]


@pytest.mark.parametrize("sampler", [abi.SAMPLER_INDEPENDENT, abi.SAMPLER_PMJ02BN, abi.SAMPLER_SOBOL], ids=["independent", "pmj02bn", "sobol"])
def test_lens_of_radius_zero_is_the_pinhole(hip_lib, sampler):
    sd = quad_scene(emissive=True)
    sd.lights = [point()]
    cfg = make_config(spp=4, max_depth=3, sampler_type=sampler, sampler_seed=5)
    pin = _render(sd, cfg)
    sd.lens = abi.LensData(0.0, 2.0)
    zero = _render(sd, cfg)
    assert n_bit_diff(pin[0], zero[0]) == 0 and pin[1] == zero[1] and np.array_equal(pin[2], zero[2])
    sd.lens = abi.LensData(0.3, 2.0)
    lens = _render(sd, cfg)
    assert n_bit_diff(pin[0], lens[0]) > 0
    if sampler == abi.SAMPLER_INDEPENDENT:  # two dimensions more per sample: the streams end elsewhere (an index sampler's state is the sample index)
        assert not np.array_equal(pin[2], lens[2])
    off = _render(sd, cfg, lens=False)  # the keyword that leaves the lens out
    assert n_bit_diff(pin[0], off[0]) == 0 and np.array_equal(pin[2], off[2])
    dark = _render(sd, cfg, lights=False, lens=False)
    sd.lights, sd.lens = [], None
    assert n_bit_diff(dark[0], _render(sd, cfg)[0]) == 0


def test_aov_ignores_lights_and_sees_the_lens():
    sd = quad_scene(emissive=True)
    a = abi.AovConfig.default()
    a.spp, a.aov = 4, 4
    plain = pyoracle.OracleScene(sd).aov_render(a)[0]
    sd.lights = [point(), sun()]
    assert n_bit_diff(plain, pyoracle.OracleScene(sd).aov_render(a)[0]) == 0
    sd.lens = abi.LensData(0.4, 1.0)
    assert n_bit_diff(plain, pyoracle.OracleScene(sd).aov_render(a)[0]) > 0


def test_gpt_and_mcmc_refuse():
    for kw in (dict(lights=[point()]), dict(lens=abi.LensData(0.1, 2.0))):
        sd = quad_scene(emissive=True)
        for k, v in kw.items():
            setattr(sd, k, v)
        osc = pyoracle.OracleScene(sd)
        g = abi.GptConfig.default()
        g.spp = 1
        film, aux = np.zeros(7 * 1024, F), np.zeros(3 * 1024 + 6 * 33 * 33, F)
        fp = C.POINTER(C.c_float)
        assert pyoracle.lib().or_gpt_render(osc.h, C.byref(g), film.ctypes.data_as(fp), aux.ctypes.data_as(fp), 1) == -5
        m = abi.McmcConfig.default()
        res, chains = np.zeros(4, np.float64), np.zeros(max(int(m.n_chains), 1), abi.MARKOV_STATE_DTYPE)
        assert pyoracle.lib().or_mcmc_render(osc.h, C.byref(m), film.ctypes.data_as(fp), res.ctypes.data_as(C.POINTER(C.c_double)),
                                             chains.ctypes.data_as(C.POINTER(C.c_uint32)), 1) == -5
