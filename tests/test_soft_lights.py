"""Soft shadows on the host: a radius for point and spot lights, an angle for the sun. The shared sampling text through
akr_host_light_sample_soft against the numpy restatement (tests/soft_light_model.py) bit for bit, size 0 against the hook of the delta lights, the
fold's record words, the setters, the scene.json reader, option soft_lights and the sun's energy. Host-only scenes (ctx = None): no GPU needed."""
import ctypes as C
import dataclasses
import math

import numpy as np
import pytest

from akari_render_amd import abi, capi
from tests import punctual_model as pm
from tests import soft_light_model as sm
from tests.test_punctual import assert_rows_equal, json_light, light_table, point, random_rows, scene_with, spot, sun, write_scene_with_lights
from tests.test_punctual import as_dict as delta_dict

F = np.float32
EPS = 2.0 ** -24
PI_BELOW = float(np.nextafter(F(math.pi), F(0)))  # the largest float32 below pi (the float32 nearest to pi is above it)


def soft(light, size):
    """the light with that radius (point, spot) or angle (sun)"""
    return dataclasses.replace(light, **({"angle": size} if light.type == abi.LIGHT_SUN else {"radius": size}))


def as_dict(l: abi.PunctualLightData) -> dict:
    return dict(delta_dict(l), radius=l.radius, angle=l.angle)


def model_records(scene):
    lights = iter(scene.punctual_lights())
    return [sm.fold(as_dict(next(lights))) if scene.light(i)[0] == capi.PUNCTUAL_LIGHT_INSTANCE else None for i in range(scene.info().n_lights)]


def random_rows9(n, seed, u_select=None):
    return np.c_[random_rows(n, seed, u_select), np.random.default_rng(seed + 1000).random((n, 2))].astype(F)


# u_sample where the text can go wrong: the corners, the centre (the warp's own special case), the last float32 below 1, one coordinate at the centre, and
# both sides of the warp's branch |sx| > |sy| on the diagonal and the anti-diagonal
U_EDGE = [(0.0, 0.0), (0.5, 0.5), (1 - EPS, 1 - EPS), (0.0, 1 - EPS), (1 - EPS, 0.0), (0.5, 0.3), (0.3, 0.5), (0.5, 0.0), (0.0, 0.5),
          (0.75, 0.75), (0.75 + 2 * EPS, 0.75), (0.75, 0.75 + 2 * EPS), (0.25, 0.75), (0.25 - EPS, 0.75), (0.25, 0.75 + 2 * EPS), (0.25, 0.25), (0.25 + EPS, 0.25)]


def edge_rows9(light: abi.PunctualLightData):
    """every point below with every u of U_EDGE: p == q, p inside the disk (closer to q than the radius, in front, behind and beside), p on the spot's axis,
    zero components of either sign, a point 10^6 units away"""
    up = (0.0, 0.0, 1.0)
    q = np.asarray(light.position, np.float64)
    pts = [(*q.astype(F), *up)]
    r = max(float(light.radius), 1e-3)
    for off in ((0.0, 0.0, -0.25 * r), (0.0, 0.0, 0.25 * r), (0.3 * r, -0.2 * r, 0.0), (0.1 * r, 0.1 * r, -0.01 * r)):
        pts.append((*(q + off).astype(F), *up))
    for z in (0.0, -0.0):
        pts.append((z, -z, z, 0.0, -0.0, 1.0))
        pts.append((0.5, z, -z, -0.0, 1.0, 0.0))
    pts.append((1e6, -1e6, 1e6, *up))
    if light.type == abi.LIGHT_SPOT:
        a = pm.fold(delta_dict(light))["a"].astype(np.float64)
        for t in (0.5 * r, 1.0, 3.0):
            pts.append((*(q + t * a).astype(F), *up))
    return np.asarray([(*pt, 0.5, *u) for pt in pts for u in U_EDGE], F)


KINDS = {"point": point(), "spot": spot(), "spot_step": spot(blend=0.0), "spot_axis_aligned": spot(position=(0.0, 0.0, 1.0), direction=(0.0, 0.0, -2.0), cone_angle=0.4, blend=0.5),
         "sun": sun(), "sun_axis_aligned": sun(direction=(0.0, 0.0, -1.0))}


def sizes(light, edge=False):
    if light.type == abi.LIGHT_SUN:
        return (1e-4, math.pi - 1e-3) if edge else (0.02, 1.0)
    return (1e-6, 1e3) if edge else (0.05, 0.7)


def check_against_model(light, rows):
    sc = scene_with([light])
    assert sc.info().n_lights == 1 and sc.light(0)[0] == capi.PUNCTUAL_LIGHT_INSTANCE
    recs = model_records(sc)
    assert sm.is_soft(recs[0])
    got = sc.host_light_sample_soft(rows)
    assert_rows_equal(got, sm.light_sample_rows(light_table(sc), recs, rows))
    return got[0]


@pytest.mark.parametrize("which", [0, 1], ids=["small", "large"])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_host_sample_equals_the_model_on_random_rows(hip_lib, kind, which):
    light = soft(KINDS[kind], sizes(KINDS[kind])[which])
    rows = random_rows9(4096, 21 + which)
    out = check_against_model(light, rows)
    assert np.all(out[:, 12] == 1) and np.all(out[:, 6] == 1)  # delta stays set; pdf = the selection probability of the only light
    assert out[:, 11].mean() > (0.02 if light.type == abi.LIGHT_SPOT else 0.99)
    # the sample does depend on u_sample: the same rows with another u give other directions
    other = rows.copy()
    other[:, 7:9] = 1 - other[:, 7:9]
    assert np.mean(np.any(scene_with([light]).host_light_sample_soft(other)[0][:, 3:6] != out[:, 3:6], axis=1)) > 0.99


@pytest.mark.parametrize("which", [0, 1, 2, 3], ids=["small", "large", "tiny", "huge"])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_host_sample_equals_the_model_on_edge_rows(hip_lib, kind, which):
    base = KINDS[kind]
    light = soft(base, (sizes(base) + sizes(base, edge=True))[which])
    rows = edge_rows9(light)
    out = check_against_model(light, rows)
    if light.type != abi.LIGHT_SUN:
        n = len(U_EDGE)
        assert not out[:n, 11].any() and not out[:n, :6].any()  # p == q is invalid whatever u
        assert np.all(out[out[:, 11] == 1][:, 0:3].min(axis=1) >= 0)
    else:
        wi = out[:, 3:6].astype(np.float64)
        assert np.all(np.abs(np.linalg.norm(wi, axis=1) - 1) < 16 * EPS)  # unit directions
        a = pm.fold(delta_dict(base))["a"].astype(np.float64)
        assert np.all(-(wi @ a) >= math.cos(0.5 * light.angle) - 16 * EPS)  # inside the cap


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_size_zero_is_the_delta_light_for_every_u(hip_lib, kind):
    """radius 0 / angle 0: the new hook answers what the old hook answers, whatever u_sample is"""
    light = KINDS[kind]
    assert light.radius == 0 and light.angle == 0
    sc = scene_with([light])
    rows = np.concatenate([random_rows9(4096, 31), edge_rows9(light)])
    got = sc.host_light_sample_soft(rows)
    assert_rows_equal(got, sc.host_light_sample(rows[:, :7]))
    assert_rows_equal(got, sm.light_sample_rows(light_table(sc), model_records(sc), rows))
    # the size the kind does not read changes nothing either
    ignored = dataclasses.replace(light, **({"radius": 0.5} if light.type == abi.LIGHT_SUN else {"angle": 0.5}))
    assert_rows_equal(scene_with([ignored]).host_light_sample_soft(rows), got)


def test_record_words_and_selection(hip_lib):
    from tests.test_punctual import two_emitter_scene
    hard = [point(), spot(), sun()]
    lights = [soft(hard[0], 0.3), soft(hard[1], 0.125), soft(hard[2], 0.4)]
    scenes = []
    for ls in (lights, hard):
        sd = two_emitter_scene()
        sd.lights, sd.environment = ls, abi.EnvironmentData(color=(0.5, 0.6, 0.7))
        scenes.append(capi.Scene(None, sd))
    sc, ref = scenes
    words = sc.array(capi.ARRAY_PUNCTUAL_LIGHTS, np.uint32).reshape(3, 16)
    for k, l in enumerate(lights):
        rec = sm.fold(as_dict(l))
        assert np.array_equal(words[k], sm.record_words(rec)), (k, words[k], sm.record_words(rec))
    assert words[0, 13:14].view(F)[0] == F(0.3) and not words[0, 14:].any() and not words[2, 13] and words[2, 14:].all()
    # size 0: what used to be padding is zero
    assert not ref.array(capi.ARRAY_PUNCTUAL_LIGHTS, np.uint32).reshape(3, 16)[:, 13:].any()
    # the selection does not look at the size
    n = sc.info().n_lights
    assert n == 6 and [sc.light(i) for i in range(n)] == [ref.light(i) for i in range(n)]
    for a, b in zip(light_table(sc), light_table(ref)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # a mixed list: each row is the sample of whichever light the table picks
    rows = random_rows9(4096, 5)
    got = sc.host_light_sample_soft(rows)
    assert_rows_equal(got, sm.light_sample_rows(light_table(sc), model_records(sc), rows))
    assert set(np.unique(got[1])) == set(range(6))


def test_setters_getters_and_struct_size(hip_lib):
    hip_lib.akr_struct_size.restype = C.c_uint32
    assert hip_lib.akr_struct_size(24) == C.sizeof(abi.PunctualLightDesc) == 60
    assert abi.PunctualLightDesc.radius.offset == 52 and abi.PunctualLightDesc.angle.offset == 56  # trailing: what came before keeps its place
    assert abi.PunctualLightData(abi.LIGHT_POINT).radius == 0.0 and abi.PunctualLightData(abi.LIGHT_SUN).angle == 0.0
    assert hip_lib.akr_version().startswith(b"akari_hip 0.3.") and int(hip_lib.akr_version().split()[1].split(b".")[2]) >= 8
    sc = scene_with([])
    sc.add_punctual_light(soft(point(), 0.25))
    sc.add_punctual_light(type=abi.LIGHT_SPOT, position=(0, 0, 1), direction=(0, 0, -1), cone_angle=0.5, radius=0.125)
    sc.add_punctual_light(type=abi.LIGHT_SUN, direction=(0, 0, -1), angle=0.5)
    sc.add_punctual_light(type=abi.LIGHT_SUN, direction=(0, 0, -1), angle=PI_BELOW)
    got = sc.punctual_lights()
    assert [(l.radius, l.angle) for l in got] == [(0.25, 0.0), (0.125, 0.0), (0.0, 0.5), (0.0, PI_BELOW)]
    assert sc.to_scene_data().lights == got
    # what the kind does not read is ignored, whatever it is, and reads back as 0
    sc.clear_punctual_lights()
    sc.add_punctual_light(type=abi.LIGHT_SUN, direction=(0, 0, -1), radius=5.0)
    sc.add_punctual_light(type=abi.LIGHT_SUN, direction=(0, 0, -1), radius=float("nan"))
    sc.add_punctual_light(type=abi.LIGHT_POINT, angle=1.0)
    sc.add_punctual_light(type=abi.LIGHT_SPOT, position=(0, 0, 1), direction=(0, 0, -1), cone_angle=0.5, angle=-4.0)
    sc.add_punctual_light(type=abi.LIGHT_POINT, radius=-0.0)  # a negative zero is zero: the record's words stay zero bits
    sc.add_punctual_light(type=abi.LIGHT_SUN, direction=(0, 0, -1), angle=-0.0)
    assert [(l.radius, l.angle) for l in sc.punctual_lights()] == [(0.0, 0.0)] * 6
    assert not np.signbit([v for l in sc.punctual_lights() for v in (l.radius, l.angle)]).any()
    assert not sc.array(capi.ARRAY_PUNCTUAL_LIGHTS, np.uint32).reshape(6, 16)[:, 13:].any()
    for bad in (dict(type=abi.LIGHT_POINT, radius=-1.0), dict(type=abi.LIGHT_POINT, radius=float("nan")), dict(type=abi.LIGHT_POINT, radius=float("inf")),
                dict(type=abi.LIGHT_SPOT, position=(0, 0, 1), direction=(0, 0, -1), cone_angle=0.5, radius=-0.5),
                dict(type=abi.LIGHT_SUN, direction=(0, 0, -1), angle=-0.1), dict(type=abi.LIGHT_SUN, direction=(0, 0, -1), angle=float("nan")),
                dict(type=abi.LIGHT_SUN, direction=(0, 0, -1), angle=float(F(math.pi))), dict(type=abi.LIGHT_SUN, direction=(0, 0, -1), angle=4.0),
                dict(type=abi.LIGHT_SUN, direction=(0, 0, -1), angle=float("inf"))):
        with pytest.raises(capi.AkariError) as e:
            sc.add_punctual_light(**bad)
        assert e.value.code == capi.ERR_INVALID_ARGUMENT, bad
    assert len(sc.punctual_lights()) == 6


def soft_json_light(l):
    j = json_light(l)
    if l.type == abi.LIGHT_SUN:
        j["data"]["angle"] = l.angle
    else:
        j["data"]["radius"] = l.radius
    return j


def records(scene):
    return scene.array(capi.ARRAY_PUNCTUAL_LIGHTS, np.uint32).copy()


def test_reader_round_trip_defaults_and_option(hip_lib, tmp_path):
    hard = [point(), spot(cone_angle=0.375, blend=0.25), sun()]
    lights = [soft(hard[0], 0.25), soft(hard[1], 0.125), soft(hard[2], 0.5)]
    path = write_scene_with_lights(tmp_path, {"a": soft_json_light(lights[0]), "b": soft_json_light(lights[1]), "c": soft_json_light(lights[2])})
    loaded, api = capi.Scene(None, path), scene_with(lights, width=16, height=16)
    assert loaded.punctual_lights() == api.punctual_lights() and [l.radius + l.angle for l in loaded.punctual_lights()] == [0.25, 0.125, 0.5]
    assert np.array_equal(records(loaded), records(api)) and records(api).reshape(3, 16)[:, 13:].any(axis=1).all()
    # defaults: a file without the keys loads to the scene it loaded to before -- size 0, zeros where the padding was
    plain = write_scene_with_lights(tmp_path, {"a": json_light(hard[0]), "b": json_light(hard[1]), "c": json_light(hard[2])})
    delta = scene_with(hard, width=16, height=16)
    assert capi.Scene(None, plain).punctual_lights() == delta.punctual_lights() and np.array_equal(records(capi.Scene(None, plain)), records(delta))
    assert not records(delta).reshape(3, 16)[:, 13:].any()
    # the key of the other kind is not read
    swapped = {"a": json_light(hard[0]), "c": json_light(hard[2])}
    swapped["a"]["data"]["angle"], swapped["c"]["data"]["radius"] = 0.5, 0.5
    assert capi.Scene(None, write_scene_with_lights(tmp_path, swapped)).punctual_lights() == [delta.punctual_lights()[0], delta.punctual_lights()[2]]
    # a bad value names the light
    bad = soft_json_light(lights[0])
    bad["data"]["radius"] = -1.0
    with pytest.raises(capi.AkariError) as e:
        capi.Scene(None, write_scene_with_lights(tmp_path, {"the_lamp": bad}))
    assert "the_lamp" in str(e.value)
    # option soft_lights = 0: every light of the file as a delta light
    path = write_scene_with_lights(tmp_path, {"a": soft_json_light(lights[0]), "b": soft_json_light(lights[1]), "c": soft_json_light(lights[2])})  # (one file name: written again)
    with capi.options(soft_lights=0):
        off = capi.Scene(None, path)
        assert off.punctual_lights() == delta.punctual_lights() and np.array_equal(records(off), records(delta))
        assert scene_with(lights).punctual_lights() == api.punctual_lights()  # (the setters are not the reader)
    assert capi.get_option("soft_lights") == 1
    with pytest.raises(capi.AkariError):
        capi.set_option("soft_lights", 2)


@pytest.mark.parametrize("angle", [0.5, 2.5])
def test_sun_energy(hip_lib, angle):
    """A surface facing the sun receives the irradiance E whatever the angle: the mean of li * max(dot(wi, n), 0) over a 256 x 256 grid of cell centres.

    The bound. li * cos = E k (1 - u.x (1 - cos_max)) is linear in u.x and does not depend on u.y, so the midpoint rule over cells of width h = 1 / 256 has
    the error h^2 / 24 * max |d^2/du^2| = 0: what is left is rounding. The grid's u are exact in float32. Per sample: k and c k are rounded once each
    (2^-24 relative each), cos is dot(wi, n) of a direction whose components carry the roundings of ct (two), st (three), sincos (2 ulp), three products
    and two sums each, dotted with the rounded axis (three products, two sums): fewer than 16 roundings of values <= 1, so < 16 x 2^-24 absolute, times
    li <= 2 E. The mean of errors is at most their maximum: |mean - E| <= 2 E x 16 x 2^-24 + E x 2 x 2^-24 < 40 x 2^-24 E."""
    light = sun(direction=(0.2, -0.1, -1.0), color=(1.0, 0.9, 0.8), strength=3.0)
    sc = scene_with([soft(light, angle)])
    n = -pm.fold(delta_dict(light))["a"]
    g = (np.arange(256) + 0.5) / 256
    u = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    rows = np.c_[np.zeros((len(u), 3)), np.repeat(n[None, :], len(u), axis=0), np.full(len(u), 0.5), u].astype(F)
    out = sc.host_light_sample_soft(rows)[0].astype(np.float64)
    assert np.all(out[:, 11] == 1)
    cos = np.maximum(out[:, 3:6] @ n.astype(np.float64), 0.0)
    mean = (out[:, 0:3] * cos[:, None]).mean(axis=0)
    E = np.asarray(light.color, F).astype(np.float64) * float(F(light.strength))
    print(f"sun energy, angle {angle}: mean / E - 1 = {mean / E - 1}")
    assert np.all(np.abs(mean - E) <= 40 * EPS * E)
    assert cos.min() < math.cos(0.5 * angle) + 0.01 and cos.max() > 1 - 0.01 * angle  # the grid does cover the cap
