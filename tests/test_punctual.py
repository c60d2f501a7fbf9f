"""Point, spot and sun lights on the host: the shared sampling text through akr_host_light_sample against the numpy restatement
(tests/punctual_model.py) bit for bit, the lights' entries in the light table, the scene.json reader, the launch plan and the refusals that need no
device. Host-only scenes (ctx = None): no GPU needed."""
import json
import math

import numpy as np
import pytest

from akari_render_amd import abi, capi
from tests import punctual_model as pm
from tests.helpers import make_config
from tests.test_environment import ALIAS, quad_scene, scene_json_text

F = np.float32
PI_2 = float(F(math.pi / 2))


def point(position=(0.3, -0.2, 1.5), color=(3.0, 2.0, 1.0), strength=2.0):
    return abi.PunctualLightData(abi.LIGHT_POINT, position=position, color=color, strength=strength)


def spot(position=(0.25, 0.5, 2.0), direction=(0.1, -0.3, -1.0), cone_angle=0.5, blend=0.3, color=(1.0, 4.0, 2.0), strength=1.5):
    return abi.PunctualLightData(abi.LIGHT_SPOT, position=position, direction=direction, color=color, strength=strength, cone_angle=cone_angle, blend=blend)


def sun(direction=(0.2, -0.1, -1.0), color=(1.0, 0.9, 0.8), strength=3.0):
    return abi.PunctualLightData(abi.LIGHT_SUN, direction=direction, color=color, strength=strength)


def as_dict(l: abi.PunctualLightData) -> dict:
    return dict(type=l.type, position=l.position, direction=l.direction, color=l.color, strength=l.strength, cone_angle=l.cone_angle, blend=l.blend)


def scene_with(lights, ctx=None, **kw) -> capi.Scene:
    sd = quad_scene(**kw)
    sd.lights = list(lights)
    return capi.Scene(ctx, sd)


def light_table(scene):
    e = scene.array(capi.ARRAY_LIGHT_ENTRIES, ALIAS)
    return e["j"].copy(), e["t"].copy(), scene.array(capi.ARRAY_LIGHT_PDF, np.float32).copy()


def model_records(scene):
    """per light of the scene's list: the model's record of the punctual ones (from the descriptions the scene holds), None for the others"""
    lights = iter(scene.punctual_lights())
    return [pm.fold(as_dict(next(lights))) if scene.light(i)[0] == capi.PUNCTUAL_LIGHT_INSTANCE else None for i in range(scene.info().n_lights)]


def random_rows(n, seed, u_select=None):
    rng = np.random.default_rng(seed)
    p = np.c_[rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(-0.2, 0.2, n)]
    nrm = rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    u = rng.random(n) if u_select is None else np.full(n, u_select)
    return np.c_[p, nrm, u].astype(F)


def edge_rows(light: abi.PunctualLightData):
    """the rows where the text can go wrong: p == q, the cone's axis, ct within an ulp of cos_o and cos_i, zero components of either sign"""
    rows = []
    up = (0.0, 0.0, 1.0)
    q = np.asarray(light.position, F)
    rows.append((*q, *up, 0.5))  # p == q (the sun has no q: an ordinary row)
    for z in (0.0, -0.0):
        rows.append((z, -z, z, 0.0, -0.0, 1.0, 0.5))
        rows.append((0.5, z, -z, -0.0, 1.0, 0.0, 0.5))
    rows.append((1e6, -1e6, 1e6, *up, 0.5))  # a light 10^6 units away
    if light.type == abi.LIGHT_SPOT:
        rec = pm.fold(as_dict(light))
        a = rec["a"].astype(np.float64)
        for t in (0.5, 1.0, 3.0):
            rows.append((*(q.astype(np.float64) + t * a).astype(F), *up, 0.5))  # on the axis
        # a fan of points whose angle to the axis steps through the two cone angles in float32 steps: perpendicular b, p = q + a + tan(theta) b
        b = np.cross(a, [1.0, 0.0, 0.0])
        b /= np.linalg.norm(b)
        for cos_edge in (float(rec["cos_o"]), float(rec["cos_i"])):
            if cos_edge <= 1e-6:
                continue
            tan0 = math.sqrt(max(1.0 - cos_edge * cos_edge, 0.0)) / cos_edge
            for k in range(-400, 401):
                tt = tan0 * (1.0 + k * 2.0 ** -24)
                rows.append((*(q.astype(np.float64) + 4.0 * (a + tt * b)).astype(F), *up, 0.5))
    return np.asarray(rows, F)


KINDS = {
    "point": [point()],
    "spot": [spot()],
    "spot_step": [spot(blend=0.0)],
    "spot_wide": [spot(cone_angle=PI_2, blend=1.0)],
    "spot_axis_aligned": [spot(position=(0.0, 0.0, 1.0), direction=(0.0, 0.0, -2.0), cone_angle=0.4, blend=0.5)],
    "sun": [sun()],
    "sun_axis_aligned": [sun(direction=(0.0, 0.0, -1.0))],
}


def assert_rows_equal(got, want):
    (go, gl), (wo, wl) = got, want
    assert np.array_equal(gl, wl)
    bad = np.nonzero((go.view(np.uint32) != wo.view(np.uint32)).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} rows differ, first {bad[0]}: {go[bad[0]]} vs {wo[bad[0]]}"


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_host_sample_equals_the_model_bit_for_bit(hip_lib, kind):
    lights = KINDS[kind]
    sc = scene_with(lights)
    assert sc.info().n_lights == 1 and sc.light(0)[0] == capi.PUNCTUAL_LIGHT_INSTANCE
    rows = np.concatenate([random_rows(4096, 11), edge_rows(lights[0])])
    got = sc.host_light_sample(rows)
    want = pm.light_sample_rows(light_table(sc), model_records(sc), rows)
    assert_rows_equal(got, want)
    out = got[0]
    assert np.all(out[:, 12] == 1) and np.all(out[:, 6] == 1)  # delta, pdf = the selection probability of the only light
    if lights[0].type != abi.LIGHT_SUN:
        assert out[4096, 11] == 0 and not out[4096, :6].any()  # p == q is invalid
    if lights[0].type == abi.LIGHT_SPOT:
        assert 0 < out[:4096, 11].mean() < 1 or kind == "spot_wide"  # both sides of the cone among the random rows
        assert np.all(out[out[:, 11] == 0][:, 0:3] == 0)  # nothing outside the cone


def test_edge_rows_reach_both_sides_of_each_cosine(hip_lib):
    """the fan of edge_rows does put ct within one ulp of cos_o and of cos_i, on either side (the model's own ct)"""
    l = spot()
    rec = pm.fold(as_dict(l))
    rows = edge_rows(l)
    d = rec["q"][None, :] - rows[:, 0:3]
    dist = np.sqrt(pm._dot(d, d))
    with np.errstate(all="ignore"):
        wi = d * (F(1) / dist)[:, None]
        ct = -pm._dot(wi, np.repeat(rec["a"][None, :], len(rows), axis=0))
    for edge in (rec["cos_o"], rec["cos_i"]):
        assert np.nextafter(edge, F(2)) in ct and np.nextafter(edge, F(-2)) in ct


def test_selection_over_a_mixed_light_list(hip_lib):
    """emitter, one light of each kind, environment: the sample of whichever the alias table picks, or just its pdf"""
    sd = quad_scene(emissive=True)
    sd.lights = [point(), spot(), sun()]
    sd.environment = abi.EnvironmentData(color=(0.5, 0.6, 0.7))
    sc = capi.Scene(None, sd)
    rows = random_rows(4096, 5)
    got = sc.host_light_sample(rows)
    assert_rows_equal(got, pm.light_sample_rows(light_table(sc), model_records(sc), rows))
    assert set(np.unique(got[1])) == set(range(5))
    assert np.all(got[0][np.isin(got[1], (0, 4))][:, 12] == 0)  # an emitter or the environment: not a delta light


def two_emitter_scene():
    sd = quad_scene(emissive=True)
    lv = np.array([[0.5, 0.5, 0.4], [0.8, 0.5, 0.4], [0.8, 0.8, 0.4], [0.5, 0.8, 0.4]], dtype=np.float32)
    sd.meshes.append(abi.MeshData(vertices=lv, indices=np.array([[0, 2, 1], [0, 3, 2]], dtype=np.uint32)))
    sd.materials.append(abi.MaterialData(kind=abi.MAT_EMISSION, emission_color=(1.0, 2.0, 0.5), emission_strength=3.0))
    sd.instances.append(abi.InstanceData(2, [2], np.eye(4, dtype=np.float32).reshape(16).copy()))
    return sd


def test_light_table_powers_and_pdfs(hip_lib):
    sd = two_emitter_scene()
    bare = capi.Scene(None, sd)
    assert bare.info().n_lights == 2
    sd.lights = [point(), spot(), sun()]
    sd.environment = abi.EnvironmentData(color=(0.5, 0.6, 0.7))
    sc = capi.Scene(None, sd)
    n = sc.info().n_lights
    assert n == 6
    inst = [sc.light(i)[0] for i in range(n)]
    assert inst[:2] == [bare.light(0)[0], bare.light(1)[0]] and inst[2:5] == [capi.PUNCTUAL_LIGHT_INSTANCE] * 3 and inst[5] == capi.ENV_LIGHT_INSTANCE
    powers = np.array([sc.light(i)[1] for i in range(n)], F)
    assert powers[0] == F(bare.light(0)[1]) and powers[1] == F(bare.light(1)[1])  # the emitters' own estimates are untouched
    verts = np.concatenate([np.asarray(m.vertices, F).reshape(-1, 3) for m in sd.meshes])  # (identity transforms)
    R = pm.bounds_radius(verts.min(axis=0), verts.max(axis=0))
    recs = [pm.fold(as_dict(l)) for l in sd.lights]
    want = np.array([pm.power(r, R) for r in recs], F)
    assert np.array_equal(powers[2:5].view(np.uint32), want.view(np.uint32)), (powers[2:5], want)
    pdf = np.array([sc.light(i)[2] for i in range(n)], F)
    assert np.array_equal(pdf.view(np.uint32), pm.selection_pdfs(powers).view(np.uint32))
    assert abs(float(np.sum(pdf.astype(np.float64))) - 1.0) <= 4 * 2.0 ** -24
    # the records the kernels read
    rec = sc.array(capi.ARRAY_PUNCTUAL_LIGHTS, np.float32).reshape(3, 16)
    for k, r in enumerate(recs):
        assert np.array_equal(rec[k, 0:3], r["q"]) and rec[k, 3:4].view(np.uint32)[0] == r["kind"]
        assert np.array_equal(rec[k, 4:7], r["a"]) and rec[k, 7] == r["cos_o"]
        assert np.array_equal(rec[k, 8:11], r["c"]) and rec[k, 11] == r["cos_i"] and rec[k, 12] == r["inv_span"]
    # only punctual lights: a valid light list
    only = scene_with([point(), sun()])
    assert only.info().n_lights == 2 and abs(only.light(0)[2] + only.light(1)[2] - 1.0) < 1e-6


def test_setters_and_no_light(hip_lib):
    sc = scene_with([])
    assert sc.punctual_lights() == [] and sc.info().n_lights == 0
    sc.add_punctual_light(point(strength=0.0))
    sc.add_punctual_light(spot(color=(0.0, 0.0, 0.0)))
    assert sc.punctual_lights() == [] and sc.info().n_lights == 0  # strength 0 / an all-zero colour: no light
    sc.add_punctual_light(spot())
    sc.add_punctual_light(type=abi.LIGHT_SUN, direction=(0, 0, -3), strength=2.0)
    got = sc.punctual_lights()
    assert len(got) == 2 and got[0].type == abi.LIGHT_SPOT and got[1].direction == (0.0, 0.0, -3.0) and sc.info().n_lights == 2
    assert sc.to_scene_data().lights == got
    for bad in (dict(type=7), dict(type=abi.LIGHT_SUN, direction=(0, 0, 0)), dict(type=abi.LIGHT_SPOT, direction=(0, float("nan"), 1), cone_angle=0.3),
                dict(type=abi.LIGHT_SPOT, direction=(0, 0, -1), cone_angle=0.0), dict(type=abi.LIGHT_SPOT, direction=(0, 0, -1), cone_angle=2.0),
                dict(type=abi.LIGHT_SPOT, direction=(0, 0, -1), cone_angle=0.3, blend=1.5), dict(type=abi.LIGHT_POINT, strength=-1.0),
                dict(type=abi.LIGHT_POINT, position=(float("inf"), 0, 0)), dict(type=abi.LIGHT_POINT, color=(1, -1, 1))):
        with pytest.raises(capi.AkariError) as e:
            sc.add_punctual_light(**bad)
        assert e.value.code == capi.ERR_INVALID_ARGUMENT
    assert len(sc.punctual_lights()) == 2
    sc.clear_punctual_lights()
    assert sc.punctual_lights() == [] and sc.info().n_lights == 0
    # with an environment the punctual lights stay in front of it, however the two are set
    sc.set_environment(color=(1, 1, 1))
    sc.add_punctual_light(point())
    assert [sc.light(i)[0] for i in range(2)] == [capi.PUNCTUAL_LIGHT_INSTANCE, capi.ENV_LIGHT_INSTANCE]
    sc.set_environment(color=(2, 1, 1))
    assert [sc.light(i)[0] for i in range(2)] == [capi.PUNCTUAL_LIGHT_INSTANCE, capi.ENV_LIGHT_INSTANCE]
    sc.clear_punctual_lights()
    assert [sc.light(i)[0] for i in range(sc.info().n_lights)] == [capi.ENV_LIGHT_INSTANCE]


# ---------------------------------------------------------------------------------------------------------------- scene.json
def write_scene_with_lights(tmp_path, lights: dict):
    path = scene_json_text(tmp_path, None, with_env=False)
    doc = json.load(open(path))
    doc["lights"] = lights
    open(path, "w").write(json.dumps(doc))
    return path


def json_light(l: abi.PunctualLightData) -> dict:
    name = {abi.LIGHT_POINT: "point", abi.LIGHT_SPOT: "spot", abi.LIGHT_SUN: "sun"}[l.type]
    data = {"color": list(l.color), "strength": l.strength}
    if l.type != abi.LIGHT_SUN:
        data["position"] = list(l.position)
    if l.type != abi.LIGHT_POINT:
        data["direction"] = list(l.direction)
    if l.type == abi.LIGHT_SPOT:
        data["spot_size"], data["spot_blend"] = 2.0 * l.cone_angle, l.blend
    return {"type": name, "data": data}


def test_reader_round_trip(hip_lib, tmp_path):
    lights = [point(), spot(cone_angle=0.375, blend=0.25), sun()]  # (values a float32 holds exactly, so that spot_size / 2 gives them back)
    path = write_scene_with_lights(tmp_path, {"a": json_light(lights[0]), "b": json_light(lights[1]), "c": json_light(lights[2]),
                                              "reference_shaped": {"type": "point", "data": {}}})
    loaded = capi.Scene(None, path)
    api = scene_with(lights, width=16, height=16)
    got, want = loaded.punctual_lights(), api.punctual_lights()
    assert len(got) == 3 and got == want
    assert np.array_equal(loaded.array(capi.ARRAY_PUNCTUAL_LIGHTS, np.uint32), api.array(capi.ARRAY_PUNCTUAL_LIGHTS, np.uint32))
    assert [loaded.light(i) for i in range(3)] == [api.light(i) for i in range(3)]
    # defaults: colour 1, 1, 1
    d = capi.Scene(None, write_scene_with_lights(tmp_path, {"p": {"type": "point", "data": {"position": [0, 0, 1], "strength": 2.0}}})).punctual_lights()
    assert d[0].color == (1.0, 1.0, 1.0) and d[0].strength == 2.0
    # the reference's own entry alone: the scene of a file without lights
    assert capi.Scene(None, write_scene_with_lights(tmp_path, {"l": {"type": "point", "data": {}}})).info().n_lights == 0
    # a strength-0 light is no light
    zero = dict(json_light(point()))
    zero["data"] = dict(zero["data"], strength=0.0)
    assert capi.Scene(None, write_scene_with_lights(tmp_path, {"z": zero})).punctual_lights() == []
    with capi.options(punctual_lights=0):
        assert capi.Scene(None, path).punctual_lights() == [] and capi.Scene(None, path).info().n_lights == 0
    assert capi.get_option("punctual_lights") == 1


@pytest.mark.parametrize("entry", [{"type": "laser", "data": {"position": [0, 0, 1]}}, {"type": "point", "data": {"strength": 1.0}},
                                   {"type": "spot", "data": {"position": [0, 0, 1], "spot_size": 1.0}}, {"type": "sun", "data": {"strength": 1.0}},
                                   {"type": "spot", "data": {"position": [0, 0, 1], "direction": [0, 0, -1]}}], ids=["type", "point_position", "spot_direction", "sun_direction", "spot_size"])
def test_reader_parse_errors(hip_lib, tmp_path, entry):
    with pytest.raises(capi.AkariError) as e:
        capi.Scene(None, write_scene_with_lights(tmp_path, {"the_lamp": entry}))
    assert e.value.code == capi.ERR_PARSE and "the_lamp" in str(e.value)


# ---------------------------------------------------------------------------------------------------------------- plans and refusals
def test_launch_plan_answers_punct(hip_lib):
    cfg = make_config(spp=4)
    lit, bare = scene_with([point()]), scene_with([])
    plan, plain = lit.launch_plan(cfg), bare.launch_plan(cfg)
    assert plan["variant"]["punct"] == 1 and plain["variant"]["punct"] == 0
    assert plan["variant"]["defer"] == 0 and plan["variant"]["simple"] == 0 and plan["simple_scene"] == 0 and plan["defer_metal"] == 0
    assert plain["variant"]["simple"] == 1  # what the light took away
    assert plan["stage_bytes"][4] == 16 and plan["stage_bytes"][6] == 16 and plan["stage_bytes"][7] == 4  # its entries in the staged light tables
    assert scene_with([point()]).launch_plan(cfg, defer_metal=1)["variant"]["defer"] == 0
    fp = lit.features_plan(cfg, feat=False)
    assert fp["variant"]["punct"] == 1 and fp["kernel_compiled"] == 1
    # a lens and an environment beside it: the other two units
    sd = quad_scene()
    sd.lights, sd.lens, sd.environment = [sun()], abi.LensData(0.05, 3.0), abi.EnvironmentData(color=(1, 1, 1))
    v = capi.Scene(None, sd).launch_plan(cfg)["variant"]
    assert (v["punct"], v["lens"], v["env"]) == (1, 1, 1)
    # three strength-0 lights: the plan of the scene without them
    same = scene_with([point(strength=0.0)] * 3).launch_plan(cfg)
    assert same == plain


def test_refusals_that_need_no_device(hip_lib):
    cfg = make_config(spp=4)
    lit = scene_with([spot()])
    for kw in (dict(), dict(wavefront=1), dict(arith=1)):
        with pytest.raises(capi.AkariError) as e:
            lit.features_plan(cfg, feat=True, **kw)
        assert e.value.code == capi.ERR_UNSUPPORTED
    with pytest.raises(capi.AkariError) as e:
        lit.features_plan(cfg, feat=True)
    assert "spot light" in str(e.value)
    # a scene kept as meshes + instances
    from tests.helpers import instanced_scene
    sd = instanced_scene()
    sd.lights = [point()]
    with capi.options(instancing=1):
        kept = capi.Scene(None, instanced_scene())
        assert kept.info().uses_bvh == 2
        with pytest.raises(capi.AkariError) as e:
            capi.Scene(None, sd)
        assert e.value.code == capi.ERR_UNSUPPORTED and "point light" in str(e.value)
        with pytest.raises(capi.AkariError) as e:
            kept.add_punctual_light(sun())
        assert e.value.code == capi.ERR_UNSUPPORTED and "sun light" in str(e.value) and kept.punctual_lights() == []
    assert capi.Scene(None, sd).info().uses_bvh == 1  # the automatic choice flattens it: lit, not refused
    assert capi.Scene(None, sd).launch_plan(cfg)["variant"]["punct"] == 1
