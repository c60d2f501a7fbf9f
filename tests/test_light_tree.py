"""The light tree on the host: the node words of akr_scene_get_array against the numpy restatement (tests/light_tree_model.py) bit for
bit, the light table with the tree's one entry, the shared walk through akr_host_light_tree_sample against the model bit for bit, the partition of
unity of the walk (independent of the model), mode off = a scene that never heard of the mode, and the variance the model predicts for a grid of lights.
Host-only scenes (ctx = None): no GPU needed."""
import json
import math

import numpy as np
import pytest

from akari_render_amd import abi, capi
from tests import light_tree_model as lt
from tests import punctual_model as pm
from tests import soft_light_model as sm
from tests.test_environment import ALIAS, quad_scene
from tests.test_punctual import json_light, light_table, point, spot, sun, two_emitter_scene, write_scene_with_lights
from tests.test_soft_lights import as_dict, random_rows9

F = np.float32
SIZES = [2, 3, 5, 8, 33, 257]
U_TOP = float(lt.U_TOP)


def local_lights(n, seed, arrangement="random"):
    """n point / spot lights over the quad: "random" (every third one soft, every fourth a spot), "repeats" (positions drawn from n / 3 + 1 places: ties
    broken by index), "line" (all on one axis-aligned line), "one_point" (all at one place)"""
    rng = np.random.default_rng(seed)
    pos = np.c_[rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(0.2, 1.5, n)]
    if arrangement == "repeats":
        pos = pos[rng.integers(0, n // 3 + 1, n)]
    elif arrangement == "line":
        pos[:, 0], pos[:, 2] = 0.25, 0.5
    elif arrangement == "one_point":
        pos[:] = (0.25, -0.5, 0.75)
    out = []
    for k in range(n):
        radius = float(F(rng.uniform(0.02, 0.3))) if k % 3 == 1 else 0.0
        strength = float(F(rng.uniform(0.5, 4.0)))
        where = tuple(float(v) for v in pos[k].astype(F))
        if k % 4 == 3:
            out.append(abi.PunctualLightData(abi.LIGHT_SPOT, position=where, direction=(0.1, -0.2, -1.0), color=(1.0, 2.0, 0.5), strength=strength, cone_angle=0.6,
                                             blend=0.3, radius=radius))
        else:
            out.append(abi.PunctualLightData(abi.LIGHT_POINT, position=where, color=(2.0, 1.0, 1.5), strength=strength, radius=radius))
    return out


def make_scene(lights, mode=1, ctx=None, mixed=False, **kw):
    """the quad with the lights given, or (mixed) two mesh emitters, the lights and an environment; created under option light_tree = mode"""
    sd = two_emitter_scene() if mixed else quad_scene(**kw)
    if mixed:
        sd.environment = abi.EnvironmentData(color=(0.5, 0.6, 0.7))
    sd.lights = list(lights)
    with capi.options(light_tree=mode):
        return capi.Scene(ctx, sd), sd


def model_of(sc, sd):
    """the model's records, weights, node words and table entries of the scene"""
    records = [sm.fold(as_dict(l)) for l in sc.punctual_lights()]
    verts = np.concatenate([np.asarray(m.vertices, F).reshape(-1, 3) for m in sd.meshes])  # (identity transforms)
    R = pm.bounds_radius(verts.min(axis=0), verts.max(axis=0))
    weights = [pm.power(r, R) for r in records]
    n_mesh = sum(1 for m in sd.materials if m.kind == abi.MAT_EMISSION)
    mode = sc.light_tree()[0]
    words = lt.build(records, weights) if lt.tree_exists(mode, records) else np.zeros((0, 8), np.uint32)
    return records, weights, words, lt.table_entries(mode, n_mesh, records, sd.environment is not None)


def assert_rows_equal(got, want):
    (go, gl, gr), (wo, wl, wr) = got, want
    assert np.array_equal(gl, wl)
    bad = np.nonzero((go.view(np.uint32) != wo.view(np.uint32)).any(axis=1) | (gr != wr))[0]
    assert bad.size == 0, f"{bad.size} rows differ, first {bad[0]}: {go[bad[0]]} / {gr[bad[0]]} vs {wo[bad[0]]} / {wr[bad[0]]}"


# ---------------------------------------------------------------------------------------------------------------- node words and the light table
@pytest.mark.parametrize("arrangement", ["random", "repeats", "line"])
@pytest.mark.parametrize("n", SIZES)
def test_node_words_equal_the_model(hip_lib, n, arrangement):
    mixed = arrangement != "line"
    lights = local_lights(n, 100 + n, arrangement)
    if mixed:  # suns between the local lights: they keep entries of their own, in the order given
        lights = lights[:1] + [sun()] + lights[1:] + [sun(direction=(0.0, 0.3, -1.0), strength=0.5)]
    sc, sd = make_scene(lights, mixed=mixed)
    records, weights, words, entries = model_of(sc, sd)
    assert sc.light_tree() == (1, 2 * n - 1) and words.shape == (2 * n - 1, 8)
    got = sc.array(capi.ARRAY_LIGHT_TREE, np.uint32).reshape(-1, 8)
    assert np.array_equal(got, words)
    # every leaf once, balanced: depth ceil(log2 n) or one less
    leaves = got[(got[:, 7] & lt.LEAF) != 0, 7] & ~np.uint32(lt.LEAF)
    assert sorted(leaves) == [k for k, r in enumerate(records) if lt.is_local(r)]
    _, depth = lt.record_pdfs(words, records, np.zeros((1, 3), F))
    deep = math.ceil(math.log2(n))
    assert set(depth[[lt.is_local(r) for r in records]]) <= {deep, deep - 1}
    # the table: mesh lights, the suns in the order given, ONE entry for the tree, the environment
    n_lights = sc.info().n_lights
    assert n_lights == len(entries) == (2 + 2 + 1 + 1 if mixed else 1)
    inst = [sc.light(i)[0] for i in range(n_lights)]
    want_inst = {"punct": capi.PUNCTUAL_LIGHT_INSTANCE, "tree": capi.LIGHT_TREE_INSTANCE, "env": capi.ENV_LIGHT_INSTANCE}
    assert capi.LIGHT_TREE_INSTANCE == lt.TREE_INST
    for i, (kind, k) in enumerate(entries):
        assert kind == "mesh" or inst[i] == want_inst[kind]
        if kind == "punct":
            assert F(sc.light(i)[1]).view(np.uint32) == F(weights[k]).view(np.uint32) and records[k]["kind"] == pm.SUN
        if kind == "tree":
            assert F(sc.light(i)[1]).view(np.uint32) == lt.tree_power(records, weights).view(np.uint32)
    powers = np.array([sc.light(i)[1] for i in range(n_lights)], F)
    pdf = np.array([sc.light(i)[2] for i in range(n_lights)], F)
    assert np.array_equal(pdf.view(np.uint32), pm.selection_pdfs(powers).view(np.uint32))
    # the records stay ALL records in the order given, whatever the mode
    off, _ = make_scene(lights, mode=0, mixed=mixed)
    assert np.array_equal(sc.array(capi.ARRAY_PUNCTUAL_LIGHTS, np.uint32), off.array(capi.ARRAY_PUNCTUAL_LIGHTS, np.uint32))
    assert np.array_equal(sc.array(capi.ARRAY_PUNCTUAL_LIGHTS, np.uint32).reshape(-1, 16), np.stack([sm.record_words(r) for r in records]))
    assert off.info().n_lights == n_lights + n - 1 and off.light_tree() == (0, 0) and off.array(capi.ARRAY_LIGHT_TREE, np.uint32).size == 0


# ---------------------------------------------------------------------------------------------------------------- the hook against the model
def edge_rows(words, records, seed):
    """p on a light, p at a node's centre (every node of a small tree, a sample of a large one), p 10^6 units away; u_select = 0 and the largest float below 1"""
    rng = np.random.default_rng(seed)
    lo, hi = words[:, 0:3].view(F), words[:, 4:7].view(F)
    centres = ((lo + hi) * F(0.5)).astype(F)
    if len(centres) > 64:
        centres = centres[rng.choice(len(centres), 64, replace=False)]
    pts = [r["q"] for r in records if lt.is_local(r)][:64] + list(centres) + [np.array([1e6, -1e6, 1e6], F), np.array([0.0, -0.0, 0.0], F)]
    rows = []
    for p in pts:
        for u in (0.0, U_TOP, 0.5, float(F(rng.random()))):
            rows.append((*p, 0.0, 0.0, 1.0, u, float(F(rng.random())), float(F(rng.random()))))
    return np.asarray(rows, F)


def threshold_rows(sc, records, words, entries, rows):
    """for rows through a table whose only entry is the tree: u_select at every branch threshold the model reports along the row's path, and one ulp either side"""
    assert [e[0] for e in entries] == ["tree"]
    (_, _, _), (sel, path) = lt.light_sample_rows(light_table(sc), entries, records, words, rows)
    out = []
    for k, i in enumerate(sel):
        for t in lt.thresholds(([l[k] for l in path[0]], [l[k] for l in path[1]]), rows[i, 6]):
            for u in (F(t), np.nextafter(F(t), F(0)), np.nextafter(F(t), F(2))):
                if 0 <= u < 1:
                    r = rows[i].copy()
                    r[6] = u
                    out.append(r)
    return np.asarray(out, F)


HOOK_SCENES = {
    "two": (2, "random", False), "five_mixed": (5, "random", True), "repeats_33": (33, "repeats", False), "mixed_33": (33, "random", True),
    "line_8": (8, "line", False), "one_point_4": (4, "one_point", False), "large_257": (257, "random", False),
}


@pytest.mark.parametrize("name", sorted(HOOK_SCENES))
def test_host_hook_equals_the_model_bit_for_bit(hip_lib, name):
    n, arrangement, mixed = HOOK_SCENES[name]
    lights = local_lights(n, 7 + n, arrangement)
    if mixed:
        lights = [sun()] + lights
    sc, sd = make_scene(lights, mixed=mixed)
    records, weights, words, entries = model_of(sc, sd)
    rows = np.concatenate([random_rows9(4096, 3 + n), edge_rows(words, records, n)])
    if not mixed:
        rows = np.concatenate([rows, threshold_rows(sc, records, words, entries, rows[:48])])
    got = sc.host_light_tree_sample(rows)
    want, _ = lt.light_sample_rows(light_table(sc), entries, records, words, rows)
    assert_rows_equal(got, want)
    out, light, record = got
    tree_entry = [e[0] for e in entries].index("tree")
    at_tree = light == tree_entry
    assert np.all(record[~at_tree] == lt.NO_RECORD) and np.all(record[at_tree] < len(records)) and at_tree.sum() > 1000
    assert len(set(record[at_tree])) >= min(n, 2) and np.all(out[at_tree, 12] == 1)
    assert np.all(out[at_tree, 6] > 0) and np.all(out[at_tree, 6] <= sc.light(tree_entry)[2])
    if mixed:  # the other entries: what the hook of the soft lights answers there
        soft = sc.host_light_sample_soft(rows)
        assert np.array_equal(soft[1], light) and np.array_equal(soft[0][~at_tree].view(np.uint32), out[~at_tree].view(np.uint32))
        assert not soft[0][at_tree][:, [0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 12]].any()  # the existing hook samples nothing at the tree's entry


def test_threshold_rows_reach_both_sides(hip_lib):
    """the rows of threshold_rows do land on both sides of the first level's threshold: the records they reach differ"""
    sc, sd = make_scene(local_lights(8, 15))
    records, weights, words, entries = model_of(sc, sd)
    base = random_rows9(16, 5)
    rows = threshold_rows(sc, records, words, entries, base)
    (out, light, record), _ = lt.light_sample_rows(light_table(sc), entries, records, words, rows)
    per_base = 3 * 3  # depth 3: three thresholds, three values each
    assert len(rows) == 16 * per_base
    reached = record.reshape(16, 3, 3)  # per level: at the threshold, one ulp below, one ulp above
    # the first level's threshold is the root's left probability itself: one ulp below goes left, at it and above go right
    assert np.all(reached[:, 0, 0] != reached[:, 0, 1]) and np.all(reached[:, 0, 0] == reached[:, 0, 2])
    # deeper thresholds are mapped back to u_select in double: the three values still straddle most of them
    assert np.mean(reached[:, 1:, 1] != reached[:, 1:, 2]) > 0.5


# ---------------------------------------------------------------------------------------------------------------- partition of unity (no model)
def test_partition_of_unity(hip_lib):
    """33 local lights and nothing else: 2^16 stratified u_select through the hook at 64 points. The fraction that reaches a record is the pdf reported for
    it within (depth + 1) 2^-16 -- every level's interval boundary cuts one stratum -- and the pdfs of the distinct records sum to 1."""
    n, m = 33, 1 << 16
    sc, _ = make_scene(local_lights(n, 41))
    nodes = sc.array(capi.ARRAY_LIGHT_TREE, np.uint32).reshape(-1, 8)
    depth_of = {}
    level = {0: 0}
    for k in range(len(nodes)):  # breadth-first: a parent comes before its children
        c = int(nodes[k, 7])
        if c & 0x80000000:
            depth_of[c & 0x7FFFFFFF] = level[k]
        else:
            level[c] = level[c + 1] = level[k] + 1
    pts = random_rows9(64, 77)
    u = ((np.arange(m) + 0.5) / m).astype(F)
    worst, worst_sum = 0.0, 0.0
    for p in pts:
        rows = np.repeat(p[None, :], m, axis=0)
        rows[:, 6] = u
        out, light, record = sc.host_light_tree_sample(rows)
        assert np.all(light == 0)
        recs, first, counts = np.unique(record, return_index=True, return_counts=True)
        assert len(recs) == n  # every light is reached: none has probability 0
        pdf = out[first, 6].astype(np.float64)
        for r, c, q in zip(recs, counts, pdf):
            assert np.all(out[record == r, 6] == F(q))  # one pdf per record, whatever u
            err = abs(c / m - q)
            worst = max(worst, err / ((depth_of[int(r)] + 1) * 2.0 ** -16))
            assert err <= (depth_of[int(r)] + 1) * 2.0 ** -16
        worst_sum = max(worst_sum, abs(pdf.sum() - 1.0))
        assert abs(pdf.sum() - 1.0) <= 1e-5
    print(f"partition of unity: worst |fraction - pdf| = {worst:.3f} of its bound, worst |sum of pdfs - 1| = {worst_sum:.3g}")


# ---------------------------------------------------------------------------------------------------------------- mode off is off
ALL_ARRAYS = range(29)


def assert_same_scene(a, b, rows):
    for which in ALL_ARRAYS:
        assert np.array_equal(a.array(which, np.uint8), b.array(which, np.uint8)), which
    assert a.info().n_lights == b.info().n_lights and [a.light(i) for i in range(a.info().n_lights)] == [b.light(i) for i in range(b.info().n_lights)]
    for hook in ("host_light_sample_soft", "host_light_tree_sample"):
        for x, y in zip(getattr(a, hook)(rows), getattr(b, hook)(rows)):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert np.array_equal(a.host_light_sample(rows[:, :7])[0].view(np.uint32), b.host_light_sample(rows[:, :7])[0].view(np.uint32))


def test_mode_off_is_the_scene_that_never_heard_of_it(hip_lib):
    rows = random_rows9(1024, 9)
    lights = [sun()] + local_lights(5, 3) + [sun(direction=(0.0, 0.3, -1.0))]
    sd = two_emitter_scene()
    sd.environment, sd.lights = abi.EnvironmentData(color=(0.5, 0.6, 0.7)), lights
    plain = capi.Scene(None, sd)  # the option's default
    assert capi.get_option("light_tree") == 0 and plain.light_tree() == (0, 0)
    off, _ = make_scene(lights, mode=0, mixed=True)
    assert_same_scene(off, plain, rows)
    # mode 1 with fewer than two local lights: no tree, every table the one of mode 0
    few = [sun(), local_lights(1, 3)[0]]
    one, sd1 = make_scene(few, mode=1, mixed=True)
    ref, _ = make_scene(few, mode=0, mixed=True)
    assert one.light_tree() == (1, 0)
    assert_same_scene(one, ref, rows)
    # the setter: on and off again gives the scene back; adding and clearing lights rebuilds the tree
    off.set_light_tree(True)
    assert off.light_tree() == (1, 9) and off.info().n_lights == plain.info().n_lights - 4
    on, _ = make_scene(lights, mode=1, mixed=True)
    assert_same_scene(off, on, rows)
    off.set_light_tree(False)
    assert_same_scene(off, plain, rows)
    on.add_punctual_light(local_lights(1, 99)[0])
    assert on.light_tree() == (1, 11)
    again, _ = make_scene(lights + local_lights(1, 99), mode=1, mixed=True)
    assert_same_scene(on, again, rows)
    on.clear_punctual_lights()
    assert on.light_tree() == (1, 0) and on.info().n_lights == 3
    on.add_punctual_light(point())
    on.add_punctual_light(spot())
    assert on.light_tree() == (1, 3) and [on.light(i)[0] for i in range(4)][2:] == [capi.LIGHT_TREE_INSTANCE, capi.ENV_LIGHT_INSTANCE]
    on.set_environment(color=(2, 1, 1))  # the environment stays last
    assert [on.light(i)[0] for i in range(4)][2:] == [capi.LIGHT_TREE_INSTANCE, capi.ENV_LIGHT_INSTANCE] and on.light_tree() == (1, 3)
    with pytest.raises(capi.AkariError):
        capi.set_option("light_tree", 2)
    assert capi.get_option("light_tree") == 0


def test_json_scene_under_the_option(hip_lib, tmp_path):
    lights = [point(), spot(cone_angle=0.375, blend=0.25), sun(), point(position=(-0.5, 0.25, 0.75))]
    path = write_scene_with_lights(tmp_path, {k: json_light(l) for k, l in zip("abcd", lights)})
    with capi.options(light_tree=1):
        loaded = capi.Scene(None, path)
    api, _ = make_scene(lights, width=16, height=16)
    assert loaded.light_tree() == api.light_tree() == (1, 5)
    assert np.array_equal(loaded.array(capi.ARRAY_LIGHT_TREE, np.uint32), api.array(capi.ARRAY_LIGHT_TREE, np.uint32))
    assert [loaded.light(i) for i in range(2)] == [api.light(i) for i in range(2)] and loaded.light(1)[0] == capi.LIGHT_TREE_INSTANCE
    assert capi.Scene(None, path).light_tree() == (0, 0)
    # the launch plan: the PUNCT kernels, with one entry fewer in the staged tables per light the tree took
    from tests.helpers import make_config
    plan, plain = loaded.launch_plan(make_config(spp=4)), capi.Scene(None, path).launch_plan(make_config(spp=4))
    assert plan["variant"] == plain["variant"] and plan["variant"]["punct"] == 1
    assert plan["stage_bytes"][4] == 32 and plain["stage_bytes"][4] == 64


def test_lds_budget_counts_the_tree_as_one_entry(hip_lib):
    """an exhaustive scene takes punctual lights until its staged tables pass the LDS budget (36 bytes an entry, tables padded to 16); with the tree the same
    lights are one entry"""
    sc, _ = make_scene([], mode=0)
    lights = local_lights(1200, 5)
    n_ok = 0
    with pytest.raises(capi.AkariError) as e:
        for l in lights:
            sc.add_punctual_light(l)
            n_ok += 1
    assert e.value.code == capi.ERR_UNSUPPORTED and "LDS budget" in str(e.value) and 500 < n_ok < 1200
    assert sc.info().n_lights == n_ok and sc.info().uses_bvh == 0
    tree, _ = make_scene(lights[:n_ok + 1])
    assert tree.info().n_lights == 1 and tree.light_tree() == (1, 2 * n_ok + 1) and tree.info().uses_bvh == 0
    with pytest.raises(capi.AkariError):
        tree.set_light_tree(False)  # refused: the change is taken back
    assert tree.light_tree() == (1, 2 * n_ok + 1) and tree.info().n_lights == 1


# ---------------------------------------------------------------------------------------------------------------- variance in the model
GRID_SPACING = 0.4  # the 4 x 4 grid of lights 0.25 above the quad (chosen with grid_variances below: the ratio at 0.4 is far above 4)


def grid_lights(spacing=GRID_SPACING, height=0.25):
    return [abi.PunctualLightData(abi.LIGHT_POINT, position=(float(F((i - 1.5) * spacing)), float(F((j - 1.5) * spacing)), height), color=(1.0, 1.0, 1.0), strength=0.05)
            for j in range(4) for i in range(4)]


def grid_contributions(lights, x, albedo=0.6):
    """f_i at the points x (n, 3) of the quad (normal +z), float64: (n, 16)"""
    q = np.array([l.position for l in lights], F).astype(np.float64)
    d = q[None, :, :] - x[:, None, :]
    r2 = np.sum(d * d, axis=-1)
    c = np.array([float(F(l.color[0]) * F(l.strength)) for l in lights])
    return albedo / math.pi * np.maximum(d[..., 2], 0.0) / np.sqrt(r2) / r2 * c[None, :]


def grid_variances(sc_tree, sd, x32):
    """the per-sample variance sum_i f_i^2 / p_i - (sum_i f_i)^2 of every point, with the tree (p_i from the model's walk) and by power alone (p_i = 1 / 16)"""
    records, weights, words, entries = model_of(sc_tree, sd)
    p_tree, _ = lt.record_pdfs(words, records, x32)
    f = grid_contributions(sc_tree.punctual_lights(), x32.astype(np.float64))
    total2 = f.sum(axis=1) ** 2
    return (f ** 2 / p_tree.astype(np.float64)).sum(axis=1) - total2, (f ** 2 * 16.0).sum(axis=1) - total2, f, p_tree


def pixel_points_host(scene):
    w, h = scene.info().width, scene.info().height
    px = np.stack(np.meshgrid(np.arange(w), np.arange(h)), -1).reshape(-1, 2).astype(np.uint32)
    half = np.full((w * h, 2), 0.5, np.float32)
    r = scene.host_lens_ray(px, half, half, abi.FILTER_BOX, 0.0).astype(np.float64)
    t = (0.0 - r[:, 2]) / r[:, 5]
    return r[:, 0:3] + t[:, None] * r[:, 3:6]


def test_variance_in_the_model(hip_lib):
    sc, sd = make_scene(grid_lights(), width=16, height=16)
    assert sc.light_tree() == (1, 31)
    x32 = pixel_points_host(sc).astype(F)
    v_tree, v_power, f, p = grid_variances(sc, sd, x32)
    assert np.all(np.abs(p.astype(np.float64).sum(axis=1) - 1.0) < 1e-5) and np.all(p > 0)
    print(f"variance in the model, summed over the film: by power {v_power.sum():.4g}, with the tree {v_tree.sum():.4g}, ratio {v_power.sum() / v_tree.sum():.2f}")
    assert v_tree.sum() * 4.0 <= v_power.sum()
