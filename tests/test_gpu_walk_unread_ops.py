"""The pair walk's margins and the light lookups after the operations nothing reads were taken out (csrc/device/disect.h trace_pair_exhaustive:
the closest-hit ray's margin without tmax - t, the shadow ray's range term computed with its plane solve, one test for the best hit;
csrc/device/dgeom.h: weighted_choice2_and_remap's one division, alias_sample_and_remap_wave's shortcut). Each removal is argued to change no
bit; these are the inputs where a wrong argument would show: bounds one float either side of a hit, rays that do not exist, rays parallel to
a plane (t = +-inf or NaN), records that share a plane and records that do not, and light tables that do or do not satisfy the shortcut.
Expectations are the oracle's, bit for bit; which lanes repeat the walk with the contract's division is the parent commit's
(tests/golden/walk_unread_ops_repeats.json; its "recorded_with" field holds the command)."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from akari_render_amd import abi, capi  # noqa: E402
from oracle import pyoracle, scene_json  # noqa: E402
from tests.helpers import box_scene, make_config  # noqa: E402
from tests.test_gpu_pair_walk import NONE, SCENES, Case, _xf, case  # noqa: E402,F401  (case: the fixture, with its cache of Case objects)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "walk_unread_ops_repeats.json")
N = 384  # rays per probe call: six waves


def _closest(c, o, d, tmax):
    """the oracle's closest hit in [0, tmax] -> found, global id, (t, u, v)"""
    r = np.zeros((o.shape[0], 8), np.float32)
    r[:, :3], r[:, 3:6], r[:, 7] = o, d, tmax
    hit, tuv = c.osc.intersect_many(r)
    off = c.osc.tri_offsets()
    return hit[:, 0] != 0, np.where(hit[:, 0] != 0, off[hit[:, 1]] + hit[:, 2], NONE).astype(np.uint32), tuv


def _any(c, o, d, tmax):
    r = np.zeros((o.shape[0], 8), np.float32)
    r[:, :3], r[:, 3:6], r[:, 7] = o, d, tmax
    return c.osc.intersect_many(r, any_hit=True)[0][:, 0] != 0


def _rays16(o, d, tmax, so, sd, stmax):
    r = np.zeros((o.shape[0], 16), np.float32)
    r[:, 0:3], r[:, 3:6], r[:, 6] = o, d, tmax
    r[:, 8:11], r[:, 11:14], r[:, 14] = so, sd, stmax
    return r


def _probe(ctx, scene, rays):
    return capi.probe_intersect_pair(ctx, scene, rays, np.full((rays.shape[0], 3), NONE, np.uint32))


def _expect(c, o, d, tmax, so, sd, stmax):
    """the oracle's answer for the pair: a ray with a negative bound does not exist"""
    found, gid, tuv = _closest(c, o, d, np.maximum(tmax, 0))
    found = found & (tmax >= 0)
    occ = _any(c, so, sd, np.maximum(stmax, 0)) & (stmax >= 0)
    return found, gid, tuv, occ


def _assert_equal(out, tuv, exp, what):
    found, gid, etuv, occ = exp
    assert np.array_equal(out[:, 0] != 0, found), what
    assert np.array_equal(out[found, 1], gid[found]), what
    assert np.array_equal(tuv[found].view(np.uint32), etuv[found].view(np.uint32)), what
    assert np.array_equal(out[:, 2] != 0, occ), what


@pytest.mark.parametrize("case", list(SCENES), indirect=True)
def test_bounds_at_the_hit_and_one_float_either_side(ctx, case):
    """tmax / stmax = the hit's t, the float below, the float above, for tie-free hits: found, id, (t, u, v) and occluded are the oracle's for
    that same bound. (At t == tmax the hit is accepted through best_t = next_up(tmax) alone now; one float above tmax it must not be.)"""
    c = case
    a = np.flatnonzero(c.c_clean)[:N]
    b = np.flatnonzero(c.s_clean)[:N]
    n = min(a.size, b.size)
    assert n >= 100, (a.size, b.size)
    a, b = a[:n], b[:n]
    o, d, so, sd = c.o[a], c.d[a], c.so[b], c.sdir[b]
    t, st = c.c_tuv[a, 0], c.s1_tuv[b, 0]
    assert np.all(t > 0) and np.all(st > 0)
    scene = capi.Scene(ctx, c.sd)
    inf = np.float32(np.inf)
    seen = []
    for what, tm, stm in (("at the hit", t, st), ("one float below", np.nextafter(t, -inf), np.nextafter(st, -inf)), ("one float above", np.nextafter(t, inf), np.nextafter(st, inf)),
                          ("closest at the hit, shadow below", t, np.nextafter(st, -inf)), ("closest below, shadow at the hit", np.nextafter(t, -inf), st)):
        tm, stm = tm.astype(np.float32), stm.astype(np.float32)
        exp = _expect(c, o, d, tm, so, sd, stm)
        out, tuv = _probe(ctx, scene, _rays16(o, d, tm, so, sd, stm))
        _assert_equal(out, tuv, exp, what)
        seen.append((int(exp[0].sum()), int(exp[3].sum())))
    print(c.n_tris, "triangles,", n, "pairs: (found, occluded) per bound", seen)
    # the oracle agrees that the bound decides: everything found / occluded at the hit and above it, nothing of it one float below
    assert seen[0] == (n, n) and seen[2] == (n, n) and seen[1] == (0, 0) and seen[3] == (n, 0) and seen[4] == (0, n)


@pytest.mark.parametrize("case", list(SCENES), indirect=True)
def test_rays_that_do_not_exist(ctx, case):
    """all four combinations of tmax < 0 and stmax < 0: a missing ray reports nothing, its partner is unaffected"""
    c = case
    i = np.arange(N)
    neg = np.where(i & 4, np.float32(-1e-30), np.float32(-1.0)).astype(np.float32)  # (the callers pass -1; any negative bound means the same)
    tmax = np.where(i & 1, neg, np.float32(1e20)).astype(np.float32)
    stmax = np.where(i & 2, neg, np.abs(c.stmax[:N]) + np.float32(0.5)).astype(np.float32)
    o, d, so, sd = c.o[:N], c.d[:N], c.so[:N], c.sdir[:N]
    exp = _expect(c, o, d, tmax, so, sd, stmax)
    scene = capi.Scene(ctx, c.sd)
    out, tuv = _probe(ctx, scene, _rays16(o, d, tmax, so, sd, stmax))
    _assert_equal(out, tuv, exp, "missing rays")
    assert not np.any(out[tmax < 0, 0]) and not np.any(out[stmax < 0, 2])
    both = (tmax < 0) & (stmax < 0)
    assert both.sum() == N // 4 and not np.any(out[both][:, [0, 2]])
    assert exp[0][stmax < 0].sum() > 8 and exp[3][tmax < 0].sum() > 8  # (the partners of missing rays do hit something)


def _parallel_rays(c):
    """N pairs on the scene: axis-parallel directions (dz = 0 on the planes along the axis: t = +-inf, or NaN where the origin is in the plane),
    the last wave's origins ON vertices of the scene (numerators at or near zero)."""
    rng = np.random.default_rng(950)
    verts = c.osc.world_vertices()
    lo, hi = verts.reshape(-1, 3).min(0) - 0.1, verts.reshape(-1, 3).max(0) + 0.1
    axes = np.eye(3, dtype=np.float32)

    def one():
        o = (rng.random((N, 3)) * (hi - lo) + lo).astype(np.float32)
        d = axes[rng.integers(0, 3, N)] * rng.choice(np.array([-1.0, 1.0], np.float32), (N, 1))
        o[N - 64:] = verts[rng.integers(0, verts.shape[0], 64), rng.integers(0, 3, 64)]
        return o, d.astype(np.float32)

    o, d = one()
    so, sd = one()
    stmax = (rng.random(N) * 3).astype(np.float32)
    return o, d, so, sd, stmax


def _parallel_runs(c):
    o, d, so, sd, stmax = _parallel_rays(c)
    far, none = np.full(N, 1e20, np.float32), np.full(N, -1.0, np.float32)
    return {"pair": (o, d, far, so, sd, stmax), "closest_only": (o, d, far, so, sd, none), "shadow_only": (o, d, none, so, sd, stmax)}


@pytest.mark.parametrize("case", ["cbox"], indirect=True)
def test_rays_parallel_to_planes(ctx, case):
    """axis-parallel rays on the cbox, with and without a partner: the oracle's answers, and the lanes that repeat the walk are the parent's"""
    c = case
    want = json.load(open(GOLDEN))["repeats"]
    scene = capi.Scene(ctx, c.sd)
    for name, r in _parallel_runs(c).items():
        out, tuv = _probe(ctx, scene, _rays16(*r))
        _assert_equal(out, tuv, _expect(c, *r), name)
        lanes = np.flatnonzero(out[:, 3]).tolist()
        print(name, "lanes in a repeated walk:", len(lanes))
        assert lanes == want[name], name
    assert any(want.values()) and not all(len(v) == N for v in want.values())  # (both kinds of wave are among them)


@pytest.mark.parametrize("case", list(SCENES), indirect=True)
def test_records_that_share_a_plane_and_records_that_do_not(ctx, case):
    """the shadow ray's range term travels with the plane solve: records that take their neighbour's plane (every second one of tri64, all
    but one pair of the cbox) and records that solve their own (tri3's three, one pair of the cbox) give the oracle's answers"""
    c = case
    shared = c.osc.shared_plane_rows()
    print(c.n_tris, "triangles,", shared, "records take their neighbour's plane")
    assert shared == {3: 0, 36: 17, 64: 32}[c.n_tris]
    k = np.arange(N) + 512  # (past the axis-parallel lanes of the Case)
    tmax, stmax = c.tmax[k], c.stmax[k]
    scene = capi.Scene(ctx, c.sd)
    out, tuv = _probe(ctx, scene, _rays16(c.o[k], c.d[k], tmax, c.so[k], c.sdir[k], stmax))
    exp = (c.c_found[k], c.c_gid[k], c.c_tuv[k], c.s_occ[k])
    assert exp[0].sum() > N // 16 and exp[3].sum() > N // 64
    _assert_equal(out, tuv, exp, "plane sharing")


# ------------------------------------------------------------------------------------------------------------ light selection
def _quad_down(x0, x1, z0, z1, x2=None, y=0.9):
    """a quad under the ceiling facing down; x2: the far edge's right end (a trapezoid: two triangles of unequal area)"""
    x2 = x1 if x2 is None else x2
    v = np.array([[x0, y, z0], [x1, y, z0], [x2, y, z1], [x0, y, z1]], dtype=np.float32)
    return abi.MeshData(vertices=v, indices=np.array([[0, 1, 2], [0, 2, 3]], dtype=np.uint32))


def _emitter(strength):
    return abi.MaterialData(base_color=(0.8, 0.8, 0.8), ior=1.0, specular_ior_level=0.0, emission_color=(strength,) * 3, emission_strength=1.0)


def two_unequal_emitters():
    sd = box_scene(emission=0.0)
    sd.meshes = [sd.meshes[0], _quad_down(-0.6, -0.2, -0.2, 0.2), _quad_down(0.2, 0.6, -0.2, 0.2)]
    sd.materials = [sd.materials[0], _emitter(4.0), _emitter(12.0)]
    eye = _xf(1.0, np.zeros(3, np.float32))
    sd.instances = [sd.instances[0], abi.InstanceData(1, [1], eye), abi.InstanceData(2, [2], eye.copy())]
    return sd


def one_emitter_of_unequal_triangles():
    sd = box_scene(emission=0.0)
    sd.meshes = [sd.meshes[0], _quad_down(-0.4, 0.4, -0.3, 0.3, x2=-0.2)]
    sd.materials = [sd.materials[0], _emitter(8.0)]
    sd.instances = [sd.instances[0], abi.InstanceData(1, [1], _xf(1.0, np.zeros(3, np.float32)))]
    return sd


def _tri_areas(mesh):
    v = mesh.vertices[mesh.indices].astype(np.float64)
    return 0.5 * np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=1)


def light_scene(name, cbox_path):
    """-> (scene, does the light table satisfy the shortcut, does every light's triangle table)"""
    if name == "cbox":
        sd = scene_json.load_scene(cbox_path, 32, 32)
    else:
        sd = two_unequal_emitters() if name == "two_emitters" else one_emitter_of_unequal_triangles()
    ent, _ = pyoracle.OracleScene(sd).light_table()
    first = bool(np.all(ent["t"] == 1.0))
    if name == "cbox":
        return sd, first, None  # (its light's two triangles are congruent; their powers are not read here)
    # a light's triangle table is build_alias_table over its triangles' powers = emission x area: the table of the areas has the same entries
    # wherever the areas are far from equal (here 1 : 1 or 3 : 1)
    second = all(bool(np.all(capi.host_alias_table(_tri_areas(m).astype(np.float32))[1] == 1.0)) for m in sd.meshes[1:])
    return sd, first, second


LIGHT_CASES = {"cbox": (1, True, None), "two_emitters": (2, False, True), "one_emitter": (1, True, False)}


@pytest.mark.parametrize("name", list(LIGHT_CASES))
def test_light_selection_with_and_without_the_shortcut(ctx, cbox_path, name):
    """32 x 32 at 16 spp: a scene whose waves always skip the lookups' division (cbox), one that never does at the light table, one that never
    does at the triangle table -- asserted from the tables, so the test cannot pass by never leaving the shortcut. Film, sampler states and
    counters are the oracle's."""
    from tests.test_gpu_parity import assert_parity, render_both
    sd, first, second = light_scene(name, cbox_path)
    n_lights, want_first, want_second = LIGHT_CASES[name]
    assert pyoracle.OracleScene(sd).num_lights() == n_lights
    assert first == want_first and second == want_second, (name, first, second)
    cfg = make_config(spp=16, spp_per_pass=16, max_depth=12, rr_depth=5)
    assert cfg.use_nee == 1 and cfg.sampler_type == abi.SAMPLER_INDEPENDENT
    w, h = sd.camera.width, sd.camera.height
    assert (w, h) == (32, 32)
    g, o, gst, ost, gstates, ostates = render_both(ctx, sd, cfg, want_states=True)
    assert_parity(g, o, w, h, gst, ost)
    assert np.array_equal(gstates, ostates)
    assert gst["n_shadow"] > w * h  # (light samples were taken and traced)


if __name__ == "__main__":  # --record OUT.json, with AKR_HIP_LIB = a library built from the parent commit
    ctx = capi.Context(0)
    c = Case(scene_json.load_scene(os.path.join(ROOT, "scenes", "cbox", "scene.json"), 32, 32), seed=len("cbox") + 100)
    scene = capi.Scene(ctx, c.sd)
    rep = {name: np.flatnonzero(_probe(ctx, scene, _rays16(*r))[0][:, 3]).tolist() for name, r in _parallel_runs(c).items()}
    out = {"recorded_with": "AKR_HIP_LIB=<libakari_hip.so built from the parent commit> python tests/test_gpu_walk_unread_ops.py --record OUT.json, MI355X",
           "n_pairs": N, "repeats": rep}
    print({k: len(v) for k, v in rep.items()})
    json.dump(out, open(sys.argv[sys.argv.index("--record") + 1], "w"), indent=1)
