"""The pair walk's bookkeeping per plane (csrc/device/disect.h WalkOpt PLANE_LT, PLANE_EXCL): one `T < best_t` for two records on one
plane, one comparison per excluded id and trip. Through akr_probe_intersect_pair, which calls the walk as the pt kernel does; found / gid /
t / u / v / occluded against the CPU oracle, bit for bit, on the inputs where a wrong identity would show:
  scenes   a quad (records 0 and 1 on one plane); a quad and a lone triangle (an odd count: the walk's tail record); a quad and a folded
           quad whose halves are not coplanar (mask bit clear); a one-triangle instance in front of two quads, so that every pair starts at an
           odd id and straddles two trips;
  rays     96 lanes (a full wave and a half-filled one): rays through the shared diagonal of the axis-aligned quad with dyadic coordinates,
           where both halves accept at the same t and the lower id must win; a hit at t == tmax; misses; lanes with only one of the two
           rays; a NaN direction;
  slots    ex0, sex0, sex1 each on the first half, on the second half or empty, sex0 and sex1 on the two halves of one pair, and a mix that
           differs from lane to lane.
The oracle's tracer takes no excluded ids from Python, so the expectation with an id excluded is the oracle's answer on the scene WITHOUT
that triangle (ids mapped back). The CPU test below shows that this reference is sound (leaving a triangle out changes no bit of the
answers that did not involve it) and that the inputs are not vacuous."""
import numpy as np
import pytest

from akari_render_amd import abi, capi
from oracle import pyoracle
from tests.helpers import box_scene

NONE = 0xFFFFFFFF
N = 96
N_DIAG = 40  # lanes 0 .. 39: both rays through the quad's shared diagonal


def _mesh(v, idx):
    return abi.MeshData(vertices=np.array(v, np.float32), indices=np.array(idx, np.uint32).reshape(-1, 3))


def _rect(x0, x1, y0, y1, z, z3=None):
    """an axis-aligned rectangle at height z, split along the diagonal v0 v2; z3: the height of v3 (a folded quad: its halves are not coplanar)"""
    return [[x0, y0, z], [x1, y0, z], [x1, y1, z], [x0, y1, z if z3 is None else z3]], [[0, 1, 2], [0, 2, 3]]


def _scene(meshes):
    sd = box_scene()
    eye = np.eye(4, dtype=np.float32).T.reshape(16)
    sd.meshes = meshes
    sd.instances = [abi.InstanceData(i, [0], eye.copy()) for i in range(len(meshes))]
    return sd


QUAD = _rect(-1.0, 1.0, -1.0, 1.0, 0.0)  # the quad every scene has; its shared diagonal is x == y


def _join(*parts):
    v, idx = [], []
    for pv, pi in parts:
        idx += [[i + len(v) for i in t] for t in pi]
        v += pv
    return _mesh(v, idx)


LONE = ([[-2.0, -2.0, -0.5], [2.0, -2.0, -0.5], [-2.0, 2.0, -0.5]], [[0, 1, 2]])  # a lone triangle under one half of the quad and beyond it
# name -> (meshes, the quad's first id, records that take their neighbour's plane)
SCENES = {
    "quad": (lambda: [_mesh(*QUAD)], 0, 1),
    "quad_tri": (lambda: [_join(QUAD, LONE)], 0, 1),
    "quad_folded": (lambda: [_join(QUAD, _rect(-1.5, 0.5, -1.5, 0.5, -0.5, z3=-0.75))], 0, 1),
    # (no plane of a scene holds a ray's origin: a numerator of exactly 0 sends the whole wave to the repeated walk, past the code under test)
    "tri_quad_quad": (lambda: [_mesh([[0.25, -0.75, 0.375], [0.75, -0.75, 0.375], [0.25, -0.25, 0.375]], [[0, 1, 2]]), _mesh(*QUAD),
                               _mesh(*_rect(-1.5, 0.5, -1.5, 0.5, -0.5))], 1, 2),
}
N_TRIS = {"quad": 2, "quad_tri": 3, "quad_folded": 4, "tri_quad_quad": 5}


def make_rays():
    """(96, 16): o d tmax - | so sd stmax -. Dyadic numbers throughout the first 48 lanes, so a ray aimed at the diagonal is on it exactly."""
    rng = np.random.default_rng(2)
    r = np.zeros((N, 16), np.float32)
    r[:, 6], r[:, 14] = 1e20, 4.0

    def aim(lanes, cols, target, slope, h):  # origin = target + h * (slope, 1), direction = -(slope, 1): reaches z = 0 at t == h
        o = np.concatenate([target[:, :2] + h[:, None] * slope, h[:, None]], 1)
        r[lanes, cols:cols + 3] = o
        r[lanes, cols + 3:cols + 6] = np.concatenate([-slope, -np.ones((len(lanes), 1))], 1)

    lanes = np.arange(N_DIAG)
    for cols, seed in ((0, 0), (8, 1)):
        s = (rng.integers(-7, 8, N_DIAG) / 8.0).astype(np.float32)  # the point (s, s, 0) of the diagonal
        slope = (rng.integers(-2, 3, (N_DIAG, 2)) / 4.0).astype(np.float32)
        h = np.array([0.5, 1.0, 2.0, 0.25], np.float32)[(lanes + seed) % 4]
        aim(lanes, cols, np.stack([s, s], 1), slope, h)
    # lanes 40 .. 47: straight down onto the interior of either half from z = 1; 40 .. 43 with the bound AT the hit (t == tmax == 1)
    lanes = np.arange(40, 48)
    p = np.array([[0.5, -0.25], [-0.5, 0.25], [0.75, 0.5], [-0.25, 0.5], [0.5, -0.5], [-0.75, 0.5], [0.25, 0.125], [-0.5, -0.25]], np.float32)
    for cols in (0, 8):
        aim(lanes, cols, p if cols == 0 else p[::-1], np.zeros((8, 2), np.float32), np.ones(8, np.float32))
    r[40:44, 6], r[40:44, 14] = 1.0, 1.0
    # lanes 48 .. 79: random rays from above towards the quads' neighbourhood (hits on every triangle, and misses past the edges)
    n = 32
    for cols in (0, 8):
        o = np.concatenate([rng.uniform(-1.5, 1.5, (n, 2)), rng.uniform(0.75, 2.0, (n, 1))], 1)
        tgt = np.concatenate([rng.uniform(-1.75, 1.25, (n, 2)), np.zeros((n, 1))], 1)
        d = tgt - o
        r[48:80, cols:cols + 3], r[48:80, cols + 3:cols + 6] = o, d / np.linalg.norm(d, axis=1, keepdims=True)
    # lanes 80 .. 95: lanes 44 .. 47 again, four times: 80 .. 83 with both rays pointing away (misses), 84 .. 87 with the closest-hit ray only,
    # 88 .. 91 with the shadow ray only, 92 .. 95 with a NaN in the direction of the closest-hit ray (92, 93) or of the shadow ray (94, 95)
    r[80:96] = np.tile(r[44:48], (4, 1))
    r[80:84, 5], r[80:84, 13] = 1.0, 1.0
    r[84:88, 14] = -1.0
    r[88:92, 6] = -1.0
    r[92:94, 3], r[94:96, 11] = np.nan, np.nan
    return r


def patterns(qa, n_tris):
    """name -> (96, 3) ex0 sex0 sex1. qa / qb: the two halves of the quad; `mix` differs from lane to lane and names every record of the scene."""
    qb = qa + 1
    out = {"none": (NONE, NONE, NONE), "ex0 first": (qa, NONE, NONE), "ex0 second": (qb, NONE, NONE), "sex0 first": (NONE, qa, NONE),
           "sex0 second": (NONE, qb, NONE), "sex1 first": (NONE, NONE, qa), "sex1 second": (NONE, NONE, qb), "sex0 first sex1 second": (NONE, qa, qb),
           "sex0 second sex1 first": (NONE, qb, qa), "all on the pair": (qa, qb, qa)}
    out = {k: np.tile(np.array([v], np.uint32), (N, 1)) for k, v in out.items()}
    ids = np.array(list(range(n_tris)) + [NONE], np.uint32)
    lane = np.arange(N)
    out["mix"] = np.stack([ids[lane % ids.size], ids[(lane // 2 + 1) % ids.size], ids[(lane // 3 + 2) % ids.size]], 1)
    return out


class Reference:
    """the oracle on a scene and on the scene without some of its triangles"""

    def __init__(self, name):
        self.name = name
        self.meshes = SCENES[name][0]()
        self.n_tris = sum(m.indices.shape[0] for m in self.meshes)
        self._sub = {}

    def scene(self):
        return _scene(self.meshes)

    def _without(self, gone):
        """-> (oracle scene, ids of its triangles in the full scene)"""
        if gone not in self._sub:
            meshes, kept, gid = [], [], 0
            for m in self.meshes:
                keep = [j for j in range(m.indices.shape[0]) if gid + j not in gone]
                kept += [gid + j for j in keep]
                gid += m.indices.shape[0]
                if keep:
                    meshes.append(abi.MeshData(vertices=m.vertices, indices=m.indices[keep].copy()))
            self._sub[gone] = (pyoracle.OracleScene(_scene(meshes)) if meshes else None, np.array(kept + [NONE], np.uint32))
        return self._sub[gone]

    def _trace(self, gone, o, d, tmax, any_hit):
        n = o.shape[0]
        osc, kept = self._without(gone)
        if osc is None:
            return np.zeros(n, bool), np.full(n, NONE, np.uint32), np.zeros((n, 3), np.float32)
        r = np.zeros((n, 8), np.float32)
        r[:, :3], r[:, 3:6], r[:, 7] = o, d, np.maximum(tmax, 0)
        hit, tuv = osc.intersect_many(r, any_hit=any_hit)
        found = (hit[:, 0] != 0) & (tmax >= 0)
        sub = np.where(found, osc.tri_offsets()[hit[:, 1]] + hit[:, 2], kept.size - 1)
        return found, kept[sub], tuv

    def expect(self, rays, ex):
        """found, gid, (t, u, v), occluded per lane"""
        n = rays.shape[0]
        found, gid, tuv, occ = np.zeros(n, bool), np.full(n, NONE, np.uint32), np.zeros((n, 3), np.float32), np.zeros(n, bool)
        ids = lambda row: frozenset(int(x) for x in row if x != NONE)
        for key in {ids(e[:1]) for e in ex}:
            m = np.array([ids(e[:1]) == key for e in ex])
            found[m], gid[m], tuv[m] = self._trace(key, rays[m, 0:3], rays[m, 3:6], rays[m, 6], False)
        for key in {ids(e[1:]) for e in ex}:
            m = np.array([ids(e[1:]) == key for e in ex])
            occ[m] = self._trace(key, rays[m, 8:11], rays[m, 11:14], rays[m, 14], True)[0]
        return found, gid, tuv, occ


_refs = {}


def reference(name):
    if name not in _refs:
        ref = Reference(name)
        rays = make_rays()
        pats = patterns(SCENES[name][1], ref.n_tris)
        _refs[name] = (ref, rays, pats, {p: ref.expect(rays, ex) for p, ex in pats.items()})
    return _refs[name]


def _same(a, b):
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1][a[0]], b[1][a[0]]) and np.array_equal(a[2][a[0]].view(np.uint32), b[2][a[0]].view(np.uint32))
            and np.array_equal(a[3], b[3]))


@pytest.mark.parametrize("name", list(SCENES))
def test_the_inputs_are_not_vacuous(name):
    """with the oracle alone: the scenes share the planes they are meant to; at least a quarter of the diagonal rays are accepted by both
    halves at one t; every exclusion pattern changes the answer of at least one lane; leaving a triangle out changes no other answer"""
    ref, rays, pats, exp = reference(name)
    qa = SCENES[name][1]
    assert ref.n_tris == N_TRIS[name]
    assert pyoracle.OracleScene(ref.scene()).shared_plane_rows() == SCENES[name][2]
    # no origin in the plane of a triangle (see SCENES)
    v = pyoracle.OracleScene(ref.scene()).world_vertices().astype(np.float64)
    nrm = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    for cols in (0, 8):
        dist = np.einsum("tk,rtk->rt", nrm, rays[:, None, cols:cols + 3].astype(np.float64) - v[None, :, 0])
        assert np.all(np.abs(dist) > 1e-3), (name, cols)
    base = exp["none"]
    first, second = exp["ex0 first"], exp["ex0 second"]
    d = np.arange(N) < N_DIAG
    # both halves accept: the full scene answers the first half, without it the second half answers at the same t (and the same point)
    both = d & base[0] & (base[1] == qa) & first[0] & (first[1] == qa + 1) & (first[2][:, 0].view(np.uint32) == base[2][:, 0].view(np.uint32))
    print(name, "diagonal lanes with both halves accepted:", int(both.sum()), "of", N_DIAG)
    assert both.sum() >= N_DIAG // 4
    if name == "quad":  # the shadow rays (the same in every scene, as is the quad): either half alone occludes, nothing does without both
        sboth = d & exp["sex0 first"][3] & exp["sex0 second"][3] & ~exp["sex0 first sex1 second"][3]
        print(name, "diagonal shadow rays that both halves block:", int(sboth.sum()))
        assert sboth.sum() >= N_DIAG // 4
    # (the second half alone excluded leaves those lanes with the first half, as the lowest-id rule has it already)
    assert np.array_equal(second[1][both], base[1][both])
    for p in pats:
        if p != "none":
            assert not _same(exp[p], base), p
    # the special lanes are what they are meant to be
    assert np.all(base[0][40:44]) and np.all(base[2][40:44, 0] == 1.0) and np.all(base[3][40:44])  # a hit at t == tmax
    assert not np.any(base[0][80:84]) and not np.any(base[3][80:84])  # misses
    assert np.all(base[0][84:88]) and not np.any(base[3][84:88]) and not np.any(base[0][88:92]) and np.all(base[3][88:92])  # one ray only
    assert not np.any(base[0][92:94]) and not np.any(base[3][94:96])  # the NaN direction's ray reports nothing
    # the reference is sound: a lane whose answer is not the triangle left out has the same answer, bit for bit, without it
    for gone in range(ref.n_tris):
        f, g, tuv = ref._trace(frozenset([gone]), rays[:, 0:3], rays[:, 3:6], rays[:, 6], False)
        m = base[0] & (base[1] != gone)
        assert np.array_equal(f[m], base[0][m]) and np.array_equal(g[m], base[1][m]) and np.array_equal(tuv[m].view(np.uint32), base[2][m].view(np.uint32)), gone


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENES))
def test_plane_bookkeeping_against_the_oracle(ctx, name):
    ref, rays, pats, exp = reference(name)
    scene = capi.Scene(ctx, ref.scene())
    for p, ex in pats.items():
        out, tuv = capi.probe_intersect_pair(ctx, scene, rays, ex)
        found, gid, etuv, occ = exp[p]
        assert not np.any(out[:, 3]), p  # (no lane leaves the walk under test for the repeat with the contract's division)
        assert np.array_equal(out[:, 0] != 0, found), p
        assert np.array_equal(out[found, 1], gid[found]), p
        assert np.array_equal(tuv[found].view(np.uint32), etuv[found].view(np.uint32)), p
        assert np.array_equal(out[:, 2] != 0, occ), p
