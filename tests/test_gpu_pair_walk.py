"""The pair walk of scenes of at most 64 triangles (csrc/device/disect.h trace_pair_exhaustive) through akr_probe_intersect_pair, which
calls it as the pt kernel does: closest hit, occlusion and the exclusion slots against the oracle, bit for bit; and the walk's repeat
with the contract's division (a numerator below the floor), in the probe and end to end in a render."""
import numpy as np
import pytest

from akari_render_amd import abi, capi
from oracle import pyoracle, scene_json
from tests.helpers import box_scene, make_config, n_bit_diff

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
N_RAYS = 4096


def _xf(scale, t):
    m = np.eye(4, dtype=np.float32)
    m[:3, :3] *= np.float32(scale)
    m[:3, 3] = t
    return m.T.reshape(16).copy()


def three_tri_scene():
    sd = box_scene()
    sd.meshes[0].indices = sd.meshes[0].indices[[0, 5, 10]].copy()  # an odd count: the walk's tail record
    return sd


def sixty_four_tri_scene():
    sd = box_scene()
    box = sd.meshes[0]
    part = abi.MeshData(vertices=box.vertices.copy(), indices=box.indices[:4].copy())
    sd.meshes = [box, part]
    rng = np.random.default_rng(64)
    inst = [abi.InstanceData(0, [0], _xf(0.2 + 0.1 * k, rng.uniform(-0.6, 0.6, 3).astype(np.float32))) for k in range(5)]
    sd.instances = inst + [abi.InstanceData(1, [0], _xf(0.9, np.zeros(3, np.float32)))]
    return sd


def _dirs(rng, n):
    d = rng.normal(size=(n, 3)).astype(np.float32)
    return d / np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)


def _make_rays(rng, verts, n):
    """(o, d) x n: half random, half aimed at vertices and edge points of the scene, some of them axis-parallel"""
    lo, hi = verts.reshape(-1, 3).min(0) - 0.1, verts.reshape(-1, 3).max(0) + 0.1
    o = (rng.random((n, 3)) * (hi - lo) + lo).astype(np.float32)
    d = _dirs(rng, n)
    h = n // 2
    tri = verts[rng.integers(0, verts.shape[0], n - h)]
    w = rng.random((n - h, 1)).astype(np.float32)
    w[: (n - h) // 2] = 0.0  # vertices; the rest: points on the edge v0 v1
    target = tri[:, 0] * (1 - w) + tri[:, 1] * w
    dd = target - o[h:]
    d[h:] = (dd / np.linalg.norm(dd, axis=1, keepdims=True)).astype(np.float32)
    k = n // 8
    d[:k] = np.eye(3, dtype=np.float32)[rng.integers(0, 3, k)] * rng.choice(np.array([-1.0, 1.0], np.float32), (k, 1))  # dz == 0 on the planes along the axis
    return o, d


def _mt_f64(o, d, verts):
    """t, u, v of every (ray, triangle) pair in f64 (Moeller-Trumbore)"""
    o, d, v = o.astype(np.float64)[:, None], d.astype(np.float64)[:, None], verts.astype(np.float64)[None]
    e1, e2 = v[:, :, 1] - v[:, :, 0], v[:, :, 2] - v[:, :, 0]
    p = np.cross(d, e2)
    with np.errstate(all="ignore"):
        inv = 1.0 / np.sum(e1 * p, -1)
        s = o - v[:, :, 0]
        u = np.sum(s * p, -1) * inv
        q = np.cross(s, e1)
        return np.sum(e2 * q, -1) * inv, u, np.sum(d * q, -1) * inv


def _no_second_candidate(o, d, verts, gid, t):
    """rays whose hit (gid, t) has no other triangle near the same point at the same distance (a tie would make 'the next hit' ambiguous)"""
    tt, u, v = _mt_f64(o, d, verts)
    eps = 1e-3
    with np.errstate(all="ignore"):
        near = (u > -eps) & (v > -eps) & (u + v < 1 + eps) & (np.abs(tt - t[:, None]) < eps * np.maximum(1.0, t[:, None]))
    near[np.arange(o.shape[0]), np.minimum(gid, verts.shape[0] - 1)] = False
    return ~near.any(1)


class Case:
    """rays, the oracle's answers and the derived exclusion cases of one scene, computed once"""

    def __init__(self, sd, seed):
        self.sd = sd
        self.osc = pyoracle.OracleScene(sd)
        verts = self.osc.world_vertices()
        off = self.osc.tri_offsets()
        rng = np.random.default_rng(seed)
        n = N_RAYS
        o, d = _make_rays(rng, verts, n)
        so, sdir = _make_rays(rng, verts, n)
        tmax = np.full(n, 1e20, np.float32)
        stmax = (rng.random(n) * 3).astype(np.float32)
        stmax[::7] = -1.0  # no shadow partner
        tmax[3::11] = -1.0  # no closest-hit ray
        self.o, self.d, self.so, self.sdir, self.tmax, self.stmax = o, d, so, sdir, tmax, stmax

        def closest(o, d, tmin, tmax):
            r = np.zeros((n, 8), np.float32)
            r[:, :3], r[:, 3:6], r[:, 6], r[:, 7] = o, d, tmin, tmax
            hit, tuv = self.osc.intersect_many(r)
            return hit[:, 0] != 0, np.where(hit[:, 0] != 0, off[hit[:, 1]] + hit[:, 2], NONE).astype(np.uint32), tuv

        def any_hit(o, d, tmin, tmax):
            r = np.zeros((n, 8), np.float32)
            r[:, :3], r[:, 3:6], r[:, 6], r[:, 7] = o, d, tmin, tmax
            return self.osc.intersect_many(r, any_hit=True)[0][:, 0] != 0

        self.closest, self.any_hit = closest, any_hit
        self.n_tris = verts.shape[0]
        self.c_found, self.c_gid, self.c_tuv = closest(o, d, 0.0, np.maximum(tmax, 0))
        self.c_found &= tmax >= 0
        self.s_occ = any_hit(so, sdir, 0.0, np.maximum(stmax, 0)) & (stmax >= 0)
        # the nearest blocker of the shadow ray and whether the hits are free of ties
        self.s1_found, self.s1_gid, self.s1_tuv = closest(so, sdir, 0.0, np.maximum(stmax, 0))
        self.s1_found &= stmax >= 0
        self.c_clean = self.c_found & _no_second_candidate(o, d, verts, self.c_gid, self.c_tuv[:, 0].astype(np.float64))
        self.s_clean = self.s1_found & _no_second_candidate(so, sdir, verts, self.s1_gid, self.s1_tuv[:, 0].astype(np.float64))

    def rays16(self):
        r = np.zeros((N_RAYS, 16), np.float32)
        r[:, 0:3], r[:, 3:6], r[:, 6] = self.o, self.d, self.tmax
        r[:, 8:11], r[:, 11:14], r[:, 14] = self.so, self.sdir, self.stmax
        return r


SCENES = {"cbox": None, "tri3": three_tri_scene, "tri64": sixty_four_tri_scene}
_cases = {}


@pytest.fixture
def case(request, cbox_path):
    name = request.param
    if name not in _cases:
        sd = scene_json.load_scene(cbox_path, 32, 32) if name == "cbox" else SCENES[name]()
        _cases[name] = Case(sd, seed=len(name) + 100)
    return _cases[name]


def _check(out, tuv, found, gid, ref_tuv, occ, what):
    assert np.array_equal(out[:, 0] != 0, found), what
    assert np.array_equal(out[found, 1], gid[found]), what
    assert np.array_equal(tuv[found].view(np.uint32), ref_tuv[found].view(np.uint32)), what
    assert np.array_equal(out[:, 2] != 0, occ), what


@pytest.mark.parametrize("case", list(SCENES), indirect=True)
def test_pair_walk_against_the_oracle(ctx, case):
    c = case
    n = N_RAYS
    assert c.n_tris <= 64
    scene = capi.Scene(ctx, c.sd)
    rays = c.rays16()
    none = np.full((n, 3), NONE, np.uint32)
    out, tuv = capi.probe_intersect_pair(ctx, scene, rays, none)
    print(f"{c.n_tris} triangles: closest hits {int(c.c_found.sum())}, occluded {int(c.s_occ.sum())}, tie-free {int(c.c_clean.sum())} / {int(c.s_clean.sum())}, "
          f"lanes in a repeated walk {int((out[:, 3] != 0).sum())}")
    assert c.c_found.sum() > n // 16 and c.s_occ.sum() > n // 64  # (the inputs are worth the run)
    _check(out, tuv, c.c_found, c.c_gid, c.c_tuv, c.s_occ, "no exclusion")

    # excluding triangles the oracle does not return changes nothing (ids at both ends of both mask halves among them)
    rng = np.random.default_rng(1)
    pool = np.array([0, 31, 32, 63, c.n_tris - 1, c.n_tris // 2], np.uint32)
    pool = pool[pool < c.n_tris]
    ex = np.stack([rng.choice(pool, n), rng.choice(pool, n), rng.integers(0, c.n_tris, n).astype(np.uint32)], 1).astype(np.uint32)
    ex[ex[:, 0] == c.c_gid, 0] = NONE
    # (a shadow ray: any blocker counts, so an excluded id must not be a blocker at all -- keep ids only where nothing occludes or where
    # the exclusion is the oracle's non-blocker by construction: drop the slots on occluded rays unless the nearest blocker differs and the ray is tie-free)
    keep = ~c.s_occ
    ex[~keep, 1] = NONE
    ex[~keep, 2] = NONE
    out2, tuv2 = capi.probe_intersect_pair(ctx, scene, rays, ex)
    _check(out2, tuv2, c.c_found, c.c_gid, c.c_tuv, c.s_occ, "exclusion of triangles that are not hit")

    # excluding the returned triangle = the oracle's answer with tmin raised just past its t (rays without a second candidate at that t)
    t1 = np.nextafter(c.c_tuv[:, 0], np.float32(np.inf))
    f2, g2, tuv_2 = c.closest(c.o, c.d, np.where(c.c_clean, t1, 0).astype(np.float32), np.maximum(c.tmax, 0))
    s1 = np.nextafter(c.s1_tuv[:, 0], np.float32(np.inf))
    occ2 = c.any_hit(c.so, c.sdir, np.where(c.s_clean, s1, 0).astype(np.float32), np.maximum(c.stmax, 0)) & (c.stmax >= 0)
    ex = np.full((n, 3), NONE, np.uint32)
    ex[c.c_clean, 0] = c.c_gid[c.c_clean]
    slot = 1 + (np.arange(n) & 1)  # alternately through either shadow slot
    ex[np.flatnonzero(c.s_clean), slot[c.s_clean]] = c.s1_gid[c.s_clean]
    f_exp = np.where(c.c_clean, f2 & (c.tmax >= 0), c.c_found)
    g_exp = np.where(c.c_clean, g2, c.c_gid).astype(np.uint32)
    tuv_exp = np.where(c.c_clean[:, None], tuv_2, c.c_tuv).astype(np.float32)
    occ_exp = np.where(c.s_clean, occ2, c.s_occ)
    assert c.c_clean.sum() > n // 32 and c.s_clean.sum() > n // 128
    out3, tuv3 = capi.probe_intersect_pair(ctx, scene, rays, ex)
    _check(out3, tuv3, f_exp, g_exp, tuv_exp, occ_exp, "exclusion of the returned triangle")
    if c.n_tris == 64:  # the upper limit: ids 31 / 32 / 63 excluded on every lane, every lane held to the oracle's next hit
        exp = excluded_31_32_63(c, f2, g2, tuv_2, s1)
        ex = np.tile(np.array([[31, 32, 63]], np.uint32), (n, 1))
        out4, tuv4 = capi.probe_intersect_pair(ctx, scene, rays, ex)
        kc, ks = exp["check_c"], exp["check_s"]
        print(f"ids 31 / 32 / 63 excluded: lanes whose hit was 31: {int(exp['hit_31'].sum())}, whose nearest blocker was 32 or 63: {int(exp['blocked'].sum())}; "
              f"lanes checked {int(kc.sum())} / {int(ks.sum())}")
        assert (exp["hit_31"] & kc).sum() > 0 and (exp["blocked"] & ks).sum() > 0  # (the inputs are worth the run)
        fnd = exp["found"] & kc
        assert np.array_equal((out4[:, 0] != 0)[kc], exp["found"][kc])
        assert np.array_equal(out4[fnd, 1], exp["gid"][fnd]) and np.array_equal(tuv4[fnd].view(np.uint32), exp["tuv"][fnd].view(np.uint32))
        assert np.array_equal((out4[:, 2] != 0)[ks], exp["occ"][ks])


def excluded_31_32_63(c, f2, g2, tuv_2, s1):
    """What the oracle says with ex0 = 31 and sex = {32, 63} on every lane. f2 / g2 / tuv_2: the closest hit past the first one (tie-free
    lanes), s1: just past the nearest blocker's t. A lane whose answer the oracle cannot give without ambiguity (a tie at the excluded hit,
    or both 32 and 63 in front of everything else) is left out of the comparison: check_c / check_s."""
    hit_31 = c.c_found & (c.c_gid == 31)
    check_c = ~hit_31 | c.c_clean
    found = np.where(hit_31, f2 & (c.tmax >= 0), c.c_found)
    gid = np.where(hit_31, g2, c.c_gid).astype(np.uint32)
    tuv = np.where(hit_31[:, None], tuv_2, c.c_tuv).astype(np.float32)
    blocked = c.s1_found & np.isin(c.s1_gid, (32, 63))
    fs2, gs2, _ = c.closest(c.so, c.sdir, np.where(blocked & c.s_clean, s1, 0).astype(np.float32), np.maximum(c.stmax, 0))
    both = blocked & fs2 & np.isin(gs2, (32, 63))
    check_s = ~blocked | (c.s_clean & ~both)
    occ = np.where(blocked, fs2, c.s_occ)
    return dict(hit_31=hit_31, blocked=blocked, check_c=check_c, check_s=check_s, found=found, gid=gid, tuv=tuv, occ=occ)


def floor_scene(width=64, height=64):
    """the closed box seen from its centre, plus a quad in the plane y = 0 behind the camera: the camera's origin lies in that plane, so
    the quad's plane row gives a numerator of exactly 0 for every camera ray -- below the walk's floor"""
    sd = box_scene(width=width, height=height)
    q = np.array([[-0.2, 0.0, 0.5], [0.2, 0.0, 0.5], [0.2, 0.0, 0.9], [-0.2, 0.0, 0.9]], dtype=np.float32)
    quad = abi.MeshData(vertices=q, indices=np.array([[0, 1, 2], [0, 2, 3]], dtype=np.uint32))
    sd.meshes = [sd.meshes[0], quad]
    sd.instances = [sd.instances[0], abi.InstanceData(1, [0], _xf(1.0, np.zeros(3, np.float32)))]
    return sd


def test_repeated_walk_end_to_end(ctx):
    sd = floor_scene()
    scene = capi.Scene(ctx, sd)
    # the probe on the camera's origin: every lane's wave repeats the walk (so the render below cannot pass by never leaving the fast path)
    n = 1024
    rng = np.random.default_rng(3)
    rays = np.zeros((n, 16), np.float32)
    rays[:, 3:6] = _dirs(rng, n)
    rays[:, 6] = 1e20
    rays[:, 14] = -1.0
    out, tuv = capi.probe_intersect_pair(ctx, scene, rays, np.full((n, 3), NONE, np.uint32))
    assert np.all(out[:, 3] == 1)
    osc = pyoracle.OracleScene(sd)
    r8 = np.zeros((n, 8), np.float32)
    r8[:, 3:6], r8[:, 7] = rays[:, 3:6], 1e20
    hit, otuv = osc.intersect_many(r8)
    assert np.array_equal(out[:, 0] != 0, hit[:, 0] != 0) and np.array_equal(tuv.view(np.uint32)[hit[:, 0] != 0], otuv.view(np.uint32)[hit[:, 0] != 0])
    # and a lane away from the plane does not repeat it
    rays[:, 1] = 0.25
    out, _ = capi.probe_intersect_pair(ctx, scene, rays, np.full((n, 3), NONE, np.uint32))
    assert np.all(out[:, 3] == 0)
    # the render: film and sampler states equal the oracle's, bit for bit
    cfg = make_config(spp=16, spp_per_pass=16, max_depth=4, rr_depth=5)
    w, h = sd.camera.width, sd.camera.height
    film = capi.Film(ctx, w, h)
    se = capi.PtSession(ctx, scene, cfg, film)
    se.passes(1, blocking=True)
    gstates = se.sampler_states(w * h)
    se.end()
    g = film.read()
    ostates = pyoracle.init_pcg32_states(w * h, cfg.sampler_seed)
    o, _ = osc.render(cfg, states=ostates)
    assert n_bit_diff(g, o) == 0
    assert np.array_equal(gstates, ostates)
