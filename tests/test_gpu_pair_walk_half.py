"""The pair walk's winner as an even id plus a lane mask (csrc/device/disect.h WalkOpt HALF_MASK) and its one record address per trip
(ONE_ADDR). During the walk `best` holds the even id of the winning trip and the mask `half` says whether the trip's second record won; the
id is put together once after the loop. Through akr_probe_intersect_pair, which calls the walk as the pt kernel does with the records staged
in LDS; found / gid / (t, u, v) / occluded against the CPU oracle, bit for bit, 96 lanes (a full wave and a half-filled one).
  scenes   quad            one quad: the winner in the first half, in the second half and on the shared diagonal (both halves accept at one t,
                           the lower id must win: `half` stays clear where the first half accepts too);
           two_quads       two quads on different planes that cross: the second trip wins by its second half after the first trip won by its
                           first (`half` set after it was clear), the reverse (`half` cleared by a later win of a first half), and lanes where
                           the later trip is hit and loses (`half` kept);
           quad_tri_quad   a quad, a triangle with a plane of its own, a quad: the second trip solves a plane per record, its first record is
                           chosen before the second solve and must clear `half`, its second record is nearer on some lanes and farther on
                           others; five records, so the second quad's other half is the walk's tail record;
           quad_quad_tri   five records ending in a lone triangle: the tail record, which runs after the id has been put together, wins over a
                           second-half winner and loses to one;
           chain37         a quad repeated 18 times at growing distances and one triangle behind them: 37 records, hit in the last trip and in
                           the tail, so ids of 32 and above are put together from an even id and a bit.
  rays     from above and from below (the order of the distances reverses); lanes with no hit (the id stays 0xffffffff), a hit at t == tmax,
           lanes with only one of the two rays, NaN directions.
  slots    ex0, sex0, sex1 each on the first and on the second half of the trips the lanes' winners come from, and two mixes that differ
           from lane to lane.
The oracle's tracer takes no excluded ids from Python, so the expectation with an id excluded is the oracle's answer on the scene WITHOUT that
triangle (ids mapped back). The CPU test shows that the cases named above are there: which record would win in which trip is asked of the
oracle on the scene reduced to that trip's records."""
import numpy as np
import pytest

from akari_render_amd import abi, capi
from oracle import pyoracle
from tests.helpers import box_scene

NONE = 0xFFFFFFFF
N = 96
N_DIAG = 24  # lanes 0 .. 23: both rays through a shared diagonal
RANDOM = slice(32, 80)


def _mesh(v, idx):
    return abi.MeshData(vertices=np.array(v, np.float32), indices=np.array(idx, np.uint32).reshape(-1, 3))


def _rect(x0, x1, y0, y1, z, flip=False):
    """a rectangle over [x0, x1] x [y0, y1] in the plane z(x, y), split along the diagonal v0 v2: from (x0, y0) to (x1, y1), or with flip from
    (x1, y0) to (x0, y1)"""
    c = [(x1, y0), (x1, y1), (x0, y1), (x0, y0)] if flip else [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]
    return [[x, y, z(x, y)] for x, y in c], [[0, 1, 2], [0, 2, 3]]


def _join(*parts):
    v, idx = [], []
    for pv, pi in parts:
        idx += [[i + len(v) for i in t] for t in pi]
        v += pv
    return _mesh(v, idx)


def _scene(meshes):
    sd = box_scene()
    eye = np.eye(4, dtype=np.float32).T.reshape(16)
    sd.meshes = meshes
    sd.instances = [abi.InstanceData(i, [0], eye.copy()) for i in range(len(meshes))]
    return sd


QUAD = _rect(-1.0, 1.0, -1.0, 1.0, lambda x, y: 0.0)  # records 0 and 1 of the first four scenes; its shared diagonal is x == y
TILTED = _rect(-1.0, 1.0, -1.0, 1.0, lambda x, y: 0.25 * x, flip=True)  # crosses QUAD along x == 0; its shared diagonal is x == -y
CHAIN_W = 0.25  # chain37: quad i over [i / 4, (i + 1) / 4] x [-1, 1] at z = -i / 8, the lone triangle far below all of them
H_OFF = 0.0625  # ... and its aimed rays start this much higher than the other scenes': between the planes z = -i / 8, not in one of them


def _chain():
    quads = [_rect(i * CHAIN_W, (i + 1) * CHAIN_W, -1.0, 1.0, (lambda zz: lambda x, y: zz)(-i / 8.0)) for i in range(18)]
    return [_join(*quads, ([[-2.0, -4.0, -4.0], [8.0, -4.0, -4.0], [-2.0, 8.0, -4.0]], [[0, 1, 2]]))]


# name -> (meshes, records that take their neighbour's plane, the trips (first ids) the exclusion patterns are laid on)
SCENES = {
    "quad": (lambda: [_mesh(*QUAD)], 1, (0,)),
    "two_quads": (lambda: [_join(QUAD, TILTED)], 2, (0, 2)),
    "quad_tri_quad": (lambda: [_join(QUAD, ([[-3.0, -1.0, -0.125], [3.0, -1.0, -0.125], [0.0, 2.0, 0.625]], [[0, 1, 2]])), _mesh(*TILTED)], 2, (0, 2)),  # z = 1 / 8 + y / 4
    "quad_quad_tri": (lambda: [_join(QUAD, TILTED, ([[-3.0, -1.0, -0.125], [3.0, -1.0, -0.125], [0.0, 2.0, 0.25]], [[0, 1, 2]]))], 2, (0, 2)),  # z = y / 8
    "chain37": (_chain, 18, (32, 34)),
}
N_TRIS = {"quad": 2, "two_quads": 4, "quad_tri_quad": 5, "quad_quad_tri": 5, "chain37": 37}


def make_rays(name):
    """(96, 16): o d tmax - | so sd stmax -. Dyadic numbers in the first 32 lanes, so a ray aimed at a diagonal is on it exactly."""
    rng = np.random.default_rng(7)
    chain = name == "chain37"
    r = np.zeros((N, 16), np.float32)
    r[:, 6], r[:, 14] = 1e20, 16.0
    h_off = np.float32(H_OFF if chain else 0.0)

    def aim(lanes, cols, target, slope, h):  # origin = target + h * (slope, 1), direction = -(slope, 1): reaches the target at t == h
        r[lanes, cols:cols + 3] = target + h[:, None] * np.concatenate([slope, np.ones((len(lanes), 1))], 1)
        r[lanes, cols + 3:cols + 6] = -np.concatenate([slope, np.ones((len(lanes), 1))], 1)

    lanes = np.arange(N_DIAG)
    for cols, seed in ((0, 0), (8, 1)):
        s = (rng.integers(-7, 8, N_DIAG) / 8.0).astype(np.float32)
        if chain:  # the diagonals of the last two quads (ids 32 .. 35): from (x0, -1) to (x0 + w, 1)
            q = 16 + (lanes + seed) % 2
            tgt = np.stack([(q + (s + 1.0) / 2.0) * CHAIN_W, s, -q / 8.0], 1).astype(np.float32)
            slope = np.zeros((N_DIAG, 2), np.float32)  # (straight down: a slanted ray would meet a nearer quad of the chain first)
        else:  # the point (s, s, 0) of QUAD's diagonal
            tgt = np.stack([s, s, np.zeros_like(s)], 1)
            slope = (rng.integers(-2, 3, (N_DIAG, 2)) / 4.0).astype(np.float32)
        aim(lanes, cols, tgt, slope, np.array([0.5, 1.0, 2.0, 0.25], np.float32)[(lanes + seed) % 4] + h_off)
    # lanes 24 .. 31: straight down onto the interior of either half from one unit above; 24 .. 27 with the bound AT the hit (t == tmax)
    lanes = np.arange(24, 32)
    p = np.array([[0.5, -0.25], [-0.5, 0.25], [0.75, 0.5], [-0.25, 0.5], [0.5, -0.5], [-0.75, 0.5], [0.25, 0.125], [-0.5, -0.25]], np.float32)
    if chain:  # the same points inside the quads 17, 16, 17, 16, ... (rows 34, 33, 35, 32, ...)
        q = np.array([17, 16, 17, 16, 17, 16, 16, 17])
        p3 = np.stack([(q + (p[:, 0] + 1.0) / 2.0) * CHAIN_W, p[:, 1], -q / 8.0], 1).astype(np.float32)
    else:
        p3 = np.concatenate([p, np.zeros((8, 1), np.float32)], 1)
    for cols in (0, 8):
        aim(lanes, cols, p3 if cols == 0 else p3[::-1], np.zeros((8, 2), np.float32), np.ones(8, np.float32) + h_off)
    if name in ("quad", "chain37"):  # (in the other scenes something lies above QUAD: the hit at t == 1 would not be the first one)
        r[24:28, 6], r[24:28, 14] = 1.0 + h_off, 1.0 + h_off
    # lanes 32 .. 79: random rays, from above and (every other lane) from below, towards the scene's neighbourhood: hits on every record, and misses
    n = RANDOM.stop - RANDOM.start
    for cols in (0, 8):
        if chain:  # the second half of the chain and the lone triangle beside it
            tgt = np.concatenate([rng.uniform(2.0, 5.0, (n, 1)), rng.uniform(-1.5, 1.5, (n, 1)), np.full((n, 1), -2.0)], 1)
            o = tgt + np.concatenate([rng.uniform(-0.25, 0.25, (n, 2)), np.full((n, 1), 3.0)], 1)
        else:
            tgt = np.concatenate([rng.uniform(-1.25, 1.25, (n, 2)), rng.uniform(0.0, 0.5, (n, 1))], 1)
            o = np.concatenate([rng.uniform(-1.5, 1.5, (n, 2)), rng.uniform(1.25, 2.0, (n, 1))], 1)
            o[1::2, 2] = -o[1::2, 2]
        d = tgt - o
        r[RANDOM, cols:cols + 3], r[RANDOM, cols + 3:cols + 6] = o, d / np.linalg.norm(d, axis=1, keepdims=True)
    # lanes 80 .. 95: lanes 28 .. 31 again, four times: 80 .. 83 with both rays pointing away (misses), 84 .. 87 with the closest-hit ray only,
    # 88 .. 91 with the shadow ray only, 92 .. 95 with a NaN in the direction of the closest-hit ray (92, 93) or of the shadow ray (94, 95)
    r[80:96] = np.tile(r[28:32], (4, 1))
    r[80:84, 5], r[80:84, 13] = 1.0, 1.0
    r[84:88, 14] = -1.0
    r[88:92, 6] = -1.0
    r[92:94, 3], r[94:96, 11] = np.nan, np.nan
    return r


def patterns(name, n_tris):
    """name -> (96, 3) ex0 sex0 sex1: every slot on either half of each trip of SCENES[name][2], and two mixes that differ from lane to lane"""
    out = {"none": (NONE, NONE, NONE)}
    for qa in SCENES[name][2]:
        qb = qa + 1
        out.update({f"{qa}: ex0 first": (qa, NONE, NONE), f"{qa}: ex0 second": (qb, NONE, NONE), f"{qa}: sex0 first": (NONE, qa, NONE),
                    f"{qa}: sex0 second": (NONE, qb, NONE), f"{qa}: sex1 first": (NONE, NONE, qa), f"{qa}: sex1 second": (NONE, NONE, qb),
                    f"{qa}: sex0 first sex1 second": (NONE, qa, qb), f"{qa}: sex0 second sex1 first": (NONE, qb, qa), f"{qa}: all on the pair": (qa, qb, qa)})
    out = {k: np.tile(np.array([v], np.uint32), (N, 1)) for k, v in out.items()}
    ids = np.array(list(range(max(0, n_tris - 7), n_tris)) + [NONE], np.uint32)  # (the last records of a long scene: few distinct sub-scenes for the oracle)
    lane = np.arange(N)
    out["mix"] = np.stack([ids[lane % ids.size], ids[(lane // 2 + 1) % ids.size], ids[(lane // 3 + 2) % ids.size]], 1)
    out["mix 2"] = np.stack([ids[(lane // 2) % ids.size], ids[(lane + 3) % ids.size], ids[(lane // 5) % ids.size]], 1)
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

    def trace(self, gone, o, d, tmax, any_hit):
        n = o.shape[0]
        osc, kept = self._without(frozenset(gone))
        if osc is None:
            return np.zeros(n, bool), np.full(n, NONE, np.uint32), np.zeros((n, 3), np.float32)
        r = np.zeros((n, 8), np.float32)
        r[:, :3], r[:, 3:6], r[:, 7] = o, d, np.maximum(tmax, 0)
        hit, tuv = osc.intersect_many(r, any_hit=any_hit)
        found = (hit[:, 0] != 0) & (tmax >= 0)
        sub = np.where(found, osc.tri_offsets()[hit[:, 1]] + hit[:, 2], kept.size - 1)
        return found, kept[sub], tuv

    def only(self, ids, rays):
        """the closest-hit rays on the scene reduced to the records `ids`: found, gid, tuv"""
        return self.trace(set(range(self.n_tris)) - set(ids), rays[:, 0:3], rays[:, 3:6], rays[:, 6], False)

    def expect(self, rays, ex):
        """found, gid, (t, u, v), occluded per lane"""
        n = rays.shape[0]
        found, gid, tuv, occ = np.zeros(n, bool), np.full(n, NONE, np.uint32), np.zeros((n, 3), np.float32), np.zeros(n, bool)
        ids = lambda row: frozenset(int(x) for x in row if x != NONE)
        for key in {ids(e[:1]) for e in ex}:
            m = np.array([ids(e[:1]) == key for e in ex])
            found[m], gid[m], tuv[m] = self.trace(key, rays[m, 0:3], rays[m, 3:6], rays[m, 6], False)
        for key in {ids(e[1:]) for e in ex}:
            m = np.array([ids(e[1:]) == key for e in ex])
            occ[m] = self.trace(key, rays[m, 8:11], rays[m, 11:14], rays[m, 14], True)[0]
        return found, gid, tuv, occ


_refs = {}


def reference(name):
    if name not in _refs:
        ref = Reference(name)
        rays = make_rays(name)
        pats = patterns(name, ref.n_tris)
        _refs[name] = (ref, rays, pats, {p: ref.expect(rays, ex) for p, ex in pats.items()})
    return _refs[name]


def _same(a, b):
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1][a[0]], b[1][a[0]]) and np.array_equal(a[2][a[0]].view(np.uint32), b[2][a[0]].view(np.uint32))
            and np.array_equal(a[3], b[3]))


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


@pytest.mark.parametrize("name", list(SCENES))
def test_the_inputs_are_not_vacuous(name):
    """with the oracle alone: the scene shares the planes it is meant to, no ray starts in a plane, and the lanes named in the module's
    docstring exist -- which record wins within a trip is the oracle's answer on the scene reduced to the trip"""
    ref, rays, pats, exp = reference(name)
    assert ref.n_tris == N_TRIS[name]
    assert pyoracle.OracleScene(ref.scene()).shared_plane_rows() == SCENES[name][1]
    # no origin in the plane of a triangle: a numerator of exactly 0 sends the whole wave to the repeated walk, past the code under test
    v = pyoracle.OracleScene(ref.scene()).world_vertices().astype(np.float64)
    nrm = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    for cols in (0, 8):
        dist = np.einsum("tk,rtk->rt", nrm, rays[:, None, cols:cols + 3].astype(np.float64) - v[None, :, 0])
        assert np.all(np.abs(dist) > 1e-3), (name, cols)
    base = exp["none"]
    found, gid, tuv = base[0], base[1], base[2]
    d = np.arange(N) < N_DIAG
    count = lambda what, m: (print(name, what + ":", int(np.sum(m))), int(np.sum(m)))[1]
    # on a shared diagonal both halves accept at one t: the full scene answers the first half, without it the second half answers at the same t
    for qa in ((32, 34) if name == "chain37" else (0,)):
        f1, g1, t1 = ref.trace({qa}, rays[:, 0:3], rays[:, 3:6], rays[:, 6], False)
        both = d & found & (gid == qa) & f1 & (g1 == qa + 1) & (_bits(t1[:, 0]) == _bits(tuv[:, 0]))
        assert count(f"diagonal lanes with both halves of trip {qa} accepted", both) >= (N_DIAG // 4 if name == "quad" else 3)  # (other layers lie in front of the diagonal in the scenes of several)
    # each half wins on its own somewhere, in the first trip and in the last one
    last = (ref.n_tris // 2 - 1) * 2
    for k in (0, 1, last, last + 1) if name != "chain37" else (32, 33, 34, 35):
        assert count(f"lanes won by record {k}", found & (gid == k)) >= 1
    if name != "quad":
        t0 = 32 if name == "chain37" else 0  # the two trips looked at: (t0, t0 + 1) and (t0 + 2, t0 + 3)
        fa, ga, ta = ref.only({t0, t0 + 1}, rays)
        fb, gb, tb = ref.only({t0 + 2, t0 + 3}, rays)
        hit2 = fa & fb  # both trips accept
        first_then_second = hit2 & (ga == t0) & (gid == t0 + 3)
        second_then_first = hit2 & (ga == t0 + 1) & (gid == t0 + 2)
        kept_second = hit2 & (ga == t0 + 1) & (gid == t0 + 1)
        kept_first = hit2 & (ga == t0) & (gid == t0)
        if name != "chain37":  # (the chain's trips are met in the order of their distances by construction: a later trip never wins there)
            assert count("`half` set after it was clear (first half, then a later trip's second half)", first_then_second) >= 2
            assert count("`half` cleared by a later first half", second_then_first) >= 2
            assert count("a later trip is hit and loses to a second half", kept_second) >= 2
            assert count("a later trip is hit and loses to a first half", kept_first) >= 2
    if name == "quad_tri_quad":  # the trip (2, 3): a plane per record
        f2, _, t2 = ref.only({2}, rays)
        f3, _, t3 = ref.only({3}, rays)
        assert count("own-plane trip: the second record nearer than the chosen first", f2 & f3 & (t3[:, 0] < t2[:, 0]) & (gid == 3)) >= 2
        assert count("own-plane trip: the second record farther than the chosen first", f2 & f3 & (t3[:, 0] > t2[:, 0]) & (gid == 2)) >= 2
        f01, g01, _ = ref.only({0, 1}, rays)
        assert count("own-plane trip: its first record takes over from a second half", f01 & (g01 == 1) & (gid == 2)) >= 1
    if name in ("quad_quad_tri", "quad_tri_quad", "chain37"):  # the tail record against the walk's winner before it
        tail = ref.n_tris - 1
        fl, gl, _ = ref.only(set(range(tail)), rays)
        ft, _, _ = ref.only({tail}, rays)
        assert count("the tail record wins", found & (gid == tail)) >= 1
        if name == "quad_quad_tri":
            assert count("the tail record wins over a second-half winner", fl & (gl % 2 == 1) & (gid == tail)) >= 2
            assert count("the tail record is hit and loses to a second-half winner", fl & ft & (gl % 2 == 1) & (gid == gl)) >= 2
            assert count("the tail record wins over a first-half winner", fl & (gl % 2 == 0) & (gid == tail)) >= 1
    if name == "chain37":
        assert count("lanes with an id of 32 or above", found & (gid >= 32)) >= 24
    # the exclusion patterns change answers. (A shadow ray that meets several layers stays occluded without one of them: in the scenes of
    # three layers a pattern of shadow slots alone may change nothing; the walk's code for those slots is the same in every scene.)
    idle = [p for p in pats if p != "none" and _same(exp[p], base)]
    print(name, "patterns that change no answer:", idle)
    assert not [p for p in idle if p.split(": ")[-1].startswith(("ex0", "all", "mix"))]
    assert not idle or name in ("quad_tri_quad", "quad_quad_tri")
    # the special lanes are what they are meant to be
    if name in ("quad", "chain37"):
        assert np.all(found[24:28]) and np.all(tuv[24:28, 0] == np.float32(1.0 + (H_OFF if name == "chain37" else 0.0))) and np.all(base[3][24:28])  # a hit at t == tmax
    assert not np.any(found[80:84]) and not np.any(base[3][80:84])  # misses
    assert np.all(found[84:88]) and not np.any(base[3][84:88]) and not np.any(found[88:92]) and np.all(base[3][88:92])  # one ray only
    assert not np.any(found[92:94]) and not np.any(base[3][94:96])  # the NaN direction's ray reports nothing
    assert count("random lanes without a hit", ~found[RANDOM]) >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENES))
def test_half_mask_against_the_oracle(ctx, name):
    ref, rays, pats, exp = reference(name)
    scene = capi.Scene(ctx, ref.scene())
    for p, ex in pats.items():
        out, tuv = capi.probe_intersect_pair(ctx, scene, rays, ex)
        found, gid, etuv, occ = exp[p]
        assert not np.any(out[:, 3]), p  # (no lane leaves the walk under test for the repeat with the contract's division)
        assert np.array_equal(out[:, 0] != 0, found), p
        assert np.all(out[~found, 1] == NONE), p  # no hit: the id stays what it was, whatever `half` holds
        assert np.array_equal(out[found, 1], gid[found]), p
        assert np.array_equal(_bits(tuv[found]), _bits(etuv[found])), p
        assert np.array_equal(out[:, 2] != 0, occ), p
