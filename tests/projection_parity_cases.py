"""The scenes, configurations and expected kernel variants of tests/test_gpu_projection_parity.py (the orthographic and the panorama camera of
DESIGN.md 4.17 on the GPU against the CPU oracle, bit for bit). They live here so that tests/test_projection_parity_cases.py can check on the CPU,
with the oracle and the library's host build alone, that every case is what it claims to be: that the session the library plans runs the LENS
kernel the case is there for, that the projection changes the film, that the aligned scenes do send axis-aligned rays along planes and through
edges and vertices, and that the panorama room is seen in all eight octants. Materials, lights, samplers, `Case`, `add`'s bookkeeping and the
oracle's side are those of tests/punct_parity_cases.py."""
import dataclasses
import functools

import numpy as np

from akari_render_amd import abi, capi
from tests import punct_parity_cases as P
from tests.helpers import make_config
from tests.punct_parity_cases import BVH, EXH, F_BVH, F_FEAT, F_LENS, F_PMJ, F_PUNCT, F_STAGE, MATERIALS, SAMPLERS, THREE, grid_lights, host_plan, lit_scene, oracle_render, tex_scene
from tests.test_gpu_env_parity import _box, _quad

F = np.float32
PD = abi.ProjectionData
F_LTREE = 256  # akr_kernel_info.kernel_flags bit 8: "walks a light tree"; the launch plan does not report it
ORTHO, PANORAMA = abi.PROJECTION_ORTHOGRAPHIC, abi.PROJECTION_PANORAMA

# the four cameras of the floor-and-box scene (the camera at (0, 0.8, 4) looks down at the box): the orthographic film spans 3 units; the lens is
# focused on the box; the window looks ahead and down, off-centre
LENS = abi.LensData(0.12, 4.2)
PROJECTIONS = {
    "ortho": (PD(type=ORTHO, ortho_scale=3.0), None),
    "ortho_lens": (PD(type=ORTHO, ortho_scale=3.0), LENS),
    "panorama": (PD(type=PANORAMA), None),
    "panorama_window": (PD(type=PANORAMA, longitude_min=-0.75, longitude_max=0.5, latitude_min=-0.875, latitude_max=0.25), None),
}

CASES = {}


def add(name, scene, cfg, opts=EXH, tags=(), **want):
    """punct_parity_cases.add into this table; every case runs LENS kernels (want lens = 1 unless said otherwise)"""
    assert name not in CASES, name
    want.setdefault("lens", True)
    want.setdefault("punct", False)
    CASES[name] = P.Case(name, scene, dict(cfg), dict(opts), P._want(opts, cfg, **want), tuple(tags))
    return name


def flags(case):
    """the kernel_flags the session must report (Case.flags, and the bits it does not know: the tree's and the guides')"""
    f = case.flags() | (F_LTREE if "ltree" in case.tags else 0) | (F_FEAT if "feat" in case.tags else 0)
    return f & ~F_BVH if case.want.get("inst") else f  # (bit 0 is the flattened scene's tree: a kept scene's two-level traversal does not set it)


def projected(sd, which):
    """`sd` through the camera PROJECTIONS[which] (a name) or a (projection, lens) pair"""
    sd.projection, sd.lens = PROJECTIONS[which] if isinstance(which, str) else which
    return sd


BASE = dict(spp=8, spp_per_pass=8, max_depth=5, rr_depth=2)

# ---------------------------------------------------------------------------------------------------------------- projections x materials x routes x lighting
MATERIAL_CASES = []
for _p in PROJECTIONS:
    for _m in MATERIALS:
        if _m not in ("diffuse", "glass", "rough_metal", "coated"):
            continue
        for _r, _o in (("exh", EXH), ("bvh", BVH)):
            for _l, _kw in (("emitter", dict(emitters=2, env=None)), ("env", dict(emitters=0, env=True))):
                MATERIAL_CASES.append(add(f"mat-{_p}-{_m}-{_r}-{_l}", functools.partial(lambda p, m, kw: projected(lit_scene(m, [], **kw), p), _p, _m, _kw), BASE, _o,
                                          env=int(_l == "env")))
assert len(MATERIAL_CASES) == 4 * 4 * 2 * 2

# ---------------------------------------------------------------------------------------------------------------- every LENS unit of the pt kernels
UNIT_CFG = dict(spp=4, spp_per_pass=4, max_depth=4, rr_depth=2)
TREE_LIGHTS = grid_lights(9)


def _unit_scene(kind, env, projection):
    lights = {"plain": [], "feat": [], "punct": THREE, "punct_tree": TREE_LIGHTS + THREE[2:]}[kind]
    return projected(lit_scene("glass", lights, emitters=1, env=True if env else None, w=16, h=16), projection)


UNIT_CASES = []
for _k in ("plain", "punct", "punct_tree", "feat"):
    for _env in (0, 1):
        for _p in ("ortho", "panorama_window"):  # (the window looks at the floor and the box, where the lights show; the full sphere is mostly sky)
            _o = dict(BVH if (_env + (_p == "ortho")) % 2 else EXH, **({"light_tree": 1} if _k == "punct_tree" else {}))
            _s = abi.SAMPLER_SOBOL if _k == "feat" else (abi.SAMPLER_PMJ02BN if _env else abi.SAMPLER_INDEPENDENT)
            UNIT_CASES.append(add(f"unit-{_k}-env{_env}-{_p}", functools.partial(_unit_scene, _k, _env, _p), dict(UNIT_CFG, sampler_type=_s, sampler_seed=7), _o,
                                  tags=(("ltree",) if _k == "punct_tree" else ()) + (("feat",) if _k == "feat" else ()) + ("kind:" + _k,),
                                  env=_env, punct=_k.startswith("punct")))

# ---------------------------------------------------------------------------------------------------------------- aligned rays
# An axis-aligned room around the film of an orthographic camera at the origin: ortho_scale 4 on 32 x 32 puts pixel edges on the multiples of 1/8
# and pixel centres on the odd multiples of 1/16 (the room is half a unit wider than the film: a kept scene's trees take origins inside its box only). The room's walls, floor and ceiling lie on pixel edges and along the rays; the
# cube A has every vertex coordinate on an odd multiple of 1/16, so its silhouette edges, its faces' diagonals and its corners lie exactly under
# pixel centres, and its side faces contain whole rows of rays; the cube B lies on pixel edges. The quarter-turned camera at (1, 0, -1) looks along
# -x and sees the same lattice in (z, y).
ALIGNED_SCALE, ALIGNED_SIZE = 4.0, 32
TURNED = np.array([[0, 0, 1, 1], [0, 1, 0, 0], [-1, 0, 0, -1], [0, 0, 0, 1]], F)  # rows; the columns: X = (0, 0, -1), Y = (0, 1, 0), Z = (1, 0, 0), T = (1, 0, -1)
BOX0 = dict(filter_type=abi.FILTER_BOX, filter_radius=0.0)


def _merge(meshes):
    v, idx, n = [], [], 0
    for m in meshes:
        v.append(m.vertices)
        idx.append(m.indices + n)
        n += len(m.vertices)
    return abi.MeshData(vertices=np.concatenate(v).astype(F), indices=np.concatenate(idx).astype(np.uint32))


def _room_mesh():
    """x, y in [-2.5, 2.5], z in [-4, 2]; normals inwards"""
    return _merge([_quad((0, -2.5, -1), (2.5, 0, 0), (0, 0, -3)), _quad((0, 2.5, -1), (2.5, 0, 0), (0, 0, 3)), _quad((-2.5, 0, -1), (0, 2.5, 0), (0, 0, 3)),
                   _quad((2.5, 0, -1), (0, 0, 3), (0, 2.5, 0)), _quad((0, 0, -4), (2.5, 0, 0), (0, 2.5, 0)), _quad((0, 0, 2), (0, 2.5, 0), (2.5, 0, 0))])


def _placed(scale, at):
    m = np.eye(4, dtype=F)
    m[0, 0] = m[1, 1] = m[2, 2] = scale
    m[:3, 3] = at
    return m.T.reshape(16).copy()


def aligned_room(material="diffuse", turned=False, w=ALIGNED_SIZE, h=ALIGNED_SIZE, projection=None, c2w=None):
    """the room, the unit cube instanced twice (A: half 7/16 at (-1/2, -1/2, -2), of `material`; B: half 1/2 at (5/8, -1, -5/2), glass), an emitter under the ceiling"""
    meshes = [_room_mesh(), _box((0, 0, 0), 1.0, 0.0), _quad((0, 1.875, -2), (0.5, 0, 0), (0, 0, 0.5))]
    mats = [MATERIALS["diffuse"], MATERIALS[material], MATERIALS["glass"], abi.MaterialData(kind=abi.MAT_EMISSION, emission_color=(6.0, 5.0, 4.0), emission_strength=4.0)]
    eye = np.eye(4, dtype=F).reshape(16).copy()
    insts = [abi.InstanceData(0, [0], eye), abi.InstanceData(1, [1], _placed(0.4375, (-0.5, -0.5, -2.0))), abi.InstanceData(1, [2], _placed(0.5, (0.625, -1.0, -2.5))),
             abi.InstanceData(2, [3], eye.copy())]
    if c2w is None:
        c2w = TURNED.T.reshape(16).copy() if turned else eye.copy()
    sd = abi.SceneData(meshes, insts, mats, abi.CameraData(c2w=np.asarray(c2w, F), fov=0.9, width=w, height=h))
    sd.ggx_table = P._ggx()
    sd.projection = projection if projection is not None else PD(type=ORTHO, ortho_scale=ALIGNED_SCALE)
    return sd


ALIGNED_ROUTES = {
    "exh": (EXH, {}),
    "bvh": (BVH, {}),
    "kept": (dict(force_bvh=1, instancing=1, wavefront=0, specialise=0), dict(inst=1, stage=False)),
    "kept_wavefront": (dict(force_bvh=1, instancing=1, wavefront=1, specialise=0), dict(inst=1, stage=False)),
    "wavefront_carried": (dict(force_bvh=1, instancing=0, wavefront=1, specialise=0, wf_carry=2), {}),
}
ALIGNED_CFG = dict(spp=8, spp_per_pass=4, max_depth=5, rr_depth=2)
ALIGNED_CASES = []
for _t in (False, True):
    for _f, _fkw in (("box0", BOX0), ("default", {})):
        for _r, (_o, _w) in ALIGNED_ROUTES.items():
            _m = "rough_metal" if _r in ("bvh", "kept_wavefront") else "diffuse"
            ALIGNED_CASES.append(add(f"aligned-{'turned' if _t else 'identity'}-{_f}-{_r}", functools.partial(aligned_room, _m, _t),
                                     dict(ALIGNED_CFG, sampler_seed=3, **_fkw), _o, tags=("aligned",) + (("box0",) if _f == "box0" else ()) + ("route:" + _r,), **_w))

# ---------------------------------------------------------------------------------------------------------------- panorama extremes
# The camera inside the closed room, full sphere: depth-0 rays in all eight octants, pole rows whose cos(latitude) is tiny, the seam columns; the
# Gaussian filter of radius 1.5 pixels carries film points past the film's edges there. A generic turn of the camera keeps the rays off the axes.
GAUSS = dict(filter_type=abi.FILTER_GAUSSIAN, filter_radius=1.5)


def _generic_c2w():
    m = np.eye(4)
    m[:3, :3] = P._rot(0.3, -0.5)
    m[:3, 3] = [0.25, 0.125, -1.0]
    return m.astype(F).T.reshape(16).copy()


def panorama_room(w, h, window=None, turned=False):
    pr = PD(type=PANORAMA) if window is None else PD(type=PANORAMA, longitude_min=window[0], longitude_max=window[1], latitude_min=window[2], latitude_max=window[3])
    return aligned_room("rough_metal", w=w, h=h, projection=pr, c2w=_generic_c2w() if turned else None)


NARROW = (0.5, float(F(0.5) + F(2.0 ** -6)), -0.75, 0.25)  # longitude_max - longitude_min = 2^-6
PANORAMA_CASES = []
for _k, (_w, _h) in enumerate(((32, 16), (31, 15))):
    for _j, _s in enumerate(SAMPLERS):
        PANORAMA_CASES.append(add(f"pano-room-{_w}x{_h}-{_s}", functools.partial(panorama_room, _w, _h, None, bool((_k + _j) % 2)),
                                  dict(BASE, sampler_type=SAMPLERS[_s], sampler_seed=5, **GAUSS), BVH if (_k + _j) % 2 else EXH, tags=("octants",)))
    PANORAMA_CASES.append(add(f"pano-narrow-{_w}x{_h}", functools.partial(panorama_room, _w, _h, NARROW, bool(_k)), dict(BASE, sampler_seed=5, **GAUSS), EXH if _k else BVH))

# ---------------------------------------------------------------------------------------------------------------- scenes of the tests outside the table
SCHED = {name: functools.partial(lambda which: projected(P.SCHED_SCENE(), which), which)
         for name, which in (("progressive", "ortho"), ("shards", "panorama"), ("ranges", "ortho_lens"), ("retired", "panorama_window"))}
ROOM_WINDOW = PD(type=PANORAMA, longitude_min=-1.5, longitude_max=1.0, latitude_min=-1.0, latitude_max=0.75)
AOV_SCENES = {"ortho": functools.partial(lambda: projected(tex_scene(32, 32, P.ROOM_LIGHTS, True), (PD(type=ORTHO, ortho_scale=1.25), None))),
              "panorama": functools.partial(lambda: projected(tex_scene(32, 32, P.ROOM_LIGHTS, True), (ROOM_WINDOW, None)))}
FEAT_SCENES = {"ortho": functools.partial(lambda: projected(lit_scene("coated", [], emitters=2, env=True), "ortho_lens")),
               "panorama": functools.partial(lambda: projected(lit_scene("coated", [], emitters=2, env=True), "panorama_window"))}
# name -> (scene, make_config's keywords): the projection must change a quarter of the film's floats
EXTRA = {
    "schedules-progressive": (SCHED["progressive"], dict(spp=12, spp_per_pass=5, max_depth=5, rr_depth=2, sampler_seed=4)),
    "schedules-shards": (SCHED["shards"], dict(spp=8, spp_per_pass=4, max_depth=5, rr_depth=2, sampler_type=abi.SAMPLER_PMJ02BN, sampler_seed=6)),
    "schedules-ranges": (SCHED["ranges"], dict(spp=12, spp_per_pass=4, max_depth=5, rr_depth=2, sampler_type=abi.SAMPLER_SOBOL, sampler_seed=5)),
    "schedules-retired": (SCHED["retired"], dict(spp=8, spp_per_pass=4, max_depth=5, rr_depth=2, sampler_seed=8, tile_w=16, tile_h=16)),
    "feat-ortho": (FEAT_SCENES["ortho"], dict(spp=8, spp_per_pass=4, max_depth=5, sampler_type=abi.SAMPLER_PMJ02BN, sampler_seed=5)),
    "feat-panorama": (FEAT_SCENES["panorama"], dict(spp=8, spp_per_pass=4, max_depth=5, sampler_type=abi.SAMPLER_SOBOL, sampler_seed=5)),
}


# ---------------------------------------------------------------------------------------------------------------- what the aligned cases claim, in float64
def pixel_centre_rays(sd):
    """the oracle's camera rays of every pixel centre (the box filter of radius 0): float64 (h * w, 6)"""
    from oracle import pyoracle
    w, h = sd.camera.width, sd.camera.height
    ys, xs = np.mgrid[0:h, 0:w]
    pixels = np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.uint32)
    half = np.full((len(pixels), 2), 0.5, F)
    return pyoracle.OracleScene(sd).lens_ray_many(pixels, half, half, abi.FILTER_BOX, 0.0).astype(np.float64)


def aligned_facts(sd):
    """Of an aligned scene, exactly (every coordinate is a small dyadic number): the common primary direction, the number of distinct scene planes
    parallel to it, the pixel centres that lie exactly on an edge two triangles share (seen along the rays) and those that lie exactly on a vertex."""
    from oracle import pyoracle
    rays = pixel_centre_rays(sd)
    d = rays[0, 3:]
    assert np.all(rays[:, 3:] == d[None, :])
    axis = int(np.argmax(np.abs(d)))
    keep = [a for a in range(3) if a != axis]
    tris = pyoracle.OracleScene(sd).world_vertices().astype(np.float64)
    n = np.cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0])
    planes = set()
    for k in np.flatnonzero(n @ d == 0.0):
        a = int(np.argmax(np.abs(n[k])))
        planes.add((a, float(tris[k, 0, a])))  # (axis-aligned scene: a plane is its axis and offset)
    edges = {}
    for k, t in enumerate(tris):
        if n[k] @ d == 0.0:
            continue  # seen edge-on: no area under the film
        for i in range(3):
            key = tuple(sorted((tuple(t[i]), tuple(t[(i + 1) % 3]))))
            edges[key] = edges.get(key, 0) + 1
    c = rays[:, :3][:, keep]
    on_edge, on_vertex = np.zeros(len(c), bool), np.zeros(len(c), bool)
    for (p, q), count in edges.items():
        if count < 2:
            continue
        p2, q2 = np.array(p)[keep], np.array(q)[keep]
        e, r = q2 - p2, c - p2[None, :]
        cross = e[0] * r[:, 1] - e[1] * r[:, 0]
        along = r @ e
        on_edge |= (cross == 0.0) & (along >= 0.0) & (along <= e @ e)
        on_vertex |= np.all(c == p2[None, :], axis=1) | np.all(c == q2[None, :], axis=1)
    return d, len(planes), on_edge, on_vertex, c


def leaf_bounds_under_pixel_centres(sd, opts):
    """the number of (leaf, axis, side) whose bound -- the extreme vertex coordinate of the leaf's triangles along an axis of the film -- equals the
    coordinate of a column or row of pixel centres: those rays start, and stay, exactly on a slab plane of that leaf"""
    from tests import bvh_model as bm
    with capi.options(**opts):
        scene = capi.Scene(None, sd)
    assert scene.info().uses_bvh == 1
    nodes = scene.array(capi.ARRAY_BVH_NODES, np.uint32)
    woop = scene.array(capi.ARRAY_WOOP, F).reshape(-1, 16)[: scene.info().n_triangles]
    world = bm._world_vertices(scene.array(capi.ARRAY_SHADE, F).reshape(-1, 32), scene.array(capi.ARRAY_INSTANCES, F).reshape(-1, 32))
    gid = woop[:, 12].view(np.uint32)
    leaves = {}
    for k, path in bm.decode_tree(nodes).items():
        leaves.setdefault(path[-1], []).append(world[gid[k]])
    d, _, _, _, c = aligned_facts(sd)
    axis = int(np.argmax(np.abs(d)))
    keep = [a for a in range(3) if a != axis]
    found = 0
    for tris in leaves.values():
        v = np.concatenate(tris).reshape(-1, 3)
        for j, a in enumerate(keep):
            for bound in (v[:, a].min(), v[:, a].max()):
                found += int(np.any(c[:, j] == bound))
    return found, len(leaves)


def aligned_visit_bound(sd, opts, eps=1e-5):
    """An upper bound, from geometry alone, on the node visits of the aligned scene's primary rays through a flattened tree: a ray along an axis can
    only reach a node if its line lies inside the box of every entry on the way down, in the two axes across the ray (closed intervals, widened by
    `eps` for the rounding of the slab test's products at 1e20; the boxes are the quantised, padded ones the device reads). Culling by the hit found
    so far and by the axis along the ray only lowers the count. Returns (bound, number of nodes, number of rays)."""
    from tests import bvh_model as bm
    with capi.options(**opts):
        scene = capi.Scene(None, sd)
    assert scene.info().uses_bvh == 1
    nodes = scene.array(capi.ARRAY_BVH_NODES, np.uint32).reshape(-1, bm.NODE_WORDS)
    d, _, _, _, c = aligned_facts(sd)
    keep = [a for a in range(3) if a != int(np.argmax(np.abs(d)))]
    total, seen, stack = 0, 0, [(0, np.ones(len(c), bool))]
    while stack:
        idx, reach = stack.pop()
        total += int(reach.sum())
        seen += 1
        n = nodes[idx]
        child_base = int(n[3] >> 24) | (int(n[4] & 0xffff) << 8)
        for e in range(6):
            meta = int((n[5] >> (8 * e)) & 0xff) if e < 4 else int((n[4] >> (16 + 8 * (e - 4))) & 0xff)
            if meta == 0 or not ((meta >> 5) == 1 and (meta & 0x1f) >= 24):
                continue  # empty, or a leaf entry: its triangles are tested inside this node's visit
            origin, scale, qlo, qhi = (v[0].astype(np.float64) for v in bm.entry_box_params(nodes, 0, [(idx, e)]))
            lo, hi = origin + qlo * scale, origin + qhi * scale
            inside = np.ones(len(c), bool)
            for j, a in enumerate(keep):
                inside &= (c[:, j] >= lo[a] - eps) & (c[:, j] <= hi[a] + eps)
            stack.append((child_base + (meta & 0x1f) - 24, reach & inside))
    return total, seen, len(c)
