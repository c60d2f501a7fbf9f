"""The conditions that keep tests/test_gpu_projection_parity.py from passing emptily, checked without a GPU: for every case of
tests/projection_parity_cases.py the library's host plan must name the LENS variant the case is there for, the film is finite and small, and the
oracle alone must show that the projection changes at least a quarter of the film's floats (the share the punctual-light and lens cases use).
For the aligned cases, in float64 on their dyadic coordinates, where the arithmetic is exact: every primary direction has two components that
are exactly 0, at least four scene planes are parallel to it, at least 8 pixel centres lie exactly on an edge two triangles share and at least 2
on a vertex, and on the BVH route a column or row of pixel centres runs exactly along a leaf's bound. For the panorama room: depth-0 rays in all
eight octants, film points beyond the film's edges, and pole rows whose cos(latitude) is below 1e-6."""
import numpy as np
import pytest

from akari_render_amd import abi, capi
from oracle import pyoracle
from tests import camera_model as cm
from tests import projection_parity_cases as J
from tests import punct_parity_cases as P
from tests.helpers import make_config, n_bit_diff

F = np.float32


def _fraction(a, b):
    return n_bit_diff(a, b) / a.size


def _plan(case, sd, cfg):
    if "feat" in case.tags:
        with capi.options(**case.opts):
            return capi.Scene(None, sd).features_plan(cfg, feat=True)
    return P.host_plan(sd, cfg, case.opts)


@pytest.mark.parametrize("name", list(J.CASES))
def test_case_is_what_it_claims(hip_lib, name):
    case = J.CASES[name]
    sd, cfg = case.scene(), case.config()
    w, h = sd.camera.width, sd.camera.height
    assert max(w, h) <= 32 and cfg.spp <= 16
    assert sd.projection is not None and sd.projection.type != abi.PROJECTION_PERSPECTIVE
    plan = _plan(case, sd, cfg)
    v = plan["variant"]
    assert case.want["lens"] == 1 and {k: v[k] for k in case.want} == case.want, (v, case.want)
    if "feat" in case.tags:
        assert v["feat"] == 1
    kw = dict(light_tree=True) if "ltree" in case.tags else {}
    if "ltree" in case.tags:
        with capi.options(**case.opts):
            assert capi.Scene(None, sd).light_tree()[1] > 0
    film, st, _ = J.oracle_render(sd, cfg, **kw)
    assert np.all(np.isfinite(film)) and np.any(film[:3 * w * h] != 0)
    pin, _, _ = J.oracle_render(sd, cfg, projection=False, **kw)
    assert _fraction(film, pin) >= 0.25, f"the projection changes {_fraction(film, pin):.3f} of the film's floats"
    if case.want["punct"]:
        assert sd.lights and st["n_shadow"] > 0 and _fraction(film, J.oracle_render(sd, cfg, lights=False, **kw)[0]) >= 0.25
    if sd.lens is not None:
        # The orthographic lens moves a sample's hit point and turns its direction by a little. Under an emitter every lit point's radiance depends
        # on where it is: a quarter of the film, as for the perspective lens. A flat diffuse surface under the environment alone looks the same from
        # every nearby point, so there the lens shows only at silhouettes and on the box.
        changed = _fraction(film, J.oracle_render(sd, cfg, lens=False, **kw)[0])
        assert changed >= 0.25 if name.endswith("-emitter") else changed > 0.0, changed


def test_the_table_names_every_lens_unit(hip_lib):
    """kernels.h PtKind x ENV for LENS = 1, flattened scenes: plain, punct, punct_tree, feat -- each under both projections"""
    seen = set()
    for name in J.UNIT_CASES:
        case = J.CASES[name]
        kind = [t[5:] for t in case.tags if t.startswith("kind:")][0]
        assert case.want["lens"] == 1 and case.want["punct"] == int(kind.startswith("punct")) and ("ltree" in case.tags) == (kind == "punct_tree") and ("feat" in case.tags) == (kind == "feat")
        seen.add((kind, case.want["env"], case.scene().projection.type))
    assert len(J.UNIT_CASES) == len(seen) == 16
    assert seen == {(k, e, p) for k in ("plain", "punct", "punct_tree", "feat") for e in (0, 1) for p in (J.ORTHO, J.PANORAMA)}  # (the panorama of these cases is a window on the floor and the box)
    # ... and the kept scenes' unit (PT_KIND_INST) is among the aligned cases, as are both schedules of it
    routes = {t[6:] for n in J.ALIGNED_CASES for t in J.CASES[n].tags if t.startswith("route:")}
    assert routes == set(J.ALIGNED_ROUTES) and all(J.CASES[n].want["inst"] == int("kept" in n) for n in J.ALIGNED_CASES)
    assert len(J.MATERIAL_CASES) == 64 and len(J.ALIGNED_CASES) == 20


@pytest.mark.parametrize("turned", [False, True], ids=["identity", "turned"])
def test_aligned_scene(hip_lib, turned):
    sd = J.aligned_room("diffuse", turned)
    c2w = np.asarray(sd.camera.c2w, F)
    assert set(np.unique(c2w)) <= {F(-1), F(0), F(1)}  # (the quarter turn's entries are exactly 0 / +-1)
    d, n_planes, on_edge, on_vertex, c = J.aligned_facts(sd)
    assert sorted(np.abs(d)) == [0.0, 0.0, 1.0] and (d == ((-1, 0, 0) if turned else (0, 0, -1))).all()
    assert n_planes >= 4, n_planes
    assert on_edge.sum() >= 8 and on_vertex.sum() >= 2, (on_edge.sum(), on_vertex.sum())
    assert np.all(np.mod(c * 16.0, 2.0) == 1.0)  # pixel centres on the odd multiples of 1/16: the lattice the cube A's vertices lie on
    # the default filter's rays are aligned as well (an offset moves the origin, not the direction)
    rng = np.random.default_rng(1)
    pixels = rng.integers(0, 32, (256, 2)).astype(np.uint32)
    u = rng.random((256, 2), dtype=F)
    cfg = make_config()
    rays = pyoracle.OracleScene(sd).lens_ray_many(pixels, u, u, cfg.filter_type, cfg.filter_radius)
    assert np.all(rays[:, 3:] == d.astype(F)[None, :])
    found, n_leaves = J.leaf_bounds_under_pixel_centres(sd, J.BVH)
    assert n_leaves >= 4 and found >= 1, (found, n_leaves)
    for route, (opts, want) in J.ALIGNED_ROUTES.items():
        with capi.options(**opts):
            info = capi.Scene(None, sd).info()
        assert info.uses_bvh == (2 if want.get("inst") else int(bool(opts["force_bvh"]))), route


@pytest.mark.parametrize("name", [n for n in J.PANORAMA_CASES if "octants" in J.CASES[n].tags])
def test_panorama_room_is_seen_in_all_eight_octants(hip_lib, name):
    case = J.CASES[name]
    sd, cfg = case.scene(), case.config()
    w, h = sd.camera.width, sd.camera.height
    osc = pyoracle.OracleScene(sd)
    rays = J.pixel_centre_rays(sd)
    m = np.asarray(sd.camera.c2w, np.float64).reshape(4, 4).T[:3, :3]
    local = rays[:, 3:] @ m  # camera-space directions
    octants = {tuple(s) for s in (local > 0).astype(int)}
    assert len(octants) == 8
    hit, _ = osc.intersect_many(np.concatenate([rays, np.zeros((len(rays), 1)), np.full((len(rays), 1), 1e20)], axis=1).astype(F))
    assert np.all(hit[:, 0] == 1)  # a closed room: every depth-0 ray hits a surface
    # the pole rows: cos(latitude) of a film point the Gaussian filter carries to the film's edge and past it
    assert cfg.filter_type == abi.FILTER_GAUSSIAN and cfg.filter_radius == 1.5
    rng = np.random.default_rng(2)
    n = 4096
    pixels = np.stack([rng.integers(0, w, n), rng.choice([0, h - 1], n)], axis=1).astype(np.uint32)
    pixels[: n // 2, 0] = rng.choice([0, w - 1], n // 2)
    u = rng.random((n, 2), dtype=F)
    pf = cm.film_point(pixels, u, cfg.filter_type, cfg.filter_radius).astype(np.float64)
    assert (pf[:, 0] < 0).any() and (pf[:, 0] > w).any() and (pf[:, 1] < 0).any() and (pf[:, 1] > h).any()  # offsets leave the film at the seam and at the poles
    got = osc.lens_ray_many(pixels, u, u, cfg.filter_type, cfg.filter_radius)
    assert np.all(np.isfinite(got))
    lat = np.pi / 2 - pf[:, 1] / h * np.pi
    assert np.abs(np.cos(lat)).min() < 1e-3


def test_narrow_window():
    case = J.CASES["pano-narrow-32x16"]
    p = case.scene().projection
    assert F(p.longitude_max) - F(p.longitude_min) == F(2.0 ** -6)


@pytest.mark.parametrize("name", list(J.EXTRA))
def test_scenes_outside_the_table(hip_lib, name):
    scene, kw = J.EXTRA[name]
    sd, cfg = scene(), make_config(**kw)
    assert max(sd.camera.width, sd.camera.height) <= 32 and cfg.spp <= 16
    with capi.options(**P.BVH):
        assert capi.Scene(None, sd).launch_plan(cfg)["variant"]["lens"] == 1  # (the trees' padding takes the orthographic film)
    film = J.oracle_render(sd, cfg)[0]
    assert np.all(np.isfinite(film)) and _fraction(film, J.oracle_render(sd, cfg, projection=False)[0]) >= 0.25


@pytest.mark.parametrize("which", list(J.AOV_SCENES))
def test_aov_scenes(hip_lib, which):
    sd = J.AOV_SCENES[which]()
    a = abi.AovConfig.default()
    a.spp, a.aov, a.remap, a.sampler_seed = 8, abi.AOV_ALBEDO, 0, 2
    o = pyoracle.OracleScene(sd).aov_render(a)[0]
    assert _fraction(o, pyoracle.OracleScene(sd, projection=False).aov_render(a)[0]) >= 0.25
    with capi.options(**P.BVH):
        assert capi.Scene(None, sd).projection() == sd.projection


@pytest.mark.parametrize("camera_type", ["orthographic", "panorama"])
def test_reader_scene(hip_lib, tmp_path, camera_type):
    """the file of the GPU test's reader case: both readers agree on it, and its projection (and the orthographic file's lens) reach the film"""
    from oracle import scene_json
    from tests.test_gpu_projection_parity import READER_CFG, projected_scene_file
    path = projected_scene_file(tmp_path, camera_type)
    sd = scene_json.load_scene(path, 32, 32, lens=True)
    with capi.options(lens=1, **P.EXH):
        there = capi.Scene(None, path, 32, 32)
        assert there.launch_plan(make_config(**READER_CFG))["variant"]["lens"] == 1
    assert sd.projection == there.projection() and sd.lens == there.lens() and sd.lights == there.punctual_lights()
    assert (sd.lens is not None) == (camera_type == "orthographic")
    cfg = make_config(**READER_CFG)
    o = J.oracle_render(sd, cfg)[0]
    assert _fraction(o, J.oracle_render(sd, cfg, projection=False)[0]) >= 0.25
    if sd.lens is not None:
        assert _fraction(o, J.oracle_render(sd, cfg, lens=False)[0]) >= 0.25


@pytest.mark.parametrize("turned", [False, True], ids=["identity", "turned"])
def test_aligned_visit_bound_can_fail(hip_lib, turned):
    """the geometric bound on node visits that the GPU test holds the aligned rays to is a real one: the tree has inner nodes, and the bound is well
    below what a traversal that ignored the two axes across the rays could visit (every node, for every ray)"""
    bound, n_nodes, n_rays = J.aligned_visit_bound(J.aligned_room("diffuse", turned), J.BVH)
    assert n_nodes >= 3 and n_rays == 32 * 32
    assert n_rays <= bound <= 0.75 * n_nodes * n_rays, (bound, n_nodes, n_rays)
