"""The light tree on the GPU (csrc/device/dlighttree.h, the PUNCT kernels): the device probe against the numpy restatement bit for bit,
16 x 16 films against the closed form with the model's probabilities (every one-sample pixel is f_i / p_i of some light, the 256-sample mean passes
the z-test, the squared error is below mode 0's), the tree beside a sun, an emitter and an environment, behind a blocker, with soft lights, through
a lens, sharded, adaptive, past the LDS budget of mode 0, and through akari-cli."""
import json
import math
import subprocess

import numpy as np
import pytest

from akari_render_amd import abi, capi
from tests import light_tree_model as lt
from tests.helpers import make_config, n_bit_diff, resolve_np
from tests.test_environment import quad_scene
from tests.test_gpu_punctual import RHO, centre_cfg, closed_form, device_points, pixel_points, render
from tests.test_light_tree import (HOOK_SCENES, assert_rows_equal, edge_rows, grid_contributions, grid_lights, local_lights, make_scene, model_of, threshold_rows)
from tests.test_punctual import json_light, light_table, point, sun, write_scene_with_lights
from tests.test_soft_lights import random_rows9

pytestmark = pytest.mark.gpu

F = np.float32
PUNCT_BIT, TREE_BIT = 128, 256


def grid_scene(ctx, mode=1, **kw):
    return make_scene(grid_lights(), mode=mode, ctx=ctx, width=16, height=16, albedo=RHO, **kw)


def grid_model(ctx, sc, sd, points=None):
    """f_i (float64, from the closed form at the kernels' own float32 points) and p_i (the model's walk at those points) of every pixel: (256, 16) each"""
    p32 = (device_points(ctx, sc) if points is None else points).reshape(-1, 3)
    records, weights, words, entries = model_of(sc, sd)
    p, _ = lt.record_pdfs(words, records, p32)
    return grid_contributions(sc.punctual_lights(), p32.astype(np.float64), RHO), p.astype(np.float64)


def z_test(mean, f, p, n, what):
    """test_selection_between_two_lights' test: |z| < 6 per pixel and the pooled mean of z within 5 / sqrt(N), the variance from the model's p_i"""
    total = f.sum(axis=1)
    var = ((f ** 2 / p).sum(axis=1) - total ** 2) / n
    z = (mean.reshape(-1) - total) / np.sqrt(var)
    print(f"{what}: max |z| = {np.abs(z).max():.2f}, pooled mean of z = {z.mean():.3f} (allowed {5 / math.sqrt(z.size):.3f})")
    assert np.all(np.abs(z) < 6)
    assert abs(z.mean()) < 5 / math.sqrt(z.size)


def one_of(img, f, p, rtol=1e-5):
    """which light every pixel's one-sample value f_i / p_i belongs to (-1: none), img (h, w) float64"""
    want = f / p
    hit = np.isclose(img.reshape(-1, 1), want, rtol=rtol, atol=0)
    return np.where(hit.any(axis=1), hit.argmax(axis=1), -1)


# ---------------------------------------------------------------------------------------------------------------- probe
@pytest.mark.parametrize("name", ["five_mixed", "large_257", "mixed_33", "one_point_4", "two"])
def test_probe_equals_the_model_bit_for_bit(ctx, name):
    n, arrangement, mixed = HOOK_SCENES[name]
    lights = local_lights(n, 7 + n, arrangement)
    if mixed:
        lights = [sun()] + lights
    sc, sd = make_scene(lights, ctx=ctx, mixed=mixed)
    records, weights, words, entries = model_of(sc, sd)
    rows = np.concatenate([random_rows9(4096, 3 + n), edge_rows(words, records, n)])
    if not mixed:
        rows = np.concatenate([rows, threshold_rows(sc, records, words, entries, rows[:48])])
    got = sc.probe_light_tree_sample(rows)
    want, _ = lt.light_sample_rows(light_table(sc), entries, records, words, rows)
    assert_rows_equal(got, want)
    assert_rows_equal(got, sc.host_light_tree_sample(rows))


# ---------------------------------------------------------------------------------------------------------------- films against the closed form
@pytest.mark.parametrize("force_bvh", [0, 1], ids=["exhaustive", "bvh"])
def test_one_sample_is_one_light_over_its_probability(ctx, force_bvh):
    with capi.options(force_bvh=force_bvh):
        sc, sd = grid_scene(ctx)
    assert sc.info().uses_bvh == force_bvh and sc.info().n_lights == 1 and sc.light_tree() == (1, 31)
    f, p = grid_model(ctx, sc, sd)
    film = capi.Film(ctx, 16, 16)
    se = capi.PtSession(ctx, sc, centre_cfg(spp=1, sampler_seed=3), film)
    se.passes(1, blocking=True)
    flags = se.kernel_info()["kernel_flags"]
    try:
        with pytest.raises(capi.AkariError) as e:  # the setter, while a session holds the scene
            sc.set_light_tree(False)
    finally:
        se.end()
    assert e.value.code == capi.ERR_INVALID_ARGUMENT and sc.light_tree() == (1, 31)
    assert flags & (PUNCT_BIT | TREE_BIT) == PUNCT_BIT | TREE_BIT
    img = resolve_np(film.read(), 16, 16)
    assert np.all(img[..., 0] == img[..., 1]) and np.all(img[..., 0] == img[..., 2])  # white lights, grey quad
    which = one_of(img[..., 0].astype(np.float64), f, p)
    assert np.all(which >= 0), f"{int((which < 0).sum())} pixels are no light's f / p"
    assert len(set(which)) >= 4


def test_mean_passes_the_z_test_and_beats_mode_0(ctx):
    """256 samples: the z-test with the model's variance. Then the same scene, seed and 16 samples under both modes: the film's summed squared error against the
    closed form is smaller with the tree (tests/test_light_tree.py test_variance_in_the_model, seen on films)."""
    sc, sd = grid_scene(ctx)
    f, p = grid_model(ctx, sc, sd)
    mean = render(ctx, sc, centre_cfg(spp=256, sampler_seed=7))[..., 0].astype(np.float64)
    z_test(mean, f, p, 256, "light tree, 4 x 4 grid")
    off, _ = grid_scene(ctx, mode=0)
    assert off.info().n_lights == 16
    se2 = []
    for s in (sc, off):
        film = capi.Film(ctx, 16, 16)
        session = capi.PtSession(ctx, s, centre_cfg(spp=16, sampler_seed=11), film)
        session.passes(1, blocking=True)
        assert bool(session.kernel_info()["kernel_flags"] & TREE_BIT) == (s is sc)
        session.end()
        se2.append(float(np.sum((resolve_np(film.read(), 16, 16)[..., 0].astype(np.float64).reshape(-1) - f.sum(axis=1)) ** 2)))
    print(f"summed squared error at 16 spp: with the tree {se2[0]:.4g}, by power alone {se2[1]:.4g}")
    assert se2[0] < se2[1]


# ---------------------------------------------------------------------------------------------------------------- composition
def test_linearity_beside_a_sun_an_emitter_and_an_environment(ctx):
    """{sun, emitter, constant environment, the tree} = {sun, emitter, environment} + the sum of the grid's closed forms, at depth 1 (the ENV unit), within 5
    standard errors per pixel and channel. test_gpu_punctual's construction with the tree in the place of its one light: per sample the scene without
    the grid gives X (mean mu, variance n V: 16 seeds); the lit scene chooses the tree with probability p and returns T / p, T the tree's own estimator
    (mean L, second moment M = sum f_i^2 / p_i), else X / (1 - p). So Var(lit render) = ((n V + mu^2) / (1 - p) + M / p - (mu + L)^2) / n, and V / 16 for
    the mean of the seeds it is compared with."""
    n = 256

    def scene(with_grid):
        sd = quad_scene(width=16, height=16, albedo=RHO, emissive=True)
        sd.meshes[1].vertices = (np.asarray(sd.meshes[1].vertices) * np.float32([1, 1, -1]) + np.float32([0.3, 0.3, 0.0])).astype(np.float32)
        sd.environment = abi.EnvironmentData(color=(0.3, 0.4, 0.5))
        sd.lights = [sun(direction=(0.3, -0.2, -1.0), strength=0.2)] + (grid_lights() if with_grid else [])
        with capi.options(light_tree=1):
            return capi.Scene(ctx, sd), sd

    def cfg(seed):
        return make_config(spp=n, max_depth=1, filter_type=abi.FILTER_BOX, filter_radius=0.0, sampler_type=abi.SAMPLER_SOBOL, sampler_seed=seed)

    (bare, _), (lit, sd) = scene(False), scene(True)
    assert [lit.light(i)[0] for i in range(4)] == [bare.light(0)[0], capi.PUNCTUAL_LIGHT_INSTANCE, capi.LIGHT_TREE_INSTANCE, capi.ENV_LIGHT_INSTANCE]
    p = float(np.float32(lit.light(2)[2]))
    assert 0.1 < p < 0.9
    seeds = np.stack([render(ctx, bare, cfg(100 + s)).astype(np.float64) for s in range(16)])
    mu, V = seeds.mean(axis=0), seeds.var(axis=0, ddof=1)
    at_emitter = pixel_points(bare, 0.5)
    floor = (np.abs(at_emitter[..., 0] - 0.3) > 0.35) | (np.abs(at_emitter[..., 1] - 0.3) > 0.35)  # pixels that see the floor, not the emitter's back
    x = pixel_points(bare)
    records, weights, words, entries = model_of(lit, sd)
    q, _ = lt.record_pdfs(words, records, x.reshape(-1, 3).astype(F))
    local = [k for k, r in enumerate(records) if lt.is_local(r)]
    f = grid_contributions(grid_lights(), x.reshape(-1, 3), RHO)
    L = f.sum(axis=1).reshape(16, 16, 1)
    M = (f ** 2 / q[:, local].astype(np.float64)).sum(axis=1).reshape(16, 16, 1)
    got = render(ctx, lit, cfg(116)).astype(np.float64)
    se = np.sqrt(np.maximum(((n * V + mu ** 2) / (1 - p) + M / p - (mu + L) ** 2) / n, 0.0) + V / 16)
    excess = np.abs(got - (mu + L))[floor] / se[floor]
    print(f"linearity: the tree's selection probability {p:.3f}; worst |difference| / standard error = {excess.max():.2f}, median {np.median(excess):.2f} over "
          f"{int(floor.sum())} pixels x 3; values where the grid alone is > 10 standard errors: {int(np.sum(np.broadcast_to(L, se.shape)[floor] > 10 * se[floor]))}")
    assert floor.sum() > 150 and np.all(se[floor] > 0)
    assert np.all(excess <= 5.0)
    assert np.sum(np.broadcast_to(L, se.shape)[floor] > 10 * se[floor]) > 100  # the grid is far above the allowance: leaving it out would fail


def test_hard_shadow(ctx):
    """four lights at ONE point, in a tree: behind a blocker the umbra is exactly black and the lit part bit for bit the open scene's"""
    lights = [point(position=(0.0, 0.0, 1.8), color=(1, 1, 1), strength=s) for s in (5.0, 1.0, 2.0, 0.5)]
    sd = quad_scene(width=16, height=16, albedo=RHO)
    with capi.options(light_tree=1):
        open_scene = capi.Scene(ctx, abi.SceneData(sd.meshes, sd.instances, sd.materials, sd.camera, lights=lights))
    # a blocker at z = 1.5 covering |x|, |y| <= 0.1: from the lights at z = 1.8 its umbra on the floor is |x|, |y| <= 0.6; the camera at z = 3 sees it in front of
    # the floor's |x|, |y| <= 0.2
    bv = np.array([[-0.1, -0.1, 1.5], [0.1, -0.1, 1.5], [0.1, 0.1, 1.5], [-0.1, 0.1, 1.5]], np.float32)
    sd.meshes.append(abi.MeshData(vertices=bv, indices=np.array([[0, 1, 2], [0, 2, 3]], np.uint32)))
    sd.materials.append(abi.MaterialData(kind=abi.MAT_DIFFUSE, base_color=(0.0, 0.0, 0.0)))
    sd.instances.append(abi.InstanceData(1, [1], np.eye(4, dtype=np.float32).reshape(16).copy()))
    sd.lights = lights
    with capi.options(light_tree=1):
        blocked = capi.Scene(ctx, sd)
    assert open_scene.light_tree() == blocked.light_tree() == (1, 7)
    a, b = render(ctx, open_scene, centre_cfg()), render(ctx, blocked, centre_cfg())
    x = pixel_points(open_scene)
    clear = 0.02  # every ray goes through its pixel's centre (a box filter of radius 0): pixels whose centre ray passes this close to an edge are left out
    sees_blocker = np.all(np.abs(pixel_points(open_scene, 1.5)[..., :2]) <= 0.1 + clear, axis=-1)
    cheb = np.max(np.abs(x[..., :2]), axis=-1)
    umbra, lit = (cheb < 0.6 - clear) & ~sees_blocker, cheb > 0.6 + clear
    assert umbra.sum() >= 8 and lit.sum() > 60
    assert np.all(b[umbra] == 0)
    assert n_bit_diff(a[lit], b[lit]) == 0
    assert np.all(a[lit] > 0)


def test_soft_lights_in_the_tree(ctx):
    """Four soft lights. A one-sample film of the tree's scene draws u_select and u_sample where the film of a scene with ONE of the lights draws them, so every pixel
    is that light's own pixel over the probability the model gives the light there."""
    rng = np.random.default_rng(3)
    lights = [abi.PunctualLightData(abi.LIGHT_POINT, position=(float(F(x)), float(F(y)), 0.5), color=(1.0, 1.0, 1.0), strength=0.3, radius=float(F(rng.uniform(0.05, 0.2))))
              for x, y in ((-0.5, -0.5), (0.5, -0.4), (-0.4, 0.5), (0.45, 0.5))]
    sc, sd = make_scene(lights, ctx=ctx, width=16, height=16, albedo=RHO)
    records, weights, words, entries = model_of(sc, sd)
    p, _ = lt.record_pdfs(words, records, device_points(ctx, sc).reshape(-1, 3))
    cfg = centre_cfg(spp=1, sampler_seed=5)
    tree = render(ctx, sc, cfg)[..., 0].astype(np.float64).reshape(-1)
    alone = np.stack([render(ctx, make_scene([l], ctx=ctx, width=16, height=16, albedo=RHO)[0], cfg)[..., 0].astype(np.float64).reshape(-1) for l in lights], axis=1)
    assert np.all(alone > 0)
    which = one_of(tree, alone, p.astype(np.float64))
    assert np.all(which >= 0) and len(set(which)) == 4
    # and the radius matters: the delta lights at the same places give other pixels
    hard = [abi.PunctualLightData(abi.LIGHT_POINT, position=l.position, color=l.color, strength=l.strength) for l in lights]
    assert not np.allclose(render(ctx, make_scene(hard, ctx=ctx, width=16, height=16, albedo=RHO)[0], cfg)[..., 0].reshape(-1), tree, rtol=1e-4)


def test_through_a_lens(ctx):
    """the LENS unit: a lens focused on the quad leaves the diffuse closed form where it is; every one-sample pixel is some light's f / p at the pixel centre's point.
    rtol 1e-4 here: the lens ray meets the quad within a few ulp of the pinhole's point, and 0.25 below a light that moves p_i and f_i by a few 1e-6 each."""
    sd = quad_scene(width=16, height=16, albedo=RHO)
    sd.lights, sd.lens = grid_lights(), abi.LensData(0.05, 3.0)
    with capi.options(light_tree=1):
        sc = capi.Scene(ctx, sd)
    pinhole, psd = grid_scene(ctx)
    f, p = grid_model(ctx, pinhole, psd)
    film = capi.Film(ctx, 16, 16)
    se = capi.PtSession(ctx, sc, centre_cfg(spp=1, sampler_seed=2), film)
    se.passes(1, blocking=True)
    assert se.kernel_info()["kernel_flags"] & (PUNCT_BIT | TREE_BIT | 32) == PUNCT_BIT | TREE_BIT | 32
    se.end()
    which = one_of(resolve_np(film.read(), 16, 16)[..., 0].astype(np.float64), f, p, rtol=1e-4)
    assert np.all(which >= 0) and len(set(which)) >= 4


def test_through_a_lens_beside_an_environment(ctx):
    """the LENS + ENV unit: the tree's scene against mode 0's (the behaviour before the tree), 16 seeds of 256 samples each way: the two means agree within 6 standard
    errors of their difference per pixel and channel, the errors taken from the seeds' spread"""
    def scene(mode):
        sd = quad_scene(width=16, height=16, albedo=RHO)
        sd.lights, sd.lens, sd.environment = grid_lights(), abi.LensData(0.05, 3.0), abi.EnvironmentData(color=(0.02, 0.03, 0.04))
        with capi.options(light_tree=mode):
            return capi.Scene(ctx, sd)

    films = []
    for mode in (1, 0):
        sc = scene(mode)
        assert sc.info().n_lights == (2 if mode else 17)
        if mode:
            se = capi.PtSession(ctx, sc, centre_cfg(spp=1), capi.Film(ctx, 16, 16))
            se.passes(1, blocking=True)
            assert se.kernel_info()["kernel_flags"] & (PUNCT_BIT | TREE_BIT | 32) == PUNCT_BIT | TREE_BIT | 32
            se.end()
        films.append(np.stack([render(ctx, sc, centre_cfg(spp=256, sampler_seed=40 + s)).astype(np.float64) for s in range(16)]))
    m1, m0 = films[0].mean(axis=0), films[1].mean(axis=0)
    se = np.sqrt(films[0].var(axis=0, ddof=1) / 16 + films[1].var(axis=0, ddof=1) / 16)
    z = (m1 - m0) / se
    print(f"lens + environment: max |z| = {np.abs(z).max():.2f}, pooled mean of z = {z.mean():.3f}; variance ratio mode 0 / tree = {films[1].var(axis=0).sum() / films[0].var(axis=0).sum():.2f}")
    assert np.all(np.abs(z) < 6) and abs(z.mean()) < 5 / math.sqrt(z.size)
    assert films[0].var(axis=0).sum() < films[1].var(axis=0).sum()


# ---------------------------------------------------------------------------------------------------------------- sharding, sample ranges, adaptive
def test_shards_and_sample_ranges_assemble_to_the_whole_film(ctx):
    sc, _ = make_scene(local_lights(9, 12), ctx=ctx, width=32, height=32, albedo=RHO)
    base = dict(spp=8, spp_per_pass=4, max_depth=3, sampler_seed=9, tile_w=16, tile_h=16, sampler_type=abi.SAMPLER_SOBOL)
    whole = capi.Film(ctx, 32, 32)
    capi.pt_render(ctx, sc, make_config(**base), whole)
    assert np.count_nonzero(whole.read()) > 0
    parts = np.zeros_like(whole.read())
    for rank in range(2):
        f = capi.Film(ctx, 32, 32)
        capi.pt_render(ctx, sc, make_config(shard_rank=rank, shard_count=2, **base), f)
        part = f.read()
        assert np.count_nonzero(part) > 0 and np.count_nonzero(parts[part != 0]) == 0
        parts += part
    assert n_bit_diff(parts, whole.read()) == 0
    ranged = capi.Film(ctx, 32, 32)  # two sample ranges into one film
    for begin in (0, 4):
        capi.pt_render(ctx, sc, make_config(sample_begin=begin, sample_count=4, **base), ranged)
    assert n_bit_diff(ranged.read(), whole.read()) == 0


def test_adaptive_render_runs(ctx):
    sc, _ = make_scene(local_lights(9, 12), ctx=ctx, width=32, height=32, albedo=RHO)
    film = capi.Film(ctx, 32, 32)
    stats, tile_spp = capi.pt_adaptive_render(ctx, sc, make_config(spp=32, spp_per_pass=4, max_depth=2, sampler_seed=4, tile_w=16, tile_h=16), film)
    img = resolve_np(film.read(), 32, 32)
    assert np.all(np.isfinite(img)) and img.max() > 0 and tile_spp is not None and tile_spp.min() >= 1


# ---------------------------------------------------------------------------------------------------------------- LDS budget
def test_a_light_count_refused_in_mode_0_renders_with_the_tree(ctx):
    rng = np.random.default_rng(8)
    lights = [abi.PunctualLightData(abi.LIGHT_POINT, position=(float(F(x)), float(F(y)), 0.25), color=(1.0, 1.0, 1.0), strength=0.002)
              for x, y in rng.uniform(-0.9, 0.9, (1200, 2))]
    off, _ = make_scene([], mode=0, ctx=ctx, width=16, height=16, albedo=RHO)
    n_ok = 0
    with pytest.raises(capi.AkariError) as e:
        for l in lights:
            off.add_punctual_light(l)
            n_ok += 1
    assert e.value.code == capi.ERR_UNSUPPORTED and "LDS budget" in str(e.value)
    lights = lights[:n_ok + 1]  # one more than mode 0 takes
    sc, sd = make_scene(lights, ctx=ctx, width=16, height=16, albedo=RHO)
    assert sc.info().uses_bvh == 0 and sc.info().n_lights == 1 and sc.light_tree() == (1, 2 * len(lights) - 1)
    p32 = device_points(ctx, sc).reshape(-1, 3)
    records, weights, words, entries = model_of(sc, sd)
    p, _ = lt.record_pdfs(words, records, p32)
    f = grid_contributions(lights, p32.astype(np.float64), RHO)
    mean = render(ctx, sc, centre_cfg(spp=256, sampler_seed=13))[..., 0].astype(np.float64)
    z_test(mean, f, p.astype(np.float64), 256, f"{len(lights)} lights past mode 0's LDS budget")


# ---------------------------------------------------------------------------------------------------------------- akari-cli
def test_cli(ctx, tmp_path):
    from akari_render_amd import build
    cli = build.build_cli()
    spath = write_scene_with_lights(tmp_path, {"l%02d" % k: json_light(l) for k, l in enumerate(grid_lights())})
    method = {"method": {"type": "pt", "spp": 4, "spp_per_pass": 4, "max_depth": 2}, "sampler": {"type": "independent", "seed": 1}, "film": {"out": str(tmp_path / "out.exr")}}
    mpath = tmp_path / "pt.json"
    mpath.write_text(json.dumps(method))

    def api_bytes(name, **opts):
        with capi.options(**opts):
            sc = capi.Scene(ctx, spath)
        film = capi.Film(ctx, 16, 16)
        cfg, _ = capi.config_from_json(json.dumps(method))
        capi.pt_render(ctx, sc, cfg, film)
        capi.image_write(str(tmp_path / name), film.resolve().reshape(16, 16, 3))
        return sc.light_tree(), open(tmp_path / name, "rb").read()

    res = subprocess.run([cli, "-s", spath, "-m", str(mpath), "--light-tree"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    with_tree = open(tmp_path / "out.exr", "rb").read()
    mode, want = api_bytes("api_tree.exr", light_tree=1)
    assert mode == (1, 31) and with_tree == want
    res = subprocess.run([cli, "-s", spath, "-m", str(mpath)], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    mode, want = api_bytes("api_plain.exr")
    assert mode == (0, 0) and open(tmp_path / "out.exr", "rb").read() == want and want != with_tree
