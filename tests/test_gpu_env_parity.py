"""The environment light on the GPU against the CPU oracle (oracle/or_env.h), bit for bit: the sampler and pdf probes on
adversarial inputs, and raw films plus ray counters over lighting, materials, configurations, samplers, colour pipelines and schedules,
and a scene.json read by both readers. Every case is small (<= 64 x 64, <= 16 spp)."""
import os

import numpy as np
import pytest

from akari_render_amd import abi, capi, distributed
from oracle import pyoracle, scene_json
from tests.helpers import instanced_scene, make_config, make_exr, n_bit_diff, resolve_np
from tests.test_environment import sample_image, scene_json_text
from tests.test_gpu_colorspace import PIPELINES
from tests.test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu

EXHAUSTIVE = dict(force_bvh=0, instancing=0, wavefront=0, specialise=0)


def _rot(ax, ay):
    cx, sx, cy, sy = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay)
    return (np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])).astype(np.float32)


def _quad(c, u, v):
    c, u, v = (np.asarray(a, np.float32) for a in (c, u, v))
    return abi.MeshData(vertices=np.array([c - u - v, c + u - v, c + u + v, c - u + v], np.float32), indices=np.array([[0, 1, 2], [0, 2, 3]], np.uint32))


def _box(c, h, ang):
    """a closed box (12 triangles, outward normals) turned by `ang` about +y"""
    R = _rot(0.0, ang)
    ex, ey, ez = R @ np.array([h, 0, 0], np.float32), R @ np.array([0, h, 0], np.float32), R @ np.array([0, 0, h], np.float32)
    c = np.asarray(c, np.float32)
    quads = [(c + ex, ez, ey), (c - ex, ey, ez), (c + ey, ex, -ez), (c - ey, ex, ez), (c + ez, ey, ex), (c - ez, ex, ey)]
    v, idx = [], []
    for k, (q, a, b) in enumerate(quads):
        m = _quad(q, a, b)
        v.append(m.vertices)
        idx.append(m.indices + 4 * k)
    return abi.MeshData(vertices=np.concatenate(v).astype(np.float32), indices=np.concatenate(idx).astype(np.uint32))


MATERIALS = {
    "diffuse": abi.MaterialData(kind=abi.MAT_DIFFUSE, base_color=(0.7, 0.6, 0.5)),
    "rough_metal": abi.MaterialData(kind=abi.MAT_PRINCIPLED, base_color=(0.9, 0.7, 0.5), metallic=1.0, roughness=0.35),
    "glass": abi.MaterialData(kind=abi.MAT_GLASS, base_color=(1.0, 1.0, 1.0), ior=1.5, roughness=0.2),
    "mirror": abi.MaterialData(kind=abi.MAT_PRINCIPLED, base_color=(0.95, 0.95, 0.95), metallic=1.0, roughness=0.0),
    "alpha": abi.MaterialData(kind=abi.MAT_DIFFUSE, base_color=(0.6, 0.7, 0.6), base_alpha=0.5),
}


def _sun_image(W=64, H=32):
    """a dim sky with two small suns of 3000 (above the clamp of 1000): one the camera sees directly, one it sees in a mirror floor"""
    img = np.zeros((H, W, 4), np.float32)
    img[:, :, 3] = 1
    img[:, :, :3] = np.linspace(0.05, 0.6, H, dtype=np.float32)[:, None, None] * np.float32([0.6, 0.7, 1.0])
    img[16:19, 15:18, :3] = 3000.0  # around (0, 0.1, -1): u = 0.25, v = 0.53
    img[21:24, 15:18, :3] = 3000.0  # around (0, 0.6, -0.8): what the floor reflects towards the camera
    return img


def env_scene(material="diffuse", emitters=0, env=None, floor="diffuse", w=32, h=32):
    """a floor, a closed box of `material`, `emitters` small emissive quads facing down, a camera looking down at the box with the sky in
    the upper rows; lit by `env` (default: a sampled image, linear, turned)"""
    meshes = [_quad((0, -1, 0), (4, 0, 0), (0, 0, -4)), _box((0, -0.4, 0), 0.6, 0.5)]
    mats = [MATERIALS[floor], MATERIALS[material]]
    for k in range(emitters):
        meshes.append(_quad((-1.5 + 1.5 * k, 1.6, -0.5), (0.3, 0, 0), (0, 0, 0.3)))  # normal -y
    if emitters:
        mats.append(abi.MaterialData(kind=abi.MAT_EMISSION, emission_color=(6.0, 5.0, 4.0), emission_strength=1.0))
    eye = np.eye(4, dtype=np.float32).reshape(16).copy()
    insts = [abi.InstanceData(i, [min(i, len(mats) - 1)], eye) for i in range(len(meshes))]
    e, t = np.array([0, 0.8, 4.0]), np.array([0, -0.4, 0.0])
    d = (t - e) / np.linalg.norm(t - e)
    right = np.cross(d, [0, 1, 0])
    right /= np.linalg.norm(right)
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = right, np.cross(right, d), -d, e
    cam = abi.CameraData(c2w=c2w.astype(np.float32).T.reshape(16).copy(), fov=0.9, width=w, height=h)
    sd = abi.SceneData(meshes, insts, mats, cam)
    sd.ggx_table = _ggx()
    sd.environment = env if env is not None else abi.EnvironmentData(image=sample_image(W=48, H=24, seed=4), strength=1.0, rotation=_rot(0.2, -0.7),
                                                                   filter=abi.TEX_FILTER_LINEAR)
    return sd


_GGX = None


def _ggx():
    global _GGX
    if _GGX is None:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        _GGX = np.fromfile(os.path.join(root, "tests", "golden", "ggx_dielectric_s.f32"), dtype=np.float32)
    return _GGX


def _render_gpu(ctx, sd, cfg):
    scene = capi.Scene(ctx, sd)
    film = capi.Film(ctx, sd.camera.width, sd.camera.height)
    st = capi.pt_render(ctx, scene, cfg, film)
    return film.read(), st


def _check(ctx, sd, cfg, opts=EXHAUSTIVE):
    if cfg.sampler_type != abi.SAMPLER_INDEPENDENT:
        pyoracle.set_pmj_tables(*capi.host_pmj02bn_tables())
    with capi.options(**opts):
        g, gst = _render_gpu(ctx, sd, cfg)
    o, ost = pyoracle.OracleScene(sd).render(cfg)
    assert_parity(g, o, sd.camera.width, sd.camera.height, gst, ost)
    return g


# ---------------------------------------------------------------------------------------------------------------- probes
def _adversarial_dirs():
    d = [[-1, 0, 0], [-1, 0, -0.0], [-1, 0.5, 0], [-1, -0.3, -0.0], [0, 1, 0], [0, -1, 0], [1e-40, 1, 0], [0, -1, -1e-40], [-1, 0, 1e-40],
         [-1, 0, -1e-40], [1, 1e-40, 0], [1e-40, 1e-40, 1], [-1, 1e-38, -1e-44], [np.nan, 0, 1], [0, np.nan, 0], [np.inf, 1, 0], [0, 0, 0]]
    for k in range(49):
        phi = (k / 48 - 0.5) * 2 * np.pi
        d.append([np.cos(phi), 0.0, np.sin(phi)])
    for k in range(25):
        lat = (k / 24 - 0.5) * np.pi
        d.append([np.cos(lat) * 0.6, np.sin(lat), np.cos(lat) * 0.8])
    return np.array(d, np.float32)


def _adversarial_u(W, H):
    one_minus = np.nextafter(np.float32(1), np.float32(0))
    edges = np.unique(np.concatenate([np.arange(W + 1) / W, np.arange(H + 1) / H])).astype(np.float32)
    e = np.concatenate([edges, np.nextafter(edges, np.float32(0)), np.nextafter(edges, np.float32(1)), [0.0, one_minus]]).astype(np.float32)
    e = np.clip(e, 0, one_minus)
    a, b = np.meshgrid(e, e)
    return np.concatenate([np.stack([a.ravel(), b.ravel()], 1), np.random.default_rng(2).random((20000, 2))]).astype(np.float32)


@pytest.mark.parametrize("filt", [abi.TEX_FILTER_NEAREST, abi.TEX_FILTER_LINEAR], ids=["nearest", "linear"])
@pytest.mark.parametrize("shape", [(48, 24), (1, 1), (1, 7), (9, 1), (13, 7)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_probes_bit_for_bit(ctx, filt, shape):
    W, H = shape
    img = (np.random.default_rng(W * 31 + H).random((H, W, 4)) * 2).astype(np.float32)
    img[H // 3, W // 4, :3] = 40.0
    if H >= 4:
        img[H // 2:, :, :3] = 0.0  # rows the marginal never picks (under nearest)
    sd = env_scene(env=abi.EnvironmentData(image=img, strength=2.5, rotation=_rot(0.3, 1.9), filter=filt))
    scene = capi.Scene(ctx, sd)
    osc = pyoracle.OracleScene(sd)
    u = _adversarial_u(W, H)
    gs, os_ = scene.probe_env_sample(u), osc.env_sample_many(u)
    assert n_bit_diff(gs, os_) == 0, f"{n_bit_diff(gs, os_)} of {gs.size} sample floats differ"
    d = np.concatenate([_adversarial_dirs(), gs[:, :3], np.random.default_rng(3).standard_normal((20000, 3)).astype(np.float32)])
    gp, op = scene.probe_env_pdf(d), osc.env_pdf_many(d)
    assert n_bit_diff(gp, op) == 0, f"{n_bit_diff(gp, op)} of {gp.size} pdf / radiance floats differ"


# ---------------------------------------------------------------------------------------------------------------- films
LIGHTING = {
    "env_alone": dict(),
    "env_and_emitters": dict(emitters=2),
    "constant": dict(env=abi.EnvironmentData(color=(0.4, 0.5, 0.7))),
    "nearest": dict(env=abi.EnvironmentData(image=sample_image(W=40, H=20, seed=5), filter=abi.TEX_FILTER_NEAREST)),
    "linear_rotated_strength": dict(env=abi.EnvironmentData(image=sample_image(W=40, H=20, seed=6), rotation=_rot(-0.6, 2.2), strength=2.5)),
    "sun_direct": dict(env=abi.EnvironmentData(image=_sun_image(), filter=abi.TEX_FILTER_NEAREST)),
    "sun_in_a_mirror": dict(env=abi.EnvironmentData(image=_sun_image(), filter=abi.TEX_FILTER_LINEAR), floor="mirror", emitters=1),
}


@pytest.mark.parametrize("name", list(LIGHTING))
def test_lighting(ctx, name):
    sd = env_scene(material="rough_metal", **LIGHTING[name])
    g = _check(ctx, sd, make_config(spp=8, spp_per_pass=8, max_depth=5))
    img = resolve_np(g, 32, 32)
    if name.startswith("sun"):  # the sky rows: a sun of 3000 seen directly is clamped to 1000 (base is not captured on a miss)
        assert img[:8].max() == 1000.0
    if name == "sun_in_a_mirror":  # the floor rows: the sun seen in the mirror, through the clamp of the indirect sum
        assert img[16:].max() == 1000.0


@pytest.mark.parametrize("material", list(MATERIALS) + ["force_diffuse"])
def test_materials(ctx, material):
    sd = env_scene(material="glass" if material == "force_diffuse" else material, emitters=1)
    _check(ctx, sd, make_config(spp=8, spp_per_pass=8, max_depth=6, force_diffuse=1 if material == "force_diffuse" else 0))


CONFIGS = {
    "no_nee": dict(use_nee=0),
    "nee": dict(use_nee=1),
    "indirect_only": dict(indirect_only=1),
    "debug_depth_1": dict(debug_depth=1),
    "debug_depth_2": dict(debug_depth=2),
    "max_depth_0": dict(max_depth=0),
    "max_depth_1": dict(max_depth=1),
    "russian_roulette": dict(rr_depth=1, max_depth=10),
}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_configs(ctx, name):
    kw = dict(spp=8, spp_per_pass=4, max_depth=6)
    kw.update(CONFIGS[name])
    _check(ctx, env_scene(material="glass", emitters=1), make_config(**kw))


SAMPLERS = {"independent": abi.SAMPLER_INDEPENDENT, "pmj02bn": abi.SAMPLER_PMJ02BN, "sobol": abi.SAMPLER_SOBOL}


# every pipeline under the independent sampler; the index samplers under the default and the ACEScg pipeline
SAMPLER_PIPELINE = [(s, p) for s in SAMPLERS for p in PIPELINES if s == "independent" or p in ("srgb_srgb", "acescg")]


@pytest.mark.parametrize("sampler,pipeline", SAMPLER_PIPELINE, ids=[f"{s}-{p}" for s, p in SAMPLER_PIPELINE])
def test_samplers_and_pipelines(ctx, sampler, pipeline):
    cfg = make_config(spp=8, spp_per_pass=8, max_depth=5, sampler_type=SAMPLERS[sampler], sampler_seed=3, color=PIPELINES[pipeline])
    _check(ctx, env_scene(material="glass", emitters=2), cfg)


SCHEDULES = {
    "exhaustive": EXHAUSTIVE,
    "bvh": dict(force_bvh=1, instancing=0, wavefront=0, specialise=0),
    "wavefront": dict(force_bvh=1, instancing=0, wavefront=1, specialise=0),
    "wavefront_carried": dict(force_bvh=1, instancing=0, wavefront=1, specialise=0, wf_carry=2),
    "specialise": dict(force_bvh=0, instancing=0, wavefront=0, specialise=1),
    "specialise_bvh": dict(force_bvh=1, instancing=0, wavefront=0, specialise=1),
    "instances": dict(force_bvh=1, instancing=1, wavefront=0, specialise=0),
    "instances_wavefront": dict(force_bvh=1, instancing=1, wavefront=1, specialise=0),
}


def _glass_instanced():
    sd = instanced_scene(n_inst=4, n=3, width=32, height=32, emissive_instances=1)
    sd.materials[0].kind, sd.materials[0].ior, sd.materials[0].roughness = abi.MAT_GLASS, 1.5, 0.1
    sd.ggx_table = _ggx()
    sd.environment = abi.EnvironmentData(image=sample_image(W=32, H=16, seed=7), strength=1.5, rotation=_rot(0.4, 0.9))
    return sd


@pytest.mark.parametrize("name", list(SCHEDULES))
def test_schedules_glass_emitters_acescg(ctx, name):
    sd = _glass_instanced() if name.startswith("instances") else env_scene(material="glass", emitters=2)
    cfg = make_config(spp=8, spp_per_pass=4, max_depth=6, color=PIPELINES["acescg"], sampler_type=abi.SAMPLER_PMJ02BN, sampler_seed=9)
    _check(ctx, sd, cfg, SCHEDULES[name])


def test_tile_shards_and_sample_ranges(ctx):
    sd = env_scene(material="glass", emitters=2)
    w, h = sd.camera.width, sd.camera.height
    cfg = make_config(spp=12, spp_per_pass=4, max_depth=6, color=PIPELINES["acescg"], sampler_type=abi.SAMPLER_SOBOL, sampler_seed=5)
    pyoracle.set_pmj_tables(*capi.host_pmj02bn_tables())
    o, _ = pyoracle.OracleScene(sd).render(cfg)
    with capi.options(force_bvh=1, instancing=0, wavefront=0, specialise=0):
        scene = capi.Scene(ctx, sd)
        acc = np.zeros(7 * w * h, np.float32)
        for r in range(8):
            film = capi.Film(ctx, w, h)
            capi.pt_render(ctx, scene, distributed.shard_config(cfg, r, 8, 8, 8), film)
            part = film.read()
            assert not np.any((acc != 0) & (part != 0))
            acc += part
    assert n_bit_diff(acc, o) == 0
    with capi.options(**EXHAUSTIVE):
        scene = capi.Scene(ctx, sd)
        film = capi.Film(ctx, w, h)
        for b, c in ((0, 5), (5, 4), (9, 3)):
            rc = cfg.copy()
            rc.sample_begin, rc.sample_count = b, c
            capi.pt_render(ctx, scene, rc, film)
    assert n_bit_diff(film.read(), o) == 0


def test_aov(ctx):
    sd = env_scene(material="glass", emitters=1)
    a = abi.AovConfig.default()
    a.spp, a.aov = 4, 4  # albedo: a miss is 0
    scene = capi.Scene(ctx, sd)
    film = capi.Film(ctx, 32, 32)
    capi.aov_render(ctx, scene, a, film)
    o, _ = pyoracle.OracleScene(sd).aov_render(a)
    assert n_bit_diff(film.read(), o) == 0


def test_scene_json_both_readers(ctx, tmp_path):
    """akr_scene_load of a scene.json with an EXR environment and a rotation renders what the oracle renders from the Python reader."""
    img = sample_image(W=40, H=20, seed=13)
    blob = make_exr({c: np.ascontiguousarray(img[::-1, :, k]) for k, c in enumerate("RGBA")}, compression=3)
    import base64
    import json
    path = scene_json_text(tmp_path, {"color": [1, 1, 1], "strength": 1.5,
                                      "transform": {"type": "trs", "data": {"translation": [0, 0, 0], "rotation": [0.3, -0.8, 0.2], "scale": [1, 1, 1],
                                                                            "coordinate_system": "Akari"}}}, fov=60.0)
    scene = json.loads(open(path).read())
    scene["buffers"]["b_env"] = {"type": "base64", "data": base64.b64encode(blob).decode(), "length": len(blob)}
    scene["buffer_views"]["v_env"] = {"buffer": {"id": "b_env"}, "offset": 0, "length": len(blob)}
    del scene["environment"]["color"]
    scene["environment"]["image"] = {"data": {"id": "v_env"}, "format": "exr", "colorspace": "none", "extension": "repeat", "interpolation": "linear",
                                     "width": 40, "height": 20, "channels": 4}
    open(path, "w").write(json.dumps(scene))
    cfg = make_config(spp=8, spp_per_pass=8, max_depth=4)
    lib_scene = capi.Scene(ctx, path, 32, 32)
    film = capi.Film(ctx, 32, 32)
    capi.pt_render(ctx, lib_scene, cfg, film)
    o, _ = pyoracle.OracleScene(scene_json.load_scene(path, 32, 32)).render(cfg)
    assert n_bit_diff(film.read(), o) == 0
