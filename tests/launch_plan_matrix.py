"""The matrix of tests/test_launch_plan.py and tests/golden/make_launch_plan_golden.py: scenes x configs x options for which
akr_host_pt_launch_plan (capi.Scene.launch_plan) says which instantiation of the pt kernel a session launches and how its LDS is laid out.
Everything here runs on the host (Scene(None, ...))."""
import copy
import hashlib
import os

import numpy as np

from akari_render_amd import abi, capi
from oracle import scene_json
from tests.helpers import cbox_variant, instanced_scene, make_config, textured_room

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CBOX = os.path.join(ROOT, "scenes", "cbox", "scene.json")
FLAT = dict(force_bvh=0, instancing=0)
SAMPLERS = (abi.SAMPLER_INDEPENDENT, abi.SAMPLER_PMJ02BN, abi.SAMPLER_SOBOL)


def strip_scene(n_tris=63, width=32, height=32) -> abi.SceneData:
    """A zigzag strip of `n_tris` floor triangles of one diffuse material under a two-triangle light: n_tris + 2 triangles in all."""
    xs = np.linspace(-1.0, 1.0, n_tris // 2 + 2, dtype=np.float32)
    verts = np.array([[x, -1.0, z] for x in xs for z in (-1.0, 1.0)], dtype=np.float32)
    idx = np.array([[k, k + 2, k + 1] if k % 2 == 0 else [k, k + 1, k + 2] for k in range(n_tris)], dtype=np.uint32)
    floor = abi.MeshData(vertices=verts, indices=idx)
    lv = np.array([[-0.3, 1.0, -0.3], [0.3, 1.0, -0.3], [0.3, 1.0, 0.3], [-0.3, 1.0, 0.3]], dtype=np.float32)
    light = abi.MeshData(vertices=lv, indices=np.array([[0, 1, 2], [0, 2, 3]], dtype=np.uint32))
    mats = [abi.MaterialData(kind=abi.MAT_DIFFUSE, base_color=(0.7, 0.6, 0.5)),
            abi.MaterialData(kind=abi.MAT_EMISSION, emission_color=(9.0, 8.0, 7.0), emission_strength=1.0)]
    eye = np.eye(4, dtype=np.float32).reshape(16).copy()
    c2w = np.eye(4, dtype=np.float32)
    c2w[:3, 3] = [0.0, 0.0, 3.0]
    cam = abi.CameraData(c2w=c2w.T.reshape(16).copy(), fov=0.9, width=width, height=height)
    return abi.SceneData([floor, light], [abi.InstanceData(0, [0], eye), abi.InstanceData(1, [1], eye)], mats, cam)


def cbox(which=None) -> abi.SceneData:
    sd = scene_json.load_scene(CBOX, 32, 32)
    return cbox_variant(sd, which) if which else sd


def one_metal() -> abi.SceneData:
    """three diffuse walls and one conductor: few enough expensive hits for DEFER"""
    sd = strip_scene(20)
    sd.materials.insert(1, abi.MaterialData(kind=abi.MAT_PRINCIPLED, base_color=(0.9, 0.7, 0.5), metallic=1.0, roughness=0.35))
    sd.materials.insert(1, abi.MaterialData(kind=abi.MAT_DIFFUSE, base_color=(0.3, 0.6, 0.5)))
    sd.materials.insert(1, abi.MaterialData(kind=abi.MAT_DIFFUSE, base_color=(0.5, 0.3, 0.7)))
    sd.meshes[0].material_slots = (np.arange(20) % 4).astype(np.uint32)
    sd.instances[0].materials = [0, 1, 2, 3]
    sd.instances[1].materials = [4]
    return sd


def textured_many_graphs(n_extra=120, sd=None) -> abi.SceneData:
    """the textured room with a tree (or `sd`, a textured room of another size), plus `n_extra` copies of its normal-mapped wall material on
    copies of that wall: more node lists than the BVH kernels stage"""
    sd = sd if sd is not None else textured_room(32, 32, n_floor=8)
    wall = sd.instances[2]
    for k in range(n_extra):
        sd.materials.append(copy.deepcopy(sd.materials[wall.materials[0]]))
        t = np.eye(4, dtype=np.float32)
        t[:3, 3] = [-3.0 - 0.01 * k, 0.0, 0.0]
        sd.instances.append(abi.InstanceData(wall.mesh, [len(sd.materials) - 1], t.T.reshape(16).copy()))
    return sd


# name -> (builder, options the scene is created under, has texture-fed materials)
BASE_SCENES = {
    "cbox": (cbox, FLAT, False),
    "tris65": (lambda: strip_scene(63), FLAT, False),
    "cbox_force_bvh": (cbox, dict(force_bvh=1, instancing=0), False),
    "tex_exhaustive": (lambda: textured_room(32, 32), FLAT, True),
    "tex_tree": (lambda: textured_room(32, 32, n_floor=8), FLAT, True),
    "tex_tree_unstaged": (textured_many_graphs, FLAT, True),
    "kept2": (lambda: instanced_scene(n_inst=2, n=4, width=32, height=32), dict(force_bvh=0, instancing=1), False),
}
EXTRA_SCENES = {
    "one_metal": (one_metal, FLAT, False),
    "coat": (lambda: cbox("glass_coat"), FLAT, False),
}
ENV = abi.EnvironmentData(color=(0.5, 0.6, 0.8), strength=1.0)
LENS = abi.LensData(1.0 / 1024, 3.0)


def camera_inside(sd: abi.SceneData) -> abi.SceneData:
    """the camera moved to within the magnitudes of the scene's box on every axis: a scene with a tree accepts a lens only there"""
    pts = []
    for inst in sd.instances:
        m = np.asarray(inst.transform, np.float64).reshape(4, 4).T
        v = np.asarray(sd.meshes[inst.mesh].vertices, np.float64).reshape(-1, 3)
        pts.append(v @ m[:3, :3].T + m[:3, 3])
    reach = 0.95 * np.abs(np.concatenate(pts)).max(axis=0)
    c2w = np.array(sd.camera.c2w, dtype=np.float32)
    c2w[12:15] = np.clip(c2w[12:15], -reach, reach).astype(np.float32)
    sd.camera.c2w = c2w
    return sd


def scenes():
    """(name, host-only capi.Scene, textured) of the matrix: every base scene without / with an environment and without / with a lens"""
    for name, (build, opts, tex) in BASE_SCENES.items():
        for env in (0, 1):
            for lens in (0, 1):
                sd = camera_inside(build()) if lens else build()
                sd.environment = ENV if env else None
                sd.lens = LENS if lens else None
                with capi.options(**opts):
                    yield f"{name}/env{env}/lens{lens}", capi.Scene(None, sd), tex
    for name, (build, opts, tex) in EXTRA_SCENES.items():
        with capi.options(**opts):
            yield name, capi.Scene(None, build()), tex


def cases(textured):
    """(key, config, options) per scene: force_diffuse x sampler x per-scene kernel at the default options, then the option sweep"""
    specs = (0, 3, 4) if textured else (0,)
    for fd in (0, 1):
        for s in SAMPLERS:
            for w in specs:
                yield f"fd{fd}/s{s}/w{w}", make_config(spp=4, force_diffuse=fd, sampler_type=s), dict(spec_waves=w)
    for w, s in ((0, abi.SAMPLER_INDEPENDENT), (3, abi.SAMPLER_PMJ02BN)) if textured else ((0, abi.SAMPLER_INDEPENDENT),):
        for dm in (-1, 0, 1):
            for sk in (0, 1):
                for don in (1, 2, 3):
                    yield (f"fd0/s{s}/w{w}/dm{dm}/sk{sk}/on{don}", make_config(spp=4, sampler_type=s),
                           dict(spec_waves=w, defer_metal=dm, simple_kernels=sk, defer_on=don))


FIELDS = ("simple_scene", "defer_metal", "defer_flags", "stage_total", "tile_offset", "bvh_tile_nodes", "park_offset", "carry_offset", "bn_offset",
          "val_offset_words", "lds_bytes", "blocks", "specialised")


def flatten(plan: dict) -> list:
    """a plan as one list: the ten variant flags, FIELDS, the 13 stage sizes, a digest of the per-scene kernel's wrapper text"""
    digest = hashlib.sha256(plan["wrapper"].encode()).hexdigest()[:16] if plan["wrapper"] else ""
    return [plan["variant"][n] for n in abi.PtLaunchPlan.VARIANT] + [plan[f] for f in FIELDS] + plan["stage_bytes"] + [digest]


def rows() -> dict:
    out = {}
    for sname, scene, tex in scenes():
        for key, cfg, opts in cases(tex):
            out[f"{sname}/{key}"] = flatten(scene.launch_plan(cfg, **opts))
        scene.close()
    return out
