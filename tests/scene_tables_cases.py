"""The scenes and setter sequences of tests/test_scene_tables.py, tests/test_gpu_scene_tables.py and tests/golden/make_scene_tables_golden.py:
the smallest scene of every route by which a scene comes to its device tables (flattened without and with a tree, textured, kept as meshes +
instances, an environment, punctual lights without and with the light tree), and the setters that upload the light tables again. For each,
what the library says it holds: info().device_bytes and every AKR_ARRAY_* array."""
import dataclasses
import hashlib
import os

import numpy as np

from akari_render_amd import abi, capi
from oracle import scene_json
from tests.helpers import instanced_scene, textured_room

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = H = 32
FLAT = dict(force_bvh=0, instancing=0, light_tree=0)
TREE = dict(FLAT, light_tree=1)
N_ARRAYS = 29  # AKR_ARRAY_WOOP .. AKR_ARRAY_LIGHT_TREE (include/akari_hip.h)

PL = abi.PunctualLightData
POINT = PL(abi.LIGHT_POINT, position=(0.5, 1.5, 0.5), color=(3.0, 2.5, 2.0), strength=2.0)
POINT2 = PL(abi.LIGHT_POINT, position=(-0.6, 0.4, 0.6), color=(1.0, 2.0, 3.0), strength=1.0, radius=0.1)
SUN = PL(abi.LIGHT_SUN, direction=(0.2, -1.0, -0.3), color=(1.0, 0.9, 0.8), strength=0.5)
THREE = [POINT, POINT2, SUN]


def env_image(w, h):
    """an image whose rows and columns all differ (no generator: the same floats everywhere)"""
    y, x, c = np.meshgrid(np.arange(h), np.arange(w), np.arange(3), indexing="ij")
    return (0.25 + ((7 * x + 13 * y + 5 * c) % 11) / 8.0).astype(np.float32)


def env(w, h):
    return abi.EnvironmentData(image=env_image(w, h), strength=0.75, filter=abi.TEX_FILTER_LINEAR)


def cbox(**more):
    return dataclasses.replace(scene_json.load_scene(os.path.join(ROOT, "scenes", "cbox", "scene.json"), W, H), **more)


def tex():
    sd = textured_room(W, H)
    sd.ggx_table = np.fromfile(os.path.join(ROOT, "tests", "golden", "ggx_dielectric_s.f32"), dtype=np.float32)  # both sides read the committed table
    return sd


# name -> (scene, options it is created under, the oracle's light_tree mode)
SCENES = {
    "cbox": (cbox, FLAT, False),
    "cbox_force_bvh": (cbox, dict(FLAT, force_bvh=1), False),
    "tex": (tex, FLAT, False),
    "kept": (lambda: instanced_scene(n_inst=2, n=4, width=W, height=H), dict(force_bvh=0, instancing=1, light_tree=0), False),
    "cbox_env_1x1": (lambda: cbox(environment=env(1, 1)), FLAT, False),
    "cbox_env_13x7": (lambda: cbox(environment=env(13, 7)), FLAT, False),
    "cbox_point": (lambda: cbox(lights=[POINT]), FLAT, False),
    "cbox_three_lights": (lambda: cbox(lights=list(THREE)), FLAT, False),
    "cbox_point_tree": (lambda: cbox(lights=[POINT]), TREE, True),
    "cbox_three_lights_tree": (lambda: cbox(lights=list(THREE)), TREE, True),
}


def _set_env(sc):
    sc.set_environment(image=env_image(13, 7), strength=0.75, filter=abi.TEX_FILTER_LINEAR)


def _add_three(sc):
    for l in THREE:
        sc.add_punctual_light(l)


# name -> (scene it starts from, [(step, what it does to the capi.Scene, the SceneData and light_tree mode a fresh scene of that state has)])
SEQUENCES = {
    "env_set_remove": ("cbox", [("set", _set_env, lambda: cbox(environment=env(13, 7)), False),
                                ("removed", lambda sc: sc.set_environment(), cbox, False)]),
    "lights_add_clear": ("cbox", [("added", _add_three, lambda: cbox(lights=list(THREE)), False),
                                  ("cleared", lambda sc: sc.clear_punctual_lights(), cbox, False)]),
    "light_tree_on_off": ("cbox_three_lights", [("on", lambda sc: sc.set_light_tree(True), lambda: cbox(lights=list(THREE)), True),
                                                ("off", lambda sc: sc.set_light_tree(False), lambda: cbox(lights=list(THREE)), False)]),
}


def make_scene(ctx, name):
    build, opts, _ = SCENES[name]
    with capi.options(**opts):
        return capi.Scene(ctx, build())


def record(sc) -> dict:
    """{device_bytes, arrays: [[bytes, sha256 of the contents] per AKR_ARRAY_* id]}"""
    arrays = []
    for which in range(N_ARRAYS):
        a = sc.array(which, np.uint8)
        arrays.append([int(a.size), hashlib.sha256(a.tobytes()).hexdigest()])
    return {"device_bytes": int(sc.info().device_bytes), "arrays": arrays}


def walk(ctx, visit):
    """visit(key, capi.Scene, () -> SceneData of that state, light_tree mode) for every scene ("name") and every step of every sequence ("name/step")"""
    for name, (build, _, tree) in SCENES.items():
        visit(name, make_scene(ctx, name), build, tree)
    for name, (start, steps) in SEQUENCES.items():
        sc = make_scene(ctx, start)
        for step, change, state, tree in steps:
            change(sc)
            visit(f"{name}/{step}", sc, state, tree)
