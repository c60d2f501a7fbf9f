"""The scenes, configurations and expected kernel variants of tests/test_gpu_light_tree_parity.py (films of scenes with a light tree, DESIGN.md 4.16,
on the GPU against the CPU oracle, bit for bit). They live here so that tests/test_light_tree_parity_cases.py can check on the CPU, with the oracle
and the library's host build alone, that every case is what it claims to be: that a tree of 2 L - 1 nodes exists, that the session the library plans
runs the kernel the case is there for, and that the tree changes the film -- against the same scene by power alone and against the scene without
lights. Scenes, materials, samplers and the oracle's side are those of tests/punct_parity_cases.py; every case's options carry light_tree = 1."""
import dataclasses
import functools

import numpy as np

from akari_render_amd import abi
from tests import punct_parity_cases as P
from tests.helpers import make_config
from tests.punct_parity_cases import BVH, EXH, LENS, PIPELINES, SAMPLERS, largest_count, lit_scene, oracle_render, tex_scene

PL = abi.PunctualLightData
F = np.float32
EXH_T, BVH_T = dict(EXH, light_tree=1), dict(BVH, light_tree=1)
F_LTREE = 256  # akr_kernel_info.kernel_flags bit 8: "walks a light tree"; the launch plan does not report it
ROUTES = (("exh", EXH_T), ("bvh", BVH_T))

_SPOT = dict(position=(-1.2, 1.6, 1.4), direction=(1.1, -2.4, -1.2), cone_angle=0.42, color=(2.0, 3.0, 4.0), strength=8.0)
# five local lights of the floor-and-box scene: delta and soft, points and spots (one with a hard edge: samples outside its cone are invalid)
FIVE = [
    PL(abi.LIGHT_POINT, position=(1.4, 0.9, 1.2), color=(3.0, 2.5, 2.0), strength=3.0),
    PL(abi.LIGHT_SPOT, blend=0.4, radius=0.2, **_SPOT),
    PL(abi.LIGHT_SPOT, position=(1.2, 1.4, -0.8), direction=(-1.0, -2.0, 0.6), cone_angle=0.5, blend=0.0, color=(4.0, 2.0, 1.0), strength=6.0),
    PL(abi.LIGHT_POINT, position=(-1.6, 0.4, 0.8), color=(1.0, 2.0, 3.0), strength=2.0, radius=0.3),
    PL(abi.LIGHT_POINT, position=(0.2, 0.5, -1.8), color=(2.0, 2.0, 2.0), strength=2.5),
]
SUNS = [PL(abi.LIGHT_SUN, direction=(0.3, -1.0, -0.25), color=(1.0, 0.9, 0.8), strength=1.5), PL(abi.LIGHT_SUN, direction=(-0.4, -1.0, 0.3), color=(0.6, 0.8, 1.0), strength=1.0, angle=0.25)]
# two suns given BEFORE and BETWEEN the local lights: their record indices (0 and 3) are not their ranks among the table's entries
SUNS_AMONG = [SUNS[0]] + FIVE[:2] + [SUNS[1]] + FIVE[2:]


def n_local(sd):
    return sum(1 for l in sd.lights if l.type != abi.LIGHT_SUN)


def tree_lights(n, seed, strength=None):
    """n local lights over the floor and around the box: every third one soft, every fourth a spot pointing down (hard-edged and blended in turn),
    unequal strengths and colours"""
    rng = np.random.default_rng(seed)
    pos = np.c_[rng.uniform(-3, 3, n), rng.uniform(-0.7, 1.6, n), rng.uniform(-3, 3, n)].astype(F)
    scale = strength if strength is not None else 6.0 / np.sqrt(n)
    out = []
    for k in range(n):
        radius = float(F(rng.uniform(0.05, 0.3))) if k % 3 == 1 else 0.0
        s = float(F(rng.uniform(0.5, 4.0) * scale))
        where = tuple(float(v) for v in pos[k])
        if k % 4 == 3:
            out.append(PL(abi.LIGHT_SPOT, position=where, direction=(0.1 * (k % 3 - 1), -1.0, 0.15), cone_angle=0.9, blend=0.4 * (k // 4 % 2), color=(1.0, 2.0, 0.5), strength=2.0 * s, radius=radius))
        else:
            out.append(PL(abi.LIGHT_POINT, position=where, color=(2.0, 1.0 + 0.25 * (k % 3), 1.5), strength=s, radius=radius))
    return out


CASES = {}


def add(name, scene, cfg, opts, tags=(), **want):
    assert name not in CASES and opts.get("light_tree") == 1, name
    CASES[name] = P.Case(name, scene, dict(cfg), dict(opts), P._want(opts, cfg, **want), tuple(tags))
    return name


def flags(case):
    """the kernel_flags the session must report: the case's, the PUNCT bit among them, and the tree's"""
    return case.flags() | P.F_PUNCT | F_LTREE


BASE = dict(spp=8, spp_per_pass=8, max_depth=5, rr_depth=2)

# ---------------------------------------------------------------------------------------------------------------- all 96 LTREE kernels
SWEEP_CFG = dict(spp=4, spp_per_pass=4, max_depth=4, rr_depth=2)
ROOM_LOCAL = P.ROOM_LIGHTS + [PL(abi.LIGHT_POINT, position=(0.5, 0.3, -0.4), color=(1.0, 2.0, 3.0), strength=0.75), PL(abi.LIGHT_POINT, position=(-0.6, 0.3, 0.3), color=(2.0, 2.0, 1.0), strength=0.5, radius=0.05),
                              PL(abi.LIGHT_SPOT, position=(0.1, 0.6, 0.6), direction=(-0.2, -1.0, -0.3), cone_angle=0.7, blend=0.0, color=(3.0, 1.0, 1.0), strength=2.0)]


def filler_suns(n):
    """n weak suns, each an entry of the light table of its own: with a tree the local lights are ONE entry and can never push a BVH scene past its LDS
    stage budget, suns can. Weak enough that the tree's entry keeps its share of the selection (the checker asserts 0.25)."""
    return [PL(abi.LIGHT_SUN, direction=(0.3 + 0.02 * (i % 7), -1.0, -0.25 + 0.02 * (i % 5)), color=(1.0, 0.9, 0.8), strength=2.5e-4 * (1 + i % 3), angle=0.1 * (i % 2)) for i in range(n)]


@functools.lru_cache(maxsize=None)
def unstaged_suns(tex, env, lens):
    """a count of filler suns past which the BVH kernels of this unit's scene no longer stage their tables: by bisection on the host"""
    mk = functools.partial(_sweep_scene, tex, env, lens, "bvh_unstaged")
    return largest_count(lambda n: mk(n_suns=n), BVH_T, make_config(**SWEEP_CFG), stage=True) + 1


def _sweep_scene(tex, env, lens, route, n_suns=None):
    if n_suns is None:
        n_suns = unstaged_suns(tex, env, lens) if route == "bvh_unstaged" else 0
    fill = filler_suns(n_suns)
    if tex:  # (the filler before and between the local lights: record indices that are no ranks)
        return tex_scene(16, 16, fill[:1] + ROOM_LOCAL[:2] + fill[1:] + ROOM_LOCAL[2:], env, abi.LensData(0.05, 1.5) if lens else None)
    return lit_scene("glass", SUNS[:1] + fill[:1] + FIVE[:3] + fill[1:] + FIVE[3:], emitters=1, env=True if env else None, lens=LENS if lens else None, w=16, h=16)


SWEEP_CASES = []
for _u, (_env, _lens) in {"plain": (0, 0), "env": (1, 0), "lens": (0, 1), "lens_env": (1, 1)}.items():
    for _route in ("exh", "bvh", "bvh_unstaged"):
        for _fd in (0, 1):
            for _tex in (0, 1):
                for _pmj in (0, 1):
                    _s = 0 if not _pmj else (abi.SAMPLER_SOBOL if (_fd, _tex) == (0, 0) else abi.SAMPLER_PMJ02BN)
                    SWEEP_CASES.append(add(f"sweep-{_u}-{_route}-fd{_fd}-tex{_tex}-pmj{_pmj}", functools.partial(_sweep_scene, _tex, _env, _lens, _route),
                                           dict(SWEEP_CFG, force_diffuse=_fd, sampler_type=_s, sampler_seed=7), EXH_T if _route == "exh" else BVH_T,
                                           tags=("filler",) if _route == "bvh_unstaged" else (), lens=bool(_lens), stage=_route != "bvh_unstaged", env=_env, fd=_fd, tex=_tex))

# ---------------------------------------------------------------------------------------------------------------- tree shapes and counts
SHAPE_CFG = dict(spp=8, spp_per_pass=8, max_depth=4, rr_depth=2)
# eight lights on one axis-aligned line with repeated places: two extents are 0 (the axis tie goes to the lowest), equal keys go to the index
LINE_8 = [PL(abi.LIGHT_POINT, position=(0.9, y, 1.0), color=(2.0, 1.0 + 0.25 * (k % 3), 1.5), strength=1.0 + 0.5 * (k % 4), radius=0.1 * (k % 2)) for k, y in enumerate((0.2, 0.8, 0.2, 0.5, 0.8, 0.5, 0.2, 1.1))]
# four lights at one point: every box is the same degenerate box, the importances are the powers at any p
ONE_POINT_4 = [PL(abi.LIGHT_POINT, position=(1.0, 0.7, 1.1), color=c, strength=s) for c, s in (((2.0, 1.0, 1.5), 2.0), ((1.0, 2.0, 0.5), 4.0), ((0.5, 1.0, 3.0), 1.5))]
ONE_POINT_4.append(PL(abi.LIGHT_SPOT, position=(1.0, 0.7, 1.1), direction=(-0.5, -1.0, -0.5), cone_angle=1.2, blend=0.3, color=(1.0, 1.0, 1.0), strength=6.0))
SHAPES = {f"L{n}": functools.partial(tree_lights, n, 40 + n) for n in (2, 3, 5, 33, 257)}  # L = 3: leaves at two depths, lanes make different trip counts
SHAPES["line_8"] = lambda: LINE_8
SHAPES["one_point_4"] = lambda: ONE_POINT_4


def shape_scene(which):
    return lit_scene("rough_metal", SHAPES[which]())


def past_exhaustive_scene():
    """one local light more than the exhaustive path's LDS budget takes in mode 0 (P.exhaustive_limit(), found on the host): refused there, one entry here"""
    return lit_scene("rough_metal", tree_lights(P.exhaustive_limit() + 1, 9))


SHAPE_CASES = [add(f"shape-{_w}-{_r}", functools.partial(shape_scene, _w), SHAPE_CFG, _o) for _w in SHAPES for _r, _o in ROUTES]
SHAPE_CASES.append(add("shape-past_exhaustive_limit-exh", past_exhaustive_scene, SHAPE_CFG, EXH_T, tags=("past_limit",)))


# ---------------------------------------------------------------------------------------------------------------- positions that reach the walk's edges
def _box_corner():
    """a top corner of the box, as the float32 vertex the mesh holds"""
    v = np.asarray(lit_scene().meshes[1].vertices, F).reshape(-1, 3)
    return tuple(float(x) for x in v[np.lexsort((v[:, 2], v[:, 0], -v[:, 1]))[0]])


def edge_scene(material="diffuse", floor="diffuse"):
    """a delta light exactly in the floor plane and one at a box corner (d2 = 0 at or near a hit point: the importance overflows, the step falls back to the
    powers) beside three ordinary ones"""
    lights = [PL(abi.LIGHT_POINT, position=(0.5, -1.0, 1.25), color=(3.0, 2.5, 2.0), strength=0.5), PL(abi.LIGHT_POINT, position=_box_corner(), color=(1.0, 2.0, 3.0), strength=0.5)] + FIVE[:3]
    return lit_scene(material, lights, emitters=1, floor=floor)


FAR = PL(abi.LIGHT_POINT, position=(3.0e5, 9.0e5, 3.0e5), color=(1.0, 1.0, 1.0), strength=2.0e11)
NEAR_STRONG = [PL(abi.LIGHT_POINT, position=(1.0, 0.2, 1.0), color=(3.0, 2.5, 2.0), strength=1.0e6), PL(abi.LIGHT_POINT, position=(-1.0, 0.0, 1.2), color=(2.0, 2.5, 3.0), strength=1.0e6),
               ]
POSITION_SCENES = {
    "on_surfaces": edge_scene,
    # a light 10^6 units away beside near ones: at the level that separates it from them its probability sits at the 2^-16 clamp, and its f / p at depth >= 2
    # meets the radiance clamp [0, 1000] of the indirect sum
    # (three lights: the far one is the root's right leaf, so one step decides it -- every sample of a near light carries the factor 1 - 2^-16, and about
    # one light sample in 65536 is the far light's)
    "far_clamp": functools.partial(lit_scene, "rough_metal", NEAR_STRONG[:1] + [FAR] + NEAR_STRONG[1:], floor="rough_metal"),
    "inside_glass_box": functools.partial(lit_scene, "glass", [PL(abi.LIGHT_POINT, position=(0.0, -0.4, 0.0), color=(3.0, 2.5, 2.0), strength=2.0), PL(abi.LIGHT_POINT, position=(0.1, -0.5, 0.1), color=(1.0, 2.0, 3.0), strength=1.0, radius=0.2)] + FIVE[:2], emitters=1),
    # below the floor plane: face_forward flips the offset of every shadow ray from the floor's upper side
    "below_floor": functools.partial(lit_scene, "rough_metal", [PL(abi.LIGHT_POINT, position=(0.5, -1.5, 1.0), color=(3.0, 2.5, 2.0), strength=4.0), PL(abi.LIGHT_SPOT, position=(-0.5, -1.6, 1.0), direction=(0.0, 1.0, 0.0), cone_angle=1.2, blend=0.5, color=(3.0, 2.5, 2.0), strength=4.0),
                                                                 PL(abi.LIGHT_POINT, position=(0.0, -1.2, -1.0), color=(1.0, 1.0, 2.0), strength=2.0, radius=0.3)] + FIVE[:2] + SUNS[:1]),
    "soft_delta_spots_mixed": functools.partial(lit_scene, "coated", FIVE + [PL(abi.LIGHT_SPOT, blend=0.0, **_SPOT), PL(abi.LIGHT_SPOT, blend=1.0, **dict(_SPOT, position=(1.3, 1.5, 1.0), direction=(-1.0, -2.2, -1.0))), P.LIGHTS["soft_point"], P.LIGHTS["soft_sun"]]),
}
POSITION_CASES = [add(f"pos-{_n}-{_r}", POSITION_SCENES[_n], dict(BASE, max_depth=6) if _n == "far_clamp" else BASE, _o, tags=("clamp",) if _n == "far_clamp" else ()) for _n in POSITION_SCENES for _r, _o in ROUTES]

# ---------------------------------------------------------------------------------------------------------------- light-table interplay
DEEP = dict(spp=8, spp_per_pass=8, max_depth=6, rr_depth=3)
INTERPLAY_CASES = []
for _e in (0, 1, 2):
    for _env in (None, True):
        for _sn, _lights in (("no_sun", FIVE), ("suns_among", SUNS_AMONG)):
            _o = BVH_T if (_e + int(bool(_env)) + int(_sn == "no_sun")) % 2 else EXH_T
            INTERPLAY_CASES.append(add(f"table-{_e}_emitters-{'env' if _env else 'no_env'}-{_sn}", functools.partial(lit_scene, "glass", _lights, emitters=_e, env=_env), DEEP, _o,
                                       tags=("interplay",), env=int(bool(_env))))
# (brighter local lights: beside two suns, an emitter and an environment the tree must still be chosen often enough to change the indirect light alone)
BRIGHT_AMONG = [l if l.type == abi.LIGHT_SUN else dataclasses.replace(l, strength=4.0 * l.strength) for l in SUNS_AMONG]
for _n, _kw in (("indirect_only", dict(indirect_only=1)), ("debug_depth_1", dict(debug_depth=1)), ("debug_depth_2", dict(debug_depth=2)), ("no_nee", dict(use_nee=0))):
    INTERPLAY_CASES.append(add(f"table-{_n}", functools.partial(lit_scene, "rough_metal", BRIGHT_AMONG, emitters=1, env=True), dict(DEEP, **_kw), BVH_T if _n.startswith("debug") else EXH_T,
                               tags=("dark_ok",) if _n == "no_nee" else ("interplay",), env=1))

# ---------------------------------------------------------------------------------------------------------------- materials (MIS at bounce >= 2)
MATERIAL_CASES = []
for _m in ("diffuse", "glass", "rough_metal", "coated", "alpha_floor", "force_diffuse"):
    for _r, _o in ROUTES:
        _scene = functools.partial(lit_scene, {"alpha_floor": "diffuse", "force_diffuse": "glass"}.get(_m, _m), FIVE, emitters=1, floor="alpha" if _m == "alpha_floor" else "diffuse")
        MATERIAL_CASES.append(add(f"mat-{_m}-{_r}", _scene, dict(BASE, force_diffuse=int(_m == "force_diffuse")), _o, fd=int(_m == "force_diffuse")))

# ---------------------------------------------------------------------------------------------------------------- colour pipelines x samplers
COLOURED = [PL(abi.LIGHT_POINT, position=(1.4, 0.9, 1.2), color=(3.0, 0.5, 1.0), strength=3.0), PL(abi.LIGHT_SUN, direction=(0.3, -1.0, -0.25), color=(0.2, 1.0, 0.6), strength=1.5, angle=0.2),
            PL(abi.LIGHT_SPOT, blend=0.4, radius=0.1, **dict(_SPOT, color=(4.0, 1.0, 0.3))), PL(abi.LIGHT_POINT, position=(-1.0, 0.5, 1.5), color=(0.3, 1.0, 4.0), strength=2.0),
            PL(abi.LIGHT_POINT, position=(0.2, 0.5, -1.8), color=(0.5, 3.0, 0.5), strength=2.0, radius=0.2)]
COLOURED_MORE = PL(abi.LIGHT_SPOT, position=(1.2, 1.4, -0.8), direction=(-1.0, -2.0, 0.6), cone_angle=0.6, blend=0.5, color=(1.0, 0.2, 3.0), strength=6.0)
COLOURED_AFTER = [COLOURED[3], COLOURED[1], PL(abi.LIGHT_POINT, position=(1.5, 0.3, 0.5), color=(3.0, 3.0, 0.2), strength=1.5), COLOURED[2]]
PIPELINE_CASES = [add(f"colour-{_s}-{_p}", functools.partial(lit_scene, "coated", COLOURED, emitters=1, floor="alpha"),
                      dict(BASE, sampler_type=SAMPLERS[_s], sampler_seed=3, color=PIPELINES[_p]), BVH_T if _s == "pmj02bn" else EXH_T)
                  for _s in SAMPLERS for _p in PIPELINES]

# ---------------------------------------------------------------------------------------------------------------- scenes of the tests outside the table
SCHED_SCENE = functools.partial(lit_scene, material="glass", lights=SUNS_AMONG, emitters=1, env=True)
SESSION_SCENE = functools.partial(lit_scene, "coated", COLOURED, emitters=1, floor="alpha")
# name -> (scene, make_config's keywords)
EXTRA = {
    "schedules-independent": (SCHED_SCENE, dict(spp=8, spp_per_pass=1, max_depth=5, rr_depth=2, sampler_seed=4)),
    "schedules-pmj02bn": (SCHED_SCENE, dict(spp=8, spp_per_pass=4, max_depth=5, rr_depth=2, sampler_type=abi.SAMPLER_PMJ02BN, sampler_seed=6)),
    "schedules-sobol": (SCHED_SCENE, dict(spp=12, spp_per_pass=4, max_depth=5, rr_depth=2, sampler_type=abi.SAMPLER_SOBOL, sampler_seed=5)),
    "sessions": (SESSION_SCENE, dict(BASE, color=PIPELINES["acescg"], sampler_seed=3)),
}


def tree_render(sd, cfg, **kw):
    """the oracle's (film, stats, final sampler states) of the scene with the mode on"""
    return oracle_render(sd, cfg, light_tree=True, **kw)
