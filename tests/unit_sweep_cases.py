"""The table of tests/test_gpu_unit_sweep.py: one case for every precompiled pt kernel without punctual lights -- the 240 instantiations of the
plain, kept (k_pt_pass_inst) and FEAT kinds that kernels.h pt_variant_compiled leaves (the other 192, the PUNCT and light-tree kinds, are swept by
tests/punct_parity_cases.py and tests/light_tree_parity_cases.py). A case is keyed by (kind, env, lens, bvh, stage, fd, tex, pmj, defer, simple) and
gives a scene, make_config's keywords, the process options and the variant the launch plan must name. The table lives here so that
tests/test_unit_sweep_cases.py can show on the CPU, with the oracle and the library's host build alone, that the keys are exactly the compiled
variants and that no case passes emptily. `Case`, the bookkeeping of `add`, the bisection, the materials and the oracle's side are those of
tests/punct_parity_cases.py; the cameras are those of tests/projection_parity_cases.py.

Every case runs the precompiled megakernel of the contract: specialise = 0, wavefront = 0, arith = 0. Frames are 20 x 12 (neither side a multiple
of 8: every launch has lanes outside the frame), 4 spp, max_depth 4 to 6, rr_depth 2."""
import functools

import numpy as np

from akari_render_amd import abi, capi
from tests import launch_plan_matrix as M
from tests import projection_parity_cases as PP
from tests import punct_parity_cases as P
from tests.helpers import instanced_scene, textured_room
from tests.test_gpu_env_parity import _quad
from tests.test_gpu_pt_features import _env

W, H = 20, 12
KEY = ("kind", "env", "lens", "bvh", "stage", "fd", "tex", "pmj", "defer", "simple")
KINDS = ("plain", "kept", "feat")
UNITS = ((0, 0), (1, 0), (0, 1), (1, 1))  # (env, lens)
ROUTES = ((0, 1), (1, 1), (1, 0))         # (bvh, stage): exhaustive + staged, BVH + staged, BVH unstaged
# the options every case sets; DEFER and SIMPLE are off unless the case is there for them (pt_plan.cpp 31-60)
OFF = dict(wavefront=0, specialise=0, arith=0, defer_metal=0, simple_kernels=0, defer_on=1)
TEX_LENS = abi.LensData(0.05, 1.5)     # the textured room: focused on its back wall region, from inside
KEPT_LENS = abi.LensData(0.125, 4.0)   # the two blobs over their floor
# an orthographic film wider than the floor looks deep (and, like "ortho_lens", through the lens): its outer rays pass the floor into the sky
ORTHO_WIDE = (PP.PD(type=PP.ORTHO, ortho_scale=6.0), PP.LENS)

# Compiled variants that no scene reaches, each with the line of pt_plan.cpp that rules it out. Empty: every one of the 240 has a case below.
UNREACHED = []


def name_of(key):
    return f"{key[0]}-" + "-".join(f"{n}{v}" for n, v in zip(KEY[1:], key[1:]))


def plan_of(sd, cfg, opts, feat=False):
    """what the library decides on the host for a session of (sd, cfg) under `opts`, guides collected or not"""
    with capi.options(**opts):
        return capi.Scene(None, sd).features_plan(cfg, feat=feat, defer_metal=opts["defer_metal"], simple_kernels=opts["simple_kernels"], defer_on=opts["defer_on"],
                                                  wavefront=opts["wavefront"], arith=opts["arith"])


# ---------------------------------------------------------------------------------------------------------------- scenes
def _extras(sd, n):
    """`n` small quads on the floor in front of the box, each an instance with a diffuse material of its own: instance and material records
    for the BVH kernels to stage, or, past their budget, to read from memory (pt_plan.cpp 62-94)"""
    if n:
        sd.meshes.append(_quad((0, -0.98, 0), (0.12, 0, 0), (0, 0, -0.12)))
    for k in range(n):
        sd.materials.append(abi.MaterialData(kind=abi.MAT_DIFFUSE, base_color=(0.2 + 0.001 * k, 0.3 + 0.1 * (k % 7), 0.9 - 0.1 * (k % 5))))
        t = np.eye(4, dtype=np.float32)
        t[:3, 3] = [-2.4 + 0.3 * (k % 17), 0.0, 3.0 - 0.3 * ((k // 17) % 6)]
        sd.instances.append(abi.InstanceData(len(sd.meshes) - 1, [len(sd.materials) - 1], t.T.reshape(16).copy()))
    return sd


def floor_scene(box, floor, env, lens, projection=None, n_extra=0):
    """tests/punct_parity_cases.py's floor, box and wall under two emitters, without punctual lights. The wall is lowered to y = -0.5: on this
    wide frame the upper three rows then see the sky (the emitters at y = 1.6 keep the scene's box over the camera, as a lens with a tree needs)"""
    sd = P.lit_scene(box, [], emitters=2, env=_env() if env else None, floor=floor, lens=P.LENS if lens else None, w=W, h=H)
    sd.meshes[-1].vertices[2:, 1] = -0.5
    if projection is not None:
        PP.projected(sd, projection)
    return _extras(sd, n_extra)


def room_scene(env, lens, n_extra=0):
    """the textured room (20 triangles), with `n_extra` more shader graphs as launch_plan_matrix.textured_many_graphs adds them; with an
    environment the room loses its ceiling and its right wall, so that camera and bounce rays leave it"""
    sd = M.textured_many_graphs(n_extra, textured_room(W, H))
    sd.ggx_table = P._ggx()
    c2w = np.eye(4, dtype=np.float32)  # pitched down: on this wide frame a level camera sees neither the floor's graph nor its conductor lobe
    c2w[:3, :3], c2w[:3, 3] = P._rot(-0.4, 0.0), [0.0, 0.2, 0.95]
    sd.camera.c2w = c2w.T.reshape(16).copy()
    if env:
        sd.environment = _env()
        del sd.instances[5], sd.instances[3]
    sd.lens = TEX_LENS if lens else None
    return sd


def kept_scene(tex, env, lens):
    sd = instanced_scene(n_inst=2, n=4, width=W, height=H, textured=bool(tex))
    sd.ggx_table = P._ggx()
    if lens:
        sd = M.camera_inside(sd)
        sd.lens = KEPT_LENS
    sd.environment = _env() if env else None
    return sd


def _projection(kind, env, lens, bvh, stage, fd, tex, pmj):
    """the cases of the lens units that look through a projection instead: both cameras in either unit"""
    if not lens or kind == "kept" or tex:
        return None
    if (bvh, stage, fd, pmj) == (0, 1, 0, 0):
        return "panorama_window" if env else "ortho_lens"
    if (bvh, stage, fd, pmj) == (1, 1, 1, 1):
        return ORTHO_WIDE if env else "panorama_window"
    return None


def _materials(defer, simple):
    """(box, floor): glass keeps a scene from being SIMPLE; a conductor floor and wall are what DEFER puts off, and SIMPLE's principled material"""
    if simple:
        return ("diffuse", "rough_metal") if defer else ("mirror", "rough_metal")
    return ("glass", "rough_metal") if defer else ("glass", "diffuse")


def _scene(key, n_extra=None):
    kind, env, lens, bvh, stage, fd, tex, pmj, defer, simple = key
    if kind == "kept":
        return kept_scene(tex, env, lens)
    if n_extra is None:
        n_extra = unstaged_count(key) if (bvh, stage) == (1, 0) else 0
    if tex:
        return room_scene(env, lens, n_extra)
    return floor_scene(*_materials(defer, simple), env, lens, _projection(*key[:8]), n_extra)


def _stages(feat, sd, opts, cfg, stage):
    return plan_of(sd, cfg, opts, feat)["variant"]["stage"] == 1


@functools.lru_cache(maxsize=None)
def unstaged_count(key):
    """the smallest number of extra instances (tex = 0) or shader graphs (tex = 1) with which this case's session no longer stages its tables:
    found on the host by bisection, for the case's own config and options (a FEAT session's larger park block leaves less room)"""
    case = CASES[name_of(key)]
    return P.largest_count(lambda n: _scene(key, n), case.opts, case.config(), True, lo=0, hi=512, accepts=functools.partial(_stages, key[0] == "feat")) + 1


# ---------------------------------------------------------------------------------------------------------------- the table
CASES, KEYS = {}, {}


def _cfg(key):
    kind, env, lens, bvh, stage, fd, tex, pmj, defer, simple = key
    sampler = abi.SAMPLER_INDEPENDENT if not pmj else (abi.SAMPLER_SOBOL if (fd + tex + bvh + stage) % 2 == 0 else abi.SAMPLER_PMJ02BN)
    return dict(spp=4, spp_per_pass=2 if fd == pmj else 4, max_depth=4 + (fd + 2 * tex + bvh) % 3, rr_depth=2, force_diffuse=fd, sampler_type=sampler, sampler_seed=7)


def _opts(key):
    kind, env, lens, bvh, stage, fd, tex, pmj, defer, simple = key
    o = dict(OFF, force_bvh=int(bvh and kind != "kept"), instancing=int(kind == "kept"))
    if defer:  # a mask: hits on the marked materials are put off in iterations with (iteration & mask) != 0
        o["defer_metal"] = 3 if pmj else 1
        if bvh and tex:  # what the BVH kernels of textured scenes put off: graphs (2), conductors and graphs (3), conductors (1)
            o["defer_on"] = {(1, 0): 2, (1, 1): 3, (0, 0): 3, (0, 1): 1}[(stage, pmj)]
    o["simple_kernels"] = simple
    return o


def add(key):
    kind, env, lens, bvh, stage, fd, tex, pmj, defer, simple = key
    name, cfg, opts = name_of(key), _cfg(key), _opts(key)
    assert name not in CASES, name
    tags = ("kind:" + kind,) + (("feat",) if kind == "feat" else ()) + (("unstaged",) if kind != "kept" and (bvh, stage) == (1, 0) else ())
    tags += ("projection",) if _projection(*key[:8]) else ()
    want = P._want(opts, cfg, lens=bool(lens), punct=False, stage=bool(stage), bvh=bvh, inst=int(kind == "kept"), defer=defer, simple=simple, env=env, fd=fd, tex=tex)
    CASES[name] = P.Case(name, functools.partial(_scene, key), cfg, opts, want, tags)
    KEYS[name] = key
    return name


for _kind in KINDS:
    for _env_, _lens in UNITS:
        for _bvh, _stage in (ROUTES if _kind != "kept" else ((1, 0),)):
            for _fd in (0, 1):
                for _tex in (0, 1):
                    for _pmj in (0, 1):
                        add((_kind, _env_, _lens, _bvh, _stage, _fd, _tex, _pmj, 0, 0))
# DEFER and SIMPLE: full-graph kernels without environment, lens or guides. DEFER: the exhaustive kernels, and the BVH kernels of textured
# scenes; SIMPLE: scenes without textures; both: the exhaustive kernel of such a scene.
for _pmj in (0, 1):
    for _bvh, _stage, _tex in ((0, 1, 0), (0, 1, 1), (1, 1, 1), (1, 0, 1)):
        add(("plain", 0, 0, _bvh, _stage, 0, _tex, _pmj, 1, 0))
    for _bvh, _stage in ROUTES:
        add(("plain", 0, 0, _bvh, _stage, 0, 0, _pmj, 0, 1))
    add(("plain", 0, 0, 0, 1, 0, 0, _pmj, 1, 1))


def flags(case):
    """the kernel_flags the session must report: Case.flags and the bits it does not know (deferral, the guides; a kept scene's traversal does not set bit 0)"""
    return PP.flags(case) | (P.F_DEFER if case.want["defer"] else 0)


# ---------------------------------------------------------------------------------------------------------------- what a case's pixels see
def centre_hits(sd):
    """per pixel, the material its centre ray hits first (an index into sd.materials; -1: the ray leaves the scene), by the oracle's camera and tracer"""
    from oracle import pyoracle
    rays = PP.pixel_centre_rays(sd).astype(np.float32)
    r8 = np.concatenate([rays, np.zeros((len(rays), 1), np.float32), np.full((len(rays), 1), 1e20, np.float32)], axis=1)
    hit, _ = pyoracle.OracleScene(sd).intersect_many(r8)
    out = np.full(len(rays), -1, np.int64)
    for i, (h, inst, prim) in enumerate(hit):
        if h:
            slots = sd.meshes[sd.instances[inst].mesh].material_slots
            out[i] = sd.instances[inst].materials[int(slots[prim]) if slots is not None else 0]
    return out


def material_flags(sd, opts):
    """DMaterial.flags of every material of the scene, as the library folds them on the host"""
    with capi.options(**opts):
        f = capi.Scene(None, sd).array(capi.ARRAY_MATERIALS, np.uint32).reshape(-1, 64)[:, 1]
    assert len(f) == len(sd.materials)
    return f
