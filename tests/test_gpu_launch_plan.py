"""A pt session runs the kernel variant that the launch plan names, in each of the eight plain and kept units of the pt kernels
(csrc/pt_unit_kernels.hip; kernels.h PtKind): flattened, with an environment light, through a lens, both, a kept scene, kept with an
environment, kept through a lens, kept with both, and a textured scene with a per-scene kernel. (The twelve units of sessions that collect
guides, of punctual lights and of the light tree: tests/test_gpu_pt_features.py, test_gpu_punct_parity.py, test_gpu_light_tree.py.) Every session renders 32 x 32 at 4 spp; akr_pt_kernel_info's kernel_flags and `specialised` equal what
akr_host_pt_launch_plan predicts for the same scene, config and options on a host-only scene (tests/test_launch_plan.py holds those
predictions to the recorded decisions), and the film is the CPU oracle's bit for bit. The sessions through a lens are held bit for bit to the same scene rendered by the
other kind's lens unit (flattened against kept), as tests/test_gpu_lens.py does, and both to the oracle's lens. This file holds one instantiation
of each unit; every one of the 432 is swept against the oracle elsewhere: the 240 plain, kept and FEAT kernels in tests/test_gpu_unit_sweep.py,
the 96 PUNCT kernels in tests/test_gpu_punct_parity.py, the 96 light-tree kernels in tests/test_gpu_light_tree_parity.py."""
import os

import numpy as np
import pytest

from akari_render_amd import abi, capi
from oracle import pyoracle
from tests import launch_plan_matrix as M
from tests.helpers import instanced_scene, make_config, n_bit_diff, textured_room
from tests.test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu

CFG = dict(spp=4, spp_per_pass=4, max_depth=6)
FLAT = dict(force_bvh=0, instancing=0, wavefront=0, specialise=0, arith=0)
KEPT = dict(force_bvh=0, instancing=1, wavefront=0, specialise=0, arith=0)


def _ggx(root):
    return np.fromfile(os.path.join(root, "tests", "golden", "ggx_dielectric_s.f32"), dtype=np.float32)


def _two_instances(root, env=False, lens=False):
    sd = instanced_scene(n_inst=2, n=4, width=32, height=32)
    sd.ggx_table = _ggx(root)
    if lens:
        sd = M.camera_inside(sd)
        sd.lens = abi.LensData(0.0625, 4.0)
    sd.environment = M.ENV if env else None
    return sd


def _session(ctx, sd, cfg, opts):
    """(film, stats, kernel_info) of a session under `opts`, after the plan's prediction for it has been checked"""
    with capi.options(**opts):
        plan = capi.Scene(None, sd).launch_plan(cfg, defer_metal=capi.get_option("defer_metal"), simple_kernels=capi.get_option("simple_kernels"),
                                                defer_on=capi.get_option("defer_on"), spec_waves=3 if opts["specialise"] else 0)
        scene = capi.Scene(ctx, sd)
        film = capi.Film(ctx, sd.camera.width, sd.camera.height)
        se = capi.PtSession(ctx, scene, cfg, film)
        se.passes(1, blocking=True)
        info = se.kernel_info()
        st = se.end()
    v = plan["variant"]
    flags = (1 if v["bvh"] and not v["inst"] else 0) | (2 if v["pmj"] else 0) | (4 if v["stage"] else 0) | (8 if v["defer"] else 0) | (32 if v["lens"] else 0)
    assert info["kernel_flags"] == flags, (info, plan)
    assert info["specialised"] == plan["specialised"], (info, plan)
    return film.read(), st, v


def _against_oracle(ctx, sd, cfg, opts, want):
    g, gst, v = _session(ctx, sd, cfg, opts)
    assert {k: v[k] for k in want} == want, v  # the session is the one this case is here for
    if cfg.sampler_type != abi.SAMPLER_INDEPENDENT:
        pyoracle.set_pmj_tables(*capi.host_pmj02bn_tables())
    o, ost = pyoracle.OracleScene(sd).render(cfg)
    assert_parity(g, o, sd.camera.width, sd.camera.height, gst, ost)


def test_flattened(ctx):
    _against_oracle(ctx, M.cbox(), make_config(**CFG), FLAT, dict(bvh=0, inst=0, env=0, lens=0, stage=1))


def test_environment(ctx):
    sd = M.cbox()
    sd.environment = M.ENV
    _against_oracle(ctx, sd, make_config(sampler_type=abi.SAMPLER_PMJ02BN, **CFG), FLAT, dict(inst=0, env=1, lens=0, pmj=1, defer=0, simple=0))


def test_kept(ctx, root):
    _against_oracle(ctx, _two_instances(root), make_config(**CFG), KEPT, dict(bvh=1, inst=1, env=0, lens=0, stage=0))


def test_kept_environment(ctx, root):
    _against_oracle(ctx, _two_instances(root, env=True), make_config(sampler_type=abi.SAMPLER_SOBOL, **CFG), KEPT, dict(inst=1, env=1, lens=0, pmj=1))


def test_textured_per_scene_kernel(ctx, root):
    sd = textured_room(32, 32)
    sd.ggx_table = _ggx(root)
    _against_oracle(ctx, sd, make_config(**CFG), dict(FLAT, specialise=1), dict(tex=1, fd=0, inst=0, env=0, lens=0))


@pytest.mark.parametrize("env", [False, True], ids=["lens", "lens_env"])
def test_lens_flattened_and_kept(ctx, root, env):
    """the units plain + LENS / plain + ENV + LENS against kept + LENS / kept + ENV + LENS and both against the oracle, and the lens does reach the film"""
    sd, cfg = _two_instances(root, env=env, lens=True), make_config(**CFG)
    flat, fst, fv = _session(ctx, sd, cfg, FLAT)
    kept, kst, kv = _session(ctx, sd, cfg, KEPT)
    assert (fv["inst"], fv["env"], fv["lens"]) == (0, int(env), 1) and (kv["inst"], kv["env"], kv["lens"]) == (1, int(env), 1)
    assert n_bit_diff(flat, kept) == 0, f"{n_bit_diff(flat, kept)} of {flat.size} film floats differ"
    assert all(fst[k] == kst[k] for k in ("n_samples", "n_closest", "n_shadow", "n_shaded"))
    o, ost = pyoracle.OracleScene(sd).render(cfg)
    assert_parity(flat, o, sd.camera.width, sd.camera.height, fst, ost)
    assert_parity(kept, o, sd.camera.width, sd.camera.height, kst, ost)
    sd.lens = None
    pin, _, _ = _session(ctx, sd, cfg, FLAT)
    assert n_bit_diff(pin, flat) > 0
