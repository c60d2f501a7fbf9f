"""Every precompiled pt kernel without punctual lights on the GPU against the CPU oracle, bit for bit: the 240 instantiations of the plain, kept
(k_pt_pass_inst) and FEAT kinds, one case each (tests/unit_sweep_cases.py; with the 96 PUNCT kernels of tests/test_gpu_punct_parity.py and the 96
light-tree kernels of tests/test_gpu_light_tree_parity.py these are the 432 of csrc/pt_unit_kernels.hip). A case asserts the kernel it ran -- the
host plan's variant, which the session follows, and the session's kernel_flags -- and holds the raw film, the ray counters and the final sampler
states to the oracle's. A FEAT case also holds its two guide films to the oracle's aov films. tests/test_unit_sweep_cases.py shows on the CPU
that the table is complete and that no case passes emptily. Every case is 20 x 12 pixels at 4 spp."""
import numpy as np
import pytest

from akari_render_amd import abi, capi
from oracle import pyoracle
from tests import punct_parity_cases as P
from tests import unit_sweep_cases as U
from tests.helpers import n_bit_diff
from tests.test_gpu_parity import assert_parity
from tests.test_gpu_punct_parity import _aov_cfg, check

pytestmark = pytest.mark.gpu


def feat_render(ctx, sd, cfg, opts):
    """test_gpu_punct_parity.gpu_render for a session with two guide films -> (film, albedo, normal, counters, final sampler states, kernel info)"""
    w, h = sd.camera.width, sd.camera.height
    with capi.options(**opts):
        scene = capi.Scene(ctx, sd)
        film, albedo, normal = (capi.Film(ctx, w, h) for _ in range(3))
        se = capi.PtSession(ctx, scene, cfg, film, albedo, normal)
        se.passes(1000, blocking=True)
        states = se.sampler_states(w * h)
        info = se.kernel_info()
        st = se.end()
    return film.read(), albedo.read(), normal.read(), st, states, info


def feat_check(ctx, case):
    """`check` for a FEAT case, and the guides: the oracle's aov albedo and shading normal of the same samples, weights as the colour film's"""
    sd, cfg = case.scene(), case.config()
    w, h = sd.camera.width, sd.camera.height
    n = w * h
    v = U.plan_of(sd, cfg, case.opts, feat=True)["variant"]
    assert {k: v[k] for k in case.want} == case.want and v["feat"] == 1, (v, case.want)
    g, albedo, normal, gst, gstates, info = feat_render(ctx, sd, cfg, case.opts)
    assert info["kernel_flags"] == U.flags(case) and info["specialised"] == 0, (info, U.flags(case))
    o, ost, ostates = P.oracle_render(sd, cfg)
    assert_parity(g, o, w, h, gst, ost)
    assert np.array_equal(gstates, ostates), f"{np.count_nonzero(gstates != ostates)} sampler state words differ"
    assert np.array_equal(albedo[6 * n:], g[6 * n:]) and np.array_equal(normal[6 * n:], g[6 * n:])
    if cfg.sampler_type == abi.SAMPLER_INDEPENDENT:
        # PCG32: pt draws what aov draws only with the camera's dimensions alone and in one pass (test_gpu_pt_features.py
        # test_guides_equal_aov_independent): a second session of the same scene, which runs the same instantiation
        cfg = cfg.copy()
        cfg.max_depth, cfg.spp_per_pass = 0, cfg.spp
        v0 = U.plan_of(sd, cfg, case.opts, feat=True)["variant"]
        assert v0 == v, (v0, v)
        g, albedo, normal, gst, gstates, info = feat_render(ctx, sd, cfg, case.opts)
        assert info["kernel_flags"] == U.flags(case) and info["specialised"] == 0 and gst["n_shaded"] == 0, (info, gst)
        o, ost, ostates = P.oracle_render(sd, cfg)
        assert_parity(g, o, w, h, gst, ost)
        assert np.array_equal(gstates, ostates) and np.array_equal(albedo[6 * n:], g[6 * n:]) and np.array_equal(normal[6 * n:], g[6 * n:])
    osc = pyoracle.OracleScene(sd)
    for name, guide, aov in (("albedo", albedo, abi.AOV_ALBEDO), ("ns", normal, abi.AOV_NS)):
        want = osc.aov_render(_aov_cfg(cfg, aov))[0]
        assert n_bit_diff(guide, want) == 0, f"{name}: {n_bit_diff(guide, want)} of {guide.size} floats differ from the oracle's aov film"


@pytest.mark.parametrize("name", list(U.CASES))
def test_kernel(ctx, name):
    case = U.CASES[name]
    if "feat" in case.tags:
        feat_check(ctx, case)
    else:
        check(ctx, case.scene(), case.config(), case.opts, U.flags(case), case.want)
