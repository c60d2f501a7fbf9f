"""What keeps tests/test_gpu_unit_sweep.py from passing emptily, checked without a GPU. The table of tests/unit_sweep_cases.py names exactly the
240 compiled pt variants without punctual lights (the rule of kernels.h pt_variant_compiled, restated here), the library's host plan names the
wanted variant for every case, and the oracle alone shows that what a case is there for reaches its film: the environment, the lens or the
projection, force_diffuse, the materials DEFER puts off, SIMPLE's principled material, the staging budget just crossed, the guides."""
import dataclasses
import itertools

import numpy as np
import pytest

from akari_render_amd import abi
from oracle import pyoracle
from tests import punct_parity_cases as P
from tests import unit_sweep_cases as U
from tests.test_gpu_punct_parity import _aov_cfg
from tests.test_punct_parity_cases import _fraction

FLAGS = ("bvh", "fd", "tex", "pmj", "stage", "defer", "simple", "inst", "env", "lens", "feat", "punct", "ltree")
# per (env, lens) unit: the plain unit without either also holds the 16 DEFER / SIMPLE kernels
COUNTS = {"plain": {(0, 0): 40, (1, 0): 24, (0, 1): 24, (1, 1): 24}, "kept": dict.fromkeys(U.UNITS, 8), "feat": dict.fromkeys(U.UNITS, 24)}


def compiled(bvh, fd, tex, pmj, stage, defer, simple, inst, env, lens, feat, punct, ltree):
    """kernels.h pt_variant_compiled"""
    return bool((bvh or stage) and not (defer and (fd or (bvh and not tex))) and not (simple and (fd or tex)) and not ((env or lens or feat or punct) and (defer or simple))
                and not (inst and not (bvh and not stage and not defer and not simple and not feat)) and not (punct and (feat or inst)) and not (ltree and not punct))


def compiled_keys():
    """the key of every compiled variant with punct = 0, as a list (a duplicate would be a mistake of this function)"""
    out = []
    for bits in itertools.product((0, 1), repeat=len(FLAGS)):
        v = dict(zip(FLAGS, bits))
        if v["punct"] or not compiled(**v):
            continue
        assert not v["ltree"]
        kind = "kept" if v["inst"] else ("feat" if v["feat"] else "plain")
        out.append((kind,) + tuple(v[k] for k in U.KEY[1:]))
    return out


def test_the_rule_counts_432():
    n = sum(compiled(*bits) for bits in itertools.product((0, 1), repeat=len(FLAGS)))
    assert n == 432 and len(compiled_keys()) == 240


def test_the_table_names_every_compiled_variant_once():
    want = compiled_keys()
    assert len(want) == len(set(want)) == 240
    keys = list(U.KEYS.values())
    unreached = [u[0] for u in U.UNREACHED]
    assert all(isinstance(u[1], str) and "pt_plan.cpp" in u[1] for u in U.UNREACHED)  # (key, the line that rules it out)
    assert len(keys) == len(set(keys)) and len(unreached) == len(set(unreached)) and not set(keys) & set(unreached)
    assert set(keys) | set(unreached) == set(want) and len(keys) + len(unreached) == 240
    assert unreached == []  # every compiled variant is reached by a scene
    for kind in U.KINDS:
        for unit in U.UNITS:
            assert sum(1 for k in want if (k[0],) + k[1:3] == (kind,) + unit) == COUNTS[kind][unit], (kind, unit)
            assert sum(1 for k in keys + unreached if (k[0],) + k[1:3] == (kind,) + unit) == COUNTS[kind][unit], (kind, unit)
    assert sum(sum(c.values()) for c in COUNTS.values()) == 240 and sum(COUNTS["plain"].values()) == 112
    assert list(U.CASES) == [U.name_of(k) for k in keys]


def test_every_unit_has_both_index_samplers_and_a_split_pass():
    for kind in U.KINDS:
        for unit in U.UNITS:
            cfgs = [U.CASES[n].cfg for n, k in U.KEYS.items() if (k[0],) + k[1:3] == (kind,) + unit]
            assert {abi.SAMPLER_SOBOL, abi.SAMPLER_PMJ02BN, abi.SAMPLER_INDEPENDENT} == {c["sampler_type"] for c in cfgs}, (kind, unit)
            assert any(c["spp_per_pass"] < c["spp"] for c in cfgs) and any(c["spp_per_pass"] == c["spp"] for c in cfgs), (kind, unit)
            assert all(c["spp"] == 4 and 4 <= c["max_depth"] <= 6 and c["rr_depth"] == 2 for c in cfgs)
    for unit in ((0, 1), (1, 1)):  # the plain lens units: both projections
        tagged = [n for n, k in U.KEYS.items() if k[:3] == ("plain",) + unit and "projection" in U.CASES[n].tags]
        assert {U.CASES[n].scene().projection.type for n in tagged} == {abi.PROJECTION_ORTHOGRAPHIC, abi.PROJECTION_PANORAMA}, unit


def _colour(film, n):
    return film[:3 * n]


@pytest.mark.parametrize("name", list(U.CASES))
def test_case_is_what_it_claims(hip_lib, name):
    case, key = U.CASES[name], U.KEYS[name]
    kind, env, lens, bvh, stage, fd, tex, pmj, defer, simple = key
    sd, cfg = case.scene(), case.config()
    w, h = sd.camera.width, sd.camera.height
    n = w * h
    assert (w, h) == (U.W, U.H) and w % 8 and h % 8
    assert (case.opts["specialise"], case.opts["wavefront"], case.opts["arith"]) == (0, 0, 0)
    plan = U.plan_of(sd, cfg, case.opts, feat=kind == "feat")
    v = plan["variant"]
    assert {k: v[k] for k in case.want} == case.want, (v, case.want)
    assert v["feat"] == int(kind == "feat") and v["punct"] == 0 and plan["kernel_compiled"] == 1 and plan["specialised"] == 0
    assert tuple(v[k] for k in U.KEY[1:]) == key[1:] and v["inst"] == int(kind == "kept")
    assert bool(U.flags(case) & P.F_FEAT) == (kind == "feat") and bool(U.flags(case) & P.F_DEFER) == bool(defer)

    film, st, _ = P.oracle_render(sd, cfg)
    assert np.all(np.isfinite(film)) and np.any(_colour(film, n) != 0)
    hits = U.centre_hits(sd)
    if env:
        assert sd.environment is not None and sd.environment.image is not None
        dark = P.oracle_render(dataclasses.replace(sd, environment=None), cfg)[0]
        assert _fraction(film, dark) >= 0.25, f"the environment changes {_fraction(film, dark):.3f} of the film's floats"
        assert (hits < 0).sum() >= 20, f"{(hits < 0).sum()} centre rays leave the scene"
    else:
        assert sd.environment is None
    if lens:
        if "projection" in case.tags:
            assert sd.projection is not None and sd.projection.type != abi.PROJECTION_PERSPECTIVE
            other = P.oracle_render(dataclasses.replace(sd, projection=None, lens=None), cfg)[0]
        else:
            assert sd.lens is not None and getattr(sd, "projection", None) is None
            other = P.oracle_render(sd, cfg, lens=False)[0]
        assert _fraction(film, other) >= 0.25, f"the lens / projection changes {_fraction(film, other):.3f} of the film's floats"
    else:
        assert sd.lens is None and getattr(sd, "projection", None) is None
    if fd:
        c0 = cfg.copy()
        c0.force_diffuse = 0
        full = P.oracle_render(sd, c0)[0]
        assert _fraction(film, full) >= 0.25, f"force_diffuse changes {_fraction(film, full):.3f} of the film's floats"
    if defer:
        marked = np.flatnonzero(U.material_flags(sd, case.opts) & plan["defer_flags"])
        assert plan["defer_metal"] == case.opts["defer_metal"] != 0 and len(marked)
        assert np.isin(hits, marked).sum() >= 20, f"{np.isin(hits, marked).sum()} centre rays hit a material DEFER puts off"
        assert (~np.isin(hits, marked) & (hits >= 0)).sum() >= 20  # ... and as many hit one it does not: both branches run
    else:
        assert plan["defer_metal"] == 0
    if simple:
        principled = [i for i, m in enumerate(sd.materials) if m.kind == abi.MAT_PRINCIPLED]
        assert plan["simple_scene"] == 1 and np.isin(hits, principled).sum() >= 20
    if "unstaged" in case.tags:
        count = U.unstaged_count(key)
        assert count >= 1 and len(sd.instances) == len(U._scene(key, 0).instances) + count
        below = U.plan_of(U._scene(key, count - 1), cfg, case.opts, feat=kind == "feat")
        assert v["stage"] == 0 and plan["stage_total"] == 0 and below["variant"]["stage"] == 1 and below["stage_total"] > 0
    if kind == "feat":
        osc = pyoracle.OracleScene(sd)
        for aov in (abi.AOV_ALBEDO, abi.AOV_NS):
            g = _colour(osc.aov_render(_aov_cfg(cfg, aov))[0], n)
            assert np.count_nonzero(g) >= 0.25 * g.size, (aov, np.count_nonzero(g) / g.size)
