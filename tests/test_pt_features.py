"""Guides collected inside the pt pass, the part that needs no GPU: the new symbols and the `denoise_features` option, what
the launch plan decides for a session that collects guides -- the FEAT variant without DEFER and SIMPLE, the larger park block, the layout
within the workgroup's LDS share, the refusals -- and that the plan of every session that does not is what it was: every row of
tests/launch_plan_matrix.py through the new hook with feat = 0 against tests/golden/pt_launch_plan.json."""
import ctypes as C
import inspect
import json
import os

import pytest

from akari_render_amd import abi, capi
from tests import launch_plan_matrix as M
from tests.helpers import instanced_scene, make_config, textured_room

SAMPLERS = (abi.SAMPLER_INDEPENDENT, abi.SAMPLER_PMJ02BN, abi.SAMPLER_SOBOL)


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_symbols_option_and_bindings(hip_lib):
    for name in ("akr_pt_begin_features", "akr_pt_render_features", "akr_host_pt_features_plan"):
        assert hasattr(hip_lib, name), name
    assert "akr_pt_begin_features" in capi.EXPORTS and "akr_pt_render_features" in capi.EXPORTS and "akr_host_pt_features_plan" in capi.TEST_EXPORTS
    assert hip_lib.akr_pt_begin_features.argtypes is not None and len(hip_lib.akr_pt_begin_features.argtypes) == 7
    assert len(hip_lib.akr_pt_render_features.argtypes) == 7
    assert capi.get_option("denoise_features") == 0
    with capi.options(denoise_features=1):
        assert capi.get_option("denoise_features") == 1
    assert capi.get_option("denoise_features") == 0
    for bad in (-1, 2):
        with pytest.raises(capi.AkariError) as e:
            capi.set_option("denoise_features", bad)
        assert e.value.code == capi.ERR_INVALID_ARGUMENT
    sig = inspect.signature(capi.PtSession.__init__)
    assert list(sig.parameters)[-2:] == ["albedo", "normal"] and sig.parameters["albedo"].default is None and sig.parameters["normal"].default is None
    assert list(inspect.signature(capi.pt_render_features).parameters) == ["ctx", "scene", "cfg", "film", "albedo", "normal"]


def test_no_device_no_guides(hip_lib):
    """a NULL context and a host-only scene are refused with the unsupported status, before the other arguments are looked at"""
    scene = capi.Scene(None, M.cbox())
    cfg = make_config(spp=4)
    h = C.c_void_p(1)
    assert hip_lib.akr_pt_begin_features(None, scene.h, C.byref(cfg), None, None, None, C.byref(h)) == capi.ERR_UNSUPPORTED
    assert not h.value and "host-only" in capi.last_error()
    assert hip_lib.akr_pt_render_features(None, scene.h, C.byref(cfg), None, None, None, None) == capi.ERR_UNSUPPORTED
    assert hip_lib.akr_pt_begin_features(None, scene.h, C.byref(cfg), None, None, None, None) == capi.ERR_INVALID_ARGUMENT
    scene.close()


# ---------------------------------------------------------------------------------------------------------------- plan
def _scene(sd, **opts):
    with capi.options(**(opts or M.FLAT)):
        return capi.Scene(None, sd)


@pytest.mark.parametrize("name", ["cbox", "cbox_force_bvh", "one_metal", "tex_exhaustive", "tex_tree", "tex_tree_unstaged"])
@pytest.mark.parametrize("env,lens", [(0, 0), (1, 0), (0, 1), (1, 1)], ids=["plain", "env", "lens", "lens_env"])
def test_feature_plan(hip_lib, name, env, lens):
    build, opts, tex = {**M.BASE_SCENES, **M.EXTRA_SCENES}[name]
    sd = M.camera_inside(build()) if lens else build()
    sd.environment = M.ENV if env else None
    sd.lens = M.LENS if lens else None
    scene = _scene(sd, **opts)
    for fd in (0, 1):
        for s in SAMPLERS:
            for spec_waves in (0, 3):
                cfg = make_config(spp=4, force_diffuse=fd, sampler_type=s)
                plain = scene.features_plan(cfg, feat=False, spec_waves=spec_waves)
                plan = scene.features_plan(cfg, feat=True, spec_waves=spec_waves)
                v, pv = plan["variant"], plain["variant"]
                assert v["feat"] == 1 and pv["feat"] == 0
                assert v["defer"] == 0 and v["simple"] == 0 and plan["defer_metal"] == 0 and plan["simple_scene"] == 0
                assert plan["kernel_compiled"] == 1 and plan["specialised"] == 0 and plan["wrapper"] == ""
                for k in ("bvh", "fd", "tex", "pmj", "inst", "env", "lens"):
                    assert v[k] == pv[k], k
                assert v["env"] == env and v["lens"] == lens and v["inst"] == 0
                # the park block: kParkSlotsFeat columns where the kernel parks (full-graph kernels of scenes with textures), none elsewhere
                parks = v["tex"] == 1 and v["fd"] == 0
                assert plan["park_slots_feat"] == 19
                assert plan["park_slots"] == (19 if parks else 0), (plan["park_slots"], parks)
                assert plan["carry_offset"] - plan["park_offset"] == plan["park_slots"] * 256
                assert plan["required_bytes"] <= plan["lds_budget"] == (53 if v["tex"] else 40) * 1024
                assert plan["required_bytes"] <= plan["lds_bytes"]
                if not v["bvh"]:
                    assert v["stage"] == 1  # the exhaustive kernels always stage
    scene.close()


def test_defer_and_simple_give_way(hip_lib):
    """scenes whose plain session runs a DEFER or a SIMPLE kernel: the feature session runs neither"""
    cfg = make_config(spp=4)
    one_metal = _scene(M.one_metal())
    assert one_metal.features_plan(cfg, feat=False)["variant"]["defer"] == 1
    assert one_metal.features_plan(cfg)["variant"]["defer"] == 0
    cbox = _scene(M.cbox())
    assert cbox.features_plan(cfg, feat=False)["variant"]["simple"] == 1
    assert cbox.features_plan(cfg)["variant"]["simple"] == 0
    tex = _scene(textured_room(32, 32, n_floor=8))
    assert tex.features_plan(cfg, feat=False, defer_metal=1)["variant"]["defer"] == 1
    assert tex.features_plan(cfg, defer_metal=1)["variant"]["defer"] == 0
    for s in (one_metal, cbox, tex):
        s.close()


def test_refusals_are_decided_on_the_host(hip_lib):
    cfg = make_config(spp=4)
    kept = _scene(instanced_scene(n_inst=2, n=4, width=32, height=32), force_bvh=0, instancing=1)
    flat = _scene(M.cbox())
    for scene, kw, word in ((kept, {}, "instances"), (flat, dict(wavefront=1), "wavefront"), (flat, dict(arith=1), "arith")):
        with pytest.raises(capi.AkariError) as e:
            scene.features_plan(cfg, **kw)
        assert e.value.code == capi.ERR_UNSUPPORTED and word in str(e.value), str(e.value)
        assert scene.features_plan(cfg, feat=False, **kw)["variant"]["feat"] == 0  # the same options without guides: a plan as ever
    assert flat.features_plan(cfg, wavefront=-1)["variant"]["feat"] == 1
    assert flat.features_plan(cfg, wavefront=0)["variant"]["feat"] == 1
    kept.close()
    flat.close()


# ---------------------------------------------------------------------------------------------------------------- sessions without guides
def test_every_recorded_plan_without_guides_is_unchanged(hip_lib, root):
    """feat = 0 through the new hook: variant and layout of every row of the matrix are the recorded ones"""
    golden = json.load(open(os.path.join(root, "tests", "golden", "pt_launch_plan.json")))
    names = list(abi.PtLaunchPlan.VARIANT) + list(M.FIELDS) + [f"stage_bytes[{i}]" for i in range(13)] + ["wrapper"]
    bad, n = [], 0
    for sname, scene, tex in M.scenes():
        for key, cfg, opts in M.cases(tex):
            plan = scene.features_plan(cfg, feat=False, **opts)
            assert plan["variant"]["feat"] == 0
            want = golden["plans"][golden["rows"][f"{sname}/{key}"]]
            bad += [f"{sname}/{key}: {f} = {a}, recorded {b}" for f, a, b in zip(names, M.flatten(plan), want) if a != b]
            n += 1
        scene.close()
    assert n == len(golden["rows"]) and n >= 300
    assert not bad, f"{len(bad)} fields differ:\n" + "\n".join(bad[:40])
