"""Procedural shader nodes on the GPU: the device's evaluation against the host build and the numpy model, bit for bit; graphs
wrapped in exact identities against the oracle's render of the unwrapped scene; one procedural scene through every route a pt session can take,
and the aov albedo pass against the model."""
import os

import numpy as np
import pytest

from akari_render_amd import abi, capi
from tests import procedural_cases as PC
from tests import procedural_model as M
from tests import punct_parity_cases as P
from tests.helpers import make_config, n_bit_diff, textured_room

pytestmark = pytest.mark.gpu

F = np.float32
N = abi.NodeData
COUNTERS = ("n_samples", "n_closest", "n_shadow", "n_shaded")


def _table(root):
    return np.fromfile(os.path.join(root, "tests", "golden", "ggx_dielectric_s.f32"), dtype=np.float32)


def _render(ctx, sd, cfg, opts):
    """one pt session to its end under `opts` -> (film, counters, final sampler states, kernel info, scene info)"""
    w, h = sd.camera.width, sd.camera.height
    with capi.options(**opts):
        scene = capi.Scene(ctx, sd)
        film = capi.Film(ctx, w, h)
        se = capi.PtSession(ctx, scene, cfg, film)
        info = se.kernel_info()
        se.passes((cfg.spp + cfg.spp_per_pass - 1) // cfg.spp_per_pass, blocking=True)
        states = se.sampler_states(w * h)
        st = se.end()
    return film.read(), st, states, info, scene.info()


# ---------------------------------------------------------------------------------------------- device against host against model
@pytest.fixture(scope="module")
def probe(ctx):
    sd, index, cases = PC.probe_scene()
    return capi.Scene(ctx, sd), index, cases, PC.probe_points()


def test_device_evaluation_equals_host_and_model(ctx, probe):
    scene, index, cases, uv = probe
    device_pow = lambda a, b: capi.probe_math2(ctx, np.ravel(a), np.ravel(b))[:, 1].reshape(np.shape(a))  # noqa: E731
    host_pow = PC.host_pow(scene, index["pow"])
    assert np.all(M.bits_equal(device_pow(uv[:, 0], uv[:, 1]), host_pow(uv[:, 0], uv[:, 1])))  # the two builds of pow_f, where the model takes POW from
    for name, m in index.items():
        d, h = capi.probe_material_inputs(ctx, scene, m, uv), capi.probe_material_inputs(None, scene, m, uv)
        assert np.all(M.bits_equal(d, h)), f"{name}: device vs host build, {np.count_nonzero(~M.bits_equal(d, h))} words"
        if name.startswith("math-"):
            want = PC.math_expected(cases[name], uv, device_pow)
        elif name.startswith("noise-"):
            want = PC.noise_expected(cases[name], uv)
        else:
            continue
        assert np.all(M.bits_equal(d[:, 1:5], want)), f"{name}: device vs model, {np.count_nonzero(~M.bits_equal(d[:, 1:5], want))} words"
    assert np.all(M.bits_equal(capi.probe_material_inputs(ctx, scene, index["fbm"], uv)[:, 6], PC.fbm_expected(uv)))


# ---------------------------------------------------------------------------------------------- identity graphs against the oracle
def _wrap_in_identities(sd, start):
    """Every texture-fed input of the room through a chain of all four exact identities, mul(x, 1), add(x, -0.0), div(x, 1), max(x, x), in an
    order that turns with the input and with `start`."""
    k = start
    for m in sd.materials:
        if m.graph is None:
            continue
        for name in list(m.graph.inputs):
            x = m.graph.inputs[name]
            for j in range(4):
                which, b = (k + j) % 4, len(m.graph.nodes)
                if which == 3:
                    m.graph.nodes.append(abi.math(abi.MATH_MAX, x, x, 0))
                else:
                    op, c = ((abi.MATH_MUL, 1.0), (abi.MATH_ADD, -0.0), (abi.MATH_DIV, 1.0))[which]
                    m.graph.nodes += [N(abi.NODE_CONST, (), (c, 0.0, 0.0)), abi.math(op, x, b, abi.MATH_BROADCAST_SECOND)]
                x = len(m.graph.nodes) - 1
            m.graph.inputs[name] = x
            k += 1
    return sd


@pytest.mark.parametrize("sampler", [abi.SAMPLER_INDEPENDENT, abi.SAMPLER_PMJ02BN], ids=["independent", "pmj02bn"])
@pytest.mark.parametrize("kernel", ["exhaustive", "bvh"])
def test_identity_wrapped_room_renders_the_oracles_film(ctx, root, kernel, sampler):
    plain = textured_room(32, 24)
    plain.ggx_table = _table(root)
    wrapped = _wrap_in_identities(textured_room(32, 24), start=(kernel == "bvh") + 2 * (sampler != abi.SAMPLER_INDEPENDENT))
    wrapped.ggx_table = plain.ggx_table
    assert sum(n.op == abi.NODE_MATH for m in wrapped.materials if m.graph is not None for n in m.graph.nodes) == 24
    cfg = make_config(spp=4, spp_per_pass=2, max_depth=8, sampler_type=sampler, sampler_seed=5)
    g, gst, gstates, info, sinfo = _render(ctx, wrapped, cfg, dict(force_bvh=int(kernel == "bvh"), instancing=0, wavefront=0, specialise=0))
    assert bool(sinfo.uses_bvh) == (kernel == "bvh") and info["specialised"] == 0
    o, ost, ostates = P.oracle_render(plain, cfg)
    assert n_bit_diff(g, o) == 0, f"{n_bit_diff(g, o)} of {g.size} film floats differ"
    assert all(gst[c] == ost[c] for c in COUNTERS) and np.array_equal(gstates, ostates)


# ---------------------------------------------------------------------------------------------- routes
ROUTES = {
    "interpreter": dict(force_bvh=0, instancing=0, wavefront=0, specialise=0),
    "interpreter-bvh": dict(force_bvh=1, instancing=0, wavefront=0, specialise=0),
    "per-scene": dict(force_bvh=0, instancing=0, wavefront=0, specialise=1),
    "wavefront": dict(force_bvh=1, instancing=0, wavefront=1, specialise=0),
    "kept": dict(force_bvh=1, instancing=1, wavefront=0, specialise=0),
}


@pytest.fixture(scope="module")
def routes_reference(ctx, root):
    sd = PC.routes_room(32, 24)
    sd.ggx_table = _table(root)
    cfg = make_config(spp=4, spp_per_pass=2, max_depth=8, sampler_seed=3)
    return sd, cfg, _render(ctx, sd, cfg, ROUTES["interpreter"])


@pytest.mark.parametrize("route", [r for r in ROUTES if r != "interpreter"])
def test_routes_agree(ctx, routes_reference, route, tmp_path, monkeypatch):
    sd, cfg, (ref, rst, rstates, rinfo, _) = routes_reference
    assert rinfo["specialised"] == 0
    monkeypatch.setenv("AKR_KERNEL_CACHE", str(tmp_path / "cache"))  # a per-scene kernel is compiled here, not found
    g, gst, gstates, info, sinfo = _render(ctx, sd, cfg, ROUTES[route])
    assert info["specialised"] == (1 if route == "per-scene" else 0), info
    if route == "per-scene":
        assert info["status"] == "ok" and info["cache_hit"] == 0
    assert ("wavefront" in info["status"]) == (route == "wavefront"), info
    if route == "kept":
        assert sinfo.uses_bvh == 2
    assert n_bit_diff(g, ref) == 0, f"{route}: {n_bit_diff(g, ref)} of {g.size} film floats differ from the interpreter's"
    assert all(gst[c] == rst[c] for c in COUNTERS) and np.array_equal(gstates, rstates)
    n = 32 * 24
    img = ref[: 3 * n].reshape(24, 32, 3) / np.maximum(ref[6 * n:].reshape(24, 32, 1), 1)
    assert np.all(np.isfinite(ref)) and img[4:20, 8:24].std(axis=(0, 1)).min() > 0.01  # the back wall's pattern is in the film


def test_aov_albedo_is_the_models_base_colour(ctx, routes_reference):
    """The albedo pass through the pixel centres (box filter of radius 0, 1 spp): on the back wall, the model's c1 + (c2 - c1) clamp(0.5 noise + 0.5)
    at the uv the device's own surface interaction reports for the hit."""
    sd = routes_reference[0]
    w, h = sd.camera.width, sd.camera.height
    with capi.options(force_bvh=1, instancing=0):
        scene = capi.Scene(ctx, sd)
        cfg = abi.AovConfig.default()
        cfg.spp, cfg.aov, cfg.remap, cfg.filter_type, cfg.filter_radius = 1, abi.AOV_ALBEDO, 0, abi.FILTER_BOX, 0.0
        film = capi.Film(ctx, w, h)
        capi.aov_render(ctx, scene, cfg, film)
        got = film.read()[: 3 * w * h].reshape(w * h, 3)
        px = np.stack(np.meshgrid(np.arange(w), np.arange(h)), -1).reshape(-1, 2).astype(np.uint32)
        half = np.full((w * h, 2), 0.5, F)
        r = scene.host_lens_ray(px, half, half, abi.FILTER_BOX, 0.0)
        hit, bary = capi.probe_intersect(ctx, scene, np.c_[r, np.zeros(w * h, F), np.full(w * h, 1e20, F)])
        assert np.all(hit[:, 0] == 1)
        si = capi.probe_surface_interaction(ctx, scene, hit[:, 1:3], bary)
    wall = si[:, 18] == 1.0
    assert np.count_nonzero(wall) > 100
    want = PC.base_color_expected(si[wall, 15:17], PC.COL1 + (1.0,), PC.COL2 + (1.0,))[:, :3]
    assert np.all(M.bits_equal(got[wall], want)), f"{np.count_nonzero(~M.bits_equal(got[wall], want))} of {want.size} floats differ"
    assert len(np.unique(want[:, 0])) > 50  # (a pattern, not a constant)
