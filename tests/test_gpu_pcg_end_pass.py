"""The end of a pass of the independent sampler on the GPU: the closed form of advance(-dim) (csrc/device/drng.h pcg_end_pass) against
the defining loop on the device and the host hook, and renders whose pass ends exercise it against the oracle -- film, stored sampler
states and counters bit for bit. The closed form has one path for every 32-bit dim, so there is no fallback to steer lanes into."""
import os

import numpy as np
import pytest

from akari_render_amd import abi, capi
from oracle import pyoracle, scene_json
from tests.helpers import make_config, n_bit_diff
from tests.test_pcg_end_pass import edge_dims, random_generators

pytestmark = pytest.mark.gpu

W = H = 64
THREADS = min(16, os.cpu_count() or 1)
COUNTERS = ("n_samples", "n_closest", "n_shadow", "n_shaded")


def test_probe_closed_form_is_the_loop(ctx):
    """64 K triples: closed form == loop on the device == the host hook."""
    n = 65536
    rng = np.random.default_rng(21)
    state, inc = random_generators(rng, n)
    dim = rng.integers(0, 2**32, size=n, dtype=np.uint64).astype(np.uint32)
    dim[:8192] = np.arange(8192)  # every small dim, lane after lane
    edges = np.array(edge_dims(), dtype=np.uint32)
    dim[8192:8192 + edges.size] = edges
    # waves whose lanes differ in one place only: lane 0 / lane 63 / every lane past 2^16, the others at a pass end's usual size
    dim[16384:16384 + 3 * 64] = 86
    dim[16384] = dim[16384 + 64 + 63] = 70000
    dim[16384 + 128:16384 + 192] = 70000 + np.arange(64)
    closed, loop = capi.probe_pcg_end_pass(ctx, state, inc, dim)
    assert np.array_equal(closed, loop), f"{np.count_nonzero(closed != loop)} of {n} differ, first at dim {dim[np.argmax(closed != loop)]}"
    host = np.array([capi.host_pcg_end_pass(int(state[i]), int(inc[i]), int(dim[i])) for i in range(n)], dtype=np.uint64)
    assert np.array_equal(host, closed), f"{np.count_nonzero(host != closed)} of {n} differ between the host hook and the device"


@pytest.fixture(scope="module")
def cbox64(cbox_path):
    sd = scene_json.load_scene(cbox_path, W, H)
    return sd, pyoracle.OracleScene(sd)


def oracle_render(osc, cfg):
    states = pyoracle.init_pcg32_states(W * H, cfg.sampler_seed)
    film, st = osc.render(cfg, n_threads=THREADS, states=states)
    return film, states, st


def gpu_render(ctx, sd, cfg, launches, **opts):
    """The session's passes in `launches` calls: 1 = all of them fused into one launch where the library can."""
    n_passes = (cfg.spp + cfg.spp_per_pass - 1) // cfg.spp_per_pass
    with capi.options(**opts):
        scene = capi.Scene(ctx, sd)
        film = capi.Film(ctx, W, H)
        se = capi.PtSession(ctx, scene, cfg, film)
    per = n_passes // launches
    for k in range(launches):
        se.passes(per if k + 1 < launches else n_passes - per * (launches - 1), blocking=True)
    states = se.sampler_states(W * H)
    st = se.end()
    return film.read(), states, st


def assert_same(got, want, what):
    (g, gs, gst), (o, os_, ost) = got, want
    assert n_bit_diff(g, o) == 0, f"{what}: {n_bit_diff(g, o)} of {g.size} film floats differ"
    assert np.array_equal(gs, os_), f"{what}: {np.count_nonzero(gs != os_)} stored sampler words differ"
    for k in COUNTERS:
        assert gst[k] == ost[k], (what, k)


def test_one_sample_passes_depth0(ctx, cbox64):
    """(a) spp_per_pass = 1, max_depth = 0, 8 passes: dim = 2 at every pass end."""
    sd, osc = cbox64
    cfg = make_config(spp=8, spp_per_pass=1, max_depth=0)
    assert_same(gpu_render(ctx, sd, cfg, 1), oracle_render(osc, cfg), "depth 0")


@pytest.fixture(scope="module")
def ragged(cbox64):
    cfg = make_config(spp=14, spp_per_pass=3, max_depth=12)  # 5 passes, the last one of 2 samples
    return cfg, oracle_render(cbox64[1], cfg)


@pytest.mark.parametrize("launches", [1, 5], ids=["fused", "five_launches"])
def test_ragged_passes(ctx, cbox64, ragged, launches):
    """(b) spp_per_pass = 3, max_depth = 12, 5 passes with the last one short: in one launch and as five."""
    cfg, want = ragged
    assert_same(gpu_render(ctx, cbox64[0], cfg, launches), want, f"{launches} launch(es)")


def test_ragged_passes_wavefront(ctx, cbox64, ragged):
    """(d) shape (b) on the wavefront schedule with a forced BVH (k_wf_shade through path_step)."""
    cfg, want = ragged
    assert_same(gpu_render(ctx, cbox64[0], cfg, 1, wavefront=1, force_bvh=1), want, "wavefront")


def test_one_pass_of_1024_spp(ctx, cbox64):
    """(c) spp_per_pass = 1024, max_depth = 12, rr_depth = 12, one pass: dim passes 2^16 in many pixels (1024 samples of up to 2 + 7 * 12
    dimensions each), which reaches the table chunks above the low 16 bits."""
    sd, osc = cbox64
    cfg = make_config(spp=1024, spp_per_pass=1024, max_depth=12, rr_depth=12)
    assert_same(gpu_render(ctx, sd, cfg, 1), oracle_render(osc, cfg), "1024 spp")


def test_aov_pass(ctx, cbox64):
    """(e) an aov pass of 4 spp. k_aov runs all its samples in one pass and ends it with the same function, but the states it stores
    cannot be read back after akr_aov_render: this test sees that the kernel with the closed form in it compiles, runs and leaves the film
    and the counter the oracle's -- not the stored state. The function itself is held by the probe and the pt renders above."""
    sd, osc = cbox64
    cfg = abi.AovConfig.default()
    cfg.spp = 4
    scene = capi.Scene(ctx, sd)
    film = capi.Film(ctx, W, H)
    st = capi.aov_render(ctx, scene, cfg, film)
    o, n_rays = osc.aov_render(cfg, n_threads=THREADS)
    assert st["n_samples"] == n_rays == W * H * 4
    assert n_bit_diff(film.read(), o) == 0
