"""Work items ordered by measured pixel cost change no bit.

A pt session on the megakernel records what every pixel cost in its first launch (closest-hit rays) and deals its pixels to lanes sorted by that
cost from its second launch on. Which lane renders a pixel decides nothing about the pixel: film (as uint32), sampler states and every counter
of akr_pt_stats are compared exactly between mode 0 (capi.cost_order_mode: never) and the ordered session after EVERY call, over the variants the mapping touches, and
with the CPU oracle. The cost map and the table are read back through the test hook akr_probe_pt_cost_order.

The frame is 72 x 40: no multiple of 8, 32 or 256 pixels, so it has partial 8 x 8 squares, partial tiles and a padded last workgroup. Three calls
of 2 passes x 4 spp: the first records, the second sorts and uses the order, the third reuses it.
"""
import numpy as np
import pytest

from akari_render_amd import abi, capi, distributed
from oracle import pyoracle, scene_json
from tests.helpers import make_config, n_bit_diff

pytestmark = pytest.mark.gpu

W, H, N = 72, 40, 72 * 40
CALLS, PASSES, PASS_SPP = 3, 2, 4
INVALID = 0xFFFFFFFF
COUNTERS = ("n_samples", "n_closest", "n_shadow", "n_shaded", "n_node_visits", "n_tri_tests")


@pytest.fixture(scope="module")
def cbox(cbox_path):
    return scene_json.load_scene(cbox_path, W, H)


def base_config(**kw):
    return make_config(spp=CALLS * PASSES * PASS_SPP, spp_per_pass=PASS_SPP, **kw)


def run(ctx, sd, cfg, order, force_bvh=0, between=None, passes=PASSES):
    """The session's state after each of the three calls of `passes` passes, on the scene's own frame: (film as uint32, sampler states, counters,
    cost-order hook, status). between(i, se): called after call i (active-tile lists)."""
    w, h = sd.camera.width, sd.camera.height
    n = w * h
    with capi.cost_order_mode(order), capi.options(force_bvh=force_bvh):
        scene = capi.Scene(ctx, sd)
        film = capi.Film(ctx, w, h)
        film.clear()
        se = capi.PtSession(ctx, scene, cfg, film)
    snaps = []
    for i in range(CALLS):
        se.passes(passes, blocking=True)
        st = se.stats()
        snaps.append((film.read().view(np.uint32).copy(), se.sampler_states(n).copy(), {k: st[k] for k in COUNTERS}, se.cost_order(n), se.kernel_info()["status"]))
        if between:
            between(i, se)
    se.end()
    return snaps


def assert_same(a, b):
    for i, (x, y) in enumerate(zip(a, b)):
        nd = int(np.count_nonzero(x[0] != y[0]))
        assert nd == 0, f"call {i}: {nd} film words differ"
        assert np.array_equal(x[1], y[1]), f"call {i}: sampler states differ"
        assert x[2] == y[2], f"call {i}: counters differ"


def assert_order_used(snaps):
    assert [s[3]["state"] for s in snaps] == [1, 2, 2]
    assert "cost order: recording" in snaps[0][4] and "cost order: in use" in snaps[1][4] and "cost order: in use" in snaps[2][4]


def check_table(table, cost, owned):
    """A permutation of the owned pixels, then padding; costs non-increasing along it, ties in ascending pixel order."""
    assert table.size % 256 == 0 and table.size >= owned.size
    n = owned.size
    pix = table[:n]
    assert np.all(table[n:] == INVALID) and np.all(pix != INVALID)
    assert np.array_equal(np.sort(pix), owned)
    c = cost[pix].astype(np.int64)
    assert np.all(np.diff(c) <= 0)
    tie = np.diff(c) == 0
    assert np.all(np.diff(pix.astype(np.int64))[tie] > 0)


VARIANTS = {
    "base": dict(),
    "force_diffuse": dict(force_diffuse=1),
    "pmj02bn": dict(sampler_type=abi.SAMPLER_PMJ02BN),
    "pmj02bn_force_diffuse": dict(sampler_type=abi.SAMPLER_PMJ02BN, force_diffuse=1),
}


@pytest.mark.parametrize("name", list(VARIANTS))
def test_ordered_session_equals_positional(ctx, cbox, name):
    cfg = base_config(**VARIANTS[name])
    ref = run(ctx, cbox, cfg, 0)
    got = run(ctx, cbox, cfg, 1)
    assert [s[3]["state"] for s in ref] == [0, 0, 0] and all("cost order" not in s[4] for s in ref)
    assert_order_used(got)
    assert_same(ref, got)
    # the cost map: what the first call's launch traced, pixel by pixel; nothing is recorded once the table exists
    cost = got[0][3]["cost"]
    assert int(cost.astype(np.uint64).sum()) == got[0][2]["n_closest"]
    assert np.all(cost >= PASSES * PASS_SPP)
    assert got[0][3]["table"].size == 0
    assert np.array_equal(got[1][3]["cost"], cost) and np.array_equal(got[2][3]["cost"], cost)
    check_table(got[1][3]["table"], cost, np.arange(N, dtype=np.uint32))
    assert np.array_equal(got[2][3]["table"], got[1][3]["table"])


@pytest.mark.parametrize("rank", [0, 1])
def test_shards_sort_their_own_pixels(ctx, cbox, rank):
    cfg = distributed.shard_config(base_config(), rank, 2)
    ref = run(ctx, cbox, cfg, 0)
    got = run(ctx, cbox, cfg, 1)
    assert_order_used(got)
    assert_same(ref, got)
    owned = np.flatnonzero(distributed.owned_pixel_mask(W, H, rank, 2).ravel()).astype(np.uint32)
    cost = got[0][3]["cost"]
    assert int(cost.astype(np.uint64).sum()) == got[0][2]["n_closest"]
    assert np.all(cost[owned] >= PASSES * PASS_SPP) and int(cost.astype(np.uint64).sum()) == int(cost[owned].astype(np.uint64).sum())
    check_table(got[1][3]["table"], cost, owned)


def test_an_active_tile_list_drops_the_order(ctx, cbox):
    """A list set after the first call: the session deals by position from then on, also once its own tiles are restored."""
    def between(i, se):
        if i == 0:
            se.set_active_tiles([4, 0, 3])
        if i == 1:
            se.set_active_tiles(None)

    cfg = base_config()
    ref = run(ctx, cbox, cfg, 0, between=between)
    got = run(ctx, cbox, cfg, 1, between=between)
    assert [s[3]["state"] for s in got] == [1, 0, 0] and "cost order" not in got[2][4]
    assert_same(ref, got)


def test_every_megakernel_session_on_the_forced_bvh(ctx, cbox):
    """Mode 2 orders the BVH kernel's items as well (the default leaves them alone): same film, states and counters."""
    cfg = base_config()
    ref = run(ctx, cbox, cfg, 0, force_bvh=1)
    off = run(ctx, cbox, cfg, 1, force_bvh=1)
    got = run(ctx, cbox, cfg, 2, force_bvh=1)
    assert ref[2][2]["n_node_visits"] > 0
    assert [s[3]["state"] for s in off] == [0, 0, 0]
    assert_order_used(got)
    assert_same(ref, got)
    check_table(got[1][3]["table"], got[0][3]["cost"], np.arange(N, dtype=np.uint32))


def test_ordered_film_is_the_oracles(ctx, cbox):
    cfg = base_config()
    got = run(ctx, cbox, cfg, 1)
    assert_order_used(got)
    o, ost = pyoracle.OracleScene(cbox).render(cfg)
    assert n_bit_diff(got[2][0].view(np.float32), o) == 0
    for k in ("n_samples", "n_closest", "n_shadow", "n_shaded"):
        assert got[2][2][k] == ost[k], k


def test_all_equal_costs_give_the_identity(ctx):
    """Every camera ray misses (the scene's one triangle, an emitter, is behind the camera): every pixel costs its samples, the table is
    the pixels in index order, and the film is the positional session's -- weight and nothing else."""
    v = np.array([[-1, -1, 5], [1, -1, 5], [0, 1, 5]], dtype=np.float32)
    mesh = abi.MeshData(vertices=v, indices=np.array([[0, 1, 2]], dtype=np.uint32))
    m = abi.MaterialData(kind=abi.MAT_PRINCIPLED, base_color=(0.5,) * 3, roughness=1.0, ior=1.0, specular_ior_level=0.0, emission_color=(1.0,) * 3, emission_strength=1.0)
    eye = np.eye(4, dtype=np.float32)
    sd = abi.SceneData([mesh], [abi.InstanceData(0, [0], eye.T.reshape(16).copy())], [m], abi.CameraData(c2w=eye.T.reshape(16).copy(), fov=1.0, width=W, height=H))
    cfg = base_config()
    ref = run(ctx, sd, cfg, 0)
    got = run(ctx, sd, cfg, 1)
    assert_order_used(got)
    assert_same(ref, got)
    assert got[2][2]["n_shaded"] == 0 and got[2][2]["n_closest"] == N * CALLS * PASSES * PASS_SPP
    assert np.all(got[0][3]["cost"] == PASSES * PASS_SPP)
    table = got[1][3]["table"]
    assert np.array_equal(table[:N], np.arange(N, dtype=np.uint32)) and np.all(table[N:] == INVALID) and table.size % 256 == 0
    film = got[2][0].view(np.float32)
    assert np.all(film[: 6 * N] == 0) and np.all(film[6 * N :] == CALLS * PASSES * PASS_SPP)
