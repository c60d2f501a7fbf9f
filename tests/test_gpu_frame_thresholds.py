"""The image-space kernels and the two device sorts on the smallest frames that change what they launch.

Their own test files stop at frames (display 130 x 67, denoise 70 x 45, gpt 56 x 40, cost order 72 x 40, sorted ray queues 96 x 72) on which the
launch code below takes one path only; the frames of the benchmark (1080p, 4K) take the other. Every threshold is read from the source named
with it, and every frame is the smallest that crosses it while staying ragged -- no multiple of 16, 64 or 256 per side. Each test asserts that
its frame does cross the threshold, so that the frame cannot be shrunk later without the test noticing.

A. k_lum_histogram (csrc/display_kernels.hip, launch_lum_histogram): the grid is min(ceil(n / 256), 2048) workgroups of 256 threads, so the
   grid-stride loop takes a second trip only past 2048 * 256 = 524 288 pixels. Frame 1031 x 767 = 790 777 pixels (odd): the threads below
   266 489 take two trips, the others one. Histogram of both shared films against the restated counts; one whole akr_display_transform
   (Hable, auto-exposure, bloom of five levels) under both blur kernels against the restatement and the host build.
B. launch_cost_order (csrc/cost_order_kernels.hip): rocprim::radix_sort_keys over 64-bit keys, bits 0 .. 64. rocPRIM sorts one workgroup's worth
   in one kernel, up to merge_sort_limit = 1024 * 1024 elements (rocprim/device/device_radix_sort_config.hpp) by merge sort, and more by its
   onesweep radix sort. cbox at 1200 x 880 = 1 056 000 pixels; the table (the sorted count, n_padded) is at least that long.
C. wf_sort_pairs (csrc/wf_sort.hip, called by csrc/host/wf_schedule.cpp from iteration 1 on): rocprim::radix_sort_pairs over 32-bit keys, bits
   0 .. 24, separate in / out buffers, one scratch buffer for every count. The closed, everywhere-emitting box at 1200 x 880 under
   rr_depth > max_depth keeps (nearly) every path alive, so the queues sorted at iteration 1 hold (nearly) W H rays.
D. k_gpt_update, k_gpt_recon (csrc/gpt_kernels.hip): x = blockIdx.x * 64 + lane, y = blockIdx.y * 4 + wave. Frame 130 x 13: three blocks
   in x, the last one two pixels wide, four in y with one row in the last; the gradient planes' pitch of W + 1, gpt_sources and gpt_shifted
   are read across the block boundaries at x = 64 and 128.
E. k_denoise_level_tiled (csrc/denoise_kernels.hip, launch_denoise_level): the grid is (tiles of the LARGEST residue class) x step^2, and the
   workgroups of a smaller class's missing tiles leave at once. Frame 261 x 259 = (16 * 16 + 5) x (16 * 16 + 3): at step 16 the classes with
   x mod 16 < 5 have 17 columns -- two tiles -- the others 16, whose second tile leaves; the same in y with y mod 16 < 3; at step 8 every class
   has three tiles per axis (33 or 32 columns, 33 or 32 rows).

The references of A and E are the numpy restatements (tests/display_model.py, tests/denoise_model.py, tests/denoise_variance_model.py), held to
the host build on the same frames without a GPU by tests/test_display.py, test_denoise.py and test_denoise_variance.py; those of C and D are the
CPU oracle's films; B compares the ordered session with the positional one, which tests/test_gpu_cost_order.py pins to the oracle.

Not covered, on purpose: k_inst_share_bits is grid-capped as well, at 2^20 workgroups -- its second trip needs more than 2^28 triangles, which
no test renders in seconds. Denoising with six to eight iterations (steps 32 .. 128) has several tiles per class only on frames above 512 ..
2048 pixels per side: left for a later change.

Wall times, measured with pytest --durations (call phase; a case's reference is computed by the first test that asks for it, which is
the slower `gather` case of each pair below). On the MI355X, the whole module: 22 tests in 4.3 s.
  A  histogram random 0.08 s, special 0.05 s; display transform gather 0.16 s, lds 0.05 s
  B  cost order 0.11 s
  C  sorted ray queues 0.45 s, the oracle's render included
  D  0.02 .. 0.03 s per case, the sharded case 0.02 s
  E  denoise gather 0.35 s, tiled 0.10 s; denoise_variance gather 0.48 s, tiled 0.14 s
The CPU references on the same frames, as the host tests without a GPU run them (16 cores): test_display.py the transform 0.45 s, the
histograms 0.10 and 0.13 s; test_denoise.py 0.78 s per case; test_denoise_variance.py 1.0 s per case.
"""
import numpy as np
import pytest

from akari_render_amd import abi, capi
from oracle import pyoracle, scene_json
from tests import denoise_model as dn
from tests import denoise_variance_model as dvm
from tests import display_model as dm
from tests import test_gpu_denoise as gpu_dn
from tests import test_gpu_denoise_variance as gpu_dvm
from tests import test_gpu_display as gpu_dm
from tests.helpers import box_scene, make_config, n_bit_diff
from tests.probe_matrix import same_bits_or_both_nan
from tests.test_gpt import both, gpt_config, make_scene, sharded_is_unsharded
from tests.test_gpu_cost_order import assert_order_used, assert_same, check_table, run

pytestmark = pytest.mark.gpu
f32 = np.float32

HISTOGRAM_GRID_CAP = 2048 * 256  # launch_lum_histogram: workgroups x threads
MERGE_SORT_LIMIT = 1024 * 1024   # rocPRIM's merge_sort_limit
SORT_W, SORT_H = 1200, 880
KERNELS, KERNEL_IDS = [0, 1], ["gather", "lds"]


# ------------------------------------------------------------------------------------------------ A
@pytest.mark.parametrize("kind", dm.KINDS)
def test_histogram_past_the_grid_cap(ctx, oracle_lib, kind):
    w, h = dm.LARGE_SHAPE
    assert HISTOGRAM_GRID_CAP < w * h < 2 * HISTOGRAM_GRID_CAP and (w * h) % 2 == 1  # some threads take two trips, the others one
    film = dm.case_film(w, h, kind)  # dm.random_film / dm.special_film of the frame, made once
    counts, skipped = capi.film_luminance_histogram(ctx, gpu_dm.film_with(ctx, w, h, film, dm.SPLAT_SCALE[kind]))
    ref_counts, ref_skipped = dm.case_histogram(w, h, kind)  # dm.histogram(dm.load(film, ..)), computed once
    assert np.array_equal(counts, ref_counts), f"bins {np.flatnonzero(counts != ref_counts)} differ"
    assert skipped == ref_skipped
    assert int(counts.astype(np.uint64).sum()) + skipped == w * h


@pytest.mark.parametrize("kernel", KERNELS, ids=KERNEL_IDS)
def test_display_transform_past_the_grid_cap(ctx, oracle_lib, kernel):
    w, h = dm.LARGE_SHAPE
    assert w * h > HISTOGRAM_GRID_CAP
    cfg = next(c for n, c in dm.cases() if n == dm.LARGE_CASE)
    assert (cfg.curve, cfg.auto_exposure, cfg.bloom_levels) == (abi.DISPLAY_HABLE, 1, 5) and cfg.bloom_strength > 0
    film, scale = dm.case_film(w, h, "random"), dm.SPLAT_SCALE["random"]
    got, raw, k = gpu_dm.device(ctx, w, h, film, cfg, scale, kernel)
    ref, k_ref = dm.case_reference(w, h, "random", dm.LARGE_CASE)  # dm.display_np of the same film and configuration, computed once
    assert f32(k).view(np.uint32) == f32(k_ref).view(np.uint32), f"exposure {k} against {k_ref}"
    same = same_bits_or_both_nan(got, ref)
    assert same.all(), f"kernel {kernel}: {np.count_nonzero(~same)} of {same.size} floats differ from the restatement, first at {np.argwhere(~same)[:4].tolist()}"
    host, k_host = capi.host_display_transform(w, h, film, cfg, scale)
    assert same_bits_or_both_nan(got, host).all() and f32(k_host).view(np.uint32) == f32(k).view(np.uint32)
    n = w * h
    assert np.array_equal(raw[:3 * n].view(np.uint32), got.reshape(-1).view(np.uint32))
    assert np.all(raw[3 * n:6 * n].view(np.uint32) == 0) and np.all(raw[6 * n:] == 1.0)


# ------------------------------------------------------------------------------------------------ B
def test_cost_order_past_the_merge_sort_limit(ctx, cbox_path):
    """Three calls of one pass of 2 spp: the first records, the second sorts 1 056 000 keys and uses the order, the third reuses it."""
    w, h = SORT_W, SORT_H
    n = w * h
    sd = scene_json.load_scene(cbox_path, w, h)
    cfg = make_config(spp=3 * 2, spp_per_pass=2)
    ref = run(ctx, sd, cfg, 0, passes=1)
    got = run(ctx, sd, cfg, 1, passes=1)
    assert [s[3]["state"] for s in ref] == [0, 0, 0]
    assert_order_used(got)
    assert_same(ref, got)
    cost, table = got[0][3]["cost"], got[1][3]["table"]
    assert table.size > MERGE_SORT_LIMIT  # the sorted count: every entry of the table is one sorted key
    assert int(cost.astype(np.uint64).sum()) == got[0][2]["n_closest"]
    assert got[0][3]["table"].size == 0
    check_table(table, cost, np.arange(n, dtype=np.uint32))
    assert np.array_equal(got[2][3]["table"], table)


# ------------------------------------------------------------------------------------------------ C
def test_sorted_ray_queues_past_the_merge_sort_limit(ctx):
    w, h = SORT_W, SORT_H
    n = w * h
    sd = box_scene(width=w, height=h)
    cfg = make_config(spp=1, spp_per_pass=1, max_depth=3, rr_depth=4)  # rr_depth > max_depth: Russian roulette ends no path

    def render(sort):
        with capi.options(wavefront=1, force_bvh=1, wf_sort=sort):
            scene = capi.Scene(ctx, sd)
            film = capi.Film(ctx, w, h)
            se = capi.PtSession(ctx, scene, cfg, film)
        se.passes(1, blocking=True)
        status, states = se.kernel_info()["status"], se.sampler_states(n).copy()
        st = se.end()
        return film.read(), states, st, status

    plain, sorted_ = render(0), render(1)
    assert "wavefront" in plain[3] and "wavefront" in sorted_[3]
    assert n_bit_diff(plain[0], sorted_[0]) == 0
    assert np.array_equal(plain[1], sorted_[1])
    for k in ("n_samples", "n_closest", "n_shadow", "n_shaded"):
        assert plain[2][k] == sorted_[2][k], k
    st = sorted_[2]
    # How many rays the queues sorted at iteration 1 held. One pass of 1 spp is one path per pixel, and a path traces one closest-hit ray per
    # iteration it is alive in: at depths 0 .. max_depth, so in at most max_depth + 1 iterations. With q_i paths alive in iteration i,
    # n_closest = q_0 + q_1 + .. and W H = q_0 >= q_1 >= q_2 >= .., hence n_closest <= W H + max_depth * q_1. (Iteration 0, the camera
    # rays, is traced unsorted; iteration 1 is the first sorted one.)
    assert st["n_samples"] == n
    q1 = (st["n_closest"] - n) / cfg.max_depth
    print(f"n_closest {st['n_closest']} = {st['n_closest'] / n:.4f} W H, n_shadow {st['n_shadow']} = {st['n_shadow'] / n:.4f} W H: at least {q1:.0f} closest-hit rays sorted at iteration 1")
    assert q1 > MERGE_SORT_LIMIT, f"at least {q1} closest-hit rays at iteration 1"
    o, ost = pyoracle.OracleScene(sd).render(cfg)
    assert n_bit_diff(sorted_[0], o) == 0, f"{n_bit_diff(sorted_[0], o)} of {o.size} film floats differ from the oracle's"
    for k in ("n_samples", "n_closest", "n_shadow", "n_shaded"):
        assert st[k] == ost[k], k


# ------------------------------------------------------------------------------------------------ D
GPT_W, GPT_H = 130, 13


@pytest.mark.parametrize("recon", range(3), ids=abi.GPT_RECON_NAMES)
@pytest.mark.parametrize("case", ["cbox_s1", "kinds_s3"])
def test_gpt_across_blocks_in_x(ctx, cbox_path, root, case, recon):
    assert GPT_W > 128 and GPT_W % 64 == 2 and GPT_H % 4 == 1  # three blocks of 64 in x, the last 2 wide; the last block in y 1 high
    name, stride = {"cbox_s1": ("cbox", 1), "kinds_s3": ("kinds", 3)}[case]
    sd = make_scene(name, cbox_path, root, GPT_W, GPT_H)
    g = both(ctx, sd, gpt_config(spp=3, max_depth=5, reconstruction=recon, reconstruction_iter=4, stride=stride))
    splat = g[3 * GPT_W * GPT_H:6 * GPT_W * GPT_H].reshape(GPT_H, GPT_W, 3)
    assert splat[:, :64].any() and splat[:, 64:128].any() and splat[:, 128:].any()  # (every block in x wrote something)


def test_gpt_sharded_across_blocks_in_x(ctx, cbox_path, root):
    assert GPT_W > 128
    sd = make_scene("kinds", cbox_path, root, GPT_W, GPT_H)
    sharded_is_unsharded(ctx, sd, gpt_config(spp=3, max_depth=5, reconstruction=abi.GPT_RECON_WEIGHTED, reconstruction_iter=4, stride=3))


# ------------------------------------------------------------------------------------------------ E
def tiles_per_class(size, step, tile=16):
    """(tiles of the largest, tiles of the smallest) residue class of `size` pixels at `step`: class r holds the pixels r, r + step, .."""
    members = [len(range(r, size, step)) for r in range(step)]
    return -(-max(members) // tile), -(-min(members) // tile)


def test_the_denoise_frame_has_several_tiles_per_class():
    w, h = dn.LARGE_SHAPE
    assert tiles_per_class(w, 16) == (2, 1) and tiles_per_class(h, 16) == (2, 1)  # step 16: two tiles, and short classes whose second one leaves
    assert tiles_per_class(w, 8) == (3, 2) and tiles_per_class(h, 8) == (3, 2)  # step 8: three (33 members), two in the classes of 32
    assert len(range(4, w, 16)) == 17 and len(range(5, w, 16)) == 16 and len(range(2, h, 16)) == 17 and len(range(3, h, 16)) == 16
    assert w % 16 and h % 16 and w > 256 and h > 256


@pytest.mark.parametrize("kernel", KERNELS, ids=gpu_dn.KERNEL_IDS)
@pytest.mark.parametrize("name", dn.LARGE_CASES)
def test_denoise_with_several_tiles_per_class(ctx, oracle_lib, name, kernel):
    w, h = dn.LARGE_SHAPE
    assert tiles_per_class(w, 16)[0] == 2 and tiles_per_class(h, 16)[0] == 2
    _, kind, use_a, use_n, cfg, scales = next(c for c in dn.cases() if c[0] == name)
    assert use_a and use_n and cfg.demodulate == 1 and cfg.iterations == 5
    color, albedo, normal = dn.case_inputs(w, h, kind)
    got, raw = gpu_dn.device(ctx, w, h, color, albedo, normal, cfg, scales, kernel)
    ref = dn.case_reference(w, h, name)
    same = same_bits_or_both_nan(got, ref)
    assert same.all(), f"{name} kernel {kernel}: {np.count_nonzero(~same)} of {same.size} floats differ from the restatement, first at {np.argwhere(~same)[:4].tolist()}"
    assert same_bits_or_both_nan(got, capi.host_denoise(w, h, color, albedo, normal, cfg, scales)).all()
    n = w * h
    assert np.array_equal(raw[:3 * n].view(np.uint32), got.reshape(-1).view(np.uint32))
    assert np.all(raw[3 * n:6 * n].view(np.uint32) == 0) and np.all(raw[6 * n:] == 1.0)


@pytest.mark.parametrize("kernel", KERNELS, ids=gpu_dvm.KERNEL_IDS)
@pytest.mark.parametrize("name", dvm.LARGE_CASES)
def test_denoise_variance_with_several_tiles_per_class(ctx, oracle_lib, name, kernel):
    w, h = dvm.LARGE_SHAPE
    assert tiles_per_class(w, 16)[0] == 2 and tiles_per_class(h, 16)[0] == 2
    _, kind, halves, use_a, use_n, cfg = next(c for c in dvm.cases() if c[0] == name)
    assert use_a and use_n and cfg.demodulate == 1 and cfg.iterations == 5
    color, half, albedo, normal = dvm.case_inputs(w, h, kind, halves)
    got, raw = gpu_dvm.device(ctx, w, h, color, half, albedo, normal, cfg, kernel)
    ref = dvm.case_reference(w, h, name)
    same = same_bits_or_both_nan(got, ref)
    assert same.all(), f"{name} kernel {kernel}: {np.count_nonzero(~same)} of {same.size} floats differ from the restatement, first at {np.argwhere(~same)[:4].tolist()}"
    assert same_bits_or_both_nan(got, capi.host_denoise_variance(w, h, color, half, albedo, normal, cfg)).all()
    n = w * h
    assert np.array_equal(raw[:3 * n].view(np.uint32), got.reshape(-1).view(np.uint32))
    assert np.all(raw[3 * n:6 * n].view(np.uint32) == 0) and np.all(raw[6 * n:] == 1.0)
