"""The two-level acceleration structure (csrc/host/scene_inst.cpp, csrc/device/dinst_trav.h) against the oracle, bit for bit.

The reference keeps meshes and instances apart (mesh.rs:259-348) and evaluates a hit from object-space buffers and the instance's
transform (mesh.rs:487-654). The oracle restates that per-hit arithmetic over a FLATTENED scene; a scene kept as meshes + instances
computes the same records at the candidate. Both must give the same film floats -- and the flattening compiler's as well."""
import os

import numpy as np
import pytest

from akari_render_amd import abi, capi, distributed, procedural
from oracle import pyoracle
from tests.helpers import instanced_scene, make_config, n_bit_diff

pytestmark = pytest.mark.gpu


def _table(root):
    return np.fromfile(os.path.join(root, "tests", "golden", "ggx_dielectric_s.f32"), dtype=np.float32)


def _index_states(w, h):
    st = np.zeros(2 * w * h, dtype=np.uint64)
    st[0::2] = 0xFFFFFFFF
    st[1::2] = (np.arange(w * h, dtype=np.uint64) % np.uint64(w)) | ((np.arange(w * h, dtype=np.uint64) // np.uint64(w)) << np.uint64(32))
    return st


def _render(ctx, sd, cfg, mode):
    with capi.options(instancing=mode):
        scene = capi.Scene(ctx, sd)
        assert scene.info().uses_bvh == (2 if mode == 1 else 1)
        film = capi.Film(ctx, sd.camera.width, sd.camera.height)
        st = capi.pt_render(ctx, scene, cfg, film)
    return film.read(), st, scene


def _oracle(sd, cfg, bvh=False):
    pyoracle.set_pmj_tables(*capi.host_pmj02bn_tables())
    w, h = sd.camera.width, sd.camera.height
    return pyoracle.OracleScene(sd, bvh=bvh).render(cfg, states=_index_states(w, h) if cfg.sampler_type != 0 else None)


CASES = {
    "plain": (dict(n_inst=6, n=4, with_normals=False, with_uvs=False, mirror=False, emissive_instances=0), dict()),
    "mirrored": (dict(n_inst=9, n=4, with_normals=False, with_uvs=False, emissive_instances=0), dict()),
    "normals_uvs": (dict(n_inst=9, n=5, emissive_instances=0), dict()),
    "lights_on_instances": (dict(n_inst=12, n=6, emissive_instances=3), dict()),
    "force_diffuse": (dict(n_inst=12, n=6, emissive_instances=1), dict(force_diffuse=1)),
    "alpha": (dict(n_inst=12, n=6, emissive_instances=1, alpha=True), dict()),
    "textured": (dict(n_inst=12, n=6, emissive_instances=2, textured=True), dict()),
    "textured_fd": (dict(n_inst=12, n=6, emissive_instances=2, textured=True), dict(force_diffuse=1)),
    "pmj02bn": (dict(n_inst=12, n=6, emissive_instances=1), dict(sampler_type=abi.SAMPLER_PMJ02BN, sampler_seed=3)),
    "sobol_textured": (dict(n_inst=12, n=6, emissive_instances=1, textured=True), dict(sampler_type=abi.SAMPLER_SOBOL, sampler_seed=11)),
    "ragged_passes": (dict(n_inst=12, n=6, emissive_instances=1), dict(spp=11, spp_per_pass=4)),
    "deep": (dict(n_inst=40, n=12, emissive_instances=2), dict(max_depth=16, rr_depth=8)),
    "tangents": (dict(n_inst=12, n=6, emissive_instances=1, tangents=True), dict()),
    "tangents_no_normals": (dict(n_inst=12, n=6, emissive_instances=1, tangents=True, with_normals=False, textured=True), dict()),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_kept_scene_matches_oracle_and_flattened_scene(ctx, root, case):
    skw, ckw = CASES[case]
    sd = instanced_scene(width=40, height=32, **skw)
    sd.ggx_table = _table(root)
    cfg = make_config(**{**dict(spp=8, spp_per_pass=8, max_depth=8), **ckw})
    kept, kst, _ = _render(ctx, sd, cfg, 1)
    flat, fst, _ = _render(ctx, sd, cfg, 0)
    o, ost = _oracle(sd, cfg)
    assert np.all(np.isfinite(kept))
    assert n_bit_diff(kept, o) == 0, f"{n_bit_diff(kept, o)} of {o.size} film floats differ from the oracle's"
    assert n_bit_diff(kept, flat) == 0
    for k in ("n_samples", "n_closest", "n_shadow", "n_shaded"):
        assert kst[k] == ost[k] == fst[k], k


def test_tile_shards_of_a_kept_scene_add_up(ctx, root):
    """Tile shards (what each GPU of a multi-GPU render gets) of a kept scene: their sum is the whole frame's film, bit for bit."""
    sd = instanced_scene(width=64, height=48, n_inst=20, n=8, emissive_instances=2)
    sd.ggx_table = _table(root)
    base = make_config(spp=4, spp_per_pass=4, max_depth=8)
    whole, _, scene = _render(ctx, sd, base, 1)
    acc = np.zeros_like(whole)
    for r in range(3):
        film = capi.Film(ctx, 64, 48)
        capi.pt_render(ctx, scene, distributed.shard_config(make_config(spp=4, spp_per_pass=4, max_depth=8), r, 3, 8, 8), film)
        part = film.read()
        assert not np.any((acc != 0) & (part != 0))
        acc += part
    assert n_bit_diff(acc, whole) == 0


def _kept_scene_data(root, textured, w=40, h=32):
    sd = instanced_scene(width=w, height=h, n_inst=9, n=6, emissive_instances=2, textured=textured, alpha=textured)
    sd.ggx_table = _table(root)
    return sd


@pytest.mark.parametrize("textured", [False, True], ids=["constant", "textured"])
def test_aov_on_a_kept_scene(ctx, root, textured):
    """aov.rs:57-173 traces the reference's two-level accel like every integrator; round 5 refused kept scenes here."""
    from tests.test_gpu_aov import both
    sd = _kept_scene_data(root, textured)
    with capi.options(instancing=1):
        assert capi.Scene(ctx, sd).info().uses_bvh == 2
        for aov in range(6):
            cfg = abi.AovConfig.default()
            cfg.spp, cfg.aov, cfg.remap = 3, aov, aov % 2
            both(ctx, sd, cfg)  # kept scene against the oracle, bit for bit


@pytest.mark.parametrize("recon", range(3), ids=abi.GPT_RECON_NAMES)
def test_gpt_on_a_kept_scene(ctx, root, recon):
    """gpt.rs:381-640 (base path + four shifted paths, reconnection vertices) over meshes + instances."""
    from tests.test_gpt import both, gpt_config
    sd = _kept_scene_data(root, textured=(recon == 1))
    with capi.options(instancing=1):
        assert capi.Scene(ctx, sd).info().uses_bvh == 2
        kept = both(ctx, sd, gpt_config(spp=4, max_depth=6, rr_depth=2, reconstruction=recon, reconstruction_iter=5))
    with capi.options(instancing=0):
        flat = both(ctx, sd, gpt_config(spp=4, max_depth=6, rr_depth=2, reconstruction=recon, reconstruction_iter=5))
    assert n_bit_diff(kept, flat) == 0


@pytest.mark.parametrize("textured", [False, True], ids=["constant", "textured"])
def test_mcmc_opt_on_a_kept_scene(ctx, root, textured):
    """mcmc_opt.rs:686-746 over meshes + instances: chain states, normalisation and the direct pass identical to the oracle's."""
    from tests.test_mcmc import both, mcmc_config
    sd = _kept_scene_data(root, textured, 36, 28)
    with capi.options(instancing=1):
        assert capi.Scene(ctx, sd).info().uses_bvh == 2
        both(ctx, sd, mcmc_config())


def test_probes_on_a_kept_scene(ctx, root):
    """Closest hits and surface interactions of random rays: kept scene against the oracle's exhaustive loop."""
    rng = np.random.default_rng(4)
    sd = _kept_scene_data(root, False)
    with capi.options(instancing=1):
        scene = capi.Scene(ctx, sd)
    assert scene.info().uses_bvh == 2
    osc = pyoracle.OracleScene(sd)
    n = 3000
    o = rng.uniform([-6, 0.1, -6], [6, 6, 6], size=(n, 3))
    t = rng.uniform([-5, 0, -5], [5, 3, 5], size=(n, 3))
    rays = np.zeros((n, 8), dtype=np.float32)
    rays[:, :3], rays[:, 3:6], rays[:, 7] = o, t - o, 1e30
    hit, bary = capi.probe_intersect(ctx, scene, rays)
    ip, bb = [], []
    for i in range(n):
        h, inst, prim, b = osc.intersect(rays[i, :3], rays[i, 3:6], float(rays[i, 6]), float(rays[i, 7]))
        assert bool(hit[i, 0]) == h, i
        if h:
            assert (int(hit[i, 1]), int(hit[i, 2])) == (inst, prim), i
            assert np.array_equal(bary[i].view(np.uint32), b.view(np.uint32)), i
            ip.append((inst, prim)); bb.append(b)
    assert len(ip) > 500
    ip, bb = np.array(ip, dtype=np.uint32), np.array(bb, dtype=np.float32)
    si = capi.probe_surface_interaction(ctx, scene, ip, bb)
    for k in range(0, len(ip), 5):
        ref = osc.surface_interaction(int(ip[k, 0]), int(ip[k, 1]), float(bb[k, 0]), float(bb[k, 1]))
        assert np.array_equal(si[k].view(np.uint32), ref.view(np.uint32)), (k, si[k], ref)


@pytest.mark.parametrize("sampler", [abi.SAMPLER_INDEPENDENT, abi.SAMPLER_SOBOL], ids=["independent", "sobol"])
def test_per_scene_kernel_of_a_kept_scene(ctx, root, sampler):
    """option specialise on a textured scene kept as meshes + instances: the hiprtc kernel renders the interpreter's film and the oracle's."""
    sd = _kept_scene_data(root, True, 48, 40)
    cfg = make_config(spp=8, spp_per_pass=4, max_depth=8, sampler_type=sampler, sampler_seed=3)
    films = {}
    for spec in (0, 1):
        with capi.options(instancing=1, specialise=spec):
            scene = capi.Scene(ctx, sd)
            film = capi.Film(ctx, 48, 40)
            se = capi.PtSession(ctx, scene, cfg, film)
            se.passes(2, blocking=True)
            ki = se.kernel_info()
            se.end()
        assert ki["specialised"] == spec, ki
        films[spec] = film.read()
    assert n_bit_diff(films[0], films[1]) == 0
    o, _ = _oracle(sd, cfg)
    assert n_bit_diff(films[1], o) == 0


@pytest.mark.parametrize("case", ["constant", "textured_alpha", "sobol_fd", "sorted", "carried"])
def test_wavefront_schedule_on_a_kept_scene(ctx, root, case):
    """Round 6: the persistent trace kernel walks the two-level structure too (k_wf_trace<.., INST>: candidates wait in the lane's pending
    slot, the wave takes the exact test in batches); the shade kernel rebuilds the hit from mesh triangle + instance. Same film as the
    megakernel's and the oracle's."""
    sd = _kept_scene_data(root, case == "textured_alpha", 48, 40)
    cfg = make_config(spp=8, spp_per_pass=4, max_depth=8, **({"sampler_type": abi.SAMPLER_SOBOL, "sampler_seed": 5, "force_diffuse": 1} if case == "sobol_fd" else {}))
    # ("carried": option wf_carry = the launch size from which a trace launch hands its last rays to the next one -- 2: every launch of this small frame)
    with capi.options(instancing=1, wavefront=1, wf_sort=1 if case == "sorted" else 0, wf_carry=2 if case == "carried" else 1):
        scene = capi.Scene(ctx, sd)
        assert scene.info().uses_bvh == 2
        film = capi.Film(ctx, 48, 40)
        se = capi.PtSession(ctx, scene, cfg, film)
        se.passes(2, blocking=True)
        status = se.kernel_info()["status"]
        st = se.end()
    if case == "textured_alpha":
        assert "wavefront" in status, status  # (the reason a textured session has no per-scene kernel: the wavefront schedule runs it)
    if case == "carried":
        assert int(status.split("; ")[1].split()[0]) > 50, status
    o, ost = _oracle(sd, cfg)
    assert n_bit_diff(film.read(), o) == 0
    for k in ("n_samples", "n_closest", "n_shadow", "n_shaded"):
        assert st[k] == ost[k], k


def _quad_panels(seed=2):
    """A mesh of 40 quads (triangles 2j, 2j+1 = the halves of quad j) standing around a ring: half of them planar up to the f32 rounding of
    their corners, the others with the fourth corner lifted out of the plane by 0.1 ... 10 times the sharing rule's tolerance (dinst.h
    share_plane_row: 1e-6 of the triangle's size) -- whether such a pair shares its plane row depends on what the instance's transform does
    to height and area."""
    rng = np.random.default_rng(seed)
    verts, idx = [], []
    for j in range(40):
        a = 2 * np.pi * j / 40
        c = np.array([1.2 * np.cos(a), 0.0, 1.2 * np.sin(a)])
        u = np.array([-np.sin(a), 0.3 * rng.normal(), np.cos(a)]) * 0.11
        v = np.array([0.2 * rng.normal(), 1.0, 0.2 * rng.normal()]) * (0.3 + 0.5 * rng.random())
        n = np.cross(u, v)
        n /= np.linalg.norm(n)
        lift = 0.0 if j % 2 == 0 else 1e-6 * np.sqrt(np.linalg.norm(np.cross(u, v)) * 4) * 10 ** rng.uniform(-1, 1)
        q = [c - u - v, c + u - v, c + u + v, c - u + v + lift * n]
        b = len(verts)
        verts += q
        idx += [[b, b + 1, b + 2], [b, b + 2, b + 3]]
    idx = np.array(idx, dtype=np.uint32)
    return abi.MeshData(vertices=np.array(verts, dtype=np.float32), indices=idx, material_slots=(np.arange(len(idx)) // 2 % 3 == 0).astype(np.uint32))


@pytest.mark.parametrize("schedule", ["megakernel", "wavefront"])
def test_quads_of_a_kept_scene_share_their_plane_rows(ctx, root, schedule):
    """The coplanar-neighbour rule on a kept scene: decided once per instance-triangle on the device (k_inst_share_bits), applied at the candidate
    (dinst_trav.h resolve_pending). Quads whose halves share in every instance, in none, and in some of the twelve instances only: the film is
    the flattened scene's and the oracle's bit for bit."""
    sd = instanced_scene(width=64, height=48, n_inst=12, n=4, emissive_instances=1, with_normals=False, with_uvs=False)
    sd.meshes[0] = _quad_panels()
    sd.ggx_table = _table(root)
    for k, inst in enumerate(sd.instances[2:]):  # stretch the copies differently along their axes: height over size is not invariant
        M = inst.transform.reshape(4, 4).T.copy()
        M[:3, :3] = M[:3, :3] @ np.diag([1.0 + 0.4 * k, 1.0, 1.0 / (1.0 + 0.3 * k)]).astype(np.float32)
        inst.transform = M.T.reshape(16).astype(np.float32).copy()
    # how the flattening compiler decided, from its records: an odd record that repeats its predecessor's plane row
    with capi.options(instancing=0):
        flat = capi.Scene(None, sd)
    gid = flat.array(capi.ARRAY_TRI_GID, np.uint32)      # traversal order -> global id; a record = 12 floats of rows + 4 words
    off = flat.array(capi.ARRAY_INST_TRI_OFFSET, np.uint32)
    rows = np.empty((len(gid), 12), dtype=np.float32)
    rows[gid] = flat.array(capi.ARRAY_WOOP, np.float32)[:16 * len(gid)].reshape(-1, 16)[:, :12]
    shares = np.zeros((12, 40), dtype=bool)
    for i in range(12):
        r = rows[off[2 + i]:off[3 + i]]
        shares[i] = np.all(r[1::2, 8:].view(np.uint32) == r[0::2, 8:].view(np.uint32), axis=1)
    per_quad = shares.sum(axis=0)
    assert (per_quad == 0).any() and (per_quad == 12).sum() >= 8 and ((per_quad > 0) & (per_quad < 12)).sum() >= 8, per_quad
    cfg = make_config(spp=8, spp_per_pass=4, max_depth=6)
    with capi.options(wavefront=1 if schedule == "wavefront" else 0):
        kept, kst, _ = _render(ctx, sd, cfg, 1)
        flattened, fst, _ = _render(ctx, sd, cfg, 0)
    assert n_bit_diff(kept, flattened) == 0
    o, ost = _oracle(sd, cfg)
    assert n_bit_diff(kept, o) == 0
    for k in ("n_samples", "n_closest", "n_shadow", "n_shaded"):
        assert kst[k] == ost[k], k


def test_rebraided_top_level_tree_and_slot_groups_change_no_bit(ctx, root):
    """Option rebraid (the top-level tree over (instance, subtree) pairs, the largest boxes opened first) and option wf_groups (the wavefront
    schedule's slots as groups on streams of their own) change which boxes cull and which launch traces a ray -- never a film float."""
    sd = procedural.instanced_forest(40, 3000, width=512, height=288)
    sd.ggx_table = _table(root)
    cfg = make_config(spp=4, spp_per_pass=4, max_depth=6)
    films, visits, leaves = {}, {}, {}
    for key, opts in {"plain": dict(wavefront=0), "rebraid": dict(wavefront=0, rebraid=8), "groups": dict(wavefront=1, wf_groups=2),
                      "both": dict(wavefront=1, wf_groups=2, rebraid=8)}.items():
        with capi.options(instancing=1, **opts):
            scene = capi.Scene(ctx, sd)
            assert scene.info().uses_bvh == 2
            leaves[key] = len(scene.array(capi.ARRAY_INST_LEAVES, np.float32)) // 16
            film = capi.Film(ctx, 512, 288)
            se = capi.PtSession(ctx, scene, cfg, film)
            se.passes(1, blocking=True)
            visits[key] = se.end()["n_node_visits"]
        films[key] = film.read()
    assert leaves["plain"] == 42 and 42 * 4 < leaves["rebraid"] <= 42 * 8  # (40 plants + ground + sky; the two quads cannot be opened)
    assert visits["rebraid"] != visits["plain"]
    for key in ("rebraid", "groups", "both"):
        assert n_bit_diff(films[key], films["plain"]) == 0, key


@pytest.mark.parametrize("kept", [1, 0], ids=["kept", "flattened"])
def test_rays_carried_from_one_trace_launch_into_the_next_change_no_bit(ctx, root, kept):
    """Option wf_carry (default 1): a wave of k_wf_trace that finds the queue empty and has few lanes left saves their traversals -- best hit, place in
    the tree(s), the stack, a candidate waiting for its exact test -- and ends; k_wf_shade leaves such a slot alone, the next trace launch resumes the
    ray. Launches of >= 65 536 rays only: the frame is large enough for it to happen (asserted), and film and counters are those of the schedule
    that traces every launch to the end, of the megakernel, and (a tile shard) of the oracle."""
    import re
    sd = procedural.instanced_forest(60, 3000, width=640, height=360)
    sd.ggx_table = _table(root)
    cfg = make_config(spp=4, spp_per_pass=2, max_depth=7)
    films, stats, carried = {}, {}, {}
    with capi.options(instancing=kept):
        scene = capi.Scene(ctx, sd)
        assert scene.info().uses_bvh == (2 if kept else 1)
        for key, opts in {"megakernel": dict(wavefront=0), "to_the_end": dict(wavefront=1, wf_carry=0), "carried": dict(wavefront=1, wf_carry=1),
                          "carried_2_groups": dict(wavefront=1, wf_carry=1, wf_groups=2)}.items():
            with capi.options(**opts):
                film = capi.Film(ctx, 640, 360)
                se = capi.PtSession(ctx, scene, cfg, film)
                se.passes(2, blocking=True)
                m = re.search(r"(\d+) rays carried", se.kernel_info()["status"])
                carried[key] = int(m.group(1)) if m else None
                stats[key] = se.end()
            films[key] = film.read()
    assert carried["megakernel"] is None and carried["to_the_end"] is None
    assert carried["carried"] > 100 and carried["carried_2_groups"] > 100, carried
    for key in ("to_the_end", "carried", "carried_2_groups"):
        assert n_bit_diff(films[key], films["megakernel"]) == 0, key
        for k in ("n_samples", "n_closest", "n_shadow", "n_shaded"):
            assert stats[key][k] == stats["megakernel"][k], (key, k)
    if not kept:  # a carried ray goes on where it stopped: not one node more. (Kept scenes: WHEN a wave takes its lanes' exact tests -- and so how
        for k in ("n_node_visits", "n_tri_tests"):  # early a closer hit shortens a ray -- depends on the wave's other lanes, under every schedule.)
            assert stats["carried"][k] == stats["to_the_end"][k], k
    shard = distributed.shard_config(cfg, 3, 64, 8, 8)
    with capi.options(instancing=kept, wavefront=1):
        film = capi.Film(ctx, 640, 360)
        capi.pt_render(ctx, scene, shard, film)
    o, _ = _oracle(sd, shard, bvh=True)
    assert n_bit_diff(film.read(), o) == 0


def test_the_library_picks_the_wavefront_schedule_for_large_kept_frames(ctx, root):
    """Option wavefront = -1 (default): pt sessions of large frames on a kept scene run the wavefront schedule (pt_plan.cpp choose_wavefront:
    1080p forest 163 -> 239 Msamples/s; "large" = from 0.7 M pixels for meshes that fit the L2s to 2 M, wf_auto_items), smaller ones and aov
    sessions the megakernel; same film either way."""
    assert capi.get_option("wavefront") == -1
    sd = procedural.instanced_forest(12, 2000, width=1920, height=1080)
    sd.ggx_table = _table(root)
    cfg = make_config(spp=1, spp_per_pass=1, max_depth=5)
    films = {}
    with capi.options(instancing=1):
        scene = capi.Scene(ctx, sd)
        for mode in (-1, 0):
            with capi.options(wavefront=mode):
                film = capi.Film(ctx, 1920, 1080)
                se = capi.PtSession(ctx, scene, cfg, film)
                assert ("wavefront" in se.kernel_info()["status"]) == (mode == -1)
                se.passes(1, blocking=True)
                se.end()
                films[mode] = film.read()
        for (w, h), wavefront in {(256, 256): False, (800, 600): False, (1024, 768): True}.items():  # (small meshes: from 0.7 M pixels)
            sd_small = procedural.instanced_forest(12, 2000, width=w, height=h)
            sd_small.ggx_table = sd.ggx_table
            small = capi.Scene(ctx, sd_small)
            se = capi.PtSession(ctx, small, cfg, capi.Film(ctx, w, h))
            assert ("wavefront" in se.kernel_info()["status"]) == wavefront, (w, h)
            se.end()
        # texture-fed materials do not change the choice (k_wf_shade interprets the graphs: forest with image-textured leaves 157 -> 193)
        tex = capi.Scene(ctx, _kept_scene_data(root, True, 2048, 1024))
        assert tex.info().uses_bvh == 2
        for mode in (-1, 0):
            with capi.options(wavefront=mode):
                film = capi.Film(ctx, 2048, 1024)
                se = capi.PtSession(ctx, tex, cfg, film)
                assert ("wavefront" in se.kernel_info()["status"]) == (mode == -1)
                se.passes(1, blocking=True)
                se.end()
                films["tex", mode] = film.read()
    assert n_bit_diff(films[-1], films[0]) == 0
    assert n_bit_diff(films["tex", -1], films["tex", 0]) == 0


def test_forest_of_ten_million_instance_triangles_on_a_tile_shard(ctx, root):
    """1000 instances x 10 k triangles, oracle with its checker-side tree (pinned to the exhaustive loop in test_oracle_accel.py and
    test_gpu_fullsize.py), one tile shard of a 512x288 frame."""
    sd = procedural.instanced_forest(1000, 10_000, width=512, height=288)
    sd.ggx_table = _table(root)
    cfg = distributed.shard_config(make_config(spp=8, spp_per_pass=8, max_depth=8), 5, 64, 8, 8)
    scene = capi.Scene(ctx, sd)  # the automatic mode: 10 M triangles would still be flattened
    assert scene.info().uses_bvh == 1
    kept, kst, ks = _render(ctx, sd, cfg, 1)
    assert ks.info().device_bytes < 32 << 20
    film = capi.Film(ctx, 512, 288)
    capi.pt_render(ctx, scene, cfg, film)
    assert n_bit_diff(kept, film.read()) == 0
    o, ost = _oracle(sd, cfg, bvh=True)
    assert n_bit_diff(kept, o) == 0
    for k in ("n_samples", "n_closest", "n_shadow", "n_shaded"):
        assert kst[k] == ost[k], k


@pytest.mark.parametrize("name", ["independent", "fd_sobol"])
def test_forest_of_a_hundred_million_instance_triangles(ctx, root, name):
    """1000 instances x 100 k triangles load in under 1 GB and a tile shard is the oracle's bit for bit. The oracle's
    film of this shard is a committed fixture (tools/make_forest_golden.py: the oracle flattens the scene -- 12 GB and minutes of
    tree building on the CPU, once)."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("make_forest_golden", os.path.join(root, "tools", "make_forest_golden.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    gold = np.load(os.path.join(root, "tests", "golden", "forest_1000x100k_shard.npz"))
    sd = procedural.instanced_forest(1000, 100_000, **mk.FOREST)
    assert sd.n_triangles() == int(gold["n_triangles"][0])
    sd.ggx_table = _table(root)
    scene = capi.Scene(ctx, sd)
    info = scene.info()
    assert info.uses_bvh == 2 and info.device_bytes < 1 << 30
    w, h = mk.FOREST["width"], mk.FOREST["height"]
    cfg = distributed.shard_config(make_config(**mk.CONFIGS[name]), *mk.SHARD)
    film = capi.Film(ctx, w, h)
    st = capi.pt_render(ctx, scene, cfg, film)
    g = film.read().view(np.uint32)
    want = np.zeros(7 * w * h, dtype=np.uint32)
    want[gold[name + "_idx"]] = gold[name + "_bits"]
    nd = int(np.count_nonzero(g != want))
    assert nd == 0, f"{nd} film floats differ from the oracle's"
    assert [st[k] for k in ("n_samples", "n_closest", "n_shadow", "n_shaded")] == [int(x) for x in gold[name + "_stats"]]
