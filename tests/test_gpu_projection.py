"""Camera projections on the GPU (through the LENS kernels): the device's camera rays against the host's, a panorama of an
environment is that environment texel for texel, a panorama sees behind the camera, the orthographic closed form with and without a lens, one
film under every route, aov and the collected guides, the refusals, and akari-cli --projection. These are bit-identities, the restated definition
(tests/camera_model.py, tests/test_projection.py) and closed forms; the comparison with the CPU oracle's own projections, film for film, is
tests/test_gpu_projection_parity.py."""
import json
import subprocess

import numpy as np
import pytest

from akari_render_amd import abi, capi, distributed
from oracle import scene_json
from tests.helpers import cbox_variant, make_config, n_bit_diff, resolve_np
from tests.test_environment import direction_uv
from tests.test_gpu_environment import _looking_along
from tests.test_gpu_lens import EMISSION, LENS_BIT, _route_scene, _session
from tests.test_lens import _camera
from tests.test_projection import CASES, FILMS, FILTERS, rows_of, set_case

pytestmark = pytest.mark.gpu
F = np.float32
ORTHO, PANORAMA = abi.PROJECTION_ORTHOGRAPHIC, abi.PROJECTION_PANORAMA


def _image(ctx, scene, cfg):
    """(H, W, 3) resolved film of one pt render"""
    w, h = scene.info().width, scene.info().height
    film = capi.Film(ctx, w, h)
    capi.pt_render(ctx, scene, cfg, film)
    return resolve_np(film.read(), w, h).reshape(h, w, 3)


def _centre_cfg(spp=4, max_depth=0, **kw):
    """every sample of a pixel through its centre: the box filter of radius 0"""
    return make_config(spp=spp, spp_per_pass=spp, max_depth=max_depth, filter_type=abi.FILTER_BOX, filter_radius=0.0, sampler_seed=5, **kw)


def _panorama_centre_dirs(w, h):
    """camera-space direction of every pixel centre of a full panorama, float64, (H, W, 3)"""
    lon = -np.pi + (np.arange(w) + 0.5) / w * 2 * np.pi
    lat = np.pi / 2 - (np.arange(h) + 0.5) / h * np.pi
    lon, lat = np.meshgrid(lon, lat)
    return np.stack([np.cos(lat) * np.sin(lon), np.sin(lat), -np.cos(lat) * np.cos(lon)], -1)


# ---------------------------------------------------------------------------------------------------------------- a. probe equals host
@pytest.mark.parametrize("rotated", [False, True], ids=["identity", "rotated"])
def test_probe_equals_host(ctx, rotated):
    for w, h in FILMS:
        scene = capi.Scene(ctx, _camera(w, h, rotated))
        pixels, u_filter, u_lens = rows_of(w, h, 100 + 7 * w + h + int(rotated))
        for case in CASES:
            set_case(scene, case)
            for ft, fr in FILTERS:
                dev = scene.probe_camera_rays(pixels, u_filter, u_lens, ft, fr)
                host = scene.host_lens_ray(pixels, u_filter, u_lens, ft, fr)
                assert np.array_equal(dev.view(np.uint32), host.view(np.uint32)), (w, h, case, ft)


# ---------------------------------------------------------------------------------------------------------------- b. a panorama of an environment
ROT_Y_90 = np.array([[0.0, 0, 1], [0, 1, 0], [-1, 0, 0]])  # camera -> world: a quarter turn about y, entries exactly 0 / +-1


def test_a_panorama_of_an_environment_is_the_environment(ctx):
    W, H, TW, TH = 64, 32, 8, 4
    texels = np.zeros((TH, TW, 4), F)
    k = np.arange(TW * TH).reshape(TH, TW)
    texels[..., 0], texels[..., 1], texels[..., 2], texels[..., 3] = (k + 1) / 64.0, (k % 5 + 1) / 8.0, (k // 3 + 1) / 16.0, 1.0
    assert len({tuple(t) for t in texels.reshape(-1, 4)[:, :3]}) == TW * TH
    env = abi.EnvironmentData(image=texels, strength=1.0, rotation=np.eye(3, dtype=F), filter=abi.TEX_FILTER_NEAREST)
    ys, xs = np.mgrid[0:H, 0:W]
    tx = np.floor((((xs + 0.5) / W - 0.25) % 1.0) * TW).astype(int)
    ty = np.floor((1.0 - (ys + 0.5) / H) * TH).astype(int)
    tri_dir = np.array([50.0, 50.0, 50.0]) / np.linalg.norm([50.0, 50.0, 50.0])
    films = []
    for R in (np.eye(3), ROT_Y_90):
        # checked here: the normative mapping of the centre rays agrees with the formula for all 2048 pixels, no centre is nearer than 1/16
        # texel to a texel edge, and no centre ray comes within 0.045 rad of the triangle (which subtends 0.001)
        d = _panorama_centre_dirs(W, H) @ R.T
        u, v = direction_uv(d)
        shift = 0 if R is not ROT_Y_90 else 16
        assert np.array_equal(np.floor((u % 1.0) * TW).astype(int), np.roll(tx, shift, axis=1)) and np.array_equal(np.floor(v * TH).astype(int), ty)
        for t, n in ((u % 1.0, TW), (v, TH)):
            frac = (t * n) % 1.0
            assert np.minimum(frac, 1.0 - frac).min() >= 1.0 / 16 - 1e-9
        assert np.arccos(np.clip(d @ tri_dir, -1, 1)).min() > 0.045
        sd = _looking_along([0, 0, -1], env)
        sd.camera.width, sd.camera.height = W, H
        c2w = np.eye(4)
        c2w[:3, :3] = R
        sd.camera.c2w = c2w.astype(F).T.reshape(16).copy()
        sd.projection = abi.ProjectionData(type=PANORAMA)
        scene = capi.Scene(ctx, sd)
        assert scene.projection().type == PANORAMA
        films.append(_image(ctx, scene, _centre_cfg(spp=4, max_depth=2)))
    want = texels[ty, tx, :3]
    bad = np.argwhere(np.any(films[0] != want, axis=2))
    assert len(bad) == 0, (len(bad), bad[:5])  # no pixel is left out
    assert np.array_equal(films[1].view(np.uint32), np.roll(films[0], 16, axis=1).view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------- c. it sees behind itself
def _emitters(quads, width, height, c2w=None, fov=0.8):
    """Emissive quads with a black base (each 4 x 3, counter-clockwise seen from the side they light), camera at the origin looking down -z -- or
    the whole arrangement moved by the rigid transform c2w (4 x 4)."""
    m = np.eye(4) if c2w is None else np.asarray(c2w, dtype=np.float64)
    v = np.concatenate([np.asarray(q, dtype=np.float64) for q in quads]) @ m[:3, :3].T + m[:3, 3]
    idx = np.concatenate([np.array([[0, 1, 2], [0, 2, 3]]) + 4 * i for i in range(len(quads))]).astype(np.uint32)
    mesh = abi.MeshData(vertices=v.astype(F), indices=idx)
    mat = abi.MaterialData(kind=abi.MAT_EMISSION, base_color=(0.0, 0.0, 0.0), emission_color=EMISSION, emission_strength=1.0)
    cam = abi.CameraData(c2w=m.astype(F).T.reshape(16).copy(), fov=fov, width=width, height=height)
    return abi.SceneData([mesh], [abi.InstanceData(0, [0], np.eye(4, dtype=F).reshape(16).copy())], [mat], cam)


def test_a_panorama_sees_behind_the_camera(ctx):
    W, H = 64, 32
    sd = _emitters([[[1, -1, 3], [-1, -1, 3], [-1, 1, 3], [1, 1, 3]]], W, H)  # x, y in [-1, 1] at z = +3, facing the origin
    scene = capi.Scene(ctx, sd)
    cfg = _centre_cfg()
    assert np.all(_image(ctx, scene, cfg) == 0)  # the perspective camera looks the other way
    scene.set_projection("panorama")
    img = _image(ctx, scene, cfg)
    d = _panorama_centre_dirs(W, H)
    behind = d[..., 2] > 0
    with np.errstate(all="ignore"):
        px, py = 3.0 * d[..., 0] / d[..., 2], 3.0 * d[..., 1] / d[..., 2]
    cheb = np.maximum(np.abs(px), np.abs(py))
    hit = behind & (cheb < 1.0)
    assert np.abs(cheb[behind] - 1.0).min() > 1e-3  # no centre ray passes within 1e-3 world units of an edge: no pixel may be left out
    assert hit.sum() == 36 and hit[:, 0].any() and hit[:, W - 1].any() and not hit[:, W // 2].any()  # they straddle the film's left and right edges
    assert np.all(img[hit] == F(EMISSION)) and np.all(img[~hit] == 0)


# ---------------------------------------------------------------------------------------------------------------- d. orthographic closed form
def _ortho_quads():
    near = [[-1.5, -0.5, -2], [-0.5, -0.5, -2], [-0.5, 0.5, -2], [-1.5, 0.5, -2]]
    far = [[0.5, -0.5, -6], [1.5, -0.5, -6], [1.5, 0.5, -6], [0.5, 0.5, -6]]
    return [near, far]


@pytest.mark.parametrize("rotated", [False, True], ids=["axis_aligned", "rotated_together"])
def test_orthographic_closed_form(ctx, rotated):
    """ortho_scale 4 on 48 x 32: a pixel is 1/12 unit; two unit quads, x in [-1.5, -0.5] at depth 2 and [0.5, 1.5] at depth 6, cover columns 6..17
    and 30..41 of rows 10..21 whatever their depth, every pixel centre 1/24 unit from every edge. With a lens of radius 1/12 focused at 2 the near
    quad stays sharp and the far one blurs by R |1 - 6 / 2| = 1/6 unit = 2 pixels."""
    W, H = 48, 32
    c2w = None
    if rotated:
        a, b = 0.6, -0.35
        c2w = np.eye(4)
        c2w[:3, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]) @ np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
        c2w[:3, 3] = [0.5, -0.25, 1.0]
    scene = capi.Scene(ctx, _emitters(_ortho_quads(), W, H, c2w))
    assert scene.info().uses_bvh == 0
    scene.set_projection("orthographic", ortho_scale=4.0)
    want = np.zeros((H, W, 3), F)
    want[10:22, 6:18] = EMISSION
    want[10:22, 30:42] = EMISSION
    img = _image(ctx, scene, _centre_cfg())
    bad = np.argwhere(np.any(img != want, axis=2))
    assert len(bad) == 0, (len(bad), bad[:5])
    persp = capi.Scene(ctx, _emitters(_ortho_quads(), W, H, c2w))
    assert np.any(_image(ctx, persp, _centre_cfg()) != want)  # (foreshortening: the far quad is smaller through the perspective camera)
    scene.set_lens(1.0 / 12.0, 2.0)
    img = _image(ctx, scene, _centre_cfg(spp=16))
    assert np.array_equal(img[:, :24], want[:, :24])  # the near quad is in focus: its block is unchanged
    ys, xs = np.mgrid[0:H, 0:W]
    ax = np.maximum(30.0 - (xs + 0.5), (xs + 0.5) - 42.0)  # pixels outside (> 0) / inside (< 0) the far quad's block, per axis
    ay = np.maximum(10.0 - (ys + 0.5), (ys + 0.5) - 22.0)
    out_by = np.maximum(ax, ay)
    right = xs >= 24
    inside, outside = right & (out_by < -3.0), right & (out_by > 3.0)
    assert inside.sum() == 6 * 6 and outside.sum() > 300
    assert np.all(img[inside] == F(EMISSION)) and np.all(img[outside] == 0)
    between = right & ~inside & ~outside
    assert np.any((img[between][:, 0] > 0) & (img[between][:, 0] < F(EMISSION[0])))


# ---------------------------------------------------------------------------------------------------------------- e. one film under every route
def _projected(sd, projection):
    sd.lens = None
    sd.projection = abi.ProjectionData(type=ORTHO, ortho_scale=ROUTE_ORTHO_SCALE) if projection == "ortho" else abi.ProjectionData(type=PANORAMA)
    return sd


ROUTE_ORTHO_SCALE = 4.0  # about what the helper's perspective camera sees of the scene, and inside what its trees' padding allows (5.3)


@pytest.mark.parametrize("projection", ["ortho", "panorama"])
@pytest.mark.parametrize("with_env", [False, True], ids=["no_env", "env"])
@pytest.mark.parametrize("sampler", [abi.SAMPLER_INDEPENDENT, abi.SAMPLER_PMJ02BN, abi.SAMPLER_SOBOL], ids=["independent", "pmj02bn", "sobol"])
def test_one_film_under_every_route(ctx, root, sampler, with_env, projection):
    sd = _projected(_route_scene(root, with_env), projection)
    w, h = sd.camera.width, sd.camera.height
    cfg = make_config(spp=12, spp_per_pass=4, max_depth=6, sampler_type=sampler, sampler_seed=7)
    with capi.options(force_bvh=0, instancing=0, wavefront=0, specialise=0):
        exh = capi.Scene(ctx, sd)
        assert exh.info().uses_bvh == 0 and exh.projection() == sd.projection and exh.lens() is None
        ref, ref_states, info = _session(ctx, exh, cfg)
        assert info["kernel_flags"] & LENS_BIT
        assert np.any(ref[: 3 * w * h] != 0)
        # the projection does reach the film
        exh.set_projection(None)
        pin, _, info = _session(ctx, exh, cfg)
        assert info["kernel_flags"] & LENS_BIT == 0
        assert n_bit_diff(pin, ref) > 0
    variants = {
        "bvh": dict(force_bvh=1, instancing=0, wavefront=0, specialise=0),
        "one_pass_at_a_time": dict(force_bvh=1, instancing=0, wavefront=0, specialise=0, max_fused_passes=1),
        "wavefront": dict(force_bvh=1, instancing=0, wavefront=1, specialise=0),
        "wavefront_carried": dict(force_bvh=1, instancing=0, wavefront=1, specialise=0, wf_carry=2),
        "sched_trial": dict(force_bvh=1, instancing=0, wavefront=-1, specialise=0, sched_trial=1),
        "instancing": dict(force_bvh=1, instancing=1, wavefront=0, specialise=0),
        "instancing_wavefront": dict(force_bvh=1, instancing=1, wavefront=1, specialise=0),
        "specialise": dict(force_bvh=0, instancing=0, wavefront=0, specialise=1),
        "specialise_bvh": dict(force_bvh=1, instancing=0, wavefront=0, specialise=1),
    }
    for name, opts in variants.items():
        with capi.options(**opts):
            scene = capi.Scene(ctx, sd)
            film, states, info = _session(ctx, scene, cfg)
        if name.startswith("specialise"):
            assert info["specialised"] == 1, info
        assert info["kernel_flags"] & LENS_BIT, name
        assert n_bit_diff(film, ref) == 0, f"{name}: {n_bit_diff(film, ref)} film floats differ"
        assert np.array_equal(states, ref_states), name
    with capi.options(force_bvh=1, instancing=0, wavefront=0, specialise=0):
        scene = capi.Scene(ctx, sd)
        acc = np.zeros(7 * w * h, np.float32)
        for r in range(8):
            film = capi.Film(ctx, w, h)
            capi.pt_render(ctx, scene, distributed.shard_config(cfg, r, 8, 8, 8), film)
            part = film.read()
            assert not np.any((acc != 0) & (part != 0))
            acc += part
    assert n_bit_diff(acc, ref) == 0
    if sampler != abi.SAMPLER_INDEPENDENT:
        with capi.options(force_bvh=0, instancing=0, wavefront=0, specialise=0):
            scene = capi.Scene(ctx, sd)
            film = capi.Film(ctx, w, h)
            for b, c in ((0, 5), (5, 4), (9, 3)):
                se = capi.PtSession(ctx, scene, make_config(spp=12, spp_per_pass=4, max_depth=6, sampler_type=sampler, sampler_seed=7,
                                                            sample_begin=b, sample_count=c), film)
                assert se.passes(1000, blocking=True) == c
                states = se.sampler_states(w * h)
                se.end()
        assert n_bit_diff(film.read(), ref) == 0
        assert np.array_equal(states, ref_states)


# ---------------------------------------------------------------------------------------------------------------- f. aov and guides
def _cbox_kinds(cbox_path, w, h, projection):
    sd = cbox_variant(scene_json.load_scene(cbox_path, w, h), "kinds")
    sd.projection = abi.ProjectionData(type=ORTHO, ortho_scale=2.5) if projection == "ortho" else abi.ProjectionData(type=PANORAMA, longitude_min=-0.25, longitude_max=0.25,
                                                                                                                        latitude_min=-0.125, latitude_max=0.125)
    return sd


@pytest.mark.parametrize("sampler", [abi.SAMPLER_PMJ02BN, abi.SAMPLER_SOBOL], ids=["pmj02bn", "sobol"])
@pytest.mark.parametrize("projection", ["ortho", "panorama"])
def test_aov_and_guides(ctx, cbox_path, projection, sampler):
    w, h = 40, 32
    cfg = make_config(spp=12, spp_per_pass=4, max_depth=6, sampler_type=sampler, sampler_seed=5)
    with capi.options(force_bvh=0, instancing=0, wavefront=0, specialise=0):
        scene = capi.Scene(ctx, _cbox_kinds(cbox_path, w, h, projection))
        film, albedo, normal = capi.Film(ctx, w, h), capi.Film(ctx, w, h), capi.Film(ctx, w, h)
        capi.pt_render_features(ctx, scene, cfg, film, albedo, normal)
        aovs = []
        for aov in (abi.AOV_ALBEDO, abi.AOV_NS):
            ac = abi.AovConfig.default()
            ac.spp, ac.aov, ac.remap = cfg.spp, aov, 0
            ac.filter_type, ac.filter_radius, ac.sampler_type, ac.sampler_seed, ac.color = cfg.filter_type, cfg.filter_radius, cfg.sampler_type, cfg.sampler_seed, cfg.color
            out = capi.Film(ctx, w, h)
            capi.aov_render(ctx, scene, ac, out)
            aovs.append(out.read())
        assert np.any(aovs[0][: 3 * w * h] != 0) and np.any(aovs[1][: 3 * w * h] != 0)
        assert n_bit_diff(albedo.read(), aovs[0]) == 0 and n_bit_diff(normal.read(), aovs[1]) == 0
        # the guides are the projection's, not the perspective camera's
        scene.set_projection(None)
        out = capi.Film(ctx, w, h)
        capi.aov_render(ctx, scene, ac, out)
        assert n_bit_diff(out.read(), aovs[1]) > 0


def test_denoiser_and_adaptive_driver_on_a_panorama_film(ctx, cbox_path):
    w, h = 64, 32
    sd = scene_json.load_scene(cbox_path, w, h)
    sd.projection = abi.ProjectionData(type=PANORAMA, longitude_min=-0.5, longitude_max=0.5, latitude_min=-0.25, latitude_max=0.25)
    scene = capi.Scene(ctx, sd)
    cfg = make_config(spp=16, spp_per_pass=4, max_depth=5, sampler_seed=2)
    film, albedo, normal, out = (capi.Film(ctx, w, h) for _ in range(4))
    capi.pt_render_features(ctx, scene, cfg, film, albedo, normal)
    capi.denoise(ctx, film, albedo, normal, out)
    den = out.read()
    assert np.all(np.isfinite(den)) and np.any(den[: 3 * w * h] != 0) and n_bit_diff(den, film.read()) > 0
    adaptive = capi.Film(ctx, w, h)
    stats, tile_spp = capi.pt_adaptive_render(ctx, scene, cfg, adaptive)
    a = adaptive.read()
    assert np.all(np.isfinite(a)) and np.any(a[: 3 * w * h] != 0)
    assert tile_spp.shape == (1, 2) and np.all(tile_spp >= 1) and np.all(tile_spp <= 16)


# ---------------------------------------------------------------------------------------------------------------- g. refusals, CLI
@pytest.mark.parametrize("projection", ["ortho", "panorama"])
def test_refusals(ctx, root, projection):
    sd = _projected(_route_scene(root, with_env=False), projection)
    word = "orthographic" if projection == "ortho" else "panorama"
    scene = capi.Scene(ctx, sd)
    w, h = sd.camera.width, sd.camera.height
    film = capi.Film(ctx, w, h)
    g = abi.GptConfig.default()
    g.spp, g.max_depth = 4, 4
    with pytest.raises(capi.AkariError) as e:
        capi.gpt_render(ctx, scene, g, film)
    assert e.value.code == capi.ERR_UNSUPPORTED and word in str(e.value)
    m = abi.McmcConfig.default()
    m.spp, m.max_depth, m.n_chains, m.n_bootstrap = 2, 4, 256, 1024
    with pytest.raises(capi.AkariError) as e:
        capi.mcmc_render(ctx, scene, m, film)
    assert e.value.code == capi.ERR_UNSUPPORTED and word in str(e.value)
    with capi.options(arith=1, wavefront=0, instancing=0):
        with pytest.raises(capi.AkariError) as e:
            capi.pt_render(ctx, scene, make_config(spp=4), film)
    assert e.value.code == capi.ERR_UNSUPPORTED and word in str(e.value)
    se = capi.PtSession(ctx, scene, make_config(spp=4), film)
    try:
        for args in (("panorama",), ("orthographic",), (None,)):
            with pytest.raises(capi.AkariError) as e:
                scene.set_projection(*args)
            assert e.value.code == capi.ERR_INVALID_ARGUMENT and "session" in str(e.value)
        assert scene.projection() == sd.projection
    finally:
        se.end()
    scene.set_projection(None)  # no session now: allowed, and the other integrators render again
    capi.gpt_render(ctx, scene, g, film)


def test_cli_projection(ctx, cbox_path, tmp_path):
    from akari_render_amd import build
    cli = build.build_cli()
    method = {"method": {"type": "pt", "spp": 16, "spp_per_pass": 16, "max_depth": 4}, "sampler": {"type": "independent", "seed": 1}}
    outs = {}
    for name, flags in (("plain", []), ("panorama", ["--projection", "panorama"]), ("perspective", ["--projection", "perspective"]),
                        ("ortho", ["--projection", "orthographic", "--ortho-scale", "2.5"])):
        out = tmp_path / f"{name}.exr"
        mpath = tmp_path / f"{name}.json"
        mpath.write_text(json.dumps(dict(method, film={"out": str(out)})))
        res = subprocess.run([cli, "-s", cbox_path, "-m", str(mpath), "--resolution", "64x32"] + flags, cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, (name, res.stdout, res.stderr)
        outs[name] = capi.host_decode_exr(open(out, "rb").read())
        assert outs[name].shape[:2] == (32, 64)
    for flags in (["--projection", "fisheye"], ["--projection"], ["--ortho-scale", "0"], ["--ortho-scale", "abc"]):
        res = subprocess.run([cli, "-s", cbox_path, "-m", str(tmp_path / "plain.json"), "--resolution", "64x32"] + flags, cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert res.returncode != 0, flags
    assert np.array_equal(outs["plain"], outs["perspective"])
    assert np.any(outs["panorama"] != outs["plain"]) and np.any(outs["ortho"] != outs["plain"]) and np.any(outs["ortho"] != outs["panorama"])
    # ... and the panorama is what the library renders for the file through the C ABI
    scene = capi.Scene(ctx, cbox_path, 64, 32)
    scene.set_projection("panorama")
    film = capi.Film(ctx, 64, 32)
    capi.pt_render(ctx, scene, make_config(spp=16, spp_per_pass=16, max_depth=4, sampler_seed=1), film)
    assert np.allclose(outs["panorama"][..., :3], resolve_np(film.read(), 64, 32).reshape(32, 64, 3), rtol=0, atol=0)
