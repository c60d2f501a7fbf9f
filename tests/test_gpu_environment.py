"""The environment light on the GPU (csrc/device/denv.h, the ENV kernels): an exact furnace, the orientation of the mapping, the
sampler's pdf and distribution, a quadrature of the direct lighting it gives, one film under every schedule and scene form, the
integrators that refuse it, and akari-cli on a scene.json with one. Every environment image is made here with numpy."""
import json
import os
import subprocess

import numpy as np
import pytest
from scipy import stats as sps

from akari_render_amd import abi, capi, distributed
from tests.helpers import instanced_scene, make_config, n_bit_diff, rel_rmse, resolve_np
from tests.test_environment import direction_uv, quad_scene, sample_image, scene_json_text

pytestmark = pytest.mark.gpu


def _render(ctx, sd_or_scene, cfg):
    scene = sd_or_scene if isinstance(sd_or_scene, capi.Scene) else capi.Scene(ctx, sd_or_scene)
    w, h = scene.info().width, scene.info().height
    film = capi.Film(ctx, w, h)
    st = capi.pt_render(ctx, scene, cfg, film)
    return resolve_np(film.read(), w, h), st


def _rot_y(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def _rot_x(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])


def test_exact_furnace(ctx):
    """Constant environment L, a diffuse quad of albedo rho, BSDF sampling only: every sample of a background pixel is L, every sample
    of a quad pixel rho L (up to the rounding of f cos / pdf)."""
    L, rho, W = 0.5, 0.6, 48
    sd = quad_scene(width=W, height=W, albedo=rho, cam_z=3.0, fov=1.2)
    sd.environment = abi.EnvironmentData(color=(L, L, L))
    img, st = _render(ctx, sd, make_config(spp=16, max_depth=4, use_nee=0))
    half = 3.0 * np.tan(0.6)  # half the frame's width at the quad
    x = ((np.arange(W) + 0.5) / W * 2 - 1) * half
    inside = (np.abs(x)[:, None] < 1 - 4 * 2 * half / W) & (np.abs(x)[None, :] < 1 - 4 * 2 * half / W)
    outside = (np.abs(x)[:, None] > 1 + 4 * 2 * half / W) | (np.abs(x)[None, :] > 1 + 4 * 2 * half / W)
    assert inside.sum() > 50 and outside.sum() > 50
    assert np.all(img[outside] == np.float32(L))
    assert np.allclose(img[inside], rho * L, rtol=1e-5, atol=0)


# ---------------------------------------------------------------------------------------------------------------- orientation
COLORS = {"sky": (0.9, 0.9, 1.0), "ground": (0.3, 0.2, 0.1), "+x": (1.0, 0.0, 0.0), "-x": (0.0, 1.0, 0.0), "+z": (0.0, 0.0, 1.0), "-z": (1.0, 1.0, 0.0)}


def _region(e):
    """Which of the six regions an environment-frame direction lies in."""
    if e[1] > 0.5:
        return "sky"
    if e[1] < -0.5:
        return "ground"
    phi = np.arctan2(e[2], e[0])
    if abs(phi) < np.pi / 4:
        return "+x"
    if np.pi / 4 <= phi < 3 * np.pi / 4:
        return "+z"
    if -3 * np.pi / 4 < phi <= -np.pi / 4:
        return "-z"
    return "-x"


def _six_region_image(W=64, H=32):
    u, v = (np.arange(W) + 0.5) / W, (np.arange(H) + 0.5) / H
    phi, lat = (u[None, :] - 0.5) * 2 * np.pi, (v[:, None] - 0.5) * np.pi
    e = np.stack([np.cos(lat) * np.cos(phi), np.sin(lat) * np.ones_like(phi), np.cos(lat) * np.sin(phi)], -1)
    img = np.zeros((H, W, 4), np.float32)
    img[:, :, 3] = 1
    for y in range(H):
        for x in range(W):
            img[y, x, :3] = COLORS[_region(e[y, x])]
    return img


def _looking_along(d, env, res=8):
    """A camera at the origin looking along d (narrow field), a tiny triangle far off every axis, and the environment."""
    d = np.asarray(d, float)
    upv = np.array([0.0, 0.0, 1.0]) if abs(d[1]) > 0.9 else np.array([0.0, 1.0, 0.0])
    right = np.cross(d, upv)
    right /= np.linalg.norm(right)
    up = np.cross(right, d)
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2] = right, up, -d
    tri = abi.MeshData(vertices=np.array([[50, 50, 50], [50.1, 50, 50], [50, 50.1, 50]], np.float32), indices=np.array([[0, 1, 2]], np.uint32))
    mat = abi.MaterialData(kind=abi.MAT_DIFFUSE, base_color=(0.5, 0.5, 0.5))
    cam = abi.CameraData(c2w=c2w.astype(np.float32).T.reshape(16).copy(), fov=0.1, width=res, height=res)
    return abi.SceneData([tri], [abi.InstanceData(0, [0], np.eye(4, dtype=np.float32).reshape(16).copy())], [mat], cam, environment=env)


@pytest.mark.parametrize("rotated", [False, True], ids=["identity", "rotated_90"])
def test_orientation_of_the_mapping(ctx, tmp_path, rotated):
    img = _six_region_image()
    tf = {"type": "trs", "data": {"translation": [0, 0, 0], "rotation": [0, np.pi / 2 if rotated else 0.0, 0], "scale": [1, 1, 1], "coordinate_system": "Akari"}}
    # through scene.json: the "transform" reader, nearest lookup from "interpolation"
    env = capi.Scene(None, scene_json_text(tmp_path, {"image": img, "interpolation": "nearest", "transform": tf})).environment()
    assert env.filter == abi.TEX_FILTER_NEAREST
    R = _rot_y(np.pi / 2) if rotated else np.eye(3)
    assert np.allclose(env.rotation, R, atol=1e-6)
    for d in ([1, 0, 0], [-1, 0, 0], [0, 0, 1], [0, 0, -1], [0, 1, 0], [0, -1, 0]):
        got, _ = _render(ctx, _looking_along(d, env), make_config(spp=4, max_depth=2))
        want = np.float32(COLORS[_region(R.T @ np.asarray(d, float))])
        assert np.all(got == want), f"looking along {d}: {got[4, 4]} instead of {want}"
    if rotated:  # the rotation does turn the sky: looking along +x shows the environment's +z sector
        assert _region(R.T @ np.array([1.0, 0, 0])) == "+z"


# ---------------------------------------------------------------------------------------------------------------- sampling
def _env_scene(ctx, img, R, filt=abi.TEX_FILTER_LINEAR, strength=1.0):
    sd = quad_scene(width=16, height=16)
    sd.environment = abi.EnvironmentData(image=img, rotation=R, filter=filt, strength=strength)
    return capi.Scene(ctx, sd)


def test_sampling_probe_pdf_and_distribution(ctx):
    W, H = 64, 32
    img = sample_image(W=W, H=H, seed=21)
    R = (_rot_y(0.7) @ _rot_x(0.3)).astype(np.float32)
    sc = _env_scene(ctx, img, R)
    n = 1_000_000
    u = np.random.default_rng(5).random((n, 2)).astype(np.float32)
    s = sc.probe_env_sample(u)
    wi, pdf, valid = s[:, :3].astype(np.float64), s[:, 3].astype(np.float64), s[:, 4]
    assert valid.mean() > 0.999
    e = wi @ R.astype(np.float64)  # R^T wi, row-wise
    uu, vv = direction_uv(e)
    fx, fy = uu * W, vv * H
    st = np.hypot(e[:, 0], e[:, 2])
    edge = np.minimum(np.abs(fx - np.round(fx)), np.abs(fy - np.round(fy)))
    keep = (valid > 0) & (edge > 1e-4) & (st > 1e-3)
    assert keep.mean() > 0.99
    q = sc.probe_env_pdf(wi[keep].astype(np.float32))
    assert np.allclose(q[:, 0], pdf[keep], rtol=1e-4), np.max(np.abs(q[:, 0] / pdf[keep] - 1))
    # chi^2 of the texel histogram against the tables
    marg = sc.array(capi.ARRAY_ENV_MARGINAL_PDF, np.float32).astype(np.float64)
    cond = sc.array(capi.ARRAY_ENV_CONDITIONAL_PDF, np.float32).astype(np.float64).reshape(H, W)
    p = (marg[:, None] * cond).ravel()
    tx = np.clip(np.floor(fx[valid > 0]).astype(int), 0, W - 1)
    ty = np.clip(np.floor(fy[valid > 0]).astype(int), 0, H - 1)
    counts = np.bincount(ty * W + tx, minlength=W * H).astype(np.float64)
    expect = p * counts.sum()
    big = expect >= 5
    assert counts[expect == 0].sum() == 0
    obs = np.append(counts[big], counts[~big].sum())
    exp = np.append(expect[big], expect[~big].sum())
    if exp[-1] == 0:
        obs, exp = obs[:-1], exp[:-1]
    chi2 = float(np.sum((obs - exp) ** 2 / exp))
    pval = float(sps.chi2.sf(chi2, len(obs) - 1))
    assert pval > 0.001, (chi2, len(obs), pval)


# ---------------------------------------------------------------------------------------------------------------- quadrature
def _bilinear(tex, u, v):
    """The kernels' bilinear lookup (texel centres at +0.5, lerp a + (b - a) t, u wraps, v clamps) in numpy."""
    H, W = tex.shape[:2]
    fx, fy = u * W - 0.5, v * H - 0.5
    x0, y0 = np.floor(fx), np.floor(fy)
    tx, ty = (fx - x0)[..., None], (fy - y0)[..., None]
    x0 = x0.astype(np.int64)
    y0 = y0.astype(np.int64)
    x1, y1 = (x0 + 1) % W, np.clip(y0 + 1, 0, H - 1)
    x0, y0 = x0 % W, np.clip(y0, 0, H - 1)
    a, b, c, d = tex[y0, x0], tex[y0, x1], tex[y1, x0], tex[y1, x1]
    ab, cd = a + (b - a) * tx, c + (d - c) * tx
    return ab + (cd - ab) * ty


def test_direct_lighting_matches_a_quadrature(ctx):
    """A diffuse plane under an HDR sky with a 5-degree sun of radiance 1000 (turned): its radiance is rho / pi * int L cos dOmega, both
    with NEE and with BSDF sampling alone; NEE has the lower error against a long render."""
    from akari_render_amd.procedural import sky_image
    sky = sky_image(256, 128, sun_dir=(0.3, 0.7, 0.4), sun_radius_deg=5.0, sun_radiance=1000.0)
    R = _rot_y(0.9) @ _rot_x(0.15)
    rho = 0.5
    v = np.array([[-20, 0, -20], [20, 0, -20], [20, 0, 20], [-20, 0, 20]], np.float32)
    plane = abi.MeshData(vertices=v, indices=np.array([[0, 2, 1], [0, 3, 2]], np.uint32))  # normal +y
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = [1, 0, 0], [0, 0, -1], [0, 1, 0], [0, 5, 0]  # looking down -y
    cam = abi.CameraData(c2w=c2w.astype(np.float32).T.reshape(16).copy(), fov=0.8, width=64, height=64)
    sd = abi.SceneData([plane], [abi.InstanceData(0, [0], np.eye(4, dtype=np.float32).reshape(16).copy())],
                       [abi.MaterialData(kind=abi.MAT_DIFFUSE, base_color=(rho,) * 3)], cam,
                       environment=abi.EnvironmentData(image=sky, rotation=R.astype(np.float32), filter=abi.TEX_FILTER_LINEAR))
    scene = capi.Scene(ctx, sd)
    tex = scene.array(capi.ARRAY_ENV_TEXELS, np.float32).reshape(128, 256, 4)[:, :, :3].astype(np.float64)
    Rf = np.asarray(scene.environment().rotation, np.float64)
    # quadrature over the upper hemisphere (world +y), midpoint rule
    nt, npf = 1200, 2400
    th = (np.arange(nt) + 0.5) * (np.pi / 2) / nt
    ph = (np.arange(npf) + 0.5) * (2 * np.pi) / npf
    E = np.zeros(3)
    for k in range(0, nt, 200):
        t = th[k:k + 200][:, None]
        d = np.stack([np.sin(t) * np.cos(ph), np.cos(t) * np.ones_like(ph), np.sin(t) * np.sin(ph)], -1)
        e = d @ Rf  # R^T d
        uu, vv = direction_uv(e)
        Lv = _bilinear(tex, uu, vv)
        E += np.sum(Lv * (np.cos(t) * np.sin(t))[..., None], axis=(0, 1)) * (np.pi / 2 / nt) * (2 * np.pi / npf)
    want = rho / np.pi * E
    nee, _ = _render(ctx, scene, make_config(spp=1024, max_depth=1, use_nee=1, sampler_seed=1))
    bsdf, _ = _render(ctx, scene, make_config(spp=1024, max_depth=1, use_nee=0, sampler_seed=2))
    ref, _ = _render(ctx, scene, make_config(spp=8192, spp_per_pass=64, max_depth=1, use_nee=1, sampler_seed=3))
    for img in (nee, bsdf):
        got = img.reshape(-1, 3).astype(np.float64).mean(axis=0)
        assert np.allclose(got, want, rtol=0.02), (got, want)
    assert rel_rmse(nee, ref) < rel_rmse(bsdf, ref)


# ---------------------------------------------------------------------------------------------------------------- schedules
def _schedule_scene(root, with_env=True):
    sd = instanced_scene(width=40, height=32, n_inst=4, n=2, emissive_instances=1, textured=True)
    sd.ggx_table = np.fromfile(os.path.join(root, "tests", "golden", "ggx_dielectric_s.f32"), dtype=np.float32)
    if with_env:
        img = sample_image(W=48, H=24, seed=4) * np.float32(0.6)
        sd.environment = abi.EnvironmentData(image=img, strength=1.5, rotation=_rot_y(-0.4).astype(np.float32), filter=abi.TEX_FILTER_LINEAR)
    return sd


def _session(ctx, scene, cfg):
    w, h = scene.info().width, scene.info().height
    film = capi.Film(ctx, w, h)
    se = capi.PtSession(ctx, scene, cfg, film)
    se.passes(1000, blocking=True)
    states = se.sampler_states(w * h)
    info = se.kernel_info()
    se.end()
    return film.read(), states, info


@pytest.mark.parametrize("sampler", [abi.SAMPLER_INDEPENDENT, abi.SAMPLER_PMJ02BN, abi.SAMPLER_SOBOL], ids=["independent", "pmj02bn", "sobol"])
def test_one_film_under_every_schedule(ctx, root, sampler):
    sd = _schedule_scene(root)
    w, h = sd.camera.width, sd.camera.height
    cfg = make_config(spp=12, spp_per_pass=4, max_depth=6, sampler_type=sampler, sampler_seed=7)
    with capi.options(force_bvh=0, instancing=0, wavefront=0, specialise=0):
        exh = capi.Scene(ctx, sd)
        assert exh.info().uses_bvh == 0
        ref, ref_states, _ = _session(ctx, exh, cfg)
    # the environment does reach the film: brighter than the same scene without it
    with capi.options(force_bvh=0, instancing=0, wavefront=0, specialise=0):
        dark, _, _ = _session(ctx, capi.Scene(ctx, _schedule_scene(root, with_env=False)), cfg)
    assert resolve_np(ref, w, h).mean() > 1.2 * resolve_np(dark, w, h).mean()
    variants = {
        "bvh": dict(force_bvh=1, instancing=0, wavefront=0, specialise=0),
        "wavefront": dict(force_bvh=1, instancing=0, wavefront=1, specialise=0),
        "wavefront_carried": dict(force_bvh=1, instancing=0, wavefront=1, specialise=0, wf_carry=2),  # (test hook: carry from launches of >= 2 rays)
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
        assert n_bit_diff(film, ref) == 0, f"{name}: {n_bit_diff(film, ref)} film floats differ"
        assert np.array_equal(states, ref_states), name
    # the summed 8-way tile shards
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
    # sample ranges, one after another on one film (index samplers): the same additions in the same order
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


def test_refusals_and_aov(ctx, root):
    sd = _schedule_scene(root)
    scene = capi.Scene(ctx, sd)
    w, h = sd.camera.width, sd.camera.height
    film = capi.Film(ctx, w, h)
    g = abi.GptConfig.default()
    g.spp, g.max_depth = 4, 4
    with pytest.raises(capi.AkariError) as e:
        capi.gpt_render(ctx, scene, g, film)
    assert e.value.code == capi.ERR_UNSUPPORTED
    m = abi.McmcConfig.default()
    m.spp, m.max_depth, m.n_chains, m.n_bootstrap = 2, 4, 256, 1024
    with pytest.raises(capi.AkariError) as e:
        capi.mcmc_render(ctx, scene, m, film)
    assert e.value.code == capi.ERR_UNSUPPORTED
    with capi.options(arith=1):
        with pytest.raises(capi.AkariError) as e:
            capi.pt_render(ctx, scene, make_config(spp=4), film)
    assert e.value.code == capi.ERR_UNSUPPORTED
    with pytest.raises(capi.AkariError):
        se = capi.PtSession(ctx, scene, make_config(spp=4), film)
        try:
            scene.set_environment()  # refused while a session holds the scene
        finally:
            se.end()
    a = abi.AovConfig.default()
    a.spp = 4
    capi.aov_render(ctx, scene, a, film)
    assert np.all(np.isfinite(film.read()))
    scene.set_environment()  # no session now: allowed


def test_cli_renders_the_environment(ctx, root, tmp_path):
    from akari_render_amd import build
    cli = build.build_cli()
    L = (0.25, 0.5, 0.75)
    spath = scene_json_text(tmp_path, {"color": list(L), "strength": 2.0}, fov=90.0)
    method = {"method": {"type": "pt", "spp": 4, "spp_per_pass": 4, "max_depth": 4}, "sampler": {"type": "independent", "seed": 1},
              "film": {"out": str(tmp_path / "out.exr")}}
    mpath = tmp_path / "pt.json"
    mpath.write_text(json.dumps(method))
    res = subprocess.run([cli, "-s", spath, "-m", str(mpath)], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    img = capi.host_decode_exr(open(tmp_path / "out.exr", "rb").read())
    assert img.shape[:2] == (16, 16)
    want = np.float32(L) * np.float32(2.0)
    for y, x in ((0, 0), (0, 15), (15, 0), (15, 15)):
        assert np.array_equal(img[y, x, :3], want), (y, x, img[y, x])
    assert not np.allclose(img[8, 8, :3], want)  # the quad
