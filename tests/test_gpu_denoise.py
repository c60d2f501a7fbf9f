"""akr_denoise on the GPU: both level kernels against the numpy restatement and the host build of the same text, bit for bit;
in-place output, the output film's planes, the NaN pixel, the refusals that need films; the `denoise` option through akr_render_task and
akari-cli against the manual composition."""
import json
import os
import subprocess

import numpy as np
import pytest

from akari_render_amd import abi, capi
from oracle import scene_json
from tests import denoise_model as dm
from tests.helpers import make_config
from tests.probe_matrix import same_bits_or_both_nan

pytestmark = pytest.mark.gpu
f32 = np.float32
CASES = dm.cases()
KERNELS = [0, 1]
KERNEL_IDS = ["gather", "tiled"]


def film_with(ctx, w, h, data, splat_scale=1.0):
    f = capi.Film(ctx, w, h)
    f.write(data)
    f.splat_scale = splat_scale
    return f


def device(ctx, w, h, color, albedo, normal, cfg, scales=(1.0, 1.0, 1.0), kernel=-1, in_place=False):
    """capi.denoise over host arrays -> (resolved output (H, W, 3), raw output film)."""
    fc = film_with(ctx, w, h, color, scales[0])
    fa = film_with(ctx, w, h, albedo, scales[1]) if albedo is not None else None
    fn = film_with(ctx, w, h, normal, scales[2]) if normal is not None else None
    out = fc if in_place else film_with(ctx, w, h, np.full(7 * w * h, 7.5, dtype=f32), 3.0)  # (whatever the output film held is overwritten)
    with capi.options(denoise_kernel=kernel):
        capi.denoise(ctx, fc, fa, fn, out, cfg)
    return out.resolve(), out.read()


@pytest.mark.parametrize("kernel", KERNELS, ids=KERNEL_IDS)
@pytest.mark.parametrize("shape", dm.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_device_equals_restatement_equals_host(ctx, oracle_lib, case, shape, kernel):
    name, kind, use_a, use_n, cfg, scales = case
    w, h = shape
    color, albedo, normal = dm.case_inputs(w, h, kind)
    albedo, normal = albedo if use_a else None, normal if use_n else None
    got, raw = device(ctx, w, h, color, albedo, normal, cfg, scales, kernel)
    ref = dm.case_reference(w, h, name)
    same = same_bits_or_both_nan(got, ref)
    assert same.all(), f"{name} {w}x{h} kernel {kernel}: {np.count_nonzero(~same)} of {same.size} floats differ from the restatement"
    assert same_bits_or_both_nan(got, capi.host_denoise(w, h, color, albedo, normal, cfg, scales)).all()
    # the output film's planes: rgb = the result, splat = 0, weight = 1
    n = w * h
    assert np.array_equal(raw[:3 * n].view(np.uint32), got.reshape(-1).view(np.uint32))
    assert np.all(raw[3 * n:6 * n].view(np.uint32) == 0) and np.all(raw[6 * n:] == 1.0)


@pytest.mark.parametrize("kernel", KERNELS, ids=KERNEL_IDS)
def test_the_output_may_be_the_colour_film(ctx, kernel):
    w, h = 70, 45
    color, albedo, normal = dm.case_inputs(w, h, "splat")
    scales = (0.25, 0.5, 2.0)
    separate, _ = device(ctx, w, h, color, albedo, normal, dm.config(), scales, kernel)
    in_place, raw = device(ctx, w, h, color, albedo, normal, dm.config(), scales, kernel, in_place=True)
    assert np.array_equal(separate.view(np.uint32), in_place.view(np.uint32))
    assert np.all(raw[3 * w * h:6 * w * h] == 0) and np.all(raw[6 * w * h:] == 1.0)


@pytest.mark.parametrize("kernel", KERNELS, ids=KERNEL_IDS)
def test_one_nan_pixel_stays_one_nan_pixel(ctx, kernel):
    dm.check_nan_pixel(lambda c, a, n: device(ctx, 41, 23, c, a, n, dm.config(), kernel=kernel)[0])


def test_refusals_that_need_films(ctx):
    a, b = capi.Film(ctx, 8, 6), capi.Film(ctx, 6, 8)
    for args in ((a, b, None, a), (a, None, b, a), (a, None, None, b)):
        with pytest.raises(capi.AkariError) as e:
            capi.denoise(ctx, *args)
        assert e.value.code == capi.ERR_INVALID_ARGUMENT and "size" in str(e.value)
    other = capi.Context(0)
    foreign = capi.Film(other, 8, 6)
    with pytest.raises(capi.AkariError) as e:
        capi.denoise(ctx, a, foreign, None, a)
    assert e.value.code == capi.ERR_INVALID_ARGUMENT and "context" in str(e.value)
    with pytest.raises(capi.AkariError) as e:
        capi.denoise(ctx, a, None, None, a, dm.config(iterations=9))
    assert e.value.code == capi.ERR_INVALID_ARGUMENT
    foreign.close()
    other.close()


METHOD = {"method": {"type": "pt", "spp": 16, "spp_per_pass": 16, "max_depth": 12, "rr_depth": 5}, "sampler": {"type": "independent", "seed": 3},
          "film": {"filter": {"type": "gaussian", "radius": 1.5}}}


def read_exr_rgb(path):
    return capi.host_decode_exr(open(path, "rb").read())[..., :3]


def test_render_task_with_the_denoise_option(ctx, cbox_path, tmp_path):
    """cbox at 96 x 96 and 16 spp: film.out is what it is without the option, the .denoised file is the manual composition bit for bit and
    closer to a 1024-spp render than the noisy film (the bar is the factor 1)."""
    w = h = 96
    scene = capi.Scene(ctx, cbox_path, w, h)
    plain, with_option = dict(METHOD), dict(METHOD)
    plain["film"] = dict(METHOD["film"], out=str(tmp_path / "plain" / "pt.exr"))
    with_option["film"] = dict(METHOD["film"], out=str(tmp_path / "dn" / "pt.exr"))
    capi.render_task(ctx, scene, json.dumps(plain))
    assert not os.path.exists(tmp_path / "plain" / "pt.denoised.exr")
    with capi.options(denoise=16):
        capi.render_task(ctx, scene, json.dumps(with_option))
    assert open(tmp_path / "plain" / "pt.exr", "rb").read() == open(tmp_path / "dn" / "pt.exr", "rb").read()
    written = read_exr_rgb(tmp_path / "dn" / "pt.denoised.exr")
    # the manual composition
    cfg = make_config(spp=16, spp_per_pass=16, sampler_seed=3)
    color, albedo, normal = (capi.Film(ctx, w, h) for _ in range(3))
    capi.pt_render(ctx, scene, cfg, color)
    noisy = color.resolve()
    for film, aov in ((albedo, abi.AOV_ALBEDO), (normal, abi.AOV_NS)):
        ac = abi.AovConfig.default()
        ac.spp, ac.aov, ac.remap, ac.sampler_seed = 16, aov, 0, 3
        capi.aov_render(ctx, scene, ac, film)
    capi.denoise(ctx, color, albedo, normal, color)
    manual = color.resolve()
    assert np.array_equal(written.view(np.uint32), manual.view(np.uint32))
    assert np.array_equal(read_exr_rgb(tmp_path / "dn" / "pt.exr").view(np.uint32), noisy.view(np.uint32))
    ref_film = capi.Film(ctx, w, h)
    capi.pt_render(ctx, scene, make_config(spp=1024, spp_per_pass=64, sampler_seed=11), ref_film)
    ref = ref_film.resolve()
    before, after = dm.rel_mse(noisy, ref), dm.rel_mse(manual, ref)
    print(f"relMSE against 1024 spp: noisy {before:.5f} denoised {after:.5f} ratio {after / before:.3f}")
    assert after < before


def test_cli_denoise(ctx, root, tmp_path):
    from akari_render_amd import build
    cli = build.build_cli()
    method = dict(METHOD)
    method["film"] = dict(METHOD["film"], out=str(tmp_path / "out" / "img.exr"))
    mpath = tmp_path / "m.json"
    mpath.write_text(json.dumps(method))
    for extra in (["--denoise"], ["--denoise", "8"]):
        res = subprocess.run([cli, "-s", os.path.join(root, "scenes/cbox/scene.json"), "-m", str(mpath), "--resolution", "96x96"] + extra,
                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=tmp_path)
        assert res.returncode == 0, res.stdout[-2000:]
        assert os.path.getsize(tmp_path / "out" / "img.exr") > 96 * 96 * 12 and os.path.getsize(tmp_path / "out" / "img.denoised.exr") > 96 * 96 * 12
        os.remove(tmp_path / "out" / "img.denoised.exr")
