"""akr_denoise_variance on the GPU (DESIGN.md 4.10 "Variance guide"): both level kernels against the numpy restatement and the host build of
the same text, bit for bit; the output film's planes, in-place output, the refusals that need films; the `denoise_variance` option through
akr_render_task and akari-cli against the manual composition."""
import json
import os
import subprocess

import numpy as np
import pytest

from akari_render_amd import abi, capi
from tests import denoise_model as dm
from tests import denoise_variance_model as dvm
from tests.helpers import make_config
from tests.probe_matrix import same_bits_or_both_nan

pytestmark = pytest.mark.gpu
f32 = np.float32
CASES = dvm.cases()
KERNELS = [0, 1]
KERNEL_IDS = ["gather", "tiled"]


def film_with(ctx, w, h, data, splat_scale=1.0):
    f = capi.Film(ctx, w, h)
    f.write(data)
    f.splat_scale = splat_scale
    return f


def device(ctx, w, h, color, half, albedo, normal, cfg, kernel=-1, in_place=False):
    """capi.denoise_variance over host arrays -> (resolved output (H, W, 3), raw output film)."""
    fc, fh = film_with(ctx, w, h, color), film_with(ctx, w, h, half)
    fa = film_with(ctx, w, h, albedo) if albedo is not None else None
    fn = film_with(ctx, w, h, normal) if normal is not None else None
    out = fc if in_place else film_with(ctx, w, h, np.full(7 * w * h, 7.5, dtype=f32), 3.0)  # (whatever the output film held is overwritten)
    with capi.options(denoise_kernel=kernel):
        capi.denoise_variance(ctx, fc, fh, fa, fn, out, cfg)
    return out.resolve(), out.read()


@pytest.mark.parametrize("kernel", KERNELS, ids=KERNEL_IDS)
@pytest.mark.parametrize("shape", dvm.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_device_equals_restatement_equals_host(ctx, oracle_lib, case, shape, kernel):
    name, kind, halves, use_a, use_n, cfg = case
    w, h = shape
    color, half, albedo, normal = dvm.case_inputs(w, h, kind, halves)
    albedo, normal = albedo if use_a else None, normal if use_n else None
    got, raw = device(ctx, w, h, color, half, albedo, normal, cfg, kernel)
    ref = dvm.case_reference(w, h, name)
    same = same_bits_or_both_nan(got, ref)
    assert same.all(), f"{name} {w}x{h} kernel {kernel}: {np.count_nonzero(~same)} of {same.size} floats differ from the restatement"
    assert same_bits_or_both_nan(got, capi.host_denoise_variance(w, h, color, half, albedo, normal, cfg)).all()
    # the output film's planes: rgb = the result, splat = 0, weight = 1
    n = w * h
    assert np.array_equal(raw[:3 * n].view(np.uint32), got.reshape(-1).view(np.uint32))
    assert np.all(raw[3 * n:6 * n].view(np.uint32) == 0) and np.all(raw[6 * n:] == 1.0)


@pytest.mark.parametrize("kernel", KERNELS, ids=KERNEL_IDS)
def test_the_output_may_be_the_colour_film(ctx, kernel):
    w, h = 70, 45
    color, half, albedo, normal = dvm.case_inputs(w, h, "intweights", "unequal")
    separate, _ = device(ctx, w, h, color, half, albedo, normal, dvm.config(), kernel)
    in_place, raw = device(ctx, w, h, color, half, albedo, normal, dvm.config(), kernel, in_place=True)
    assert np.array_equal(separate.view(np.uint32), in_place.view(np.uint32))
    assert np.all(raw[3 * w * h:6 * w * h] == 0) and np.all(raw[6 * w * h:] == 1.0)


@pytest.mark.parametrize("kernel", KERNELS, ids=KERNEL_IDS)
def test_one_nan_pixel_stays_one_nan_pixel(ctx, kernel):
    def run(c, a, n):
        half = (np.asarray(c, dtype=f32) * f32(0.5)).astype(f32)
        k = 41 * 23
        half[:3 * k] = (half[:3 * k] * np.random.default_rng(9).uniform(0.8, 1.2, size=3 * k)).astype(f32)
        return device(ctx, 41, 23, c, half, a, n, dvm.config(), kernel=kernel)[0]
    dm.check_nan_pixel(run)


def test_refusals_that_need_films(ctx):
    a, a2, b = capi.Film(ctx, 8, 6), capi.Film(ctx, 8, 6), capi.Film(ctx, 6, 8)
    with pytest.raises(capi.AkariError) as e:
        capi.denoise_variance(ctx, a, a2, None, None, a2)  # half == out
    assert e.value.code == capi.ERR_INVALID_ARGUMENT and "half" in str(e.value)
    with pytest.raises(capi.AkariError) as e:
        capi.denoise_variance(ctx, a, None, None, None, a)  # no half
    assert e.value.code == capi.ERR_INVALID_ARGUMENT
    for args in ((a, b, None, None, a), (a, a2, b, None, a), (a, a2, None, b, a), (a, a2, None, None, b)):
        with pytest.raises(capi.AkariError) as e:
            capi.denoise_variance(ctx, *args)
        assert e.value.code == capi.ERR_INVALID_ARGUMENT and "size" in str(e.value)
    other = capi.Context(0)
    foreign = capi.Film(other, 8, 6)
    with pytest.raises(capi.AkariError) as e:
        capi.denoise_variance(ctx, a, foreign, None, None, a)
    assert e.value.code == capi.ERR_INVALID_ARGUMENT and "context" in str(e.value)
    for bad in (dict(iterations=9), dict(sigma_variance=0.0), dict(sigma_variance=1e-15)):
        with pytest.raises(capi.AkariError) as e:
            capi.denoise_variance(ctx, a, a2, None, None, a, dvm.config(**bad))
        assert e.value.code == capi.ERR_INVALID_ARGUMENT
    capi.denoise_variance(ctx, a, a2, None, None, a)  # (and the same films with the default configuration pass)
    foreign.close()
    other.close()


def method(spp_per_pass):
    return {"method": {"type": "pt", "spp": 16, "spp_per_pass": spp_per_pass, "max_depth": 12, "rr_depth": 5}, "sampler": {"type": "independent", "seed": 3},
            "film": {"filter": {"type": "gaussian", "radius": 1.5}}}


def read_exr_rgb(path):
    return capi.host_decode_exr(open(path, "rb").read())[..., :3]


def test_render_task_with_the_denoise_variance_option(ctx, cbox_path, tmp_path):
    """cbox at 96 x 96, 16 spp in two passes of 8: film.out is what it is without the options, the .denoised file is the manual composition
    (one pass, the film read back as the half, one pass, the aov guides, akr_denoise_variance) bit for bit; a task of one pass is refused."""
    w = h = 96
    scene = capi.Scene(ctx, cbox_path, w, h)
    plain, with_option = method(8), method(8)
    plain["film"]["out"] = str(tmp_path / "plain" / "pt.exr")
    with_option["film"]["out"] = str(tmp_path / "dn" / "pt.exr")
    capi.render_task(ctx, scene, json.dumps(plain))
    with capi.options(denoise=16, denoise_variance=1):
        capi.render_task(ctx, scene, json.dumps(with_option))
    assert open(tmp_path / "plain" / "pt.exr", "rb").read() == open(tmp_path / "dn" / "pt.exr", "rb").read()
    written = read_exr_rgb(tmp_path / "dn" / "pt.denoised.exr")
    # the manual composition
    cfg = make_config(spp=16, spp_per_pass=8, sampler_seed=3)
    color, half, albedo, normal = (capi.Film(ctx, w, h) for _ in range(4))
    se = capi.PtSession(ctx, scene, cfg, color)
    assert se.passes(1, blocking=True) == 8
    half.write(color.read())
    assert se.passes(1, blocking=True) == 16
    se.end()
    for film, aov in ((albedo, abi.AOV_ALBEDO), (normal, abi.AOV_NS)):
        ac = abi.AovConfig.default()
        ac.spp, ac.aov, ac.remap, ac.sampler_seed = 16, aov, 0, 3
        capi.aov_render(ctx, scene, ac, film)
    capi.denoise_variance(ctx, color, half, albedo, normal, color)
    manual = color.resolve()
    assert np.array_equal(written.view(np.uint32), manual.view(np.uint32))
    # not what the fixed-sigma step writes
    with capi.options(denoise=16):
        capi.render_task(ctx, scene, json.dumps(with_option))
    assert not np.array_equal(read_exr_rgb(tmp_path / "dn" / "pt.denoised.exr").view(np.uint32), manual.view(np.uint32))
    # one pass: no half, no silent fall-back
    single = method(16)
    single["film"]["out"] = str(tmp_path / "single" / "pt.exr")
    with capi.options(denoise=16, denoise_variance=1):
        with pytest.raises(capi.AkariError) as e:
            capi.render_task(ctx, scene, json.dumps(single))
    assert e.value.code == capi.ERR_INVALID_ARGUMENT and "spp = 16" in str(e.value) and "spp_per_pass = 16" in str(e.value)
    assert not os.path.exists(tmp_path / "single" / "pt.denoised.exr")
    with capi.options(denoise_variance=1):  # without `denoise` the option does nothing
        capi.render_task(ctx, scene, json.dumps(single))
    assert os.path.exists(tmp_path / "single" / "pt.exr") and not os.path.exists(tmp_path / "single" / "pt.denoised.exr")


def test_cli_denoise_variance(ctx, root, tmp_path):
    from akari_render_amd import build
    cli = build.build_cli()
    m = method(8)
    m["film"]["out"] = str(tmp_path / "out" / "img.exr")
    mpath = tmp_path / "m.json"
    mpath.write_text(json.dumps(m))
    res = subprocess.run([cli, "-s", os.path.join(root, "scenes/cbox/scene.json"), "-m", str(mpath), "--resolution", "96x96", "--denoise", "16", "--denoise-variance"],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=tmp_path)
    assert res.returncode == 0, res.stdout[-2000:]
    assert os.path.getsize(tmp_path / "out" / "img.exr") > 96 * 96 * 12 and os.path.getsize(tmp_path / "out" / "img.denoised.exr") > 96 * 96 * 12
