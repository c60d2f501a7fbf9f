"""akr_display_transform on the GPU: the kernels under both blur implementations against the numpy restatement and the host
build of the same text, bit for bit; the histogram kernel against the restated counts, the contention case included; in-place output, the
output film's planes, the refusals that need films; the `display` option through akr_render_task and akari-cli against the manual
composition."""
import json
import os
import subprocess

import numpy as np
import pytest

from akari_render_amd import abi, capi
from tests import display_model as dm
from tests.denoise_model import film_of
from tests.helpers import make_config
from tests.probe_matrix import same_bits_or_both_nan

pytestmark = pytest.mark.gpu
f32 = np.float32
CASES = dm.cases()
KERNELS = [0, 1]
KERNEL_IDS = ["gather", "lds"]


def film_with(ctx, w, h, data, splat_scale=1.0):
    f = capi.Film(ctx, w, h)
    f.write(data)
    f.splat_scale = splat_scale
    return f


def device(ctx, w, h, film, cfg, splat_scale=1.0, kernel=-1, in_place=False):
    """capi.display_transform over a host array -> (resolved output (H, W, 3), raw output film, k)."""
    src = film_with(ctx, w, h, film, splat_scale)
    out = src if in_place else film_with(ctx, w, h, np.full(7 * w * h, 7.5, dtype=f32), 3.0)  # (whatever the output film held is overwritten)
    with capi.options(display_kernel=kernel):
        k = capi.display_transform(ctx, src, out, cfg)
    return out.resolve(), out.read(), k


@pytest.mark.parametrize("kernel", KERNELS, ids=KERNEL_IDS)
@pytest.mark.parametrize("shape", dm.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_device_equals_restatement_equals_host(ctx, oracle_lib, case, shape, kernel):
    name, cfg = case
    w, h = shape
    n = w * h
    for kind in dm.KINDS:
        film, scale = dm.case_film(w, h, kind), dm.SPLAT_SCALE[kind]
        got, raw, k = device(ctx, w, h, film, cfg, scale, kernel)
        ref, k_ref = dm.case_reference(w, h, kind, name)
        assert f32(k).view(np.uint32) == f32(k_ref).view(np.uint32), f"{name} {w}x{h} {kind}: exposure {k} against {k_ref}"
        same = same_bits_or_both_nan(got, ref)
        assert same.all(), f"{name} {w}x{h} {kind} kernel {kernel}: {np.count_nonzero(~same)} of {same.size} floats differ from the restatement"
        host, k_host = capi.host_display_transform(w, h, film, cfg, scale)
        assert same_bits_or_both_nan(got, host).all() and f32(k_host).view(np.uint32) == f32(k).view(np.uint32)
        # the output film's planes: rgb = the result, splat = 0, weight = 1
        assert np.array_equal(raw[:3 * n].view(np.uint32), got.reshape(-1).view(np.uint32))
        assert np.all(raw[3 * n:6 * n].view(np.uint32) == 0) and np.all(raw[6 * n:] == 1.0)


@pytest.mark.parametrize("kind", dm.KINDS)
@pytest.mark.parametrize("shape", dm.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_histogram_equals_the_restated_counts(ctx, oracle_lib, shape, kind):
    w, h = shape
    counts, skipped = capi.film_luminance_histogram(ctx, film_with(ctx, w, h, dm.case_film(w, h, kind), dm.SPLAT_SCALE[kind]))
    ref_counts, ref_skipped = dm.case_histogram(w, h, kind)
    assert np.array_equal(counts, ref_counts) and skipped == ref_skipped


def test_histogram_of_a_constant_image(ctx, oracle_lib):
    """256 x 256 pixels of one value: 65 536 hits on one bin, every lane of every wave on the same counter. And of a value below 2^-20: all skipped."""
    w = h = 256
    for value in (0.37, 1e-8):
        film = film_of(np.full((h, w, 3), value, dtype=f32))
        counts, skipped = capi.film_luminance_histogram(ctx, film_with(ctx, w, h, film))
        ref_counts, ref_skipped = dm.histogram(dm.load(film, w, h))
        assert np.array_equal(counts, ref_counts) and skipped == ref_skipped
        assert int(counts.max()) + skipped == w * h and np.count_nonzero(counts) == (1 if value > 1e-6 else 0)


@pytest.mark.parametrize("kernel", KERNELS, ids=KERNEL_IDS)
def test_the_output_may_be_the_film(ctx, kernel):
    w, h = 130, 67
    cfg = dm.config(curve=abi.DISPLAY_HABLE, auto_exposure=1, bloom_strength=0.5, bloom_levels=5)
    film = dm.case_film(w, h, "random")
    separate, _, k0 = device(ctx, w, h, film, cfg, 0.375, kernel)
    in_place, raw, k1 = device(ctx, w, h, film, cfg, 0.375, kernel, in_place=True)
    assert k0 == k1 and np.array_equal(separate.view(np.uint32), in_place.view(np.uint32))
    assert np.all(raw[3 * w * h:6 * w * h] == 0) and np.all(raw[6 * w * h:] == 1.0)


def test_refusals_that_need_films(ctx):
    a, b = capi.Film(ctx, 8, 6), capi.Film(ctx, 6, 8)
    with pytest.raises(capi.AkariError) as e:
        capi.display_transform(ctx, a, b)
    assert e.value.code == capi.ERR_INVALID_ARGUMENT and "size" in str(e.value)
    other = capi.Context(0)
    foreign = capi.Film(other, 8, 6)
    for args in ((a, foreign), (foreign, a)):
        with pytest.raises(capi.AkariError) as e:
            capi.display_transform(ctx, *args)
        assert e.value.code == capi.ERR_INVALID_ARGUMENT and "context" in str(e.value)
    with pytest.raises(capi.AkariError) as e:
        capi.film_luminance_histogram(ctx, foreign)
    assert e.value.code == capi.ERR_INVALID_ARGUMENT and "context" in str(e.value)
    with pytest.raises(capi.AkariError) as e:
        capi.display_transform(ctx, a, a, dm.config(curve=7))
    assert e.value.code == capi.ERR_INVALID_ARGUMENT
    foreign.close()
    other.close()


METHOD = {"method": {"type": "pt", "spp": 4, "spp_per_pass": 4, "max_depth": 12, "rr_depth": 5}, "sampler": {"type": "independent", "seed": 3},
          "film": {"filter": {"type": "gaussian", "radius": 1.5}}}
W = H = 64


def front_end_config():
    """What --display aces --auto-exposure --bloom 0.25 and options(display=3, display_auto_exposure=1, display_bloom=256) ask for."""
    c = abi.DisplayConfig.default()
    c.curve, c.auto_exposure, c.bloom_strength = abi.DISPLAY_ACES, 1, 0.25
    return c


def manual_png(ctx, scene, path, denoise_spp=0):
    """render -> (denoise ->) capi.display_transform -> akr_image_write; -> the file's bytes."""
    color = capi.Film(ctx, W, H)
    capi.pt_render(ctx, scene, make_config(spp=4, spp_per_pass=4, sampler_seed=3), color)
    if denoise_spp:
        albedo, normal = capi.Film(ctx, W, H), capi.Film(ctx, W, H)
        for film, aov in ((albedo, abi.AOV_ALBEDO), (normal, abi.AOV_NS)):
            ac = abi.AovConfig.default()
            ac.spp, ac.aov, ac.remap, ac.sampler_seed = denoise_spp, aov, 0, 3
            capi.aov_render(ctx, scene, ac, film)
        capi.denoise(ctx, color, albedo, normal, color)
    capi.display_transform(ctx, color, color, front_end_config())
    capi.image_write(path, color.resolve())
    return open(path, "rb").read()


def task(tmp_path, sub):
    m = dict(METHOD)
    m["film"] = dict(METHOD["film"], out=str(tmp_path / sub / "pt.exr"))
    return json.dumps(m)


@pytest.mark.parametrize("denoise_spp", [0, 4], ids=["plain", "denoised"])
def test_render_task_with_the_display_option(ctx, cbox_path, tmp_path, denoise_spp):
    """cbox at 64 x 64 and 4 spp: {stem}.display.png is the manual composition byte for byte (made from the denoised film when `denoise` is on);
    without the option there is no such file; film.out and the denoised image are the same files with and without it."""
    scene = capi.Scene(ctx, cbox_path, W, H)
    with capi.options(denoise=denoise_spp):
        capi.render_task(ctx, scene, task(tmp_path, "off"))
        with capi.options(display=3, display_auto_exposure=1, display_bloom=256):
            capi.render_task(ctx, scene, task(tmp_path, "on"))
    assert sorted(os.listdir(tmp_path / "off")) == (["pt.denoised.exr", "pt.exr"] if denoise_spp else ["pt.exr"])
    assert sorted(os.listdir(tmp_path / "on")) == sorted(os.listdir(tmp_path / "off") + ["pt.display.png"])
    for name in os.listdir(tmp_path / "off"):
        assert open(tmp_path / "off" / name, "rb").read() == open(tmp_path / "on" / name, "rb").read()
    assert open(tmp_path / "on" / "pt.display.png", "rb").read() == manual_png(ctx, scene, tmp_path / "manual.png", denoise_spp)
    # and the file is a picture of the box, not of nothing: decoded, it has dark and bright pixels
    img = capi.host_decode_png(open(tmp_path / "on" / "pt.display.png", "rb").read())
    assert img.shape[:2] == (H, W) and img[..., :3].min() < 64 and img[..., :3].max() > 192


def test_render_task_display_after_an_adaptive_render(ctx, cbox_path, tmp_path):
    scene = capi.Scene(ctx, cbox_path, W, H)
    m = dict(METHOD)
    m["method"] = dict(METHOD["method"], spp=8, spp_per_pass=2)
    m["film"] = dict(METHOD["film"], out=str(tmp_path / "ad" / "pt.exr"))
    with capi.options(adaptive=64, display=4):
        capi.render_task(ctx, scene, json.dumps(m))
    exr = capi.host_decode_exr(open(tmp_path / "ad" / "pt.exr", "rb").read())[..., :3]
    film = capi.Film(ctx, W, H)
    film.write(film_of(exr))
    capi.display_transform(ctx, film, film, dm.config(curve=abi.DISPLAY_HABLE))
    capi.image_write(tmp_path / "manual.png", film.resolve())
    assert open(tmp_path / "ad" / "pt.display.png", "rb").read() == open(tmp_path / "manual.png", "rb").read()


def test_cli_display(ctx, root, cbox_path, tmp_path):
    from akari_render_amd import build
    cli = build.build_cli()
    method = dict(METHOD)
    method["film"] = dict(METHOD["film"], out=str(tmp_path / "out" / "img.exr"))
    mpath = tmp_path / "m.json"
    mpath.write_text(json.dumps(method))
    res = subprocess.run([cli, "-s", os.path.join(root, "scenes/cbox/scene.json"), "-m", str(mpath), "--resolution", f"{W}x{H}",
                          "--display", "aces", "--auto-exposure", "--bloom", "0.25"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=tmp_path)
    assert res.returncode == 0, res.stdout[-2000:]
    assert sorted(os.listdir(tmp_path / "out")) == ["img.display.png", "img.exr"]
    scene = capi.Scene(ctx, cbox_path, W, H)
    assert open(tmp_path / "out" / "img.display.png", "rb").read() == manual_png(ctx, scene, tmp_path / "manual.png")
