"""Device probes over the whole matrix (inputs, references and recorded bounds: tests/probe_matrix.py): every elementary function of the
arithmetic contract bit for bit against the oracle and within the oracle's own error of float64, the texture sampler in all 16 modes x 6
shapes, the BSDF on its thresholds. The CPU halves of the same checks are in tests/test_oracle_kat.py and tests/test_textures.py.

NaN rule: where both sides may legitimately be NaN, two NaNs are equal whatever their payload (as in tests/test_gpu_div_unscaled.py);
everything else is compared as uint32."""
import numpy as np
import pytest

from akari_render_amd import abi, capi
from oracle import pyoracle
from tests import probe_matrix as pm
from tests.helpers import make_config, n_bit_diff, textured_room

pytestmark = pytest.mark.gpu

EXP, POW, ATAN2, SQRT, RCP, SRGB = range(6)  # columns of capi.probe_math2


def assert_same(dev, ora, what):
    dev, ora = np.asarray(dev), np.asarray(ora)
    assert dev.shape == ora.shape, what
    bad = np.argwhere(~pm.same_bits_or_both_nan(dev, ora))
    first = [(tuple(int(k) for k in i), float(dev[tuple(i)]), float(ora[tuple(i)])) for i in bad[:5]]
    assert len(bad) == 0, f"{what}: {len(bad)} of {dev.size} differ; (index, device, oracle): {first}"


@pytest.fixture(scope="module")
def device_math(ctx):
    """Every elementary function on its own input set, once for the bit-exact and the accuracy tests."""
    x = pm.exp_inputs()
    px, py = pm.pow_inputs()
    ay, ax = pm.atan2_inputs()
    sx = pm.srgb_inputs()
    t = pm.sincos_inputs()
    s, c, l = capi.probe_math(ctx, t)
    return {"exp": capi.probe_math2(ctx, x, np.zeros_like(x))[:, EXP].copy(), "pow": capi.probe_math2(ctx, px, py)[:, POW].copy(),
            "atan2": capi.probe_math2(ctx, ax, ay)[:, ATAN2].copy(), "srgb": capi.probe_math2(ctx, sx, np.zeros_like(sx))[:, SRGB].copy(),
            "sin": s, "cos": c, "log": l}


# ------------------------------------------------------------------------------------------------ B1: bit for bit
def test_exp_matches_oracle(device_math, oracle_lib):
    x = pm.exp_inputs()
    assert x.size > 16000 and np.isnan(x).sum() == 1
    assert_same(device_math["exp"], pm.oracle_exp(x), "exp_f")
    # the cut-offs: inf above 88.7228... (float32(88.72283905...) lies above ln(FLT_MAX): there the scaling itself overflows), 0 below -103.2789...
    e = lambda v: device_math["exp"][np.nonzero(x == v)[0][0]]  # noqa: E731
    assert np.isfinite(e(np.nextafter(pm.EXP_HI, -pm.INF))) and e(np.nextafter(pm.EXP_HI, pm.INF)) == np.inf
    assert e(pm.EXP_LO) > 0.0 and e(np.nextafter(pm.EXP_LO, -pm.INF)) == 0.0


def test_pow_matches_oracle(device_math, oracle_lib):
    px, py = pm.pow_inputs()
    assert_same(device_math["pow"], pm.oracle_pow(px, py), "pow_f")
    assert np.all(device_math["pow"][px == 0] == 0.0) and np.all(device_math["pow"][px == 1] == 1.0)


def test_atan2_matches_oracle(device_math, oracle_lib):
    ay, ax = pm.atan2_inputs()
    assert_same(device_math["atan2"], pyoracle.atan2_many(ay, ax), "atan2_f")
    assert not np.isnan(device_math["atan2"]).any()


def test_sincos_log_match_oracle_on_negative_arguments(device_math, oracle_lib):
    """[-2 pi, 4 pi] and +-k pi / 2 +- 1 ulp: (int)kf is negative on half of the set (denv.h calls sincos_f on [-pi, pi] and [-pi / 2, pi / 2]);
    log_f of the same numbers is NaN below zero, -inf at zero."""
    t = pm.sincos_inputs()
    assert (t < 0).sum() > 5000
    so, co = pm.oracle_sincos(t)
    assert np.array_equal(device_math["sin"].view(np.uint32), so.view(np.uint32))
    assert np.array_equal(device_math["cos"].view(np.uint32), co.view(np.uint32))
    assert_same(device_math["log"], pm.oracle_log(t), "log_f")
    assert np.isnan(device_math["log"][t < 0]).all()


def test_sqrt_and_rcp_are_correctly_rounded(ctx):
    x = pm.sqrt_rcp_inputs()
    out = capi.probe_math2(ctx, x, np.zeros_like(x))
    sq, rc = pm.numpy_sqrt_rcp(x)
    assert_same(out[:, SQRT], sq, "sqrt_f")
    assert_same(out[:, RCP], rc, "rcp_f")
    finite_pos = np.isfinite(x) & (x >= 0)
    assert not np.isnan(out[finite_pos, SQRT]).any() and not np.isnan(out[~np.isnan(x), RCP]).any()


def test_srgb_decode_matches_oracle(device_math, oracle_lib):
    sx = pm.srgb_inputs()
    assert_same(device_math["srgb"], pm.oracle_srgb(sx), "srgb_to_linear1")
    assert not np.isnan(device_math["srgb"]).any()


def test_srgb_ramp_through_the_texture_path(ctx):
    """All 256 byte values through an sRGB image node (arg[2] = 1): a 256 x 1 nearest RGBA8 ramp looked up at every texel centre -- unorm8,
    then srgb_to_linear1 and its pow_f on the device -- against the oracle, the host build and the probe of srgb_to_linear1 itself."""
    sd = textured_room()
    ramp = np.zeros((1, 256, 4), dtype=np.uint8)
    ramp[0, :, 0] = np.arange(256)
    ramp[0, :, 1] = np.arange(256)[::-1]
    ramp[0, :, 2] = (np.arange(256) * 7 + 3) % 256
    ramp[0, :, 3] = np.arange(256)
    sd.images.append(abi.ImageData(ramp, abi.TEX_FILTER_NEAREST, abi.TEX_EXTEND))
    g = abi.GraphData([abi.NodeData(abi.NODE_IMAGE, (len(sd.images) - 1, abi.NODE_NONE, 1))], {"base_color": 0})
    sd.materials.append(abi.MaterialData(roughness=0.9, ior=1.0, specular_ior_level=0.0, graph=g))
    m = len(sd.materials) - 1
    scene = capi.Scene(ctx, sd)
    uv = np.stack([(np.arange(256, dtype=np.float32) + 0.5) / 256.0, np.full(256, 0.5, np.float32)], axis=1).astype(np.float32)
    d = capi.probe_material_inputs(ctx, scene, m, uv)
    assert n_bit_diff(d, pyoracle.OracleScene(sd).material_inputs(m, uv)) == 0
    assert n_bit_diff(d, capi.probe_material_inputs(None, scene, m, uv)) == 0
    byte = np.arange(256, dtype=np.float32) / np.float32(255.0)
    lin = capi.probe_math2(ctx, byte, np.zeros_like(byte))[:, SRGB]
    assert np.array_equal(d[:, 1].view(np.uint32), lin.view(np.uint32)) and np.array_equal(d[:, 2].view(np.uint32), lin[::-1].view(np.uint32))
    assert np.array_equal(d[:, 4], byte)  # alpha is not decoded
    assert np.all(np.diff(d[:, 1]) > 0) and d[0, 1] == 0.0 and d[255, 1] == 1.0


# ------------------------------------------------------------------------------------------------ B2: accuracy against float64
# The oracle's worst error on these inputs is recorded in pm.ORACLE_WORST (measured on the CPU, held by tests/test_oracle_kat.py):
#   exp 0.955 ulp, pow 115.2 ulp (|y log x| <= 80), atan2 2.73 ulp, srgb_to_linear1 8.19 ulp, log 0.726 ulp,
#   sin 7.94e-8 absolute / 1.40 ulp where |sin| >= 1/4, cos 8.81e-8 absolute / 1.48 ulp where |cos| >= 1/4.
# The device must stay within twice each.
def test_elementary_functions_within_the_oracles_error_of_float64(device_math):
    fig = pm.accuracy_figures(device_math["exp"], device_math["pow"], device_math["atan2"], device_math["srgb"], device_math["sin"],
                              device_math["cos"], device_math["log"])
    print("device error against float64:", fig)
    assert set(fig) == set(pm.ORACLE_WORST)
    for name, worst in pm.ORACLE_WORST.items():
        assert fig[name] <= 2.0 * worst, (name, fig[name], worst)


# ------------------------------------------------------------------------------------------------ B3: the sampler matrix
@pytest.fixture(scope="module")
def sampler(ctx):
    sd, first = pm.sampler_scene()
    return sd, first, capi.Scene(ctx, sd), pyoracle.OracleScene(sd)


@pytest.mark.parametrize("filt", pm.FILTERS, ids=["nearest", "linear"])
@pytest.mark.parametrize("address", pm.ADDRESSES, ids=["repeat", "clip", "mirror", "extend"])
@pytest.mark.parametrize("fmt", pm.FORMATS, ids=["rgba8", "rgba32f"])
def test_sampler_mode_on_device(ctx, sampler, filt, address, fmt):
    """One of the 16 sampler modes at all six shapes: device == oracle (scene evaluation and the bare sampler) == host build bit for bit, and
    the properties of pm.check_sampler_properties on the device's values."""
    sd, first, scene, osc = sampler
    cases = pm.sampler_cases()
    n_shapes = 0
    for shape in pm.SHAPES:
        case = (filt, address, fmt, shape)
        m = first + cases.index(case)
        uv, parts = pm.sampler_uv(shape)
        d = capi.probe_material_inputs(ctx, scene, m, uv)
        assert_same(d, osc.material_inputs(m, uv), f"{case}: device vs oracle")
        assert_same(d, capi.probe_material_inputs(None, scene, m, uv), f"{case}: device vs host build")
        rgba = np.ascontiguousarray(d[:, 1:5])
        assert_same(rgba, pyoracle.tex_sample(pm.sampler_image(case), uv), f"{case}: device vs or_tex_sample")
        n_centres, _ = pm.check_sampler_properties(case, uv, parts, rgba)
        assert n_centres > 0
        n_shapes += 1
    assert n_shapes == 6


# ------------------------------------------------------------------------------------------------ B4: BSDF thresholds
@pytest.mark.parametrize("name", list(pm.THRESHOLD_MATERIALS))
def test_bsdf_on_thresholds(ctx, root, name):
    """Materials on the branch thresholds of dbsdf.h, outgoing directions at and next to grazing: device == oracle with the NaN rule; no row
    holds a NaN except for the two ior = 1.0 materials, whose NaN rows (the transmission lobe: half vector normalize(wo - wo), as in the
    reference) are never valid."""
    m = pm.THRESHOLD_MATERIALS[name]
    table = pm.ggx_table(root)
    wo, u, wi = pm.threshold_inputs()
    n_nan = 0
    for w in wo:
        g = capi.probe_bsdf(ctx, m, 1, w, u, table)
        assert_same(g, pyoracle.bsdf_sample_many(m, w, u, table), f"{name} sample wo={w}")
        ge = capi.probe_bsdf(ctx, m, 0, w, wi, table)
        assert_same(ge, pyoracle.bsdf_eval_many(m, w, wi, table), f"{name} evaluate wo={w}")
        nan_rows = np.isnan(g).any(axis=1)
        n_nan += int(nan_rows.sum()) + int(np.isnan(ge).any(axis=1).sum())
        assert not (nan_rows & (g[:, 7] != 0.0)).any(), f"{name}: a sample with a NaN is marked valid"
        assert np.isin(g[:, 7], (0.0, 1.0)).all()
    if name in pm.IOR_1_MATERIALS:
        assert n_nan > 1000  # about 6100 sample rows and 2 evaluate rows (wi = -wo exactly) of 16416 + 16432
    else:
        assert n_nan == 0


def test_film_behind_an_ior_one_glass_quad(ctx):
    """with eta = 1 every sample of the transmission lobe evaluates to NaN (pdf NaN -> not valid), so the path ends at the quad.
    The film equals the oracle's bit for bit and IS finite (the NaN stays in the dead path's throughput); the quad shows as a dark
    square in front of the emitting walls instead of being invisible -- what the reference's arithmetic gives as well."""
    sd = pm.ior_one_glass_box()
    cfg = make_config(spp=8, spp_per_pass=8, max_depth=6)
    film = capi.Film(ctx, 32, 32)
    gst = capi.pt_render(ctx, capi.Scene(ctx, sd), cfg, film)
    g = film.read()
    o, ost = pyoracle.OracleScene(sd).render(cfg)
    assert n_bit_diff(g, o) == 0 and gst["n_samples"] == ost["n_samples"] == 32 * 32 * 8
    pm.check_ior_one_film(g)
