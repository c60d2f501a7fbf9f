"""Inputs, references and recorded bounds shared by the probe-matrix tests: tests/test_gpu_probe_matrix.py runs them on the device,
tests/test_oracle_kat.py and tests/test_textures.py hold the oracle to the same properties where there is no GPU (so every bound
below is a measurement of the reference, never of the code under test)."""
import ctypes as C
import math

import numpy as np

from akari_render_amd import abi
from oracle import pyoracle, scene_json
from tests.helpers import box_scene, textured_room

f32 = np.float32
INF, NAN = f32(np.inf), f32(np.nan)
TINY, HUGE = f32(1.17549435e-38), f32(3.4028235e38)  # smallest and largest normal
DENORM_MIN = f32(1.4e-45)


def around(values, ulps=1):
    """Every value with its neighbours at +-1..ulps ulp, as float32."""
    v = np.asarray(values, dtype=f32).reshape(-1)
    out = [v]
    lo = hi = v
    with np.errstate(over="ignore"):  # (the neighbour above the largest normal is inf, on purpose)
        for _ in range(ulps):
            lo, hi = np.nextafter(lo, -INF), np.nextafter(hi, INF)
            out += [lo, hi]
    return np.concatenate(out).astype(f32)


def same_bits_or_both_nan(a, b):
    """The NaN rule: two NaNs are equal whatever their payload, everything else is compared as uint32. -> mask of agreeing elements."""
    a, b = np.asarray(a, dtype=f32), np.asarray(b, dtype=f32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def ulp_error(got, ref64):
    """|got - ref| in units of the float32 spacing at ref (the spacing of the smallest normal below it), ref in float64."""
    got, ref64 = np.asarray(got, dtype=np.float64), np.asarray(ref64, dtype=np.float64)
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(np.maximum(np.abs(ref64), float(TINY))))
    return np.abs(got - ref64) / np.exp2(e - 23)


# ------------------------------------------------------------------------------------------------ elementary functions: inputs
EXP_HI, EXP_LO = f32(88.72283905206835), f32(-103.278929903431851103)  # dmath.h exp_f: inf above, 0 below


def exp_inputs():
    rng = np.random.default_rng(101)
    ln2 = np.arange(-149, 129, dtype=np.float64) * math.log(2.0)  # the floor and the n1 / n2 split at every n
    return np.concatenate([np.linspace(-104, 89, 8001), rng.uniform(-104, 89, 8000), around([EXP_HI, EXP_LO]),
                           [0.0, -0.0, NAN, INF, -INF], around(ln2.astype(f32))]).astype(f32)


def pow_inputs():
    """(x, y): the sRGB call, the wide box, x = 0 with y > 0, x = 1."""
    rng = np.random.default_rng(102)
    xs = np.concatenate([np.arange(1, 6001) / 6000.0, (np.arange(256) / f32(255.0) + f32(0.055)) / f32(1.055)])
    x = [xs, np.exp(rng.uniform(math.log(1e-6), math.log(1e3), 10000)), np.zeros(6), np.ones(201), [1e-6, 1e3, 1e-6, 1e3]]
    y = [np.full(xs.size, 2.4), rng.uniform(-8, 8, 10000), [1e-3, 0.5, 1.0, 2.4, 8.0, 1e-30], np.linspace(-8, 8, 201), [-8, -8, 8, 8]]
    return np.concatenate(x).astype(f32), np.concatenate(y).astype(f32)


def atan2_inputs():
    """(y, x): the four quadrants, both axes with +-0, |y| = |x|, ratios 2^+-60, denormals, the (e.y, sin_theta >= 0) half-plane of denv.h env_uv."""
    rng = np.random.default_rng(103)
    q = rng.normal(size=(8000, 2)) * np.exp(rng.uniform(-6, 6, size=(8000, 1)))
    sg = [(a, b) for a in (1.0, -1.0) for b in (1.0, -1.0)]
    axes = [(a * 0.0, b * m) for a, b in sg for m in (0.0, 1.0, 3e-39, 2.5e30)] + [(a * m, b * 0.0) for a, b in sg for m in (1.0, 3e-39, 2.5e30)]
    mags = np.concatenate([np.exp(rng.uniform(-80, 80, 200)), [1.0, float(TINY), float(HUGE), 3e-39, float(DENORM_MIN)]])
    diag = [(a * m, b * m) for a, b in sg for m in mags]
    ratio = [(a * m, b * n) for a, b in sg for m, n in ((1.0, 2.0**60), (2.0**60, 1.0), (2.0**-60, 1.0), (1.0, 2.0**-60), (2.0**-30, 2.0**30), (0.41421357, 1.0), (0.41421354, 1.0))]
    den = [(a * m, b * n) for a, b in sg for m, n in ((1e-40, 1e-40), (1.4e-45, 1.0), (1.0, 1.4e-45), (3e-39, 2e-39), (1.4e-45, 4.2e-45), (1e-41, 1.1754944e-38))]
    ey = np.concatenate([np.linspace(-1, 1, 3001), rng.uniform(-1, 1, 1000)]).astype(f32)
    half = np.stack([ey, np.sqrt(np.maximum(f32(1) - ey * ey, f32(0))).astype(f32)], axis=1)
    a = np.concatenate([q, axes, diag, ratio, den, half]).astype(f32)
    return a[:, 0].copy(), a[:, 1].copy()


def sincos_inputs():
    rng = np.random.default_rng(104)
    k = np.arange(-8, 9, dtype=np.float64) * (math.pi / 2)
    return np.concatenate([np.linspace(-2 * math.pi, 4 * math.pi, 8001), rng.uniform(-2 * math.pi, 4 * math.pi, 8000), around(k.astype(f32))]).astype(f32)


def sqrt_rcp_inputs():
    """Denormals, the smallest and largest normals, exact squares, powers of two, every exponent with random mantissas, both signs, zeros, inf, NaN."""
    rng = np.random.default_rng(105)
    bits = rng.integers(0, 0x7F800000, 12000, dtype=np.uint32) | (rng.integers(0, 2, 12000, dtype=np.uint32) << 31)
    sq = np.arange(1, 2049, dtype=f32) ** 2
    p2 = np.exp2(np.arange(-149, 128, dtype=np.float64)).astype(f32)
    den = np.concatenate([around([DENORM_MIN, TINY], 2), (rng.integers(1, 0x00800000, 500, dtype=np.uint32)).view(f32)])
    sp = np.array([0.0, -0.0, INF, -INF, NAN, 1.0, -1.0, 3.0, 1.0 / 3.0, 255.0, 12.92, 1.055], dtype=f32)
    return np.concatenate([bits.view(f32), sq, np.sqrt(sq) * f32(0.25), p2, -p2, den, -den, around([HUGE, -HUGE, f32(2.0**126), f32(2.0**-126)], 1), sp]).astype(f32)


def srgb_inputs():
    """All 256 byte values b / 255, both sides of the 0.04045 knee, a grid over [0, 1]."""
    return np.concatenate([np.arange(256, dtype=f32) / f32(255.0), around([f32(0.04045)], 3), np.linspace(0, 1, 4001), [0.0, 1.0]]).astype(f32)


# ------------------------------------------------------------------------------------------------ elementary functions: the oracle
def _each(fn, *cols):
    return np.array([fn(*(float(v) for v in row)) for row in zip(*cols)], dtype=f32)


def oracle_exp(x):
    return pyoracle.exp_many(x)  # (one call for the whole array: the restatements pass whole frames)


def oracle_pow(x, y):
    return _each(pyoracle.lib().or_kat_pow, x, y)


def oracle_log(x):
    return pyoracle.log_many(x)


def oracle_sincos(x):
    L, a, b = pyoracle.lib(), C.c_float(), C.c_float()
    s, c = np.zeros(len(x), dtype=f32), np.zeros(len(x), dtype=f32)
    for i, v in enumerate(x):
        L.or_kat_sincos(float(v), C.byref(a), C.byref(b))
        s[i], c[i] = a.value, b.value
    return s, c


def oracle_srgb(x):
    """or_tex.h or_srgb_to_linear: the knee and the two divisions in float32, the oracle's pow."""
    return scene_json._srgb_to_linear(np.asarray(x, dtype=f32))


def numpy_sqrt_rcp(x):
    """numpy's float32 sqrt and 1 / x: IEEE operations of the host, correctly rounded."""
    x = np.asarray(x, dtype=f32)
    with np.errstate(all="ignore"):
        return np.sqrt(x), (f32(1.0) / x).astype(f32)


# ------------------------------------------------------------------------------------------------ accuracy against float64
# The oracle's worst error on the input sets above, measured on the CPU (tests/test_oracle_kat.py::test_elementary_function_error_against_f64
# prints the figures and holds the oracle to these records). The device has to stay within TWICE each record; as it equals the oracle
# bit for bit the margin only guards against edits of the input sets.
#   exp, pow, atan2, srgb: ulps of the float64 result (pow without the inputs whose |y log x| > 80, where y log x itself has lost the
#   digits; atan2 without the pairs whose larger component is denormal, where the quotient lo / hi has few bits to begin with, and with y = -0
#   read as +0: atan2_f takes the sign of the result from y < 0, so on the cut x < 0 it answers +pi for both zeros)
#   sin, cos: absolute error over the whole set (near the zeros of the result an ulp count is meaningless) and ulps where |result| >= 1/4
#   log: ulps, on the positive inputs of the sincos set
ORACLE_WORST = {
    "exp_ulp": 0.9544, "pow_ulp": 115.2, "atan2_ulp": 2.728, "srgb_ulp": 8.181, "log_ulp": 0.7259,
    "sin_abs": 7.939e-8, "sin_ulp": 1.399, "cos_abs": 8.806e-8, "cos_ulp": 1.478,
}


def accuracy_figures(exp_v, pow_v, atan2_v, srgb_v, sin_v, cos_v, log_v):
    """The figures ORACLE_WORST records, for one implementation's results on the input sets above."""
    out = {}
    x = exp_inputs().astype(np.float64)
    with np.errstate(over="ignore"):
        ref = np.exp(x)
    ok = np.isfinite(x) & (ref <= float(HUGE)) & (ref >= float(DENORM_MIN))
    out["exp_ulp"] = float(ulp_error(exp_v[ok], ref[ok]).max())
    px, py = (a.astype(np.float64) for a in pow_inputs())
    with np.errstate(divide="ignore"):
        ok = (px > 0) & (np.abs(py * np.log(np.where(px > 0, px, 1.0))) <= 80.0)
    out["pow_ulp"] = float(ulp_error(pow_v[ok], np.power(px[ok], py[ok])).max())
    ay, ax = (a.astype(np.float64) for a in atan2_inputs())
    ok = np.maximum(np.abs(ax), np.abs(ay)) >= float(TINY)
    out["atan2_ulp"] = float(ulp_error(atan2_v[ok], np.arctan2(ay[ok] + 0.0, ax[ok])).max())  # (-0 + 0 = +0: see ORACLE_WORST)
    s = srgb_inputs().astype(np.float64)
    # the knee is the float32 constant, the arithmetic exact
    ref = np.where(s <= float(f32(0.04045)), s / 12.92, np.power((s + 0.055) / 1.055, 2.4))
    out["srgb_ulp"] = float(ulp_error(srgb_v, ref).max())
    t = sincos_inputs().astype(np.float64)
    for name, got, ref in (("sin", sin_v, np.sin(t)), ("cos", cos_v, np.cos(t))):
        out[name + "_abs"] = float(np.abs(got.astype(np.float64) - ref).max())
        big = np.abs(ref) >= 0.25
        out[name + "_ulp"] = float(ulp_error(got[big], ref[big]).max())
    pos = t > 0
    out["log_ulp"] = float(ulp_error(log_v[pos], np.log(t[pos])).max())
    return out


# ------------------------------------------------------------------------------------------------ the sampler matrix
FILTERS = [abi.TEX_FILTER_NEAREST, abi.TEX_FILTER_LINEAR]
ADDRESSES = [abi.TEX_REPEAT, abi.TEX_CLIP, abi.TEX_MIRROR, abi.TEX_EXTEND]
FORMATS = [np.uint8, np.float32]
SHAPES = [(1, 1), (1, 7), (5, 1), (5, 7), (8, 8), (3, 16)]  # (H, W): one texel, one row, one column, odd, power of two, wide


def sampler_texels(fmt, shape):
    """One image per (format, shape), the same for every filter and address mode. No channel of any texel is 0 (a clipped lookup is told
    from a stored one), float texels are spread over [0.05, 6)."""
    h, w = shape
    rng = np.random.default_rng(1000 + 100 * h + w + (0 if fmt == np.uint8 else 7))
    if fmt == np.uint8:
        return rng.integers(1, 256, size=(h, w, 4), dtype=np.uint8)
    return (0.05 + rng.random((h, w, 4)) * np.exp(rng.uniform(-2, 1.75, size=(h, w, 4)))).astype(f32)


def sampler_cases():
    """(filter, address, format, shape) of all 96 images, in the order of sampler_scene's images and materials."""
    return [(fl, ad, fm, sh) for fl in FILTERS for ad in ADDRESSES for fm in FORMATS for sh in SHAPES]


def sampler_image(case) -> abi.ImageData:
    fl, ad, fm, sh = case
    return abi.ImageData(sampler_texels(fm, sh), fl, ad)


def sampler_scene():
    """The textured room with one more material per case: base_color <- NODE_IMAGE(image of the case, si.uv, srgb = 0), nothing between the
    sampler and the input (columns 1..4 of the evaluated inputs are the lookup's rgb and alpha). -> (scene, index of the first such material)."""
    sd = textured_room()
    first_img, first_mat = len(sd.images), len(sd.materials)
    for k, case in enumerate(sampler_cases()):
        sd.images.append(sampler_image(case))
        g = abi.GraphData([abi.NodeData(abi.NODE_IMAGE, (first_img + k, abi.NODE_NONE, 0))], {"base_color": 0})
        sd.materials.append(abi.MaterialData(roughness=0.9, ior=1.0, specular_ior_level=0.0, graph=g))
    return sd, first_mat


def sampler_uv(shape):
    """-> (uv, parts: name -> slice). 400 random points of [-2.5, 3.5]^2 and 200 of [0, 1]^2, every texel centre, every pair of texel edges
    k / w, l / h, the corners and the values the clamps of tex_floor_to_int exist for."""
    h, w = shape
    rng = np.random.default_rng(50 + 10 * h + w)
    sets = {
        "random": rng.uniform(-2.5, 3.5, size=(400, 2)),
        "inside": rng.uniform(0.0, 1.0, size=(200, 2)),
        "centres": np.array([[(i + 0.5) / w, (j + 0.5) / h] for j in range(h) for i in range(w)]),
        "edges": np.array([[k / w, l / h] for l in range(h + 1) for k in range(w + 1)]),
        "special": np.array([[0, 0], [1, 1], [-0.0, 2.0], [-1e-9, 1 - 6e-8], [1e9, -1e9], [3e38, 3e38], [-3e38, -3e38], [3e38, -3e38], [np.nan, 0.3],
                             [0.3, np.nan], [np.inf, -np.inf], [-np.inf, 0.5]]),
    }
    parts, at = {}, 0
    for name, a in sets.items():
        parts[name] = slice(at, at + len(a))
        at += len(a)
    return np.concatenate(list(sets.values())).astype(f32), parts


def exact_centres(uv, cen, shape):
    """The texel centres the sampler sees as such: f32(u) * w == i + 0.5 and f32(v) * h == j + 0.5 exactly, the product rounded to float32 as
    the sampler's own is (its one rounding per axis). -> (indices into uv, i, j)"""
    h, w = shape
    c = uv[cen]
    i, j = np.meshgrid(np.arange(w), np.arange(h))
    i, j = i.reshape(-1), j.reshape(-1)
    ok = ((c[:, 0] * f32(w)).astype(f32) == i + 0.5) & ((c[:, 1] * f32(h)).astype(f32) == j + 0.5)
    return np.arange(cen.start, cen.stop)[ok], i[ok], j[ok]


def texels_f32(tex):
    return (tex.astype(f32) / f32(255.0)).astype(f32) if tex.dtype == np.uint8 else tex.astype(f32)


def clip_far_outside(uv, shape):
    """Points a clip-addressed image answers with zeros whatever the filter: u or v outside [0, 1) by more than one texel (or not a number: the
    clamp of tex_floor_to_int sends NaN to -1e9)."""
    h, w = shape
    u, v = uv[:, 0].astype(np.float64), uv[:, 1].astype(np.float64)
    with np.errstate(invalid="ignore"):
        return (u < -1.0 / w) | (u >= 1 + 1.0 / w) | (v < -1.0 / h) | (v >= 1 + 1.0 / h) | np.isnan(u) | np.isnan(v)


def sample_f64(tex, filt, address, uv):
    """Nearest / bilinear evaluation of `tex` in float64 for uv in [0, 1]^2, written from the definition (texel centres at +0.5, taps beyond the
    border by the address mode: repeat wraps, mirror and extend clamp -- inside one period a mirrored image continues with its own border
    texel --, clip reads zero). -> (values (n, 4), distance of each point to the nearest texel edge in u or v)"""
    t = texels_f32(tex).astype(np.float64)
    h, w = t.shape[:2]

    def tap(i, j):
        if address == abi.TEX_REPEAT:
            return t[j % h, i % w]
        v = t[np.clip(j, 0, h - 1), np.clip(i, 0, w - 1)]
        if address == abi.TEX_CLIP:
            v = np.where(((i >= 0) & (i < w) & (j >= 0) & (j < h))[:, None], v, 0.0)
        return v

    x, y = uv[:, 0].astype(np.float64) * w, uv[:, 1].astype(np.float64) * h
    edge = np.minimum(np.abs(x - np.round(x)) / w, np.abs(y - np.round(y)) / h)
    if filt == abi.TEX_FILTER_NEAREST:
        return tap(np.floor(x).astype(int), np.floor(y).astype(int)), edge
    x, y = x - 0.5, y - 0.5
    i, j = np.floor(x).astype(int), np.floor(y).astype(int)
    tx, ty = (x - i)[:, None], (y - j)[:, None]
    r0, r1 = tap(i, j) + (tap(i + 1, j) - tap(i, j)) * tx, tap(i, j + 1) + (tap(i + 1, j + 1) - tap(i, j + 1)) * tx
    return r0 + (r1 - r0) * ty, edge


def check_sampler_properties(case, uv, parts, got):
    """What a lookup owes the definition whatever code computed it (`got` = rgba of `uv`): texel centres return the texel, clip returns zeros
    outside, [0, 1]^2 agrees with float64. -> (centres checked, worst error of (3) as a fraction of its bound)"""
    fl, ad, fm, sh = case
    h, w = sh
    tex = sampler_texels(fm, sh)
    tf = texels_f32(tex)
    # (1) a texel centre that float32 holds exactly returns the texel itself, under both filters (the bilinear weights are exactly 0, and
    # a + (b - a) * 0 is a); for RGBA8 that is byte / 255 in float32. At most 10 % of the centres may fail the exactness condition.
    idx, ci, cj = exact_centres(uv, parts["centres"], sh)
    assert len(idx) >= 0.9 * (h * w) and len(idx) > 0, (case, len(idx))
    assert np.array_equal(got[idx].view(np.uint32), tf[cj, ci].view(np.uint32)), case
    # (2) clip: zeros in all four channels beyond one texel outside
    if ad == abi.TEX_CLIP:
        far = clip_far_outside(uv, sh)
        assert far.sum() >= 100 and np.all(got[far].view(np.uint32) == 0), case
    # (3) the float64 evaluation on [0, 1]^2: one rounding of u * w per axis feeding the weights + the roundings of three lerps.
    # Nearest: a point within 2^-20 of a texel edge may fall either way and is left out -- at most 1 % of the points that were not put on
    # an edge on purpose (the "edges" and "special" parts of the set lie on edges by construction).
    with np.errstate(invalid="ignore"):
        unit = (uv[:, 0] >= 0) & (uv[:, 0] <= 1) & (uv[:, 1] >= 0) & (uv[:, 1] <= 1)
    ref, edge = sample_f64(tex, fl, ad, uv[unit])
    keep = np.ones(int(unit.sum()), dtype=bool)
    if fl == abi.TEX_FILTER_NEAREST:
        keep = edge > 2.0**-20
        free = np.zeros(len(uv), dtype=bool)
        for name in ("random", "inside", "centres"):
            free[parts[name]] = True
        free = free[unit]
        assert (free & ~keep).sum() <= 0.01 * free.sum(), case
    assert keep.sum() >= 100, case
    bound = (2 * max(w, h) + 9) * 2.0**-24 * float(tf.max())
    err = float(np.abs(got[unit][keep].astype(np.float64) - ref[keep]).max())
    assert err <= bound, (case, err, bound)
    return len(idx), err / bound


# ------------------------------------------------------------------------------------------------ BSDF thresholds
def _up(x):
    return float(np.nextafter(f32(x), INF))


M = abi.MaterialData
THRESHOLD_MATERIALS = {
    "roughness_0": M(base_color=(0.7, 0.6, 0.5), roughness=0.0, ior=1.5),
    "roughness_1": M(base_color=(0.7, 0.6, 0.5), roughness=1.0, ior=1.5),
    "metallic_1e-4": M(base_color=(0.9, 0.7, 0.3), metallic=1e-4, roughness=0.3),
    "metallic_above_1e-4": M(base_color=(0.9, 0.7, 0.3), metallic=_up(1e-4), roughness=0.3),
    "metallic_1_minus_1e-4": M(base_color=(0.9, 0.7, 0.3), metallic=float(f32(1.0) - f32(1e-4)), roughness=0.3),
    "metallic_1_mirror_white": M(base_color=(1.0, 1.0, 1.0), metallic=1.0, roughness=0.0),
    "transmission_above_1e-4": M(base_color=(0.8, 0.9, 1.0), roughness=0.2, ior=1.5, transmission_weight=_up(1e-4)),
    "transmission_1_smooth": M(base_color=(0.8, 0.9, 1.0), roughness=0.0, ior=1.5, transmission_weight=1.0),
    "ior_below_1": M(base_color=(0.8, 0.9, 1.0), roughness=0.2, ior=0.8, transmission_weight=0.6),
    "no_specular_layer": M(base_color=(0.7, 0.6, 0.5), roughness=0.5, ior=1.5, specular_ior_level=0.0),
    "smooth_coat_over_rough": M(base_color=(0.8, 0.2, 0.2), roughness=1.0, ior=1.45, coat_weight=1.0, coat_roughness=0.0, coat_ior=1.5),
    "black_base": M(base_color=(0.0, 0.0, 0.0), roughness=0.4, ior=1.5, metallic=0.5, transmission_weight=0.5),
    "glass_node_rough_2.5": M(kind=abi.MAT_GLASS, base_color=(1, 1, 1), ior=2.5, roughness=1.0),
    "glass_node_ior_1": M(kind=abi.MAT_GLASS, base_color=(1, 1, 1), ior=1.0, roughness=0.25),
    "transmission_ior_1": M(base_color=(0.8, 0.9, 1.0), roughness=0.25, ior=1.0, transmission_weight=1.0),
}
# eta == 1 makes the refracted direction -wo and the half vector of MicrofacetTransmission normalize(wo + wi * 1) = 0 / 0: the reference
# computes the same NaN (svm/surface/mod.rs:923-924); DESIGN.md section 2. Every other material above is NaN-free.
IOR_1_MATERIALS = ("glass_node_ior_1", "transmission_ior_1")
THRESHOLD_WO = [(0, 0, 1), (0, 0, -1), (1, 0, 0), (0.6, 0.8, 0), (1, 0, 1e-4), (1, 0, -1e-4), (0.7, 0.7, 1e-7), (0.3, 0.2, -0.9327)]


def threshold_inputs():
    """-> (wo (8, 3) normalised in float32, u (2052, 3), wi (2054, 3)), the same for every material."""
    rng = np.random.default_rng(77)
    wo = np.array(THRESHOLD_WO, dtype=f32)
    wo = (wo / np.sqrt((wo * wo).sum(axis=1, dtype=f32))[:, None].astype(f32)).astype(f32)
    u = np.concatenate([rng.random((2048, 3), dtype=f32), np.array([[0, 0, 0], [1, 1, 1], [1, 0, 1], [0.999999, 0.5, 0.5]], dtype=f32)])
    d = rng.normal(size=(2048, 3)).astype(f32)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
    ax = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=f32)
    return wo, u, np.concatenate([d, ax])


def ggx_table(root):
    import os
    return np.fromfile(os.path.join(root, "tests", "golden", "ggx_dielectric_s.f32"), dtype=f32)


def ior_one_glass_box() -> abi.SceneData:
    """The emitting closed box of helpers.box_scene with a Glass quad of ior = 1.0 in front of the camera, covering the middle of the view."""
    sd = box_scene(albedo=0.5, emission=1.0, width=32, height=32)
    q = np.array([[-0.15, -0.15, -0.5], [0.15, -0.15, -0.5], [0.15, 0.15, -0.5], [-0.15, 0.15, -0.5]], dtype=f32)
    sd.meshes.append(abi.MeshData(vertices=q, indices=np.array([[0, 1, 2], [0, 2, 3]], dtype=np.uint32)))
    sd.materials.append(abi.MaterialData(kind=abi.MAT_GLASS, base_color=(1, 1, 1), ior=1.0, roughness=0.25))
    sd.instances.append(abi.InstanceData(1, [1], np.eye(4, dtype=f32).reshape(16).copy()))
    return sd


def check_ior_one_film(film):
    """The film of ior_one_glass_box is finite, and the quad shows as a dark square in front of the emitting walls."""
    print("film finite:", bool(np.isfinite(film).all()))
    assert np.isfinite(film).all()
    n = 32 * 32
    img = film[: 3 * n].reshape(32, 32, 3) / np.maximum(film[6 * n : 7 * n].reshape(32, 32, 1), 1)
    assert img[14:18, 14:18].max() < 0.05 * img[:4, :4].min()
