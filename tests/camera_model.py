"""The camera projections of DESIGN.md 4.17 restated in numpy f32, operation for operation: the film point with both filters, the orthographic
camera's raster -> camera matrix (camera_matrices' chain with half the ortho scale for tan(fov / 2)), the orthographic ray with and without a
lens, the panorama ray, and camera -> world as section 4.9 step 4 does it. No library call: sincos_f and log_f come through the oracle's
known-answer entries (tests/test_math pins the library's to them), everything else is IEEE f32 +, -, *, /, sqrt in the order the definition gives."""
import numpy as np

from oracle import pyoracle
from tests.test_lens import _concentric_disk, _is_identity, _normalize, _rot, _sincos

F = np.float32
PERSPECTIVE, ORTHOGRAPHIC, PANORAMA = 0, 1, 2
PI_F, HALF_PI_F = F(np.pi), F(np.pi / 2)  # the f32 nearest to pi and pi / 2: the inclusive bounds of a panorama's window
FILTER_BOX, FILTER_GAUSSIAN = 0, 1


def _max_f(a, b):
    return np.where(a > b, a, b).astype(F)  # b when a is NaN (dmath.h max_f)


def _min_f(a, b):
    return np.where(a < b, a, b).astype(F)


def filter_offset(u, filter_type, radius):
    """filter_sample (film.rs:32-49): box = (u - 0.5) * radius; Gaussian = Box-Muller with sigma = radius / 3, clamped to +- radius."""
    u = np.asarray(u, F)
    radius = F(radius)
    if filter_type == FILTER_BOX:
        return ((u - F(0.5)).astype(F) * radius).astype(F)
    sigma = (radius / F(3.0)).astype(F)
    with np.errstate(all="ignore"):
        r = np.sqrt((F(-2.0) * pyoracle.log_many(u[:, 0])).astype(F)).astype(F)
        theta = ((F(2.0) * PI_F).astype(F) * u[:, 1]).astype(F)
        sn, cs = _sincos(theta)
        off = np.stack([((r * cs).astype(F) * sigma).astype(F), ((r * sn).astype(F) * sigma).astype(F)], axis=1)
    return _min_f(_max_f(off, -radius), radius)


def film_point(pixels, u_filter, filter_type, radius):
    """pf = (px + 0.5 + offset.x, py + 0.5 + offset.y)"""
    return ((np.asarray(pixels).astype(F) + F(0.5)).astype(F) + filter_offset(u_filter, filter_type, radius)).astype(F)


# ------------------------------------------------------------------------------------------------------------ the host's matrix chain
def _m4_mul(a, b):
    """out = a * b, column-major, un-fused: ((a0 b0 + a1 b1) + a2 b2) + a3 b3 per element"""
    r = np.zeros(16, F)
    for c in range(4):
        for i in range(4):
            r[c * 4 + i] = F(F(F(a[i] * b[c * 4]) + F(a[4 + i] * b[c * 4 + 1])) + F(a[8 + i] * b[c * 4 + 2])) + F(a[12 + i] * b[c * 4 + 3])
    return r


def _m4_scale(x, y, z):
    m = np.zeros(16, F)
    m[0], m[5], m[10], m[15] = F(x), F(y), F(z), F(1)
    return m


def _m4_translate(x, y, z):
    m = _m4_scale(1, 1, 1)
    m[12], m[13], m[14] = F(x), F(y), F(z)
    return m


def r2c_matrix(width, height, t):
    """camera_matrices (camera/mod.rs:119-153) with `t` in the place of tan(fov / 2): an orthographic camera has t = 0.5f * ortho_scale."""
    fw, fh, t = F(width), F(height), F(t)
    m = _m4_scale(1, 1, 1)
    m = _m4_mul(_m4_scale(F(1) / fw, F(1) / fh, 1), m)
    m = _m4_mul(_m4_scale(2, 2, 1), m)
    m = _m4_mul(_m4_translate(-1, -1, 0), m)
    m = _m4_mul(_m4_scale(1, -1, 1), m)
    s = _m4_scale(t, F(F(t * fh) / fw), 1) if width > height else _m4_scale(F(F(t * fw) / fh), t, 1)
    m = _m4_mul(s, m)
    return _m4_mul(_m4_translate(0, 0, -1), m)


def ortho_r2c(width, height, ortho_scale):
    return r2c_matrix(width, height, F(0.5) * F(ortho_scale))


# ------------------------------------------------------------------------------------------------------------ the rays
def _to_world(c2w, o, d):
    """Section 4.9 step 4: nothing for an identity c2w; else o = c2w . point(o') / w, d = c2w . vector(d'), rows summed left to right."""
    c = np.asarray(c2w, F)
    if _is_identity(c):
        return np.concatenate([o, d], axis=1).astype(F)

    def row(k):
        return ((((c[k] * o[:, 0]).astype(F) + (c[4 + k] * o[:, 1]).astype(F)).astype(F) + (c[8 + k] * o[:, 2]).astype(F)).astype(F) + c[12 + k] * F(1.0)).astype(F)

    inv = (F(1.0) / row(3)).astype(F)
    ow = (np.stack([row(0), row(1), row(2)], axis=1) * inv[:, None]).astype(F)
    return np.concatenate([ow, _rot(c, d)], axis=1).astype(F)


def ortho_rays(r2c, c2w, pixels, u_filter, u_lens, filter_type, radius, R=0.0, Fd=0.0):
    """q = r2c . (pf, 0, 1); s = q.xyz * (1 / q.w); o' = (s.x, s.y, 0), d' = (0, 0, -1); with a lens o' += l, d' = normalize(-l.x, -l.y, -F)."""
    m = np.asarray(r2c, F)
    pf = film_point(pixels, u_filter, filter_type, radius)
    x, y = pf[:, 0], pf[:, 1]

    def row(k):
        return ((((m[k] * x).astype(F) + (m[4 + k] * y).astype(F)).astype(F) + m[8 + k] * F(0.0)).astype(F) + m[12 + k] * F(1.0)).astype(F)

    inv = (F(1.0) / row(3)).astype(F)
    sx, sy = (row(0) * inv).astype(F), (row(1) * inv).astype(F)
    n = len(x)
    if R > 0.0:
        ab = _concentric_disk(np.asarray(u_lens, F))
        lx, ly = (F(R) * ab[:, 0]).astype(F), (F(R) * ab[:, 1]).astype(F)
        o = np.stack([(sx + lx).astype(F), (sy + ly).astype(F), np.zeros(n, F)], axis=1)
        d = _normalize(np.stack([-lx, -ly, np.full(n, -F(Fd), F)], axis=1).astype(F))
    else:
        o = np.stack([sx, sy, np.zeros(n, F)], axis=1)
        d = np.tile(np.array([0, 0, -1], F), (n, 1))
    return _to_world(c2w, o, d)


def panorama_fold(width, height, lon_min=-PI_F, lon_max=PI_F, lat_min=-HALF_PI_F, lat_max=HALF_PI_F):
    """The host's fold, each value rounded once: lon0, dlon, lat1, dlat, inv_w, inv_h."""
    return F(lon_min), F(F(lon_max) - F(lon_min)), F(lat_max), F(F(lat_max) - F(lat_min)), F(F(1.0) / F(width)), F(F(1.0) / F(height))


def panorama_rays(c2w, width, height, pixels, u_filter, filter_type, radius, window=()):
    lon0, dlon, lat1, dlat, inv_w, inv_h = panorama_fold(width, height, *window)
    pf = film_point(pixels, u_filter, filter_type, radius)
    lon = (lon0 + ((pf[:, 0] * inv_w).astype(F) * dlon).astype(F)).astype(F)
    lat = (lat1 - ((pf[:, 1] * inv_h).astype(F) * dlat).astype(F)).astype(F)
    sl, cl = _sincos(lon)
    sp, cp = _sincos(lat)
    d = _normalize(np.stack([(cp * sl).astype(F), sp, -(cp * cl).astype(F)], axis=1).astype(F))
    return _to_world(c2w, np.zeros_like(d), d)


def panorama_angles(width, height, pixels, window=(-np.pi, np.pi, -np.pi / 2, np.pi / 2)):
    """The closed form in float64 for pixel centres: (longitude, latitude)."""
    px = np.asarray(pixels, np.float64)
    lon = window[0] + (px[:, 0] + 0.5) / width * (window[1] - window[0])
    lat = window[3] - (px[:, 1] + 0.5) / height * (window[3] - window[2])
    return lon, lat
