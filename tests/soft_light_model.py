"""The numpy restatement of the soft punctual lights: a point or spot light with a radius, a sun with an angle -- the host fold of the
three record words, and the light sample that draws its point from u_sample, in float32 with the operand orders the section gives. What a delta light
shares with them (the fold of everything else, the dot product, the ray-origin offset, the selection) comes from tests/punctual_model.py; a light of
size 0 IS that model's light. It shares no text with the library: tests/test_soft_lights.py holds the host hook to it bit for bit,
tests/test_gpu_soft_lights.py the device probe."""
import math

import numpy as np

from tests import punctual_model as pm

F = np.float32
POINT, SPOT, SUN = pm.POINT, pm.SPOT, pm.SUN


def fma(a, b, c):
    """fma of float32 operands, correctly rounded once. The product is exact in float64; the sum s = p + c is rounded to 53 bits with the exact
    error e (two-sum). Rounding s to float32 is the rounding of p + c itself unless s sits exactly half way between two float32 neighbours, where e
    says which side the true value is on."""
    a, b, c = (np.asarray(v, F).astype(np.float64) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        r = s.astype(F)
        d = s - r.astype(np.float64)
        nb = np.nextafter(r, np.where(d > 0, F(np.inf), F(-np.inf)).astype(F))
        tie = (d != 0) & np.isfinite(s) & ((s - r.astype(np.float64)) == (nb.astype(np.float64) - s))
        fix = tie & (e != 0) & ((e > 0) == (d > 0))
    return np.where(fix, nb, r).astype(F)


def sincos(x):
    """sin and cos as the library's contract tier computes them: reduction by pi/2 in three fused steps, then the Cephes single-precision polynomials"""
    x = np.asarray(x, F)
    with np.errstate(all="ignore"):
        kf = np.rint(x * F(0.636619772367581343)).astype(F)
        r = fma(-kf, F(1.5703125), x)
        r = fma(-kf, F(4.837512969970703125e-4), r)
        r = fma(-kf, F(7.54978995489188216e-8), r)
        z = r * r
        ps = fma(fma(F(-1.9515295891e-4), z, F(8.3321608736e-3)), z, F(-1.6666654611e-1))
        sn = fma(r * z, ps, r)
        pc = fma(fma(F(2.443315711809948e-5), z, F(-1.388731625493765e-3)), z, F(4.166664568298827e-2))
        cs = fma(z * z, pc, fma(F(-0.5), z, F(1.0)))
        k = kf.astype(np.int32)
    odd = (k & 1) != 0
    s, c = np.where(odd, cs, sn), np.where(odd, sn, cs)
    s = np.where((k & 2) != 0, -s, s)
    c = np.where(((k + 1) & 2) != 0, -c, c)
    return s.astype(F), c.astype(F)


def concentric_disk(u):
    """Shirley-Chiu, unit square -> unit disk, (rows, 2) -> (rows, 2): the warp the lens uses"""
    u = np.asarray(u, F)
    with np.errstate(all="ignore"):
        sx, sy = F(2) * u[:, 0] - F(1), F(2) * u[:, 1] - F(1)
        first = np.abs(sx) > np.abs(sy)
        r = np.where(first, sx, sy)
        theta = np.where(first, F(0.785398163397448310) * (sy / sx), F(1.570796326794896619) - F(0.785398163397448310) * (sx / sy)).astype(F)
        sn, cs = sincos(theta)
        out = np.stack([r * cs, r * sn], axis=1)
    out[(sx == 0) & (sy == 0)] = 0
    return out.astype(F)


def frame(n):
    """the tangent frame (t, s) around unit vectors n (rows, 3): t in the plane of the two larger-by-rule components, s = n x t"""
    n = np.asarray(n, F)
    x, y, z = n[:, 0], n[:, 1], n[:, 2]
    zero = np.zeros_like(x)
    with np.errstate(all="ignore"):
        first = np.abs(x) > np.abs(y)
        ta = np.stack([-z, zero, x], axis=1) * (F(1) / np.sqrt(x * x + z * z))[:, None]
        tb = np.stack([zero, z, -y], axis=1) * (F(1) / np.sqrt(y * y + z * z))[:, None]
        t = np.where(first[:, None], ta, tb).astype(F)
        s = np.stack([y * t[:, 2] - z * t[:, 1], z * t[:, 0] - x * t[:, 2], x * t[:, 1] - y * t[:, 0]], axis=1).astype(F)
    return t, s


def fold(light, color_pipeline=0):
    """light: punctual_model's dict plus radius (point, spot) and angle (sun, the full angular diameter) -> its record plus radius, cos_max, k"""
    rec = pm.fold(light, color_pipeline)
    rec["radius"], rec["cos_max"], rec["k"] = F(0), F(0), F(0)
    if rec["kind"] != SUN:
        rec["radius"] = F(light.get("radius", 0.0))
    elif float(F(light.get("angle", 0.0))) > 0:
        cm = math.cos(0.5 * float(F(light["angle"])))
        rec["cos_max"], rec["k"] = F(cm), F(2.0 / (1.0 + cm))
    return rec


def record_words(rec):
    """the sixteen 32-bit words of the record the kernels read, as uint32"""
    w = np.zeros(16, F)
    w[0:3], w[4:7], w[7], w[8:11], w[11], w[12] = rec["q"], rec["a"], rec["cos_o"], rec["c"], rec["cos_i"], rec["inv_span"]
    w[13], w[14], w[15] = rec["radius"], rec["cos_max"], rec["k"]
    w = w.view(np.uint32).copy()
    w[3] = rec["kind"]
    return w


def is_soft(rec):
    return bool(rec["cos_max"] != 0) if rec["kind"] == SUN else bool(rec["radius"] != 0)


def falloff(rec, ct):
    with np.errstate(all="ignore"):
        if rec["inv_span"] != 0:
            x = (ct - rec["cos_o"]) * rec["inv_span"]
            s = np.where(np.isnan(x), F(0), np.minimum(np.maximum(x, F(0)), F(1))).astype(F)
            return ((s * s) * (F(3) - F(2) * s)).astype(F)
        return np.where(ct > rec["cos_o"], F(1), F(0)).astype(F)


def sample(rec, p, n, u):
    """The light's sample at points p with normals n for the numbers u ((rows, 3), (rows, 3), (rows, 2), float32) -> li, wi, ro (rows, 3), tmax, valid.
    A record without a size: punctual_model's sample, which never looks at u."""
    if not is_soft(rec):
        return pm.sample(rec, p, n)
    p, n, u = np.ascontiguousarray(p, F), np.ascontiguousarray(n, F), np.ascontiguousarray(u, F)
    rows = p.shape[0]
    c = rec["c"][None, :]
    with np.errstate(all="ignore"):
        if rec["kind"] == SUN:
            ct = F(1) - u[:, 0] * (F(1) - rec["cos_max"])
            st = np.sqrt(np.maximum(F(1) - ct * ct, F(0)))
            sp, cp = sincos((F(2) * F(math.pi)) * u[:, 1])
            axis = np.repeat(-rec["a"][None, :], rows, axis=0)
            t, s = frame(axis)
            wi = (t * (st * cp)[:, None] + s * (st * sp)[:, None]) + axis * ct[:, None]
            li = np.repeat(c * rec["k"], rows, axis=0)
            tmax = np.full(rows, F(1e20), F)
            ok = np.ones(rows, bool)
            zero = np.zeros(rows, bool)
        else:
            q = rec["q"][None, :]
            d = q - p
            dist2 = pm._dot(d, d)
            zero = dist2 == 0
            nd = -(d * (F(1) / np.sqrt(dist2))[:, None])
            t, s = frame(nd)
            dd = concentric_disk(u)
            y = q + (t * (rec["radius"] * dd[:, 0])[:, None] + s * (rec["radius"] * dd[:, 1])[:, None])
            w = y - p
            w2 = pm._dot(w, w)
            dist = np.sqrt(w2)
            wi = w * (F(1) / dist)[:, None]
            cosl = -pm._dot(wi, nd)
            if rec["kind"] == POINT:
                li = (c * cosl[:, None]) * (F(1) / w2)[:, None]
                ok = np.ones(rows, bool)
            else:
                f = falloff(rec, -pm._dot(wi, np.repeat(rec["a"][None, :], rows, axis=0)))
                li = ((c * f[:, None]) * cosl[:, None]) * (F(1) / w2)[:, None]
                ok = f > 0
            ok = ok & (cosl > 0)
            tmax = dist * (F(1) - F(1e-3))
        nf = np.where((pm._dot(n, wi) < 0)[:, None], -n, n)
        ro = pm.offset_ray_origin(p, nf)
        valid = ok & np.all(np.isfinite(li), axis=1)
    li, wi, ro, tmax = li.astype(F), wi.astype(F), ro.astype(F), tmax.astype(F)
    li[zero], wi[zero], ro[zero], tmax[zero], valid[zero] = 0, 0, 0, 0, False  # p == q: nothing is computed
    return li, wi, ro, tmax, valid


def light_sample_rows(table, records, rows):
    """punctual_model.light_sample_rows for rows (n, 9) = p, n, u_select, u_sample: what akr_host_light_sample_soft answers"""
    rows = np.ascontiguousarray(rows, F).reshape(-1, 9)
    idx, pdf = pm.alias_pick(table[0], table[1], table[2], rows[:, 6])
    out = np.zeros((rows.shape[0], 13), F)
    out[:, 6] = pdf
    for l, rec in enumerate(records):
        sel = idx == l
        if rec is None or not sel.any():
            continue
        li, wi, ro, tmax, valid = sample(rec, rows[sel, 0:3], rows[sel, 3:6], rows[sel, 7:9])
        o = out[sel]
        o[:, 0:3], o[:, 3:6], o[:, 7:10], o[:, 10], o[:, 11], o[:, 12] = li, wi, ro, tmax, valid.astype(F), 1.0
        out[sel] = o
    return out, idx.astype(np.uint32)
