"""The numpy restatement of the punctual lights: the host fold of a light into its record, the selection weights, and the light
sample, in float32 with the operand orders the section gives. It shares no text with the library: tests/test_punctual.py holds the host hook to it
bit for bit, tests/test_gpu_punctual.py the device probe."""
import math

import numpy as np

F = np.float32
POINT, SPOT, SUN = 0, 1, 2
PUNCT_INST = 0xFFFFFFFE


def _dot(a, b):
    """(ax bx + ay by) + az bz, float32, over the last axis"""
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def fold(light, color_pipeline=0):
    """light: dict(type, position, direction, color, strength, cone_angle, blend) -> the record: double arithmetic, every value rounded once"""
    assert color_pipeline == 0, "the model states the default colour pipeline only"
    t = int(light["type"])
    rec = {"kind": t, "q": np.zeros(3, F), "a": np.zeros(3, F), "cos_o": F(0), "cos_i": F(0), "inv_span": F(0)}
    if t != SUN:
        rec["q"] = np.asarray(light["position"], F)
    if t != POINT:
        d = np.asarray(light["direction"], F).astype(np.float64)
        ln = math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        rec["a"] = (d / ln).astype(F)
    if t == SPOT:
        cone, blend = float(F(light["cone_angle"])), float(F(light.get("blend", 0.0)))
        rec["cos_o"] = F(math.cos(cone))
        rec["cos_i"] = F(math.cos(cone * (1.0 - blend)))
        rec["inv_span"] = F(0) if rec["cos_i"] == rec["cos_o"] else F(1) / (rec["cos_i"] - rec["cos_o"])
    rec["c"] = np.asarray(light.get("color", (1, 1, 1)), F) * F(light.get("strength", 1.0))
    return rec


def is_light(light):
    return float(light.get("strength", 1.0)) > 0 and max(light.get("color", (1, 1, 1))) > 0


def bounds_radius(lo, hi):
    ext = np.asarray(hi, F).astype(np.float64) - np.asarray(lo, F).astype(np.float64)
    r = 0.5 * math.sqrt(float(np.sum(ext * ext)))
    return r if (r > 0 and math.isfinite(r)) else 1.0


def power(rec, R):
    m = float(np.max(rec["c"]))
    if rec["kind"] == POINT:
        return F((4.0 * math.pi) * m)
    if rec["kind"] == SPOT:
        return F(((2.0 * math.pi) * (1.0 - 0.5 * (float(rec["cos_i"]) + float(rec["cos_o"])))) * m)
    return F(((math.pi * R) * R) * m)


def selection_pdfs(powers):
    """AliasTable's pdf: w / sum with the sum accumulated in float32, in order"""
    w = np.asarray(powers, F)
    s = F(0)
    for v in w:
        s = F(s + v)
    return (w / s).astype(F)


def alias_pick(j, t, pdf, u):
    """alias_sample_and_remap over the table (j, t, pdf) for float32 u: the index taken and its pdf"""
    n = len(j)
    u = np.asarray(u, F)
    fn = F(n)
    fi = np.floor(u * fn)
    i = np.clip(fi.astype(np.int64), 0, n - 1)
    u1 = (u * fn - i.astype(F)).astype(F)
    first = u1 < t[i]
    idx = np.where(first, i, j[i].astype(np.int64))
    return idx, pdf[idx]


def _offset_comp(p, n):
    with np.errstate(over="ignore", invalid="ignore"):
        of_i = (F(256.0) * n).astype(np.int32)  # truncates towards zero, as the cast does
        bits = p.view(np.int32)
        pi = np.where(p < 0, bits - of_i, bits + of_i).astype(np.int32)
        p_i = pi.view(F)
        return np.where(np.abs(p) < F(1.0 / 32.0), p + F(1.0 / 65536.0) * n, p_i).astype(F)


def offset_ray_origin(p, n):
    return np.stack([_offset_comp(np.ascontiguousarray(p[:, k]), np.ascontiguousarray(n[:, k])) for k in range(3)], axis=1)


def cone_cosine(rec, p):
    """ct = -dot(wi, a) of a POINT / SPOT record at points p (rows, 3), float32, as the sample computes it"""
    p = np.ascontiguousarray(p, F)
    with np.errstate(all="ignore"):
        d = rec["q"][None, :] - p
        dist = np.sqrt(_dot(d, d))
        wi = d * (F(1) / dist)[:, None]
        return (-_dot(wi, np.repeat(rec["a"][None, :], p.shape[0], axis=0))).astype(F)


def sample(rec, p, n):
    """The light's sample at points p with normals n ((rows, 3) float32 each) -> li, wi, ro (rows, 3), tmax, valid (rows,)"""
    p, n = np.ascontiguousarray(p, F), np.ascontiguousarray(n, F)
    rows = p.shape[0]
    c = rec["c"][None, :]
    with np.errstate(all="ignore"):
        if rec["kind"] == SUN:
            wi = np.repeat(-rec["a"][None, :], rows, axis=0)
            li = np.repeat(c, rows, axis=0)
            tmax = np.full(rows, F(1e20), F)
            ok = np.ones(rows, bool)
            zero = np.zeros(rows, bool)
        else:
            d = rec["q"][None, :] - p
            dist2 = _dot(d, d)
            zero = dist2 == 0
            dist = np.sqrt(dist2)
            wi = d * (F(1) / dist)[:, None]
            if rec["kind"] == POINT:
                li = c * (F(1) / dist2)[:, None]
                ok = np.ones(rows, bool)
            else:
                ct = cone_cosine(rec, p)
                if rec["inv_span"] != 0:
                    s = np.minimum(np.maximum((ct - rec["cos_o"]) * rec["inv_span"], F(0)), F(1))
                    s = np.where(np.isnan((ct - rec["cos_o"]) * rec["inv_span"]), F(0), s).astype(F)  # max_f / min_f give the bound for a NaN
                    f = (s * s) * (F(3) - F(2) * s)
                else:
                    f = np.where(ct > rec["cos_o"], F(1), F(0)).astype(F)
                li = (c * f[:, None]) * (F(1) / dist2)[:, None]
                ok = f > 0
            tmax = dist * (F(1) - F(1e-3))
        nf = np.where((_dot(n, wi) < 0)[:, None], -n, n)
        ro = offset_ray_origin(p, nf)
        valid = ok & np.all(np.isfinite(li), axis=1)
    li, wi, ro, tmax = li.astype(F), wi.astype(F), ro.astype(F), tmax.astype(F)
    # p == q: nothing is computed
    li[zero], wi[zero], ro[zero], tmax[zero], valid[zero] = 0, 0, 0, 0, False
    return li, wi, ro, tmax, valid


def light_sample_rows(table, records, rows):
    """table: (j, t, pdf) of the light list; records: per light its record, or None for an emitter / the environment; rows (n, 7) = p, n, u_select
    -> out (n, 13) = li, wi, pdf, ro, tmax, valid, delta and the light index, as akr_host_light_sample answers"""
    rows = np.ascontiguousarray(rows, F).reshape(-1, 7)
    idx, pdf = alias_pick(table[0], table[1], table[2], rows[:, 6])
    out = np.zeros((rows.shape[0], 13), F)
    out[:, 6] = pdf
    for l, rec in enumerate(records):
        sel = idx == l
        if rec is None or not sel.any():
            continue
        li, wi, ro, tmax, valid = sample(rec, rows[sel, 0:3], rows[sel, 3:6])
        o = out[sel]
        o[:, 0:3], o[:, 3:6], o[:, 7:10], o[:, 10], o[:, 11], o[:, 12] = li, wi, ro, tmax, valid.astype(F), 1.0
        out[sel] = o
    return out, idx.astype(np.uint32)
