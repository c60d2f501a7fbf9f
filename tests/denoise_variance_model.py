"""akr_denoise_variance restated in numpy float32 from DESIGN.md 4.10 "Variance guide" -- one numpy operation per written operation, the taps
in the stated order, exp_f through the oracle -- and the inputs its tests share (tests/test_denoise_variance.py on the host,
tests/test_gpu_denoise_variance.py on the device). The helpers are those of tests/denoise_model.py. Nothing here reads the library under test."""
import functools
import os

import numpy as np

from tests import denoise_model as dm
from tests.denoise_model import _dist2, _exp, _k, f32

G3 = [f32(1 / 4), f32(1 / 2), f32(1 / 4)]
SIGMA_VARIANCE = 8.0  # akr_denoise_config_default's (the sigma_variance table)
SHAPES = dm.SHAPES
LARGE_SHAPE, LARGE_CASES = dm.LARGE_SHAPE, dm.LARGE_CASES  # (the names are cases of this file's cases() as well)


def config(sigma_variance=SIGMA_VARIANCE, **kw):
    c = dm.config(**kw)
    c.sigma_variance = sigma_variance
    return c


def _window(w, h, ox, oy):
    """The centres P whose tap Q = P + (ox, oy) lies inside the image, as two slice pairs (None if there is none)."""
    y0, y1, x0, x1 = max(0, -oy), min(h, h - oy), max(0, -ox), min(w, w - ox)
    if y0 >= y1 or x0 >= x1:
        return None
    return (slice(y0, y1), slice(x0, x1)), (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))


def denoise_variance_np(w, h, color, half, albedo=None, normal=None, cfg=None, splat_scales=(1.0, 1.0, 1.0), valid_override=None) -> np.ndarray:
    """The definition. color / half / albedo / normal: film accumulators (7 N floats); albedo / normal may be None. -> (H, W, 3) float32."""
    cfg = cfg or config()
    N = w * h
    zero = np.zeros((h, w, 3), dtype=f32)
    color, half = np.asarray(color, dtype=f32), np.asarray(half, dtype=f32)
    c = dm.resolve_np(color, w, h, splat_scales[0])
    a = dm.resolve_np(albedo, w, h, splat_scales[1]) if albedo is not None else zero
    n = dm.resolve_np(normal, w, h, splat_scales[2]) if normal is not None else zero
    floor = f32(cfg.albedo_floor)
    with np.errstate(all="ignore"):
        d = np.where(a > floor, a, floor).astype(f32) if (cfg.demodulate and albedo is not None) else np.ones((h, w, 3), dtype=f32)
        x = (c / d).astype(f32)
        valid = np.isfinite(x).all(-1) & np.isfinite(n).all(-1) & np.isfinite(a).all(-1)
        if valid_override is not None:
            valid = valid & valid_override
        # prepare: the two-half estimate
        crgb, hrgb = color[:3 * N].reshape(h, w, 3), half[:3 * N].reshape(h, w, 3)
        wc, wa = color[6 * N:].reshape(h, w), half[6 * N:].reshape(h, w)
        wb = wc - wa
        xa = ((hrgb / wa[..., None]) / d).astype(f32)
        xb = (((crgb - hrgb) / wb[..., None]) / d).astype(f32)
        f = (wa * wb) / (wc * wc)
        r = _dist2(xa, xb) * f
        est = valid & (wa > 0) & (wb > 0) & np.isfinite(r)
        kn = _k(cfg.sigma_normal) if normal is not None else f32(0)
        ka = _k(cfg.sigma_albedo) if albedo is not None else f32(0)
        sv = f32(cfg.sigma_variance)
        kv = f32(1) / (sv * sv)
        # prefilter
        num = np.zeros((h, w), dtype=f32)
        den = np.zeros((h, w), dtype=f32)
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                pq = _window(w, h, dx, dy)
                if pq is None:
                    continue
                P, Q = pq
                m = valid[P] & est[Q]
                if not m.any():
                    continue
                wt = np.zeros(m.shape, dtype=f32)
                wt[m] = _exp(-(_dist2(n[P], n[Q]) * kn + _dist2(a[P], a[Q]) * ka)[m])
                num[P] = np.where(m, num[P] + wt * np.where(m, r[Q], f32(0)), num[P])
                den[P] = np.where(m, den[P] + wt, den[P])
        v = np.where(den > 0, num / np.where(den > 0, den, f32(1)), f32(0)).astype(f32)
        v = np.where(valid, v, f32(0)).astype(f32)
        # levels
        for i in range(cfg.iterations):
            s = 1 << i
            gn = np.zeros((h, w), dtype=f32)
            gd = np.zeros((h, w), dtype=f32)
            for dy in range(-1, 2):
                for dx in range(-1, 2):
                    pq = _window(w, h, s * dx, s * dy)
                    if pq is None:
                        continue
                    P, Q = pq
                    m = valid[P] & valid[Q]
                    gw = G3[dx + 1] * G3[dy + 1]
                    gn[P] = np.where(m, gn[P] + gw * v[Q], gn[P])
                    gd[P] = np.where(m, gd[P] + gw, gd[P])
            g = gn / gd
            kcp = kv / (g + f32(1e-10))
            acc = np.zeros((h, w, 3), dtype=f32)
            vacc = np.zeros((h, w), dtype=f32)
            wsum = np.zeros((h, w), dtype=f32)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    pq = _window(w, h, s * dx, s * dy)
                    if pq is None:
                        continue
                    P, Q = pq
                    m = valid[P] & valid[Q]
                    if not m.any():
                        continue
                    e = (_dist2(x[P], x[Q]) * kcp[P] + _dist2(n[P], n[Q]) * kn) + _dist2(a[P], a[Q]) * ka
                    wt = np.zeros(m.shape, dtype=f32)
                    wt[m] = (dm.B3[dx + 2] * dm.B3[dy + 2]) * _exp(-e[m])
                    acc[P] = np.where(m[..., None], acc[P] + wt[..., None] * x[Q], acc[P])
                    vacc[P] = np.where(m, vacc[P] + (wt * wt) * v[Q], vacc[P])
                    wsum[P] = np.where(m, wsum[P] + wt, wsum[P])
            x = np.where(valid[..., None], acc / wsum[..., None], x).astype(f32)
            v = np.where(valid, vacc / (wsum * wsum), v).astype(f32)
        return (x * d).astype(f32)


# ------------------------------------------------------------------------------------------------ shared inputs
def halves_of(w, h, kind, color_film, seed=0):
    """(C, H): a colour film C and a half film H of it. H is an independent seeded "first half" and C.rgb = H.rgb + B.rgb, C.w = H.w + B.w with
    B the given film, so that wB = C.w - H.w is exact wherever the sums are (weights of a few bits). kind "unequal": wA != wB, some wA = 0."""
    rng = np.random.default_rng(77 * w + h + seed)
    n = w * h
    B = np.asarray(color_film, dtype=f32)
    brgb = B[:3 * n].reshape(n, 3)
    bw = B[6 * n:]
    bres = brgb / np.where(bw == 0, f32(1), bw)[:, None]
    if kind == "unequal":
        hw = rng.integers(1, 9, size=n).astype(f32)  # small integers: bw + hw and (bw + hw) - hw are exact for the integer weights used with it
        hw[rng.random(n) < 0.1] = 0
    else:
        hw = bw.copy()
    hres = (bres * rng.uniform(0.7, 1.3, size=(n, 3))).astype(f32)  # the other half: the same image, 30 % noise
    H = np.concatenate([(hres * hw[:, None]).astype(f32).reshape(-1), np.zeros(3 * n, dtype=f32), hw])
    Cf = np.concatenate([(H[:3 * n] + B[:3 * n]).astype(f32), B[3 * n:6 * n], (hw + bw).astype(f32)])
    return Cf, H


# (name, films kind, halves kind, use albedo, use normal, config): the configurations both test files run on every shape
def cases():
    out = []
    for kind in ("random", "edge"):
        out.append((f"{kind}-all-demod-5", kind, "equal", True, True, config()))
    out.append(("random-all-demod-1", "random", "equal", True, True, config(iterations=1)))
    out.append(("random-all-demod-0", "random", "equal", True, True, config(iterations=0)))
    out.append(("random-colour-only-5", "random", "equal", False, False, config()))
    out.append(("random-unequal-halves-5", "intweights", "unequal", True, True, config()))
    out.append(("random-sigma-variance-0.75-5", "random", "equal", True, True, config(sigma_variance=0.75)))
    return out


@functools.lru_cache(maxsize=None)
def case_inputs(w, h, kind, halves):
    """(C, H, albedo, normal) of one shape: the films of tests/denoise_model.py as the second half, plus a first half."""
    if kind == "intweights":  # random films with integer weights 1 .. 16, so that the unequal halves' weight sums are exact
        rng = np.random.default_rng(5 * w + h)
        color, albedo, normal = dm.random_films(w, h, seed=2)
        n = w * h
        wt = rng.integers(1, 17, size=n).astype(f32)
        color = dm.film_of(dm.resolve_np(color, w, h), wt)
    else:
        color, albedo, normal = dm.case_inputs(w, h, kind)
    Cf, H = halves_of(w, h, halves, color)
    for f in (Cf, H):
        f.setflags(write=False)
    return Cf, H, albedo, normal


@functools.lru_cache(maxsize=None)
def case_reference(w, h, name):
    """The restatement's result for one (shape, configuration): computed once per process, never modified."""
    _, kind, halves, use_a, use_n, cfg = next(c for c in cases() if c[0] == name)
    Cf, H, albedo, normal = case_inputs(w, h, kind, halves)
    out = denoise_variance_np(w, h, Cf, H, albedo if use_a else None, normal if use_n else None, cfg)
    out.setflags(write=False)
    return out


def golden_halves(root):
    """Oracle pt films of scenes/cbox at 64 x 64, 16 spp at spp_per_pass 8, seed 3 (tests/golden/make_denoise_halves_golden.py): the film after
    pass 1 (`half`) and after pass 2 (`full`)."""
    g = np.load(os.path.join(root, "tests", "golden", "cbox_64x64_halves.npz"))
    return g["half"], g["full"]
