"""akr_display_transform restated in numpy float32 from DESIGN.md 4.12 -- one numpy operation per written operation, in the stated operand
order, exp_f and log_f through the oracle -- and the inputs the display tests share (tests/test_display.py on the host,
tests/test_gpu_display.py on the device). Nothing here reads the library under test."""
import functools

import numpy as np

from akari_render_amd import abi
from tests.denoise_model import film_of, resolve_np
from tests.probe_matrix import oracle_exp, oracle_log

f32 = np.float32
LN2, INV_LN2 = f32(0.6931471805599453), f32(1.4426950408889634)
# (W, H): a pyramid that is 1 x 1 from the start; one that reaches 1 x 1 at level 3; odd sizes at every level (41 -> 21 -> 11 -> 6 -> 3 -> 2 -> 1);
# a frame wider than 64 and one wider than 128 and taller than 64, whose levels 1 and 2 cross the 16-pixel tiles of the LDS blur unevenly
SHAPES = [(1, 1), (7, 5), (41, 23), (70, 45), (130, 67)]
# One frame past the histogram kernel's grid cap of 2048 workgroups x 256 threads (tests/test_gpu_frame_thresholds.py derives it): 790 777
# pixels, odd, no multiple of 16, 64 or 256 per side. It runs the histogram and ONE configuration of cases(), not the whole matrix.
LARGE_SHAPE = (1031, 767)
LARGE_CASE = "hable-auto-bloom5"
CURVES = [abi.DISPLAY_LINEAR, abi.DISPLAY_REINHARD, abi.DISPLAY_ACES, abi.DISPLAY_HABLE]
KINDS = ["random", "special"]
SPLAT_SCALE = {"random": 0.375, "special": 1.0}


def config(curve=abi.DISPLAY_ACES, auto_exposure=0, exposure_ev=0.0, key=0.18, low_permille=50, high_permille=20, white=0.0, bloom_strength=0.0,
           bloom_threshold=1.0, bloom_levels=5) -> abi.DisplayConfig:
    c = abi.DisplayConfig()
    c.curve, c.auto_exposure, c.exposure_ev, c.key = curve, auto_exposure, exposure_ev, key
    c.low_permille, c.high_permille, c.white = low_permille, high_permille, white
    c.bloom_strength, c.bloom_threshold, c.bloom_levels = bloom_strength, bloom_threshold, bloom_levels
    return c


def _through(fn, v):
    """An oracle function of every element, each distinct bit pattern once."""
    v = np.ascontiguousarray(v, dtype=f32)
    u, inv = np.unique(v.view(np.uint32).reshape(-1), return_inverse=True)
    return fn(u.view(f32))[inv.reshape(-1)].reshape(v.shape).astype(f32)


def _exp1(x) -> np.float32:
    return f32(oracle_exp(np.array([x], dtype=f32))[0])


def max_f(a, b):
    return np.where(a > b, a, b).astype(f32)  # b when a is NaN


def min_f(a, b):
    return np.where(a < b, a, b).astype(f32)


def clamp_f(x, lo, hi):
    return min_f(max_f(x, f32(lo)), f32(hi))


def load(film, w, h, splat_scale=1.0) -> np.ndarray:
    """The input stage: resolve as akr_film_resolve does, then s(x) = clamp_f(x, 0, 65504). -> (H, W, 3)."""
    return clamp_f(resolve_np(film, w, h, splat_scale), 0.0, 65504.0)


def lum(c):
    return (f32(0.2126) * c[..., 0] + f32(0.7152) * c[..., 1]) + f32(0.0722) * c[..., 2]


def bins(c):
    """-> (bin per pixel, -1 = skipped) of sanitised pixels c (..., 3)."""
    L = lum(c).reshape(-1)
    out = np.full(L.shape, -1, dtype=np.int64)
    keep = ~(L < f32(2.0 ** -20))
    if keep.any():
        b = np.floor((_through(oracle_log, L[keep]) * INV_LN2 + f32(20)) * f32(8))
        out[keep] = np.clip(b.astype(np.int64), 0, 255)
    return out


def histogram(c):
    """-> (counts uint32[256], skipped): np.bincount of the restated bins."""
    b = bins(c)
    return np.bincount(b[b >= 0], minlength=256).astype(np.uint32), int(np.count_nonzero(b < 0))


def manual_exposure(cfg) -> np.float32:
    return _exp1(f32(cfg.exposure_ev) * LN2)


def exposure(cfg, counts) -> np.float32:
    """akr_display_exposure: integers and doubles as Python has them."""
    cnt = [int(v) for v in counts]
    total = sum(cnt)
    lo, hi = total * int(cfg.low_permille) // 1000, total * int(cfg.high_permille) // 1000
    for i in range(256):
        t = min(cnt[i], lo)
        cnt[i] -= t
        lo -= t
    for i in range(255, -1, -1):
        t = min(cnt[i], hi)
        cnt[i] -= t
        hi -= t
    num, den = 0.0, 0
    for i in range(256):
        num += float(cnt[i]) * (i + 0.5)
        den += cnt[i]
    if den == 0:
        return manual_exposure(cfg)
    avg = f32(num / float(den) / 8.0 - 20.0)
    return (f32(cfg.key) * _exp1(-avg * LN2)) * manual_exposure(cfg)


def box(src):
    sh, sw = src.shape[:2]
    dw, dh = (sw + 1) // 2, (sh + 1) // 2
    x0, y0 = 2 * np.arange(dw), 2 * np.arange(dh)
    x1, y1 = np.minimum(x0 + 1, sw - 1), np.minimum(y0 + 1, sh - 1)
    p00, p10, p01, p11 = src[y0][:, x0], src[y0][:, x1], src[y1][:, x0], src[y1][:, x1]
    return (((p00 + p10) + (p01 + p11)) * f32(0.25)).astype(f32)


def blur_pass(a, axis):
    n = a.shape[axis]
    tap = lambda d: np.take(a, np.clip(np.arange(n) + d, 0, n - 1), axis=axis)  # noqa: E731
    return (((tap(-2) + tap(2)) * f32(0.0625) + (tap(-1) + tap(1)) * f32(0.25)) + tap(0) * f32(0.375)).astype(f32)


def blur(a):
    return blur_pass(blur_pass(a, 1), 0)  # horizontal, then vertical


def up(src, dw, dh):
    sh, sw = src.shape[:2]
    x, y = np.arange(dw), np.arange(dh)
    x0, x1 = np.clip((x - 1) // 2, 0, sw - 1), np.clip((x - 1) // 2 + 1, 0, sw - 1)
    y0, y1 = np.clip((y - 1) // 2, 0, sh - 1), np.clip((y - 1) // 2 + 1, 0, sh - 1)
    wx0 = np.where(x & 1, f32(0.75), f32(0.25)).astype(f32)[None, :, None]
    wy0 = np.where(y & 1, f32(0.75), f32(0.25)).astype(f32)[:, None, None]
    wx1, wy1 = f32(1) - wx0, f32(1) - wy0  # (3/4 or 1/4: exact)
    c00, c10, c01, c11 = src[y0][:, x0], src[y0][:, x1], src[y1][:, x0], src[y1][:, x1]
    return (wy0 * (wx0 * c00 + wx1 * c10) + wy1 * (wx0 * c01 + wx1 * c11)).astype(f32)


def hable(x):
    A, B, Cc, D, E, F = f32(0.15), f32(0.5), f32(0.1), f32(0.2), f32(0.02), f32(0.3)
    return (x * (A * x + Cc * B) + D * E) / (x * (A * x + B) + D * F) - (D * E) / (D * F)


def curve(x, cfg):
    x = np.asarray(x, dtype=f32)
    white = f32(cfg.white) if cfg.white != 0 else (f32(11.2) if cfg.curve == abi.DISPLAY_HABLE else f32(4.0))
    with np.errstate(all="ignore"):
        if cfg.curve == abi.DISPLAY_REINHARD:
            y = (x * (f32(1) + x / (white * white))) / (f32(1) + x)
        elif cfg.curve == abi.DISPLAY_ACES:
            y = (x * (f32(2.51) * x + f32(0.03))) / (x * (f32(2.43) * x + f32(0.59)) + f32(0.14))
        elif cfg.curve == abi.DISPLAY_HABLE:
            y = hable(x) / hable(white)
        else:
            y = x
    return clamp_f(y, 0.0, 1.0)


def display_np(w, h, film, cfg, splat_scale=1.0):
    """The definition. film: a film accumulator (7 N floats). -> ((H, W, 3) float32, the exposure k)."""
    c = load(film, w, h, splat_scale)
    k = exposure(cfg, histogram(c)[0]) if cfg.auto_exposure else manual_exposure(cfg)
    e = (k * c).astype(f32)
    if cfg.bloom_strength != 0:
        Le = lum(e)
        b = (e * (max_f(Le - f32(cfg.bloom_threshold), f32(0)) / max_f(Le, f32(1e-4)))[..., None]).astype(f32)
        D = [b]
        for _ in range(cfg.bloom_levels):
            D.append(box(D[-1]))
        G = [None] + [blur(d) for d in D[1:]]
        U = G[cfg.bloom_levels]
        for l in range(cfg.bloom_levels - 1, 0, -1):
            U = (G[l] + up(U, G[l].shape[1], G[l].shape[0])).astype(f32)
        e = (e + f32(cfg.bloom_strength) * (up(U, w, h) * (f32(1) / f32(cfg.bloom_levels)))).astype(f32)
    return curve(e, cfg), k


# ------------------------------------------------------------------------------------------------ shared inputs
def random_film(w, h, seed=0):
    """A seeded HDR film: colours spread over seven decades around 1, weights other than 1 (some 0) and a splat plane."""
    rng = np.random.default_rng(1000 * w + h + seed)
    n = w * h
    color = (rng.random((h, w, 3)) * np.exp(rng.uniform(-8, 8, size=(h, w, 1)))).astype(f32)
    wt = rng.uniform(0.5, 20.0, size=n).astype(f32)
    wt[rng.random(n) < 0.05] = 0
    return film_of(color, wt, (rng.random((n, 3)) * 0.1).astype(f32))


def special_film(w, h):
    """A random film of weight 1 with a NaN, +inf, -inf, negative, zero and 1e6 pixel (whole pixels and single channels), spread over the frame."""
    rng = np.random.default_rng(77 * w + h)
    n = w * h
    film = film_of((rng.random((h, w, 3)) * np.exp(rng.uniform(-3, 3, size=(h, w, 1)))).astype(f32))
    specials = [(np.nan,) * 3, (np.inf,) * 3, (-np.inf,) * 3, (-2.5,) * 3, (0.0,) * 3, (1e6,) * 3, (0.5, np.nan, 0.5), (np.inf, 0.1, -1.0), (1e6, 0.0, 3.0)]
    for j, v in enumerate(specials):
        p = (j * 7919 + 3) % n
        film[3 * p:3 * p + 3] = np.array(v, dtype=f32)
    return film


@functools.lru_cache(maxsize=None)
def case_film(w, h, kind):
    f = random_film(w, h) if kind == "random" else special_film(w, h)
    f.setflags(write=False)
    return f


# (name, configuration): every curve x {manual, auto} x {bloom off, 1, 5, 8 levels}
def cases():
    out = []
    for cv in CURVES:
        for auto in (0, 1):
            for levels in (0, 1, 5, 8):
                cfg = config(curve=cv, auto_exposure=auto, exposure_ev=-0.5 if auto else 0.75, white=6.0 if auto else 0.0,
                             bloom_strength=0.5 if levels else 0.0, bloom_threshold=1.0, bloom_levels=levels if levels else 5)
                out.append((f"{abi.DISPLAY_CURVE_NAMES[cv]}-{'auto' if auto else 'manual'}-bloom{levels}", cfg))
    return out


@functools.lru_cache(maxsize=None)
def case_reference(w, h, kind, name):
    """The restatement's (image, k) for one (shape, film, configuration): computed once per process, never modified."""
    cfg = next(c for n, c in cases() if n == name)
    out, k = display_np(w, h, case_film(w, h, kind), cfg, SPLAT_SCALE[kind])
    out.setflags(write=False)
    return out, k


@functools.lru_cache(maxsize=None)
def case_histogram(w, h, kind):
    return histogram(load(case_film(w, h, kind), w, h, SPLAT_SCALE[kind]))
