"""akr_denoise restated in numpy float32 from DESIGN.md 4.10 -- one numpy operation per written operation, the 25 taps in the stated
order, exp_f through the oracle -- and the inputs the denoiser tests share (tests/test_denoise.py on the host, tests/test_gpu_denoise.py on
the device). Nothing here reads the library under test."""
import functools
import os

import numpy as np

from akari_render_amd import abi
from tests.probe_matrix import oracle_exp

f32 = np.float32
B3 = [f32(1 / 16), f32(1 / 4), f32(3 / 8), f32(1 / 4), f32(1 / 16)]
# (W, H). At 33 x 17 and step 16 the rows 1 .. 15 have no tap row but their own inside the image (y - 16 < 0, y + 16 >= 17); at 70 x 45 the taps
# of step 16 reach 32 pixels, two 16-wide tiles, to both sides of the columns 32 .. 37.
SHAPES = [(1, 1), (1, 7), (7, 1), (5, 5), (33, 17), (70, 45)]
# One frame on which the residue classes of steps 8 and 16 span several 16-wide tiles in both axes and differ in size (261 = 16 * 16 + 5,
# 259 = 16 * 16 + 3: tests/test_gpu_frame_thresholds.py derives it). It runs LARGE_CASES of cases(), not the whole matrix.
LARGE_SHAPE = (261, 259)
LARGE_CASES = ["random-all-demod-5", "edge-all-demod-5"]


def config(iterations=5, demodulate=1, sigma_color=2.0, sigma_normal=0.125, sigma_albedo=0.0625, albedo_floor=1e-3) -> abi.DenoiseConfig:
    c = abi.DenoiseConfig()
    c.iterations, c.demodulate = iterations, demodulate
    c.sigma_color, c.sigma_normal, c.sigma_albedo, c.albedo_floor = sigma_color, sigma_normal, sigma_albedo, albedo_floor
    return c


def film_of(rgb, weight=None, splat=None) -> np.ndarray:
    """A film accumulator [rgb 3N | splat 3N | weight N] whose rgb plane is `rgb` (H, W, 3) times the per-pixel weight."""
    rgb = np.asarray(rgb, dtype=f32)
    h, w = rgb.shape[:2]
    n = w * h
    wt = np.ones(n, dtype=f32) if weight is None else np.asarray(weight, dtype=f32).reshape(n)
    sp = np.zeros((n, 3), dtype=f32) if splat is None else np.asarray(splat, dtype=f32).reshape(n, 3)
    return np.concatenate([(rgb.reshape(n, 3) * wt[:, None]).astype(f32).reshape(-1), sp.reshape(-1), wt])


def resolve_np(film, w, h, splat_scale=1.0) -> np.ndarray:
    """k_film_resolve: rgb / (w == 0 ? 1 : w) + splat * splat_scale."""
    n = w * h
    film = np.asarray(film, dtype=f32)
    wt = film[6 * n:7 * n]
    inv = np.where(wt == 0, f32(1), wt).astype(f32)
    with np.errstate(all="ignore"):
        return (film[:3 * n].reshape(n, 3) / inv[:, None] + film[3 * n:6 * n].reshape(n, 3) * f32(splat_scale)).reshape(h, w, 3)


def _exp(v: np.ndarray) -> np.ndarray:
    """exp_f of every element through the oracle, each distinct bit pattern once."""
    v = np.ascontiguousarray(v, dtype=f32)
    u, inv = np.unique(v.view(np.uint32).reshape(-1), return_inverse=True)
    return oracle_exp(u.view(f32))[inv].reshape(v.shape)


def _dist2(p, q):
    d = p - q
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _k(sigma):
    sigma = f32(sigma)
    with np.errstate(all="ignore"):
        return f32(0) if sigma == 0 else f32(1) / (sigma * sigma)


def denoise_np(w, h, color, albedo=None, normal=None, cfg=None, splat_scales=(1.0, 1.0, 1.0), valid_override=None) -> np.ndarray:
    """The definition. color / albedo / normal: film accumulators (7 N floats) or None. valid_override: a mask ANDed into the validity (the
    NaN-pixel property marks a pixel invalid with it). -> (H, W, 3) float32."""
    cfg = cfg or config()
    zero = np.zeros((h, w, 3), dtype=f32)
    c = resolve_np(color, w, h, splat_scales[0])
    a = resolve_np(albedo, w, h, splat_scales[1]) if albedo is not None else zero
    n = resolve_np(normal, w, h, splat_scales[2]) if normal is not None else zero
    floor = f32(cfg.albedo_floor)
    with np.errstate(all="ignore"):
        d = np.where(a > floor, a, floor).astype(f32) if (cfg.demodulate and albedo is not None) else np.ones((h, w, 3), dtype=f32)
        x = (c / d).astype(f32)
        valid = np.isfinite(x).all(-1) & np.isfinite(n).all(-1) & np.isfinite(a).all(-1)
        if valid_override is not None:
            valid = valid & valid_override
        kn = _k(cfg.sigma_normal) if normal is not None else f32(0)
        ka = _k(cfg.sigma_albedo) if albedo is not None else f32(0)
        for i in range(cfg.iterations):
            s = 1 << i
            kc = _k(f32(cfg.sigma_color) * f32(2.0 ** -i))
            acc = np.zeros((h, w, 3), dtype=f32)
            wsum = np.zeros((h, w), dtype=f32)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    y0, y1, x0, x1 = max(0, -s * dy), min(h, h - s * dy), max(0, -s * dx), min(w, w - s * dx)
                    if y0 >= y1 or x0 >= x1:
                        continue  # every such tap lies outside the image
                    P = (slice(y0, y1), slice(x0, x1))
                    Q = (slice(y0 + s * dy, y1 + s * dy), slice(x0 + s * dx, x1 + s * dx))
                    m = valid[P] & valid[Q]
                    if not m.any():
                        continue
                    e = (_dist2(x[P], x[Q]) * kc + _dist2(n[P], n[Q]) * kn) + _dist2(a[P], a[Q]) * ka
                    wt = np.zeros(m.shape, dtype=f32)
                    wt[m] = (B3[dx + 2] * B3[dy + 2]) * _exp(-e[m])
                    acc[P] = np.where(m[..., None], acc[P] + wt[..., None] * x[Q], acc[P])
                    wsum[P] = np.where(m, wsum[P] + wt, wsum[P])
            x = np.where(valid[..., None], acc / wsum[..., None], x).astype(f32)
        return (x * d).astype(f32)


# ------------------------------------------------------------------------------------------------ shared inputs
def random_films(w, h, seed=0, weights=False, splat=False):
    """Seeded random colour / albedo / normal films of one frame: colours spread over a few decades, albedos in (0, 1] with some below the
    default floor, unit normals -- albedos and normals close enough to one another that taps weigh in under the default sigmas. weights: film weights other than 1 (and some 0); splat: a non-zero splat plane."""
    rng = np.random.default_rng(1000 * w + h + seed)
    n = w * h
    color = (rng.random((h, w, 3)) * np.exp(rng.uniform(-3, 2, size=(h, w, 1)))).astype(f32)
    albedo = (np.array([0.6, 0.4, 0.3]) + rng.uniform(-0.03, 0.03, size=(h, w, 3))).astype(f32)
    albedo[rng.random((h, w)) < 0.1] = f32(2e-4)
    normal = (np.array([0.0, 0.0, 1.0]) + 0.05 * rng.normal(size=(h, w, 3))).astype(f32)
    normal = (normal / np.linalg.norm(normal, axis=-1, keepdims=True)).astype(f32)
    wt = None
    if weights:
        wt = rng.uniform(0.5, 20.0, size=n).astype(f32)
        wt[rng.random(n) < 0.05] = 0
    sp = [rng.random((n, 3)).astype(f32) if splat else None for _ in range(3)]
    return film_of(color, wt, sp[0]), film_of(albedo, wt, sp[1]), film_of(normal, wt, sp[2])


def step_edge_films(w, h):
    """Two flat regions split down the middle: colour, albedo and normal all jump there, with a little seeded noise on the colour."""
    rng = np.random.default_rng(7 * w + h)
    left = (np.arange(w) < (w + 1) // 2)[None, :, None]
    color = np.where(left, f32(0.8), f32(0.1)) * np.ones((h, w, 3), dtype=f32) + (rng.random((h, w, 3)) * 0.05).astype(f32)
    albedo = np.where(left, f32(0.7), f32(0.2)) * np.ones((h, w, 3), dtype=f32)
    normal = np.where(left, np.array([0, 0, 1], dtype=f32), np.array([1, 0, 0], dtype=f32)) * np.ones((h, w, 3), dtype=f32)
    return film_of(color.astype(f32)), film_of(albedo.astype(f32)), film_of(normal.astype(f32))


# (name, films kind, use albedo, use normal, config, splat scales): the configurations both test files run on every shape
def cases():
    out = []
    for kind in ("random", "edge"):
        out.append((f"{kind}-all-demod-5", kind, True, True, config(), (1.0, 1.0, 1.0)))
    out.append(("random-all-nodemod-5", "random", True, True, config(demodulate=0), (1.0, 1.0, 1.0)))
    out.append(("random-colour-only-5", "random", False, False, config(), (1.0, 1.0, 1.0)))
    out.append(("random-all-demod-1", "random", True, True, config(iterations=1), (1.0, 1.0, 1.0)))
    out.append(("random-all-demod-0", "random", True, True, config(iterations=0), (1.0, 1.0, 1.0)))
    out.append(("random-normal-only-1", "random", False, True, config(iterations=1, sigma_color=0.5), (1.0, 1.0, 1.0)))
    out.append(("weights-all-demod-5", "weights", True, True, config(), (1.0, 1.0, 1.0)))
    out.append(("splat-all-demod-1", "splat", True, True, config(iterations=1), (0.25, 0.5, 2.0)))
    return out


@functools.lru_cache(maxsize=None)
def case_inputs(w, h, kind):
    if kind == "edge":
        return step_edge_films(w, h)
    return random_films(w, h, weights=kind == "weights", splat=kind == "splat")


@functools.lru_cache(maxsize=None)
def case_reference(w, h, name):
    """The restatement's result for one (shape, configuration): computed once per process, never modified."""
    _, kind, use_a, use_n, cfg, scales = next(c for c in cases() if c[0] == name)
    color, albedo, normal = case_inputs(w, h, kind)
    out = denoise_np(w, h, color, albedo if use_a else None, normal if use_n else None, cfg, scales)
    out.setflags(write=False)
    return out


def nan_pixel_inputs(w=41, h=23, at=(9, 17)):
    color, albedo, normal = random_films(w, h, seed=3)
    bad = color.copy()
    bad[3 * (at[0] * w + at[1]) + 1] = np.nan  # the green channel of one pixel
    # the same pixel made invalid by another route: a finite colour, a NaN in its normal
    marked = normal.copy()
    marked[3 * (at[0] * w + at[1])] = np.nan
    return w, h, at, color, albedo, normal, bad, marked


def check_nan_pixel(run):
    """run(color, albedo, normal) -> (H, W, 3). One NaN colour pixel is one NaN output pixel, in place, and no other pixel can tell that pixel
    from one that is invalid for another reason."""
    w, h, at, color, albedo, normal, bad, marked = nan_pixel_inputs()
    out = run(bad, albedo, normal)
    nan_pixels = np.isnan(out).any(-1)
    assert nan_pixels.sum() == 1 and nan_pixels[at]
    ref = run(color, albedo, marked)
    assert np.isfinite(ref).all()  # (the marked pixel passes its finite colour through)
    rest = ~nan_pixels
    assert np.array_equal(out[rest].view(np.uint32), ref[rest].view(np.uint32))
    clean = run(color, albedo, normal)
    assert not np.array_equal(clean[rest].view(np.uint32), out[rest].view(np.uint32))  # (the pixel did count while it was valid)


def rel_mse(img, ref) -> float:
    """mean over pixels and channels of (img - ref)^2 / (ref^2 + 0.01)."""
    img, ref = np.asarray(img, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.mean((img - ref) ** 2 / (ref ** 2 + 1e-2)))


def golden_cbox(root):
    """Oracle films of scenes/cbox at 64 x 64 (tests/golden/make_denoise_golden.py): the 16-spp pt film of cbox_64x64_16spp.npz, the albedo and
    ns (not remapped) films of 16 spp, and the resolved 2048-spp image."""
    g = np.load(os.path.join(root, "tests", "golden", "cbox_64x64_denoise.npz"))
    noisy = np.load(os.path.join(root, "tests", "golden", "cbox_64x64_16spp.npz"))["full"]
    return noisy, g["albedo"], g["ns"], g["ref"]
