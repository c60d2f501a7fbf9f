"""Numpy restatement of adaptive sampling (csrc/device/dadapt.h, host/api_adapt.cpp): the tile error estimate, the half film's
open / close passes and the whole adaptive render as a pure function of the oracle's prefix films -- pixels are independent, so the film of a
pixel that received the samples of k rounds is the oracle's film after k rounds at that pixel. Every operation is one f32 numpy operation in
the order the header writes it."""
import functools

import numpy as np

f32 = np.float32
INF = f32(np.inf)

# (frame w, frame h, tile w, tile h): an edge column of half-empty tiles; one wave; 192 slots in a tree of 256; 1024; 4096 (the cap)
SHAPES = [(40, 24, 16, 8), (24, 16, 8, 8), (50, 20, 24, 8), (70, 40, 32, 32), (100, 70, 64, 64)]


def grid(w, h, tw, th):
    return (w + tw - 1) // tw, (h + th - 1) // th


def tile_mask(w, h, tw, th, tiles) -> np.ndarray:
    """(h, w) bool: the pixels of the listed tiles."""
    tiles_x, tiles_y = grid(w, h, tw, th)
    on = np.zeros(tiles_x * tiles_y, dtype=bool)
    on[np.asarray(tiles, dtype=np.int64)] = True
    ys, xs = np.mgrid[0:h, 0:w]
    return on[(ys // th) * tiles_x + xs // tw]


def pixel_error(w, h, film, half):
    """-> (e (h, w) f32 with +0 where the pixel has no estimate, has (h, w) bool)."""
    n = w * h
    film, half = np.asarray(film, dtype=f32), np.asarray(half, dtype=f32)
    c, hf = film[:3 * n].reshape(n, 3), half[:3 * n].reshape(n, 3)
    wc, wa = film[6 * n:], half[6 * n:]
    with np.errstate(all="ignore"):
        wb = wc - wa
        ca = hf / wa[:, None]
        cb = (c - hf) / wb[:, None]
        d = (np.abs(ca[:, 0] - cb[:, 0]) + np.abs(ca[:, 1] - cb[:, 1])) + np.abs(ca[:, 2] - cb[:, 2])
        f = np.sqrt((wa * wb) / (wc * wc))
        m = c / wc[:, None]
        l = (m[:, 0] + m[:, 1]) + m[:, 2]
        e = (d * f) / np.sqrt(l + f32(0.01))
    assert e.dtype == f32
    has = (wa > 0) & (wb > 0) & np.isfinite(e)
    return np.where(has, e, f32(0)).reshape(h, w), has.reshape(h, w)


def tile_error(w, h, film, half, tw, th, tiles) -> np.ndarray:
    """akr_film_tile_error: per listed tile the fixed tree's sum of the pixels' estimates over their count, +inf without one."""
    e, has = pixel_error(w, h, film, half)
    tiles_x, _ = grid(w, h, tw, th)
    P = 1
    while P < tw * th:
        P *= 2
    out = np.zeros(len(tiles), dtype=f32)
    for j, t in enumerate(np.asarray(tiles, dtype=np.int64)):
        ty, tx = divmod(int(t), tiles_x)
        s = np.zeros(P, dtype=f32)
        leaves = np.zeros((th, tw), dtype=f32)
        y1, x1 = min(h, (ty + 1) * th), min(w, (tx + 1) * tw)
        leaves[:y1 - ty * th, :x1 - tx * tw] = e[ty * th:y1, tx * tw:x1]
        s[:tw * th] = leaves.reshape(-1)
        n_est = int(np.count_nonzero(has[ty * th:y1, tx * tw:x1]))
        stride = P // 2
        while stride >= 1:
            s[:stride] = s[:stride] + s[stride:2 * stride]
            stride //= 2
        with np.errstate(all="ignore"):
            out[j] = s[0] / f32(n_est) if n_est > 0 else INF
    return out


def half_bracket(w, h, film, half, tw, th, tiles, close: bool) -> np.ndarray:
    """k_half_open (half - film) / k_half_close (half + film) on the rgb and weight planes of the listed tiles' pixels -> the new half film."""
    n = w * h
    film = np.asarray(film, dtype=f32)
    out = np.array(half, dtype=f32, copy=True)
    m = tile_mask(w, h, tw, th, tiles).reshape(-1)
    m3 = np.repeat(m, 3)
    with np.errstate(all="ignore"):
        out[:3 * n][m3] = (out[:3 * n][m3] + film[:3 * n][m3]) if close else (out[:3 * n][m3] - film[:3 * n][m3])
        out[6 * n:][m] = (out[6 * n:][m] + film[6 * n:][m]) if close else (out[6 * n:][m] - film[6 * n:][m])
    return out


def round_ends(spp, spp_per_pass, round_passes):
    """Samples per pixel after each round of a render that runs to spp: rounds of round_passes passes, the last one possibly shorter."""
    rs, out = spp_per_pass * round_passes, []
    while not out or out[-1] < spp:
        out.append(min(spp, (out[-1] if out else 0) + rs))
    return out


def adaptive(prefix, w, h, tw, th, spp, spp_per_pass, round_passes, threshold, min_spp, tiles=None):
    """akr_pt_adaptive_render from the prefix films: prefix[k] = the uniform film after round k + 1 (round_ends). tiles: the session's own
    (None = all). -> (film, half, tile_spp (tiles_y, tiles_x) u32, samples drawn, rounds, errors per check [(tiles, err)])."""
    ends = round_ends(spp, spp_per_pass, round_passes)
    assert len(prefix) == len(ends) >= 2
    rs = spp_per_pass * round_passes
    n = w * h
    tiles_x, tiles_y = grid(w, h, tw, th)
    active = list(range(tiles_x * tiles_y)) if tiles is None else [int(t) for t in tiles]
    film, half = np.zeros(7 * n, dtype=f32), np.zeros(7 * n, dtype=f32)
    tile_spp = np.zeros(tiles_x * tiles_y, dtype=np.uint32)
    done, rounds, drawn, checks = 0, 0, 0, []
    threshold = f32(threshold)
    while active and done < spp:
        a_round = rounds % 2 == 0
        m = tile_mask(w, h, tw, th, active).reshape(-1)
        if a_round:
            half = half_bracket(w, h, film, half, tw, th, active, False)
        p = np.asarray(prefix[rounds], dtype=f32)
        film[:3 * n][np.repeat(m, 3)] = p[:3 * n][np.repeat(m, 3)]
        film[6 * n:][m] = p[6 * n:][m]
        if a_round:
            half = half_bracket(w, h, film, half, tw, th, active, True)
        now = ends[rounds]
        full = now - done == rs
        drawn += (now - done) * int(np.count_nonzero(m))
        done = now
        rounds += 1
        tile_spp[active] = done
        if a_round or not full or done >= spp or done < min_spp:
            continue
        err = tile_error(w, h, film, half, tw, th, active)
        checks.append((list(active), err))
        active = [t for t, e in zip(active, err) if not (np.isfinite(e) and e <= threshold)]
    return film, half, tile_spp.reshape(tiles_y, tiles_x), drawn, rounds, checks


# ------------------------------------------------------------------------------------------------ shared inputs
@functools.lru_cache(maxsize=None)
def random_films(w, h, tw, th, seed=0):
    """(film, half): a random film with integer weights and an A-half of it, with the cases the definition names: pixels with wA = 0, with
    wB = 0, with a NaN channel, and tile 1 without any estimate (all of its pixels have wA = 0)."""
    rng = np.random.default_rng(1000 * w + 10 * h + tw + seed)
    n = w * h
    wa = rng.integers(1, 9, size=n).astype(f32)
    wb = rng.integers(1, 9, size=n).astype(f32)
    mean = rng.uniform(0.0, 2.0, size=(n, 3))
    mean[rng.random(n) < 0.05] = 0.0  # black pixels: l = 0, the regulariser alone under the root
    a = (mean * rng.uniform(0.6, 1.4, size=(n, 3)) * wa[:, None]).astype(f32)
    b = (mean * rng.uniform(0.6, 1.4, size=(n, 3)) * wb[:, None]).astype(f32)
    pick = rng.random(n)
    wa[pick < 0.04] = 0
    a[pick < 0.04] = 0
    wb[(pick >= 0.04) & (pick < 0.08)] = 0
    b[(pick >= 0.04) & (pick < 0.08)] = 0
    a[(pick >= 0.08) & (pick < 0.10), 1] = np.nan
    m = tile_mask(w, h, tw, th, [1]).reshape(-1)
    wa[m] = 0
    a[m] = 0
    splat = rng.uniform(0, 1, size=3 * n).astype(f32)  # never read
    film = np.concatenate([(a + b).astype(f32).reshape(-1), splat, (wa + wb).astype(f32)])
    half = np.concatenate([a.reshape(-1), np.zeros(3 * n, dtype=f32), wa])
    film.setflags(write=False)
    half.setflags(write=False)
    return film, half


def all_tiles(w, h, tw, th):
    """Every tile of the grid, in an order that is not sorted."""
    tiles_x, tiles_y = grid(w, h, tw, th)
    t = np.arange(tiles_x * tiles_y, dtype=np.uint32)
    return np.concatenate([t[1::2], t[0::2]])


@functools.lru_cache(maxsize=None)
def reference_errors(w, h, tw, th):
    film, half = random_films(w, h, tw, th)
    out = tile_error(w, h, film, half, tw, th, all_tiles(w, h, tw, th))
    out.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------ oracle prefix films
CBOX = dict(w=64, h=64, tw=8, th=8, spp=32, spp_per_pass=2, round_passes=2, seed=3)


def index_states(w, h):
    """The initial per-pixel state of the index samplers (pmj02bn, sobol): sample index u32::MAX, the pixel's coordinates."""
    st = np.zeros(2 * w * h, dtype=np.uint64)
    st[0::2] = 0xFFFFFFFF
    st[1::2] = (np.arange(w * h, dtype=np.uint64) % np.uint64(w)) | ((np.arange(w * h, dtype=np.uint64) // np.uint64(w)) << np.uint64(32))
    return st


def oracle_prefix_films(root, w, h, spp, spp_per_pass, round_passes, seed=3, sampler=0, chunk=None, want_states=False, bvh=False):
    """The CPU oracle's film of scenes/cbox (max_depth 12, rr_depth 5) after every round of a render of `spp` samples: one render carried from
    round to round through its film and sampler states. chunk: the samples per step instead of a round's. -> [film] (, [states])."""
    import os

    from akari_render_amd import abi, capi
    from oracle import pyoracle, scene_json

    sd = scene_json.load_scene(os.path.join(root, "scenes", "cbox", "scene.json"), w, h)
    sd.ggx_table = np.fromfile(os.path.join(root, "tests", "golden", "ggx_dielectric_s.f32"), dtype=f32)
    if sampler == abi.SAMPLER_PMJ02BN:
        pyoracle.set_pmj_tables(*capi.host_pmj02bn_tables())
    sc = pyoracle.OracleScene(sd, bvh=bvh)
    cfg = abi.PtConfig.default()
    cfg.spp_per_pass, cfg.max_depth, cfg.rr_depth, cfg.sampler_seed, cfg.sampler_type = spp_per_pass, 12, 5, seed, sampler
    states = pyoracle.init_pcg32_states(w * h, seed) if sampler == 0 else index_states(w, h)
    film = np.zeros(7 * w * h, dtype=f32)
    ends = round_ends(spp, spp_per_pass, round_passes) if chunk is None else list(range(chunk, spp + 1, chunk))
    films, all_states, done = [], [], 0
    for e in ends:
        if sampler == 0:
            cfg.spp = e - done  # the independent sampler goes on from the pixel's stream
        else:
            cfg.spp, cfg.sample_begin, cfg.sample_count = spp, done, e - done  # the index samplers stratify for the whole render
        film, _ = sc.render(cfg, film=film, states=states)
        films.append(film.copy())
        all_states.append(states.copy())
        done = e
    return (films, all_states) if want_states else films


@functools.lru_cache(maxsize=None)
def cbox_prefix(root):
    films = oracle_prefix_films(root, CBOX["w"], CBOX["h"], CBOX["spp"], CBOX["spp_per_pass"], CBOX["round_passes"], CBOX["seed"])
    for f in films:
        f.setflags(write=False)
    return films
