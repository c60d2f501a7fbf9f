"""Times the display transform on the device, scenes/cbox films at 1920 x 1080 and 3840 x 2160, HIP events, 3 warm-up + 20 timed
runs (median and range) per kernel group -- the histogram, the bloom source, the downsamples, the blurs under both implementations, the
upsamples, the apply pass -- each beside the bytes it has to move, the rate that implies against the achievable HBM rate (6.3 TB/s), and the
time of one 8-spp pass of the uniform render of the same frame.

    python tools/display_bench.py [--runs 20] [--levels 5] [--sizes 1920x1080,3840x2160]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from akari_render_amd import abi, capi  # noqa: E402

HBM_ACHIEVABLE = 6.3e12  # bytes / s: a float4 copy on an MI355X


def stat(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def bytes_moved(w, h, levels):
    """What each kernel group has to read and write at least, from the shapes alone: a film pixel is 28 bytes, a level record 16."""
    n = [w * h]
    ww, hh = w, h
    for _ in range(levels):
        ww, hh = (ww + 1) // 2, (hh + 1) // 2
        n.append(ww * hh)
    return {
        "histogram": 28 * n[0],
        "source": 28 * n[0] + 16 * n[1],
        "down": sum(16 * n[l] + 16 * n[l + 1] for l in range(1, levels)),
        "blur_gather": sum(64 * n[l] for l in range(1, levels + 1)),  # two passes, each reads and writes the level
        "blur_lds": sum(32 * n[l] for l in range(1, levels + 1)),  # one read, one write (the halo rows read twice are not counted)
        "blur_level1_gather": 64 * n[1],
        "blur_level1_lds": 32 * n[1],
        "up": sum(32 * n[l] + 16 * n[l + 1] for l in range(1, levels)),
        "apply": 56 * n[0] + 16 * n[1],
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--levels", type=int, default=5)
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    a = ap.parse_args()
    ctx = capi.Context(0)
    for size in a.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        scene = capi.Scene(ctx, os.path.join(ROOT, "scenes", "cbox", "scene.json"), w, h)
        cfg = abi.PtConfig.default()
        cfg.spp, cfg.spp_per_pass, cfg.max_depth, cfg.rr_depth, cfg.sampler_seed = 8, 8, 12, 5, 3
        film, out = capi.Film(ctx, w, h), capi.Film(ctx, w, h)
        rounds = []
        for i in range(3 + a.runs):  # one 8-spp pass of the uniform render; the last one's film is what the transform is timed on
            film.clear()
            se = capi.PtSession(ctx, scene, cfg, film)
            se.passes(1, blocking=True)
            ms = se.end()["kernel_ms"]
            if i >= 3:
                rounds.append(ms)
        print(json.dumps({"what": "one 8-spp pass of the uniform render", "frame": [w, h], "ms": stat(rounds)}), flush=True)
        dc = abi.DisplayConfig.default()
        dc.auto_exposure, dc.bloom_strength, dc.bloom_levels = 1, 0.25, a.levels
        need = bytes_moved(w, h, a.levels)
        for kernel, blur in ((0, "gather"), (1, "lds")):
            times = {}
            for i in range(3 + a.runs):
                t = capi.display_times(ctx, film, out, kernel, dc)
                if i >= 3:
                    for k, v in t.items():
                        times.setdefault(k, []).append(v)
            row = {"what": "display transform", "frame": [w, h], "blur": blur, "levels": a.levels, "one_pass_ms": float(np.median(rounds))}
            for k, v in times.items():
                s = stat(v)
                key = {"blur": "blur_" + blur, "blur_level1": "blur_level1_" + blur}.get(k, k)
                if key in need:
                    s["bytes"] = need[key]
                    s["TB_per_s"] = need[key] / (s["median"] * 1e-3) / 1e12 if s["median"] > 0 else None
                    s["share_of_hbm"] = s["TB_per_s"] * 1e12 / HBM_ACHIEVABLE if s["TB_per_s"] else None
                row[k] = s
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
