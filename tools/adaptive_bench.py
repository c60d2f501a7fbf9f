"""Times adaptive sampling on the device, scenes/cbox at 1920 x 1080, HIP events, 3 warm-up + 20 timed runs (median and range):
the three kernels k_tile_error / k_half_open / k_half_close over all tiles against one round's pass time, and an adaptive render at the
default threshold against the uniform render of the same spp.

    python tools/adaptive_bench.py [--spp 128] [--spp-per-pass 8] [--runs 20]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from akari_render_amd import abi, capi  # noqa: E402


def stat(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", type=int, default=128)
    ap.add_argument("--spp-per-pass", type=int, default=8)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    a = ap.parse_args()
    w, h = a.width, a.height
    ctx = capi.Context(0)
    scene = capi.Scene(ctx, os.path.join(ROOT, "scenes", "cbox", "scene.json"), w, h)
    cfg = abi.PtConfig.default()
    cfg.spp, cfg.spp_per_pass, cfg.max_depth, cfg.rr_depth, cfg.sampler_seed = a.spp, a.spp_per_pass, 12, 5, 3
    acfg = abi.AdaptiveConfig.default()
    film, half = capi.Film(ctx, w, h), capi.Film(ctx, w, h)
    tiles = np.arange(((w + 31) // 32) * ((h + 31) // 32), dtype=np.uint32)
    # one adaptive render leaves a film and its half to time the kernels on
    capi.pt_adaptive_render(ctx, scene, cfg, film, acfg, half)
    times = {k: [] for k in ("tile_error", "half_open", "half_close")}
    for i in range(3 + a.runs):
        t = capi.adapt_times(ctx, film, half, 32, 32, tiles)
        if i >= 3:
            for k in times:
                times[k].append(t[k])
    print(json.dumps({"what": "kernels", "frame": [w, h], "tiles": int(tiles.size), **{k: stat(v) for k, v in times.items()}}))
    # one round (round_passes passes of spp_per_pass samples) of the uniform render
    rounds = []
    for i in range(3 + a.runs):
        f = capi.Film(ctx, w, h)
        se = capi.PtSession(ctx, scene, cfg, f)
        se.passes(acfg.round_passes, blocking=True)
        ms = se.end()["kernel_ms"]
        if i >= 3:
            rounds.append(ms)
    print(json.dumps({"what": "one round's passes", "samples_per_pixel": acfg.round_passes * a.spp_per_pass, "ms": stat(rounds)}))
    uni, ada, drawn = [], [], None
    for i in range(3 + a.runs):
        f = capi.Film(ctx, w, h)
        u = capi.pt_render(ctx, scene, cfg, f)
        f.clear()
        s, _ = capi.pt_adaptive_render(ctx, scene, cfg, f, acfg)
        if i >= 3:
            uni.append(u["kernel_ms"])
            ada.append(s["pt"]["kernel_ms"])
        drawn = (s["samples_drawn"], s["samples_uniform"], s["rounds"], s["tiles_retired"])
    print(json.dumps({"what": "render", "spp": a.spp, "spp_per_pass": a.spp_per_pass, "threshold": acfg.threshold, "min_spp": acfg.min_spp,
                      "uniform_kernel_ms": stat(uni), "adaptive_pass_kernel_ms": stat(ada), "samples_drawn": drawn[0], "samples_uniform": drawn[1],
                      "rounds": drawn[2], "tiles_retired": drawn[3]}))


if __name__ == "__main__":
    main()
