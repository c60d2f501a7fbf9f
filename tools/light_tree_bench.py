"""What the light tree buys and costs: scenes/cbox at 1920 x 1080 with 256 point lights on a 16 x 16 grid under the ceiling, in mode 0 (every
light an entry of the light list, chosen by power) and in mode 1 (the tree). Per mode: ms per 8-spp pass (HIP events: the session's kernel_ms, 3 warm-up + 20
timed runs, median and range) and the relMSE of a 64-spp render against a 16 384-spp render of the MODE-0 scene -- the yardstick is the behaviour without the
tree. Reports the efficiency ratio (time x relMSE) of mode 0 over mode 1: above 1, the tree is worth having. The mean over pixels is what the ratio is defined with; the median pixel's relative squared error is printed beside it, because the mean of a
64-spp film is carried by its few brightest samples. One JSON line per result.

    python tools/light_tree_bench.py [--runs 20] [--size 1920x1080] [--ref-spp 16384] [--spp 64] [--grid 16]
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


def config(spp, per_pass, seed):
    cfg = abi.PtConfig.default()
    cfg.spp, cfg.spp_per_pass, cfg.max_depth, cfg.rr_depth, cfg.sampler_seed = spp, per_pass, 12, 5, seed
    return cfg


def render(ctx, scene, cfg, w, h):
    film = capi.Film(ctx, w, h)
    capi.pt_render(ctx, scene, cfg, film)
    return film.resolve().reshape(h, w, 3).astype(np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--ref-spp", type=int, default=16384)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--grid", type=int, default=16)
    a = ap.parse_args()
    w, h = (int(v) for v in a.size.split("x"))
    ctx = capi.Context(0)
    scene = capi.Scene(ctx, os.path.join(ROOT, "scenes", "cbox", "scene.json"), w, h)
    g = a.grid
    for j in range(g):  # under the ceiling of the box (x, z in [-1, 1], y up to 2), each as bright as the others
        for i in range(g):
            scene.add_punctual_light(type=abi.LIGHT_POINT, position=(-0.9 + 1.8 * i / (g - 1), 1.9, -0.9 + 1.8 * j / (g - 1)), color=(1.0, 1.0, 1.0), strength=2.0 / (g * g))
    scene.set_light_tree(False)
    ref = render(ctx, scene, config(a.ref_spp, 64, 1000), w, h)
    results = {}
    for mode in (0, 1):
        scene.set_light_tree(bool(mode))
        n_lights = scene.info().n_lights
        share = sum(scene.light(i)[2] for i in range(n_lights) if scene.light(i)[0] in (capi.PUNCTUAL_LIGHT_INSTANCE, capi.LIGHT_TREE_INSTANCE))
        film = capi.Film(ctx, w, h)
        times, flags = [], 0
        for i in range(3 + a.runs):
            film.clear()
            se = capi.PtSession(ctx, scene, config(8, 8, 3), film)
            se.passes(1, blocking=True)
            flags = se.kernel_info()["kernel_flags"]
            st = se.end()
            if i >= 3:
                times.append(st["kernel_ms"])
        img = render(ctx, scene, config(a.spp, 8, 7), w, h)
        rel = (img - ref) ** 2 / (ref ** 2 + 1e-4)
        rel_mse = float(np.mean(rel))
        results[mode] = {"ms": stat(times), "relMSE": rel_mse, "median": float(np.median(rel))}
        print(json.dumps({"what": "scenes/cbox with %d point lights under the ceiling" % (g * g), "frame": [w, h], "light_tree": mode, "light_list_entries": n_lights,
                          "selection_share_of_the_point_lights": share, "tree_nodes": scene.light_tree()[1], "kernel_flags": flags, "ms_per_8spp_pass": results[mode]["ms"],
                          "relMSE_at_%d_spp_against_%d_spp_of_mode_0" % (a.spp, a.ref_spp): rel_mse,
                          "median_relative_squared_error_of_a_pixel": results[mode]["median"]}), flush=True)
    t0, t1 = results[0]["ms"]["median"], results[1]["ms"]["median"]
    print(json.dumps({"what": "efficiency ratio (time x relMSE) of mode 0 over mode 1", "time_ratio_mode1_over_mode0": t1 / t0,
                      "relMSE_ratio_mode0_over_mode1": results[0]["relMSE"] / results[1]["relMSE"],
                      "efficiency_ratio": (t0 * results[0]["relMSE"]) / (t1 * results[1]["relMSE"]),
                      "the_same_with_the_median_pixel_in_place_of_the_mean": (t0 * results[0]["median"]) / (t1 * results[1]["median"])}), flush=True)


if __name__ == "__main__":
    main()
