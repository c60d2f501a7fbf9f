"""Times what a punctual light costs the pt megakernel: scenes/cbox at 1920 x 1080 with its emitter alone, with one point light added,
with 64 of them, and with the one light given a radius (soft shadows), one 8-spp pass each, HIP events (the session's kernel_ms), 3 warm-up + 20 timed
runs, median and range.

    python tools/punctual_bench.py [--runs 20] [--size 1920x1080] [--legs 0,1,64,soft]
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
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--legs", default="0,1,64,soft", help="number of point lights per leg; soft = one light of radius 0.1")
    a = ap.parse_args()
    w, h = (int(v) for v in a.size.split("x"))
    ctx = capi.Context(0)
    scene = capi.Scene(ctx, os.path.join(ROOT, "scenes", "cbox", "scene.json"), w, h)
    cfg = abi.PtConfig.default()
    cfg.spp, cfg.spp_per_pass, cfg.max_depth, cfg.rr_depth, cfg.sampler_seed = 8, 8, 12, 5, 3
    film = capi.Film(ctx, w, h)
    rng = np.random.default_rng(1)
    for leg in a.legs.split(","):
        n_lights, radius = (1, 0.1) if leg == "soft" else (int(leg), 0.0)
        scene.clear_punctual_lights()
        for k in range(n_lights):  # inside the box, dim enough to leave the emitter most of the selection probability
            pos = (0.0, 1.0, 0.0) if k == 0 else tuple(float(v) for v in rng.uniform((-0.8, 0.2, -0.8), (0.8, 1.8, 0.8)))
            scene.add_punctual_light(type=abi.LIGHT_POINT, position=pos, color=(1.0, 1.0, 1.0), strength=0.5 / max(n_lights, 1), radius=radius)
        times, flags = [], 0
        for i in range(3 + a.runs):
            film.clear()
            se = capi.PtSession(ctx, scene, cfg, film)
            se.passes(1, blocking=True)
            flags = se.kernel_info()["kernel_flags"]
            st = se.end()
            if i >= 3:
                times.append(st["kernel_ms"])
        s = stat(times)
        print(json.dumps({"what": "one 8-spp pass of scenes/cbox", "frame": [w, h], "punctual_lights": n_lights, "radius": radius, "kernel_flags": flags, "ms": s,
                          "Msamples_per_s": w * h * 8 / (s["median"] * 1e-3) / 1e6}), flush=True)


if __name__ == "__main__":
    main()
