"""What a thin lens costs: C2 and C3 (scenes/cbox, the bench's two full-graph configurations) and the 1080p forest of 1000 x 100 k
triangles kept as meshes + instances, under both schedules, without a lens and with one focused mid-scene. Reports Msamples/s and closest / shadow
rays per sample, one JSON line per leg, appended to profiles/lens_bench.jsonl.   python tools/lens_bench.py [--quick] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from akari_render_amd import abi, capi, procedural  # noqa: E402


def leg(ctx, scene, cfg, warm_spp, name, lens, schedule, out):
    w, h = scene.info().width, scene.info().height
    film = capi.Film(ctx, w, h)
    with capi.options(wavefront=1 if schedule == "wavefront" else 0):
        se = capi.PtSession(ctx, scene, cfg, film)
        se.passes(max(1, warm_spp // cfg.spp_per_pass), blocking=True)
        a = se.stats()
        se.passes(1 << 20, blocking=True)
        b = se.stats()
        info = se.kernel_info()
        se.end()
    n = b["n_samples"] - a["n_samples"]
    ms = b["kernel_ms"] - a["kernel_ms"]
    row = {"scene": name, "schedule": schedule, "lens": lens, "msamples_per_s": n / ms * 1e-3, "closest_per_sample": (b["n_closest"] - a["n_closest"]) / n,
           "shadow_per_sample": (b["n_shadow"] - a["n_shadow"]) / n, "samples": n, "kernel_flags": info["kernel_flags"], "device": ctx.device_info()["name"]}
    print(json.dumps(row))
    with open(out, "a") as f:
        f.write(json.dumps(row) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small frames (a smoke run of the tool, not a measurement)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lens_bench.jsonl"))
    args = ap.parse_args()
    ctx = capi.Context(0)
    res = (256, 144) if args.quick else (1920, 1080)
    legs = []
    cbox = os.path.join(ROOT, "scenes", "cbox", "scene.json")
    for name, fd in (("C2", 1), ("C3", 0)):
        cfg = abi.PtConfig.default()
        cfg.spp, cfg.spp_per_pass, cfg.max_depth, cfg.rr_depth, cfg.force_diffuse = (32 if args.quick else 320), 16, 12, 5, fd
        # (the cbox is on the exhaustive path: no tree, so no wavefront leg)
        legs.append((name, lambda: capi.Scene(ctx, cbox, *res), cfg, ("megakernel",)))
    forest = procedural.instanced_forest(n_instances=1000, tris_per_mesh=100_000, width=res[0], height=res[1]) if not args.quick else \
        procedural.instanced_forest(n_instances=50, tris_per_mesh=2_000, width=res[0], height=res[1])
    cfg = abi.PtConfig.default()
    cfg.spp, cfg.spp_per_pass, cfg.max_depth, cfg.rr_depth = (8 if args.quick else 32), 8, 12, 5

    def kept():
        with capi.options(instancing=1):
            return capi.Scene(ctx, forest)
    legs.append(("forest_1000x100k_kept", kept, cfg, ("megakernel", "wavefront")))
    for name, make, cfg, schedules in legs:
        scene = make()
        lo, hi = scene_box(scene)
        c2w = scene.array(capi.ARRAY_C2W, np.float32)
        focus = float(np.linalg.norm(0.5 * (lo + hi) - c2w[12:15]))  # mid-scene
        for schedule in schedules:
            scene.set_lens(None)
            leg(ctx, scene, cfg, cfg.spp_per_pass, name, None, schedule, args.out)
            radius = largest_radius(scene, focus, want=0.02 * focus)
            if radius > 0.0:
                leg(ctx, scene, cfg, cfg.spp_per_pass, name, {"radius": radius, "focal_distance": focus}, schedule, args.out)
            else:
                print(json.dumps({"scene": name, "schedule": schedule, "lens": "refused: the camera is outside the padded coordinate range"}))


def scene_box(scene):
    inst = scene.array(capi.ARRAY_INSTANCES, np.float32).reshape(-1, 32)
    t = inst[:, 12:15]
    return t.min(0) - 1.0, t.max(0) + 1.0  # (instance origins: enough to find the middle of the scene)


def largest_radius(scene, focus, want):
    r = want
    for _ in range(12):
        try:
            scene.set_lens(r, focus)
            return r
        except capi.AkariError:
            r *= 0.5
    scene.set_lens(None)
    return 0.0


if __name__ == "__main__":
    main()
