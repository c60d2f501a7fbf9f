"""procedural.instanced_forest at 1080p lit by its sky-light quad against the same forest lit by an environment sky (procedural.sky_image:
gradient + 5-degree sun, importance-sampled), under both schedules of the pt integrator (megakernel / wavefront), kept as meshes + instances.
Prints one JSON line per (sky, schedule): Msamples/s of a timed pass after a warm-up pass, rays per sample, mean colour.
python tools/env_bench.py [n_instances tris_per_mesh spp]   (defaults 1000 100000 8)"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from akari_render_amd import abi, capi, procedural

n_inst = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
tris = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000
spp = int(sys.argv[3]) if len(sys.argv) > 3 else 8
W, H = 1920, 1080
ctx = capi.Context(0)
for sky_name, sky in (("quad", None), ("environment", {})):
    sd = procedural.instanced_forest(n_inst, tris, width=W, height=H, sky=sky)
    with capi.options(instancing=1):
        scene = capi.Scene(ctx, sd)
    info = scene.info()
    for schedule in ("megakernel", "wavefront"):
        with capi.options(wavefront=1 if schedule == "wavefront" else 0, sched_trial=0):
            film = capi.Film(ctx, W, H)
            cfg = abi.PtConfig.default(); cfg.spp = spp * 3; cfg.spp_per_pass = spp; cfg.max_depth = 12; cfg.rr_depth = 5
            se = capi.PtSession(ctx, scene, cfg, film)
            se.passes(1, blocking=True); s0 = se.stats()
            ta = time.perf_counter(); se.passes(2, blocking=True); tb = time.perf_counter()
            s1 = se.end()
        d = {k: s1[k] - s0[k] for k in s1 if k not in ("n_launches",)}
        img = film.resolve()
        print(json.dumps({"sky": sky_name, "schedule": schedule, "n_instances": n_inst, "tris_per_mesh": tris, "n_tris": info.n_triangles,
                          "n_lights": info.n_lights, "spp_timed": 2 * spp, "msamples_per_s": round(d["n_samples"] / (tb - ta) / 1e6, 2),
                          "closest_per_sample": round(d["n_closest"] / d["n_samples"], 3), "shadow_per_sample": round(d["n_shadow"] / d["n_samples"], 3),
                          "nodes_per_ray": round(d["n_node_visits"] / max(1, d["n_closest"] + d["n_shadow"]), 2),
                          "mean_rgb": [round(float(x), 5) for x in img.mean(axis=(0, 1))], "finite": bool(np.isfinite(img).all())}), flush=True)
        del se, film
    del scene
