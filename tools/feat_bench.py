"""What collecting the denoiser's guides inside the pt pass costs and saves. At 1920 x 1080, on the full-graph cbox and on the
textured room (tests/helpers.py), rounds that alternate in one process:
  (a) the parent route: a pt render of 64 spp, then the two aov passes (albedo, ns) of 16 spp each -- what option "denoise" = 16 runs;
  (b) the features route: akr_pt_render_features of the same 64 spp.
FEAT kernels exist without DEFER and without SIMPLE (kernels.h pt_variant_compiled), so a third leg renders the plain session under options
simple_kernels = 0 and defer_metal = 0: the FEAT kernel's twin, which separates what the flag costs from what the exclusions cost.
Per route the wall time of the calls (session begin and film allocation included) and the kernel time of their launches (HIP events); for the pt
kernel alone its rate in Msamples/s with FEAT off (a) and on (b). Medians over the rounds; every round's numbers are kept. The guides of (b)
come from the 64 spp of the colour film's own rays, those of (a) from 16 spp of other rays: the routes are compared by cost, not by output.

    python tools/feat_bench.py [--quick] [--rounds N] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from akari_render_amd import abi, capi  # noqa: E402
from tests.helpers import textured_room  # noqa: E402


def median(v):
    return float(np.median(np.asarray(v, dtype=np.float64)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="a small frame (a smoke run of the tool, not a measurement)")
    ap.add_argument("--rounds", type=int, default=5, help="alternating rounds per scene (>= 3)")
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--aov-spp", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feat_bench.json"))
    args = ap.parse_args()
    assert args.rounds >= 3
    w, h = (256, 144) if args.quick else (1920, 1080)
    ctx = capi.Context(0)
    scenes = {"cbox_full_graph": lambda: capi.Scene(ctx, os.path.join(ROOT, "scenes", "cbox", "scene.json"), w, h),
              "textured_room": lambda: capi.Scene(ctx, textured_room(w, h))}
    cfg = abi.PtConfig.default()
    cfg.spp, cfg.spp_per_pass, cfg.max_depth, cfg.rr_depth, cfg.sampler_seed = args.spp, 16, 12, 5, 3
    result = {"width": w, "height": h, "spp": args.spp, "aov_spp": args.aov_spp, "rounds": args.rounds, "device": ctx.device_info()["name"], "scenes": {}}
    for name, make in scenes.items():
        scene = make()
        films = [capi.Film(ctx, w, h) for _ in range(3)]

        def clear():
            for f in films:
                f.clear()

        def route_a():
            clear()
            t0 = time.perf_counter()
            pt = capi.pt_render(ctx, scene, cfg, films[0])
            aov_ms = 0.0
            for film, aov in ((films[1], abi.AOV_ALBEDO), (films[2], abi.AOV_NS)):
                ac = abi.AovConfig.default()
                ac.spp, ac.aov, ac.remap, ac.sampler_seed = args.aov_spp, aov, 0, cfg.sampler_seed
                aov_ms += capi.aov_render(ctx, scene, ac, film)["kernel_ms"]
            wall = (time.perf_counter() - t0) * 1e3
            return {"wall_ms": wall, "pt_kernel_ms": pt["kernel_ms"], "aov_kernel_ms": aov_ms, "kernel_ms": pt["kernel_ms"] + aov_ms,
                    "pt_msamples_per_s": pt["n_samples"] / (pt["kernel_ms"] * 1e3)}

        def route_b():
            clear()
            t0 = time.perf_counter()
            pt = capi.pt_render_features(ctx, scene, cfg, *films)
            wall = (time.perf_counter() - t0) * 1e3
            return {"wall_ms": wall, "pt_kernel_ms": pt["kernel_ms"], "kernel_ms": pt["kernel_ms"], "pt_msamples_per_s": pt["n_samples"] / (pt["kernel_ms"] * 1e3)}

        def twin():  # the plain session on the kernel FEAT's is the twin of: no SIMPLE, no DEFER
            films[0].clear()
            with capi.options(simple_kernels=0, defer_metal=0):
                pt = capi.pt_render(ctx, scene, cfg, films[0])
            return {"pt_kernel_ms": pt["kernel_ms"], "pt_msamples_per_s": pt["n_samples"] / (pt["kernel_ms"] * 1e3)}

        def kernel_of(*guides):  # which kernel a session of this process runs right now (a cached per-scene kernel is taken by a plain session, never by a feature session)
            se = capi.PtSession(ctx, scene, cfg, films[0], *guides)
            ki = se.kernel_info()
            se.end()
            return {"specialised": ki["specialised"], "kernel_flags": ki["kernel_flags"], "status": ki["status"]}

        kernels = {"plain": kernel_of(), "features": kernel_of(films[1], films[2])}
        route_a()  # warm-up of the routes (first launches, the aov kernels)
        route_b()
        twin()
        a_runs, b_runs, t_runs = [], [], []
        for _ in range(args.rounds):
            a_runs.append(route_a())
            b_runs.append(route_b())
            t_runs.append(twin())
        row = {"kernels": kernels, "a_parent_route": {k: median([r[k] for r in a_runs]) for k in a_runs[0]}, "b_features_route": {k: median([r[k] for r in b_runs]) for k in b_runs[0]},
               "twin_no_simple_no_defer": {k: median([r[k] for r in t_runs]) for k in t_runs[0]}, "a_runs": a_runs, "b_runs": b_runs, "twin_runs": t_runs}
        a, b = row["a_parent_route"], row["b_features_route"]
        row["b_over_a_wall"] = b["wall_ms"] / a["wall_ms"]
        row["b_over_a_kernel"] = b["kernel_ms"] / a["kernel_ms"]
        row["pt_rate_feat_over_plain"] = b["pt_msamples_per_s"] / a["pt_msamples_per_s"]
        row["pt_rate_feat_over_twin"] = b["pt_msamples_per_s"] / row["twin_no_simple_no_defer"]["pt_msamples_per_s"]
        result["scenes"][name] = row
        print(f"{name}: (a) wall {a['wall_ms']:.1f} ms, kernels {a['kernel_ms']:.1f} ms (pt {a['pt_kernel_ms']:.1f} + aov {a['aov_kernel_ms']:.1f}); "
              f"(b) wall {b['wall_ms']:.1f} ms, kernels {b['kernel_ms']:.1f} ms; pt kernel {a['pt_msamples_per_s']:.0f} (plain{', per-scene kernel' if kernels['plain']['specialised'] else ''}) / {row['twin_no_simple_no_defer']['pt_msamples_per_s']:.0f} (twin: no SIMPLE, no DEFER) -> {b['pt_msamples_per_s']:.0f} Msamples/s with FEAT")
        scene.close()
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
