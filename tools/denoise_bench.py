"""What akr_denoise costs: at 1920 x 1080, HIP-event time of prepare, of every level (steps 1 .. 16) under both level kernels,
of finish and of the whole call, and the same under the schedule akr_denoise ships (row "auto": the library's choice of kernel per step)
-- warm-up calls first, then repeated calls, median / min / max reported -- next to the level's byte floor
(48 B read + 16 B written per pixel) and to the kernel time of one 16-spp C2 render (scenes/cbox, force_diffuse: bench.py's headline
configuration) of the same frame. One JSON line per kernel, appended to profiles/denoise_bench.jsonl.
--variance times akr_denoise_variance instead (rows "mode": "variance"): the frame is rendered in two passes of 8 spp, the film after the
first is the half film, and "prepare" is prepare + the variance prefilter.

    python tools/denoise_bench.py [--quick] [--variance] [--out FILE] [--runs N]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from akari_render_amd import abi, capi  # noqa: E402

HBM_BYTES_PER_S = 8.0e12  # MI355X peak


def spread(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="a small frame (a smoke run of the tool, not a measurement)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_bench.jsonl"))
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--variance", action="store_true", help="time akr_denoise_variance (half film = the frame after the first of two passes)")
    args = ap.parse_args()
    w, h = (256, 144) if args.quick else (1920, 1080)
    ctx = capi.Context(0)
    scene = capi.Scene(ctx, os.path.join(ROOT, "scenes", "cbox", "scene.json"), w, h)
    cfg = abi.PtConfig.default()
    cfg.spp, cfg.spp_per_pass, cfg.max_depth, cfg.rr_depth, cfg.force_diffuse = 16, 16, 12, 5, 1
    color, albedo, normal, out = (capi.Film(ctx, w, h) for _ in range(4))
    capi.pt_render(ctx, scene, cfg, color)  # warm-up of the render itself
    color.clear()
    frame_ms = capi.pt_render(ctx, scene, cfg, color)["kernel_ms"]
    half = None
    if args.variance:  # the same 16 spp in two passes of 8, the film after the first kept as the half
        color.clear()
        cfg.spp_per_pass = 8
        half = capi.Film(ctx, w, h)
        se = capi.PtSession(ctx, scene, cfg, color)
        se.passes(1, blocking=True)
        half.write(color.read())
        se.passes(1, blocking=True)
        frame_ms = se.end()["kernel_ms"]
    feature_ms = 0.0
    for film, aov in ((albedo, abi.AOV_ALBEDO), (normal, abi.AOV_NS)):
        ac = abi.AovConfig.default()
        ac.spp, ac.aov, ac.remap = 16, aov, 0
        feature_ms += capi.aov_render(ctx, scene, ac, film)["kernel_ms"]
    dc = abi.DenoiseConfig.default()
    floor_ms = 64.0 * w * h / HBM_BYTES_PER_S * 1e3
    results = []
    def times(kernel):
        if half is not None:
            return capi.denoise_variance_times(ctx, color, half, albedo, normal, out, kernel, dc)
        return capi.denoise_times(ctx, color, albedo, normal, out, kernel, dc)

    for kernel, name in ((0, "gather"), (1, "tiled"), (-1, "auto")):
        for _ in range(args.warmup):
            times(kernel)
        runs = [times(kernel) for _ in range(args.runs)]
        results.append(out.resolve())
        row = {"mode": "variance" if half is not None else "fixed", "kernel": name, "width": w, "height": h, "runs": args.runs, "warmup": args.warmup, "device": ctx.device_info()["name"],
               "prepare_ms": spread([r["prepare"] for r in runs]), "finish_ms": spread([r["finish"] for r in runs]),
               "total_ms": spread([r["total"] for r in runs]),
               "level_ms": {str(1 << i): spread([r["levels"][i] for r in runs]) for i in range(dc.iterations)},
               "level_byte_floor_ms": floor_ms, "c2_16spp_frame_kernel_ms": frame_ms, "feature_passes_16spp_kernel_ms": feature_ms}
        row["level_over_floor"] = {k: v["median"] / floor_ms for k, v in row["level_ms"].items()}
        row["total_over_frame"] = row["total_ms"]["median"] / frame_ms
        print(json.dumps(row))
        with open(args.out, "a") as f:
            f.write(json.dumps(row) + "\n")
    assert all(np.array_equal(results[0].view(np.uint32), r.view(np.uint32)) for r in results[1:]), "the level kernels disagree"


if __name__ == "__main__":
    main()
