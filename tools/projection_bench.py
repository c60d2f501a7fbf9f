"""What a camera projection costs: C2 (scenes/cbox at 1080p, force_diffuse, the bench's headline configuration) through the pinhole,
a perspective lens, an orthographic camera, an orthographic camera with a lens and a full-sphere panorama. A library without projections (the parent
of the change that brought them: tools/ of this tree run against that tree with --root) runs the first two legs, so the cost of the extra branch in
the LENS kernels can be read from two trees alternating on one machine. Msamples/s from the kernels' HIP-event time, one JSON line per leg.
    python tools/projection_bench.py [--root TREE] [--repeat N] [--quick] [--out FILE]"""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the tree whose akari_render_amd is measured")
ap.add_argument("--repeat", type=int, default=3)
ap.add_argument("--quick", action="store_true", help="a small frame (a smoke run of the tool, not a measurement)")
ap.add_argument("--label", default="")
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, args.root)
from akari_render_amd import abi, capi  # noqa: E402


def leg(ctx, scene, cfg, name):
    w, h = scene.info().width, scene.info().height
    film = capi.Film(ctx, w, h)
    se = capi.PtSession(ctx, scene, cfg, film)
    se.passes(2, blocking=True)  # warm-up
    a = se.stats()
    se.passes(1 << 20, blocking=True)
    b = se.stats()
    info = se.kernel_info()
    se.end()
    n, ms = b["n_samples"] - a["n_samples"], b["kernel_ms"] - a["kernel_ms"]
    return {"label": args.label, "leg": name, "msamples_per_s": n / ms * 1e-3, "samples": n, "kernel_flags": info["kernel_flags"], "device": ctx.device_info()["name"]}


def main():
    ctx = capi.Context(0)
    res = (256, 144) if args.quick else (1920, 1080)
    scene = capi.Scene(ctx, os.path.join(args.root, "scenes", "cbox", "scene.json"), *res)
    cfg = abi.PtConfig.default()
    cfg.spp, cfg.spp_per_pass, cfg.max_depth, cfg.rr_depth, cfg.force_diffuse = (48 if args.quick else 320), 16, 12, 5, 1
    lens = (0.05, 10.0)  # (the file's focal distance; the cbox is on the exhaustive path, which takes any lens and any film)
    legs = [("pinhole", None, None), ("lens", None, lens)]
    if hasattr(scene, "set_projection"):
        legs += [("orthographic", dict(projection="orthographic", ortho_scale=2.5), None), ("orthographic_lens", dict(projection="orthographic", ortho_scale=2.5), lens),
                 ("panorama", dict(projection="panorama"), None)]
    for _ in range(args.repeat):
        for name, proj, ln in legs:
            scene.set_lens(None)
            if hasattr(scene, "set_projection"):
                scene.set_projection(**proj) if proj else scene.set_projection(None)
            if ln:
                scene.set_lens(*ln)
            row = leg(ctx, scene, cfg, name)
            print(json.dumps(row), flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
