"""The grid behind akr_denoise_config_default's three sigmas: relMSE of the denoised 16-spp oracle film of scenes/cbox at
64 x 64 against the oracle's 2048-spp image, over a small grid, computed with the numpy restatement of the filter (no GPU, no library).

    python tools/denoise_sigma_grid.py [--markdown]
"""
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import denoise_model as dm  # noqa: E402

SIGMA_COLOR = [0.25, 0.5, 1.0, 2.0, 4.0]
SIGMA_NORMAL = [0.125, 0.25, 0.5, 1.0]
SIGMA_ALBEDO = [0.0625, 0.125, 0.25, 0.5]


def main():
    noisy, albedo, ns, ref = dm.golden_cbox(ROOT)
    base = dm.rel_mse(dm.resolve_np(noisy, 64, 64), ref)
    print(f"noisy 16 spp: relMSE {base:.5f}")
    rows = []
    for sc, sn, sa in itertools.product(SIGMA_COLOR, SIGMA_NORMAL, SIGMA_ALBEDO):
        out = dm.denoise_np(64, 64, noisy, albedo, ns, dm.config(sigma_color=sc, sigma_normal=sn, sigma_albedo=sa))
        rows.append((dm.rel_mse(out, ref), sc, sn, sa))
        print(f"sigma_color {sc:<5} sigma_normal {sn:<6} sigma_albedo {sa:<7} relMSE {rows[-1][0]:.5f}  ratio {rows[-1][0] / base:.3f}", flush=True)
    best = min(rows)
    print(f"best: sigma_color {best[1]} sigma_normal {best[2]} sigma_albedo {best[3]}: relMSE {best[0]:.5f} = {best[0] / base:.3f} x noisy")
    if "--markdown" in sys.argv:  # sigma_color down, (sigma_normal, sigma_albedo) across
        cols = list(itertools.product(SIGMA_NORMAL, SIGMA_ALBEDO))
        print("| sigma_color \\ (sigma_normal, sigma_albedo) | " + " | ".join(f"{n}, {a}" for n, a in cols) + " |")
        print("|---|" + "---|" * len(cols))
        for sc in SIGMA_COLOR:
            print(f"| {sc} | " + " | ".join(f"{next(r[0] for r in rows if r[1:] == (sc, n, a)):.4f}" for n, a in cols) + " |")


if __name__ == "__main__":
    main()
