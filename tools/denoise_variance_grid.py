"""The grid behind akr_denoise_config_default's sigma_variance: relMSE of the variance-guided filter on the oracle's 16-spp film
of scenes/cbox at 64 x 64 (tests/golden/cbox_64x64_halves.npz: the film after pass 1 of 2 is the half film) against the oracle's 2048-spp
image, over sigma_variance, computed with the numpy restatement (no GPU, no library) -- and, on the same film, the relMSE of akr_denoise
with its fixed default sigmas.

    python tools/denoise_variance_grid.py [--markdown]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import denoise_model as dm  # noqa: E402
from tests import denoise_variance_model as dvm  # noqa: E402

SIGMA_VARIANCE = [0.5, 1.0, 2.0, 4.0, 8.0]


def main():
    _, albedo, ns, ref = dm.golden_cbox(ROOT)
    half, full = dvm.golden_halves(ROOT)
    base = dm.rel_mse(dm.resolve_np(full, 64, 64), ref)
    print(f"noisy 16 spp (seed 3, 2 passes of 8): relMSE {base:.5f}")
    fixed = dm.rel_mse(dm.denoise_np(64, 64, full, albedo, ns, dm.config()), ref)
    print(f"akr_denoise, default sigmas: relMSE {fixed:.5f}  ratio {fixed / base:.3f}")
    rows = []
    for sv in SIGMA_VARIANCE:
        out = dvm.denoise_variance_np(64, 64, full, half, albedo, ns, dvm.config(sigma_variance=sv))
        rows.append((dm.rel_mse(out, ref), sv))
        print(f"sigma_variance {sv:<4} relMSE {rows[-1][0]:.5f}  ratio {rows[-1][0] / base:.3f}", flush=True)
    best = min(rows)
    print(f"best: sigma_variance {best[1]}: relMSE {best[0]:.5f} = {best[0] / base:.3f} x noisy")
    if "--markdown" in sys.argv:
        print("| | noisy | `akr_denoise`, default sigmas | " + " | ".join(f"`sigma_variance` {sv}" for _, sv in rows) + " |")
        print("|---|---|---|" + "---|" * len(rows))
        print(f"| relMSE | {base:.4f} | {fixed:.4f} | " + " | ".join(f"{r:.4f}" for r, _ in rows) + " |")
        print(f"| × noisy | 1 | {fixed / base:.3f} | " + " | ".join(f"{r / base:.3f}" for r, _ in rows) + " |")


if __name__ == "__main__":
    main()
