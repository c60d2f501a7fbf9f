"""The grid behind akr_adaptive_config_default's threshold: scenes/cbox at 64 x 64 in 8 x 8 tiles, at most 128 spp in rounds of
one pass of 4 samples, min_spp 16 (independent sampler, seed 3). The adaptive render is a pure function of the CPU oracle's prefix films
(tests/adaptive_model.py: no GPU, no library); per threshold of a factor-of-two ladder: its relMSE against the oracle's 2048-spp image and the
samples it drew, next to the uniform oracle film with the largest spp whose samples do not exceed that.

    python tools/adaptive_grid.py [--markdown]
"""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import adaptive_model as am  # noqa: E402
from tests import denoise_model as dm  # noqa: E402

W = H = 64
TW = TH = 8
SPP, SPP_PER_PASS, ROUND_PASSES, MIN_SPP = 128, 4, 1, 16
THRESHOLDS = [2.0 ** -k for k in range(8, 0, -1)]  # 1/256 ... 1/2


@functools.lru_cache(maxsize=None)
def round_films(root):
    """The oracle's film after every round of the uniform render."""
    from oracle import pyoracle
    pyoracle.build()
    return am.oracle_prefix_films(root, W, H, SPP, SPP_PER_PASS, ROUND_PASSES, seed=3)


@functools.lru_cache(maxsize=None)
def uniform_film(root, spp):
    """The oracle's uniform film of `spp` samples: the first spp samples of the same render (a pixel's film is its samples in order, whatever the passes)."""
    ends = am.round_ends(SPP, SPP_PER_PASS, ROUND_PASSES)
    if spp in ends:
        return round_films(root)[ends.index(spp)]
    return am.oracle_prefix_films(root, W, H, spp, SPP_PER_PASS, ROUND_PASSES, seed=3, chunk=spp)[-1]


def grid(root, thresholds):
    """-> [(threshold, relMSE, samples drawn, spp of the uniform neighbour, its relMSE)]"""
    ref = dm.golden_cbox(root)[3]
    prefix = round_films(root)
    rows = []
    for t in thresholds:
        film, _, _, drawn, _, _ = am.adaptive(prefix, W, H, TW, TH, SPP, SPP_PER_PASS, ROUND_PASSES, t, MIN_SPP)
        u_spp = max(1, drawn // (W * H))
        rows.append((t, dm.rel_mse(dm.resolve_np(film, W, H), ref), drawn, u_spp, dm.rel_mse(dm.resolve_np(uniform_film(root, u_spp), W, H), ref)))
    return rows


def main():
    rows = grid(ROOT, THRESHOLDS)
    for t, rel, drawn, u_spp, u_rel in rows:
        print(f"threshold {t:<10.6g} relMSE {rel:.5f}  samples {drawn:>7} ({drawn / (W * H * SPP):.3f} of uniform {SPP} spp)  |  uniform {u_spp:>3} spp: relMSE {u_rel:.5f}  ratio {rel / u_rel:.3f}")
    best = min(rows, key=lambda r: r[1] / r[4])
    print(f"best ratio: threshold {best[0]:g}: {best[1] / best[4]:.3f}")
    if "--markdown" in sys.argv:
        print("| threshold | relMSE | samples drawn | of 128 spp | uniform neighbour | its relMSE | ratio |")
        print("|---|---|---|---|---|---|---|")
        for t, rel, drawn, u_spp, u_rel in rows:
            print(f"| 1/{round(1 / t)} | {rel:.5f} | {drawn} | {drawn / (W * H * SPP):.3f} | {u_spp} spp | {u_rel:.5f} | {rel / u_rel:.3f} |")


if __name__ == "__main__":
    main()
