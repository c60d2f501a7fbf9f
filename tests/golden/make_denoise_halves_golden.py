"""Regenerates tests/golden/cbox_64x64_halves.npz: what the variance-guided denoiser's quality test and the sigma_variance grid of
DESIGN.md 4.10 read.

    python tests/golden/make_denoise_halves_golden.py

Output of the CPU oracle on scenes/cbox at 64 x 64 (independent sampler, seed 3, max_depth 12, rr_depth 5): the pt film of 16 spp at
spp_per_pass 8 as it stands after pass 1 (`half`, 8 spp) and after pass 2 (`full`, 16 spp) -- one render of two passes, its film and
sampler states carried from the first to the second. The guides and the 2048-spp image are those of cbox_64x64_denoise.npz."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from akari_render_amd import abi  # noqa: E402
from oracle import pyoracle, scene_json  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    w = h = 64
    sd = scene_json.load_scene(os.path.join(ROOT, "scenes", "cbox", "scene.json"), w, h)
    sd.ggx_table = np.fromfile(os.path.join(HERE, "ggx_dielectric_s.f32"), dtype=np.float32)
    sc = pyoracle.OracleScene(sd)
    cfg = abi.PtConfig.default()
    cfg.spp, cfg.spp_per_pass, cfg.max_depth, cfg.rr_depth, cfg.sampler_seed = 8, 8, 12, 5, 3
    states = pyoracle.init_pcg32_states(w * h, cfg.sampler_seed)
    film, _ = sc.render(cfg, states=states)  # pass 1
    half = film.copy()
    full, _ = sc.render(cfg, film=film, states=states)  # pass 2: into the same film, the samplers where pass 1 left them
    cfg.spp = 16
    whole, _ = sc.render(cfg)
    assert np.array_equal(full.view(np.uint32), whole.view(np.uint32)), "the two passes are not the one-shot render"
    np.savez_compressed(os.path.join(HERE, "cbox_64x64_halves.npz"), half=half, full=full)


if __name__ == "__main__":
    main()
