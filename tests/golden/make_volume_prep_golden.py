#!/usr/bin/env python3
"""Writes tests/golden/volume_prep_pillow.npz: inputs and PILLOW's outputs (not the reference's, not this project's) for the size pairs of
tests/volume_prep_restate.py with S <= 128, so that the anchor of the restatement travels to machines without Pillow.

Per pair i: x_i uint8 [H0, W0] and bic_i uint8 [S, S] = one channel of `Image.fromarray(x).convert("RGB").resize((S, S))` (the three are
equal, checked here); m_i / near_i: a boolean mask and `Image.fromarray(m).resize((S, S))`, bit-packed; pairs int64 [n, 3] = (H0, W0, S).
The images are `sample_image` with its noise kept to the upper left quarter and 16 grey levels elsewhere, so that the file compresses to
well under 200 KB."""
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import volume_prep_restate as R  # noqa: E402


def golden_image(H0, W0, seed):
    noisy, calm = R.sample_image(H0, W0, seed), R.sample_image(H0, W0, seed, noise=0.0) // 16 * 16
    calm[: (H0 + 1) // 2, : (W0 + 1) // 2] = noisy[: (H0 + 1) // 2, : (W0 + 1) // 2]
    return calm


def main():
    import PIL
    pairs = [p for p in R.PAIRS if p[2] <= 128]
    out = {"pairs": np.array(pairs, dtype=np.int64), "pillow_version": np.array(PIL.__version__)}
    for i, (H0, W0, S) in enumerate(pairs):
        x = golden_image(H0, W0, 100 + i)
        rgb = np.array(Image.fromarray(x).convert("RGB").resize((S, S)))
        assert rgb.shape == (S, S, 3) and (rgb[..., 0] == rgb[..., 1]).all() and (rgb[..., 0] == rgb[..., 2]).all()
        m = x > 140
        near = np.array(Image.fromarray(m).resize((S, S)))
        assert near.dtype == bool and near.shape == (S, S)
        out[f"x_{i}"], out[f"bic_{i}"] = x, rgb[..., 0].copy()
        out[f"m_{i}"], out[f"near_{i}"] = np.packbits(m), np.packbits(near)
    path = os.path.join(HERE, "volume_prep_pillow.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, Pillow {PIL.__version__}")


if __name__ == "__main__":
    main()
