"""Capture shower-shape golden vectors from the REFERENCE (run in the build container only).

Pins calculate_image_features and get_max_value_image_coordinates (train/utils.py:81-112) against the
reference's own functions on six float32 images per shape:
  0  all zeros (the reference's w / 2, h / 2 centre)
  1  one positive pixel, in the last row
  2  a positive image whose maximum occurs twice (the first occurrence is the peak)
  3  no value above zero, negative sums
  4  expm1(relu(normal)), dense hits
  5  expm1(relu(normal - 1)), sparse hits

Output: tests/golden/image_features.npz.   Usage:  python tests/golden/make_feature_goldens.py
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens as mg  # noqa: E402  (reference loader, by path)

SHAPES = [(1, 1), (2, 3), (7, 5), (44, 44), (56, 30), (56, 56)]


def images_for(h, w, rng):
    imgs = np.zeros((6, h, w), dtype=np.float32)
    imgs[1, h - 1, w // 2] = np.float32(3.25)
    dup = np.expm1(np.abs(rng.standard_normal((h, w)))).astype(np.float32)
    if h * w >= 2:
        a, b = sorted(rng.choice(h * w, size=2, replace=False))
        top = np.float32(dup.max() * np.float32(1.5))
        dup.reshape(-1)[a] = top
        dup.reshape(-1)[b] = top
    imgs[2] = dup
    neg = -np.abs(rng.standard_normal((h, w))).astype(np.float32)
    neg[rng.random((h, w)) < 0.25] = 0.0
    if h * w == 1:
        neg[...] = np.float32(-0.5)
    imgs[3] = neg
    imgs[4] = np.expm1(np.maximum(rng.standard_normal((h, w)), 0.0)).astype(np.float32)
    imgs[5] = np.expm1(np.maximum(rng.standard_normal((h, w)) - 1.0, 0.0)).astype(np.float32)
    return imgs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    for stub in ("seaborn", "wandb"):
        sys.modules.setdefault(stub, types.ModuleType(stub))
    if args.ref not in sys.path:
        sys.path.insert(0, args.ref)
    U = mg._load_path("_ref_utils", os.path.join(args.ref, "expertsim", "train", "utils.py"))
    rng = np.random.default_rng(81112)
    out = {}
    for h, w in SHAPES:
        imgs = images_for(h, w, rng)
        feat = np.asarray(U.calculate_image_features(imgs), dtype=np.float64)
        peak = np.array([U.get_max_value_image_coordinates(im) for im in imgs], dtype=np.int32)
        assert feat.shape == (5, 6) and peak.shape == (6, 2)
        out[f"{h}x{w}/images"] = imgs
        out[f"{h}x{w}/features"] = feat
        out[f"{h}x{w}/peak"] = peak
    out["meta"] = np.array(json.dumps(dict(shapes=SHAPES, seed=81112, numpy=np.__version__)))
    path = os.path.join(HERE, "image_features.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path) / 1e3:.1f} kB")


if __name__ == "__main__":
    main()
