"""Writes tests/golden/morph_vectors.npz from scipy alone: what cellsegmentation_amd.morph is pinned to.

* masks: ``distance_transform_edt`` squared and rounded to integers, towards the nearest True and the nearest False pixel, and
  ``scipy.ndimage.binary_{dilation,erosion,opening,closing}`` with ``structure = (dx^2 + dy^2 <= r2)`` on the
  ``(2 floor(sqrt(r2)) + 1)^2`` grid for r2 in R2S and both border values.
* label images (``ndimage.label`` of blob maps): for an expansion by r2, the set of zero pixels whose nearest label pixel lies
  within r2, the label under each of them, and the mask of those whose equally near label pixels carry more than one label -- the
  only pixels where an implementation's tie rule shows, and the only ones a comparison may skip.  At most 3 % of the filled pixels
  of every vector (asserted).  The nearest label pixels are found by brute force here.

tests/test_morph_host.py checks tests/morph_ref.py against this file, tests/test_morph_gpu.py the kernels.

    python tests/golden/make_morph_golden.py          (needs scipy; run on scipy 1.15.3)
"""
import os
import sys

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import edt_ref as E  # noqa: E402

R2S = (0, 1, 2, 4, 5, 13, 25, 56)
OPS = ("dilation", "erosion", "opening", "closing")
AMBIGUOUS_CAP = 0.03
# name: (shape, seed, density, blob radius, expansion r2)
LABEL_CASES = {"lab64x80": ((64, 80), 1, 1 / 300.0, (2, 5), 9),
               "lab130x97a": ((130, 97), 2, 1 / 400.0, (2, 6), 25),
               "lab130x97b": ((130, 97), 3, 1 / 150.0, (2, 4), 64),
               "lab40x300": ((40, 300), 4, 1 / 200.0, (2, 5), 6)}


def disk(r2):
    k = 0
    while (k + 1) ** 2 <= r2:
        k += 1
    yy, xx = np.mgrid[-k:k + 1, -k:k + 1]
    return yy * yy + xx * xx <= r2


def masks():
    """name -> boolean mask"""
    out = {"blobs64x80": E.blob_mask(64, 80, seed=1) > 10,
           "blobs70x53": E.blob_mask(70, 53, seed=5, density=1 / 80.0, radius=(1, 4)) > 10,
           "noise40x61": E.random_mask(40, 61, 0.5, seed=6) > 10,
           "sparse33x47": E.random_mask(33, 47, 0.97, seed=7) > 10,
           "rand5x3": np.random.RandomState(2).rand(5, 3) > 0.4}
    return out


def d2_to(sites):
    """rounded square of scipy's distance to the nearest True pixel of ``sites``"""
    return np.rint(ndimage.distance_transform_edt(~sites) ** 2).astype(np.int32)


def expansion(labels, r2):
    """(filled bool, label int32 under the filled pixels, ambiguous bool) by brute force over the label pixels"""
    H, W = labels.shape
    sy, sx = np.nonzero(labels)
    sl = labels[sy, sx]
    filled = np.zeros((H, W), bool)
    under = np.zeros((H, W), np.int32)
    ambiguous = np.zeros((H, W), bool)
    for y in range(H):
        for x in range(W):
            if labels[y, x]:
                continue
            d = (sy - y) ** 2 + (sx - x) ** 2
            m = d.min()
            if m > r2:
                continue
            near = sl[d == m]
            filled[y, x] = True
            under[y, x] = near[0]
            ambiguous[y, x] = (near != near[0]).any()
    return filled, under, ambiguous


def main():
    vec = {}
    for name, m in masks().items():
        assert m.any() and not m.all()
        vec[f"mask/{name}.shape"] = np.asarray(m.shape, np.int32)
        vec[f"mask/{name}.mask"] = np.packbits(m, axis=1)
        vec[f"mask/{name}.d2_true"] = d2_to(m)
        vec[f"mask/{name}.d2_false"] = d2_to(~m)
        for r2 in R2S:
            for bv in (0, 1):
                for op in OPS:
                    res = getattr(ndimage, f"binary_{op}")(m, structure=disk(r2), iterations=1, border_value=bv)
                    vec[f"mask/{name}.{op}.{r2}.{bv}"] = np.packbits(res, axis=1)
    for name, ((H, W), seed, density, radius, r2) in LABEL_CASES.items():
        labels = ndimage.label(E.blob_mask(H, W, seed=seed, density=density, radius=radius) > 127)[0].astype(np.int32)
        filled, under, ambiguous = expansion(labels, r2)
        share = ambiguous.sum() / max(1, filled.sum())
        print(f"{name}: {labels.max()} labels, {filled.sum()} filled, {ambiguous.sum()} ambiguous ({100 * share:.2f} %)")
        assert filled.sum() > 0 and share <= AMBIGUOUS_CAP, (name, share)
        vec[f"labels/{name}.labels"] = labels
        vec[f"labels/{name}.r2"] = np.asarray(r2, np.int32)
        vec[f"labels/{name}.filled"] = np.packbits(filled, axis=1)
        vec[f"labels/{name}.under"] = under
        vec[f"labels/{name}.ambiguous"] = np.packbits(ambiguous, axis=1)
    np.savez_compressed(os.path.join(HERE, "morph_vectors.npz"), **vec)


if __name__ == "__main__":
    main()
