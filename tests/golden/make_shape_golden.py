"""Writes tests/golden/shape_vectors.npz: a handful of small label images with the edge map, the perimeter tallies and the
box-relative second moments of ``regions.shape_labels``, by scipy.ndimage constructions that share nothing with tests/shape_ref.py:
the edge map of object l is ``(lab == l) & ~binary_erosion(lab == l, cross, border_value=0)``; the tallies are the ``bincount`` of
``convolve(edge map of l, [[10, 2, 10], [2, 1, 2], [10, 2, 10]], mode="constant")`` on its edge pixels (the construction of
scikit-image's ``perimeter`` with neighbourhood 4) summed over the codes of each class; Sxx, Syy, Sxy are ``sum_labels`` of the
squared coordinates relative to the corner of ``find_objects``' slice.  The host test holds the reference to these bytes; the GPU
test holds the kernels to them.

    python tests/golden/make_shape_golden.py
"""
import os
import sys

import numpy as np
from scipy import ndimage as ndi

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import regions_ref as R  # noqa: E402  (the inputs only)
import shape_ref as SR  # noqa: E402  (the inputs only: random_labels, disc)
import split_ref as S  # noqa: E402

CROSS = ndi.generate_binary_structure(2, 1)
WEIGHTS = np.array([[10, 2, 10], [2, 1, 2], [10, 2, 10]])
CLASSES = ((5, 7, 15, 17, 25, 27), (21, 33), (13, 23))


def cases():
    """name -> int32 [H, W] label image, at most 96 x 96"""
    sq = np.zeros((9, 11), np.int32)
    sq[2:7, 3:8] = 1
    yield "square5", sq
    yield "disc20", SR.disc(64, 64, (32, 32), 20).astype(np.int32)
    yield "blobs", R.label(R.blobs(1, 70, 90, seed=5, density=1 / 200.0)[0])[0].astype(np.int32)
    m, pts = S.two_discs()
    yield "split_discs", S.split(m, pts)["labels"][:, 30:126].astype(np.int32)        # two cells that touch along a seam
    yield "random", SR.random_labels(1, 70, 90, seed=11)[0]
    lab = SR.random_labels(1, 33, 65, seed=12, top=9)[0]
    lab[lab == 4] = 0                                                                  # a label without a pixel
    yield "gap", lab


def tables(lab):
    lab = np.maximum(lab, 0)
    cap = max(1, int(lab.max()))
    edges = np.zeros(lab.shape, bool)
    tallies, moments = np.zeros((cap, 4), np.int32), np.zeros((cap, 3), np.int64)
    rows, cols = np.mgrid[:lab.shape[0], :lab.shape[1]]
    for k, sl in enumerate(ndi.find_objects(lab, max_label=cap)):
        if sl is None:
            continue
        obj = lab == k + 1
        edge = obj & ~ndi.binary_erosion(obj, CROSS, border_value=0)
        edges |= edge
        hist = np.bincount(ndi.convolve(edge.astype(np.int64), WEIGHTS, mode="constant", cval=0)[edge], minlength=50)
        tallies[k] = [int(edge.sum())] + [int(hist[list(c)].sum()) for c in CLASSES]
        x, y = rows - sl[0].start, cols - sl[1].start
        moments[k] = [int(np.rint(ndi.sum_labels(v, lab, k + 1))) for v in (x * x, y * y, x * y)]
    return edges, tallies, moments


def main():
    out = {}
    for name, lab in cases():
        assert lab.dtype == np.int32 and max(lab.shape) <= 96
        edges, tallies, moments = tables(lab)
        out[f"{name}.labels"] = lab.astype(np.int8) if lab.min() >= -128 and lab.max() < 128 else lab
        out[f"{name}.edges"] = np.packbits(edges, axis=1)
        out[f"{name}.tallies"], out[f"{name}.moments"] = tallies, moments
    assert out["square5.tallies"].tolist() == [[16, 16, 0, 0]] and out["disc20.tallies"].tolist() == [[112, 32, 16, 64]]
    path = os.path.join(HERE, "shape_vectors.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
