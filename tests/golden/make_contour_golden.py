"""Writes tests/golden/contour_vectors.npz: a handful of small label images and, for both connectivities, what the ring of
``regions.contour_labels`` must enclose, by constructions that share nothing with the tracer of tests/contour_ref.py:

* ``<name>.filled<conn>`` uint8 [cap, H, W]: per label, ``scipy.ndimage.label`` of its pixels with the structure of the
  connectivity, the component that holds the label's first pixel in row-major order, and ``binary_fill_holes`` of that component
  with the COMPLEMENTARY structure (a hole of a 4-connected object is an 8-connected piece of background cut off from the
  outside, and the reverse).  All zero for a label without a pixel.
* ``<name>.cracks_all`` int32 [cap]: per label, the sides of its pixels across which the neighbour is not the label, counted by
  four shifted comparisons of the zero-padded mask.

The host test holds the restatement to these arrays: the winding-number fill of its ring equals ``filled``, and twice the filled
pixel count equals its shoelace sum.

    python tests/golden/make_contour_golden.py
"""
import os
import sys

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import regions_ref as R  # noqa: E402  (the inputs only)
import shape_ref as SR  # noqa: E402  (the inputs only: random_labels, disc)

CROSS = ndimage.generate_binary_structure(2, 1)
FULL = ndimage.generate_binary_structure(2, 2)


def cases():
    """name -> int32 [H, W] label image, at most 48 x 64"""
    yield "pinch", np.array([[1, 0, 2], [0, 1, 2], [1, 1, 0]], np.int32)
    frame = np.ones((3, 3), np.int32)
    frame[1, 1] = 0
    yield "frame3", frame
    sq = np.zeros((7, 7), np.int32)
    sq[1:6, 1:6] = 1
    yield "square5", sq
    ring = np.zeros((24, 26), np.int32)
    ring[SR.disc(24, 26, (12, 13), 10)] = 1
    ring[SR.disc(24, 26, (12, 13), 6)] = 0
    ring[11:14, 12:15] = 2                                                            # a dot inside the ring's hole
    yield "ring_dot", ring
    checker = (np.indices((6, 9)).sum(0) % 2).astype(np.int32)                        # one 8-connected piece, 27 4-connected ones
    yield "checker", checker
    yield "blobs", R.label(R.blobs(1, 40, 60, seed=5, density=1 / 150.0)[0])[0].astype(np.int32)
    yield "random", SR.random_labels(1, 40, 60, seed=11)[0]                            # scattered, disconnected labels, holes
    lab = SR.random_labels(1, 33, 64, seed=12, top=9)[0]
    lab[lab == 4] = 0                                                                  # a label without a pixel
    yield "gap", lab


def filled(obj, conn):
    """bool [H, W], one label -> the filled component of its first pixel"""
    if not obj.any():
        return np.zeros(obj.shape, bool)
    comp, _ = ndimage.label(obj, structure=CROSS if conn == 1 else FULL)
    first = comp.ravel()[np.flatnonzero(obj.ravel())[0]]
    return ndimage.binary_fill_holes(comp == first, structure=FULL if conn == 1 else CROSS)


def cracks(obj):
    p = np.pad(obj, 1)
    inner = p[1:-1, 1:-1]
    return int(sum((inner & ~s).sum() for s in (p[:-2, 1:-1], p[2:, 1:-1], p[1:-1, :-2], p[1:-1, 2:])))


def main():
    out = {}
    for name, lab in cases():
        assert lab.dtype == np.int32 and lab.shape[0] <= 48 and lab.shape[1] <= 64 and -128 <= lab.min() and lab.max() < 128
        cap = max(1, int(lab.max()))
        out[f"{name}.labels"] = lab.astype(np.int8)
        for conn in (1, 2):
            out[f"{name}.filled{conn}"] = np.stack([filled(lab == k + 1, conn) for k in range(cap)]).astype(np.uint8)
        out[f"{name}.cracks_all"] = np.asarray([cracks(lab == k + 1) for k in range(cap)], np.int32)
    assert out["pinch.cracks_all"].tolist() == [12, 6] and out["frame3.cracks_all"].tolist() == [16]
    assert out["frame3.filled1"].sum() == 9 and out["pinch.filled1"][0].sum() == 1 and out["pinch.filled2"][0].sum() == 4
    path = os.path.join(HERE, "contour_vectors.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
