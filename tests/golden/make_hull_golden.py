"""Writes tests/golden/hull_vectors.npz: a handful of small label images with the hull table of ``regions.hull_labels``, by a
construction that shares nothing with tests/hull_ref.py: ``scipy.spatial.ConvexHull`` (qhull) over ALL four corners of every pixel
of every object, not the row extremes.  ``area2`` is the shoelace sum over ``hull.vertices`` in int64; collinear vertices, should
qhull report any, are dropped before ``n_vertices`` is counted; ``feret_max2`` comes from all vertex pairs; the width is a
``fractions.Fraction`` minimised over the hull's edges, each against ALL points of the object.  The host test holds the reference
to these bytes; the GPU test holds the kernel to them.

    python tests/golden/make_hull_golden.py
"""
import os
import sys
from fractions import Fraction

import numpy as np
from scipy.spatial import ConvexHull

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import regions_ref as R  # noqa: E402  (the inputs only)
import shape_ref as SR  # noqa: E402  (the inputs only: random_labels, disc)
import split_ref as S  # noqa: E402

CLOSED_FORMS = {"pixel": (4, 2, 2, 1, 1), "square5": (4, 50, 50, 25, 25), "line7": (4, 14, 50, 7, 49),
                "diagonal6": (6, 22, 72, 10, 50), "disc20": (24, 2626, 1714, 247, 37)}


def cases():
    """name -> int32 [H, W] label image, at most 96 x 96"""
    sq = np.zeros((9, 11), np.int32)
    sq[2:7, 3:8] = 1
    yield "square5", sq
    yield "disc20", SR.disc(64, 64, (32, 32), 20).astype(np.int32)
    one = np.zeros((3, 4), np.int32)
    one[1, 2] = 1
    yield "pixel", one
    line = np.zeros((3, 9), np.int32)
    line[1, 1:8] = 1
    yield "line7", line
    diag = np.zeros((8, 8), np.int32)
    diag[np.arange(1, 7), np.arange(1, 7)] = 1
    yield "diagonal6", diag
    yield "blobs", R.label(R.blobs(1, 70, 90, seed=5, density=1 / 200.0)[0])[0].astype(np.int32)
    m, pts = S.two_discs()
    yield "split_discs", S.split(m, pts)["labels"][:, 30:126].astype(np.int32)        # two cells that touch along a seam
    yield "random", SR.random_labels(1, 70, 90, seed=11)[0]                            # scattered, disconnected labels
    lab = SR.random_labels(1, 33, 65, seed=12, top=9)[0]
    lab[lab == 4] = 0                                                                  # a label without a pixel
    yield "gap", lab


def row_of(obj):
    """bool [H, W], one object -> (n_vertices, area2, feret_max2, width_cross, width_len2)"""
    rr, cc = np.nonzero(obj)
    pts = np.unique(np.concatenate([np.stack([rr + dr, cc + dc], axis=1) for dr in (0, 1) for dc in (0, 1)]), axis=0).astype(np.int64)
    ring = pts[ConvexHull(pts).vertices]                                               # in order round the hull (2-D)
    n = len(ring)
    cross = lambda o, a, b: int((a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0]))  # noqa: E731
    ring = [ring[k] for k in range(n) if cross(ring[k - 1], ring[k], ring[(k + 1) % n]) != 0]
    n = len(ring)
    area2 = abs(sum(int(ring[k][0] * ring[(k + 1) % n][1] - ring[(k + 1) % n][0] * ring[k][1]) for k in range(n)))
    d = np.asarray(ring)[:, None, :] - np.asarray(ring)[None, :, :]
    far2 = int((d * d).sum(-1).max())
    best = None
    for k in range(n):
        a, b = ring[k], ring[(k + 1) % n]
        e = b - a
        c = int(np.abs(e[0] * (pts[:, 1] - a[1]) - e[1] * (pts[:, 0] - a[0])).max())
        len2 = int(e @ e)
        key = (Fraction(c * c, len2), len2, c)
        best = key if best is None else min(best, key)
    return n, area2, far2, best[2], best[1]


def table(lab):
    cap = max(1, int(lab.max()))
    out = np.zeros((cap, 5), np.int32)
    for k in range(cap):
        if (lab == k + 1).any():
            out[k] = row_of(lab == k + 1)
    return out


def main():
    out = {}
    for name, lab in cases():
        assert lab.dtype == np.int32 and max(lab.shape) <= 96
        out[f"{name}.labels"] = lab.astype(np.int8) if lab.min() >= -128 and lab.max() < 128 else lab
        out[f"{name}.hull"] = table(lab)
    for name, want in CLOSED_FORMS.items():
        assert out[f"{name}.hull"].tolist() == [list(want)], (name, out[f"{name}.hull"].tolist())
    path = os.path.join(HERE, "hull_vectors.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
