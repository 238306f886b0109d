"""Writes tests/golden/adjacency_vectors.npz: small label images and what tests/adjacency_ref.py (dense tables of sides and corners,
every rule in Python integers) makes of them at both connectivities -- the tables and the pair list of ``regions.adjacency_labels``.
The host test checks the reference against these bytes, so a change of the reference's behaviour shows; the GPU test checks the
kernels against the same bytes.

Before anything is written the numbers are held against two statements that share nothing with the reference (``pins``): a pair is
listed at connectivity 1 iff ``scipy.ndimage.binary_dilation(lab == a, cross) & (lab == b)`` is non-empty, at connectivity 2 with
the 3 x 3 structure; and ``contact + background + outside`` equals tests/contour_ref.py's ``cracks_all`` of the label.

    python tests/golden/make_adjacency_golden.py
"""
import os
import sys

import numpy as np
import scipy.ndimage as ndi

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import adjacency_ref as A  # noqa: E402
import contour_ref as C  # noqa: E402
import match_ref as M  # noqa: E402
import regions_ref as R  # noqa: E402
import split_ref as S  # noqa: E402


def cases():
    """name -> (labels int32 [N, H, W], cap or None)"""
    yield "hand", (A.stacked()[1], None)
    yield "blocks", (M.blocks(8, 12)[None], None)
    masks = R.blobs(3, 63, 65, seed=11, density=1 / 150.0)              # blobs as scipy.ndimage.label finds them, cut at seeds
    pts, off = S.random_seeds(masks, 14, seed=5)
    lab = S.split(masks, pts, off)["labels"]
    yield "blobs", (lab, None)
    yield "blobs_capped", (lab, 9)


def pins(labels, t):
    """the two independent statements, for the ids the table of capacity t["cap"] sees; raises AssertionError"""
    cap, conn = t["cap"], t["connectivity"]
    structure = ndi.generate_binary_structure(2, conn)
    listed = set(zip(*(col.tolist() for col in t["pairs"][:3])))
    for n, lab in enumerate(np.asarray(labels)):
        ids = np.where((lab >= 1) & (lab <= cap), lab, 0)
        for a in range(1, cap + 1):
            grown = ndi.binary_dilation(ids == a, structure)
            for b in range(a + 1, cap + 1):
                assert ((n, a, b) in listed) == bool((grown & (ids == b)).any()), (n, a, b)
            assert int(A.boundary(t)[n, a - 1]) == C.cracks_all(ids == a), (n, a)


def main():
    out = {}
    for name, (labels, cap) in cases():
        out[f"{name}.labels"] = labels
        for conn in (1, 2):
            t = A.adjacency(labels, cap, conn)
            pins(labels, t)
            out[f"{name}.cap"] = np.asarray([t["cap"]], np.int32)
            for key in A.TABLES:
                out[f"{name}.c{conn}.{key}"] = t[key]
            for key, col in zip(A.PAIRS, t["pairs"]):
                out[f"{name}.c{conn}.pair_{key}"] = col
    path = os.path.join(HERE, "adjacency_vectors.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
