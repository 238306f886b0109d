"""Writes tests/golden/geodesic_vectors.npz: small masks with seed points and what tests/geodesic_ref.py (scipy.ndimage.label plus
a heap Dijkstra on (distance, seed) keys) makes of them, in the layout of split_vectors.npz.  The host test checks the reference
against these bytes, so a change of scipy's or of the reference's behaviour shows; the GPU test checks the kernels against the same
bytes.

    python tests/golden/make_geodesic_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import geodesic_ref as G  # noqa: E402
import split_ref as S  # noqa: E402

KEYS = ("labels", "counts", "n_seeds", "live", "distance")


def cases():
    """name -> (masks bool [N, H, W], points [P, 2], offsets [N + 1], limits [N] or None, connectivity)"""
    m, pts = G.horseshoe()
    yield "horseshoe", (m[None], pts, [0, 2], None, 1)
    m, pts = G.serpentine()
    yield "serpentine", (m[None], pts, [0, 1], None, 1)
    m, pts = G.two_discs()
    yield "tie", (m[None], pts, [0, 2], None, 1)
    masks = G.noise_masks(1, 70, 90, seed=3, density=0.8)
    pts, off = S.random_seeds(masks, 14, seed=4)
    yield "noise_70x90", (masks, pts, off, None, 2)
    masks = G.noise_masks(3, 130, 67, seed=5, density=0.8)
    masks[1, :40] = False
    pts, off = S.random_seeds(masks, 14, seed=6)
    pts, off = pts[:off[3] - 5], np.asarray([0, 14, 14, 37], np.int64)      # ragged: 14, none, 23 of which the limit keeps 9
    for conn in (1, 2):
        yield f"batch{conn}", (masks, pts, off, [14, 3, 9], conn)


def build():
    out = {}
    for name, (masks, pts, off, lim, conn) in cases():
        ref = G.split(masks, pts, off, lim, conn)
        out[f"{name}.shape"] = np.asarray(masks.shape, np.int32)
        out[f"{name}.mask"] = np.packbits(masks.reshape(-1, masks.shape[-1]), axis=1)
        out[f"{name}.points"], out[f"{name}.offsets"] = np.asarray(pts, np.int64), np.asarray(off, np.int64)
        out[f"{name}.limits"] = np.asarray([] if lim is None else lim, np.int32)
        out[f"{name}.connectivity"] = np.int32(conn)
        for key in KEYS:
            out[f"{name}.{key}"] = ref[key]
    return out


def main():
    path = os.path.join(HERE, "geodesic_vectors.npz")
    np.savez_compressed(path, **build())
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
