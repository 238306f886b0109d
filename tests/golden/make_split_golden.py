"""Writes tests/golden/split_vectors.npz: small masks with seed points and what tests/split_ref.py (scipy.ndimage.label plus a
brute-force nearest-seed loop; scipy.ndimage sum / maximum / find_objects for the tables) makes of them.  The host test checks
the reference against these bytes, so a change of scipy's or of the reference's behaviour shows; the GPU test checks the kernels
against the same bytes.

    python tests/golden/make_split_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import regions_ref as R  # noqa: E402
import split_ref as S  # noqa: E402


def cases():
    """name -> (masks bool [N, H, W], points [P, 2], offsets [N + 1], limits [N] or None, connectivity)"""
    m, pts = S.two_discs()
    yield "tie", (m[None], pts, [0, 2], None, 1)
    yield "tie_swapped", (m[None], pts[::-1].copy(), [0, 2], None, 1)
    m, pts = S.foreign_seed()
    yield "foreign", (m[None], pts, [0, 2], None, 1)
    masks = R.blobs(4, 70, 90, seed=5, density=1 / 300.0)
    masks[1] = False                                                    # all background, with points
    pts, off = S.random_seeds(masks, 9, seed=6)
    pts, off = np.concatenate([pts[:off[2]], pts[off[3]:]]), np.concatenate([off[:3], off[3:] - 9])     # image 2: no points
    for conn in (1, 2):
        yield f"batch{conn}", (masks, pts, off, [9, 9, 9, 6], conn)


def main():
    out = {}
    for name, (masks, pts, off, lim, conn) in cases():
        ref = S.split(masks, pts, off, lim, conn)
        v = np.random.RandomState(len(name)).randint(0, 256, size=masks.shape).astype(np.uint8)
        t = S.tables(ref["labels"], v, counts=ref["counts"])
        out[f"{name}.shape"] = np.asarray(masks.shape, np.int32)
        out[f"{name}.mask"] = np.packbits(masks.reshape(-1, masks.shape[-1]), axis=1)
        out[f"{name}.points"], out[f"{name}.offsets"] = np.asarray(pts, np.int64), np.asarray(off, np.int64)
        out[f"{name}.limits"] = np.asarray([] if lim is None else lim, np.int32)
        out[f"{name}.connectivity"] = np.int32(conn)
        out[f"{name}.intensity"] = v
        out[f"{name}.labels"], out[f"{name}.counts"] = ref["labels"], ref["counts"]
        out[f"{name}.n_seeds"], out[f"{name}.live"] = ref["n_seeds"], ref["live"]
        for key in ("area", "bbox", "sum_rc", "intensity_sum", "intensity_max"):
            out[f"{name}.{key}"] = t[key]
    path = os.path.join(HERE, "split_vectors.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
