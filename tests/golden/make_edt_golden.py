"""Writes tests/golden/edt_vectors.npz: exact squared Euclidean distances of a few small foreground masks to their nearest
background pixel, from scipy.ndimage.distance_transform_edt(fg, return_indices=True).  The squares are computed in integers from
the returned nearest-background indices, so no float is squared or rounded.  tests/test_edt_host.py checks tests/edt_ref.py against
this file, tests/test_edt_gpu.py the kernels.  (cv2.distanceTransform, which the reference calls, is not a dependency; its
float32 result is not pinned.)

    python tests/golden/make_edt_golden.py          (needs scipy; run on scipy 1.15.3)
"""
import os
import sys

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import edt_ref as E  # noqa: E402


def masks():
    """name -> boolean foreground"""
    out = {"rand64x80_half": np.random.RandomState(0).rand(64, 80) > 0.5,
           "rand64x80_sparse": np.random.RandomState(1).rand(64, 80) > 0.02,
           "rand5x3": np.random.RandomState(2).rand(5, 3) > 0.4,
           "blobs70x90": E.blob_mask(70, 90, seed=3) > 10,
           "checker9x8": (np.indices((9, 8)).sum(0) % 2).astype(bool)}
    corner = np.ones((40, 33), bool)
    corner[39, 0] = False
    out["corner40x33"] = corner
    bars = np.zeros((48, 61), bool)
    bars[:, 5:24] = True
    bars[:, 30:61] = True
    bars[20:23, :] = False
    out["bars48x61"] = bars
    return out


def main():
    vec = {}
    for name, fg in masks().items():
        H, W = fg.shape
        _, idx = ndimage.distance_transform_edt(fg, return_indices=True)
        yy, xx = np.mgrid[0:H, 0:W]
        d2 = (idx[0].astype(np.int64) - yy) ** 2 + (idx[1].astype(np.int64) - xx) ** 2
        assert (d2[~fg] == 0).all() and (d2[fg] > 0).all()
        vec[f"{name}.mask"] = np.packbits(fg, axis=1)
        vec[f"{name}.shape"] = np.asarray(fg.shape, np.int32)
        vec[f"{name}.d2"] = d2.astype(np.int32)
    assert int(vec["corner40x33.d2"].max()) == 39 * 39 + 32 * 32
    np.savez_compressed(os.path.join(HERE, "edt_vectors.npz"), **vec)


if __name__ == "__main__":
    main()
