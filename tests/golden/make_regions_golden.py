"""Writes tests/golden/regions_vectors.npz: scipy.ndimage.label of a few small masks, both connectivities, and the cleaned masks
that scikit-image's two wrappers give when restated over it (scikit-image itself is not a dependency, so parity with it is not
pinned; the labelling it calls is).  tests/test_regions_host.py checks tests/regions_ref.py against this file.

    python tests/golden/make_regions_golden.py          (needs scipy; run on scipy 1.15.3)
"""
import os
import sys

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import regions_ref as R  # noqa: E402

STRUCT = {1: ndimage.generate_binary_structure(2, 1), 2: ndimage.generate_binary_structure(2, 2)}


def remove_small_objects(m, min_size, connectivity):
    """skimage.morphology.remove_small_objects for a boolean array, restated over scipy.ndimage.label."""
    out = m.copy()
    if min_size == 0:
        return out
    lab, _ = ndimage.label(m, STRUCT[connectivity])
    too_small = np.bincount(lab.ravel()) < min_size
    out[too_small[lab]] = False           # scikit-image clears label 0 as well when it is small: those pixels are False already
    return out


def remove_small_regions(m, min_object_size, hole_area_threshold, connectivity):
    m = remove_small_objects(m, min_object_size, connectivity)
    return ~remove_small_objects(~m, hole_area_threshold, connectivity)


def masks():
    rs = np.random.RandomState(0)
    out = {"rand64x80": rs.rand(64, 80) > 0.45}
    out["rand5x3"] = np.random.RandomState(1).rand(5, 3) > 0.5
    out["blobs70x90"] = R.blobs(1, 70, 90, seed=2, density=1 / 150.0)[0]
    out["checker6x7"] = (np.indices((6, 7)).sum(0) % 2).astype(bool)
    out["serpentine9x6"] = R.serpentine(9, 6)
    return out


def main():
    vec = {}
    for name, m in masks().items():
        vec[f"{name}.mask"] = np.packbits(m, axis=1)
        vec[f"{name}.shape"] = np.asarray(m.shape, np.int32)
        for conn in (1, 2):
            lab, n = ndimage.label(m, STRUCT[conn])
            vec[f"{name}.labels{conn}"] = lab.astype(np.int16)
            vec[f"{name}.count{conn}"] = np.int32(n)
            for mo, ho in ((30, 10), (4, 3)):
                vec[f"{name}.clean{conn}_{mo}_{ho}"] = np.packbits(remove_small_regions(m, mo, ho, conn), axis=1)
    m = masks()["rand64x80"]
    assert vec["rand64x80.count1"] == 286 and vec["rand64x80.count2"] == 14
    assert int((remove_small_regions(m, 30, 10, 1) != m).sum()) == 1256
    np.savez_compressed(os.path.join(HERE, "regions_vectors.npz"), **vec)


if __name__ == "__main__":
    main()
