"""Writes tests/golden/props_vectors.npz: scipy.ndimage's per-label measurements of the masks of make_regions_golden.masks() with
a seeded uint8 intensity image each, both connectivities: label's count and, per label, center_of_mass, sum, mean, maximum and
the find_objects bounds.  tests/test_props_host.py checks tests/props_ref.py against this file, tests/test_props_gpu.py the
device tables.

    python tests/golden/make_props_golden.py          (needs scipy; run on scipy 1.15.3)
"""
import os
import sys

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_regions_golden import STRUCT, masks  # noqa: E402


def intensity(name, shape):
    seed = sum(name.encode()) + 1000
    return np.random.RandomState(seed).randint(0, 256, size=shape).astype(np.uint8)


def exact(values):
    """scipy's per-label sums (float64) and maxima (uint8) as int32, checked to be the same numbers"""
    a = np.asarray(values)
    out = a.astype(np.int32)
    assert np.array_equal(out, a)
    return out


def main():
    vec = {}
    for name, m in masks().items():
        v = intensity(name, m.shape)
        vec[f"{name}.intensity"] = v
        vec[f"{name}.counts"] = np.asarray([ndimage.label(m, STRUCT[conn])[1] for conn in (1, 2)], np.int32)
        for conn in (1, 2):
            lab, n = ndimage.label(m, STRUCT[conn])
            idx = np.arange(1, n + 1)
            com = np.asarray(ndimage.center_of_mass(m, lab, idx), np.float64).reshape(n, 2)
            mean = np.asarray(ndimage.mean(v, lab, idx), np.float64).reshape(n, 1)
            bounds = np.asarray([[s[0].start, s[1].start, s[0].stop, s[1].stop] for s in ndimage.find_objects(lab)], np.int32).reshape(n, 4)
            ints = [exact(ndimage.sum(m, lab, idx)), exact(ndimage.sum(v, lab, idx)), exact(ndimage.maximum(v, lab, idx))]
            # one array per number format keeps the archive small: (centre row, centre column, mean) and
            # (area, intensity sum, intensity maximum, r0, c0, r1, c1) per label; label's count is the number of rows (and `counts`)
            vec[f"{name}.f64_{conn}"] = np.concatenate([com, mean], axis=1)
            vec[f"{name}.i32_{conn}"] = np.concatenate([np.stack(ints, axis=1).reshape(n, 3), bounds], axis=1)
    assert len(vec["rand64x80.i32_1"]) == 286 and len(vec["rand64x80.i32_2"]) == 14
    np.savez_compressed(os.path.join(HERE, "props_vectors.npz"), **vec)


if __name__ == "__main__":
    main()
