"""CPU: the numpy restatement of the small-region clean-up (tests/regions_ref.py) against vectors made with scipy.ndimage.label
(tests/golden/make_regions_golden.py), and the argument errors of cellsegmentation_amd.regions / stage.preprocess_masks, which
are raised before any device work."""
import os

import numpy as np
import pytest
import torch

import regions_ref as R
from cellsegmentation_amd import _lib, regions, stage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "regions_vectors.npz"), allow_pickle=False)
NAMES = sorted(k[:-len(".mask")] for k in GOLD.files if k.endswith(".mask"))


def _bits(name, key):
    H, W = GOLD[f"{name}.shape"]
    return np.unpackbits(GOLD[f"{name}.{key}"], axis=1)[:, :W].astype(bool)


def test_golden_holds_the_pinned_masks():
    assert set(NAMES) >= {"rand64x80", "rand5x3", "blobs70x90", "checker6x7", "serpentine9x6"}
    m = _bits("rand64x80", "mask")
    assert np.array_equal(m, np.random.RandomState(0).rand(64, 80) > 0.45)
    assert int(GOLD["rand64x80.count1"]) == 286 and int(GOLD["rand64x80.count2"]) == 14
    assert int((_bits("rand64x80", "clean1_30_10") != m).sum()) == 1256


@pytest.mark.parametrize("connectivity", [1, 2])
@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_scipy_vectors(name, connectivity):
    m = _bits(name, "mask")
    lab, n = R.label(m, connectivity)
    assert lab.dtype == np.int32 and n == int(GOLD[f"{name}.count{connectivity}"])
    assert np.array_equal(lab, GOLD[f"{name}.labels{connectivity}"].astype(np.int32))
    for mo, ho in ((30, 10), (4, 3)):
        assert np.array_equal(R.remove_small_regions(m, mo, ho, connectivity), _bits(name, f"clean{connectivity}_{mo}_{ho}"))


def test_restatement_wrappers():
    m = _bits("blobs70x90", "mask")
    assert np.array_equal(R.remove_small_objects(m, 0), m)
    assert np.array_equal(R.remove_small_holes(m, 7, 2), ~R.remove_small_objects(~m, 7, 2))
    areas = R.component_areas(m)
    lab, _ = R.label(m)
    assert np.array_equal(areas[m], np.bincount(lab.ravel())[lab[m]])
    assert int(areas[~m].max()) == int(np.bincount(R.label(~m)[0].ravel())[1:].max())
    # a background pocket at the border is a hole like any other
    p = np.ones((6, 6), bool)
    p[0, 0] = p[0, 1] = False
    assert R.remove_small_holes(p, 3).all() and not R.remove_small_holes(p, 2)[0, 0]
    s = R.serpentine(9, 6)
    assert R.label(s)[1] == 1 and int(s.sum()) == 5 * 6 + 4 and R.label(~s, 2)[1] == 4


def test_abi_version_is_10():
    assert _lib.load().cs_abi_version() == 10


def test_argument_errors_come_before_device_work():
    m = np.zeros((4, 5), bool)
    fns = (regions.label, regions.component_areas, regions.remove_small_objects, regions.remove_small_holes,
           lambda x, **kw: regions.remove_small_regions(x, 3, 2, **kw))
    for fn in fns:
        for bad in (m.astype(np.uint8), m.astype(np.int32), m.astype(np.float32), torch.zeros(4, 5, dtype=torch.int64)):
            with pytest.raises(TypeError):
                fn(bad)
        with pytest.raises(TypeError):
            fn([[True, False]])
        for bad in (np.zeros(5, bool), np.zeros((1, 2, 3, 4), bool), np.zeros((0, 5), bool)):
            with pytest.raises(ValueError):
                fn(bad)
        for conn in (0, 3, 1.5, None):
            with pytest.raises(ValueError):
                fn(m, connectivity=conn)
    for bad in (-1, 2.5, True):
        with pytest.raises(ValueError):
            regions.remove_small_objects(m, min_size=bad)
        with pytest.raises(ValueError):
            regions.remove_small_holes(m, area_threshold=bad)
        with pytest.raises(ValueError):
            regions.remove_small_regions(m, bad, 1)
        with pytest.raises(ValueError):
            regions.remove_small_regions(m, 1, bad)
    with pytest.raises(ValueError):
        regions.remove_small_regions(m, 1, 1, out=torch.zeros(4, 5, dtype=torch.bool))        # out must live on the device
    with pytest.raises(TypeError):
        regions.threshold(np.zeros((4, 5), np.float64), 0.5)
    img = np.zeros((4, 5, 3), np.uint8)
    with pytest.raises(TypeError):
        stage.preprocess_masks(img.astype(np.float32), m)
    with pytest.raises(TypeError):
        stage.preprocess_masks(img, m.astype(np.float32))
    with pytest.raises(ValueError):
        stage.preprocess_masks(img[:, :4], m)
    with pytest.raises(ValueError):
        stage.preprocess_masks(img, m, min_object_size=-1)


def test_defaults_follow_scikit_image():
    import inspect
    assert inspect.signature(regions.remove_small_objects).parameters["min_size"].default == 64
    assert inspect.signature(regions.remove_small_holes).parameters["area_threshold"].default == 64
    for fn in (regions.label, regions.remove_small_objects, regions.remove_small_holes, regions.remove_small_regions):
        assert inspect.signature(fn).parameters["connectivity"].default == 1
    sig = inspect.signature(stage.preprocess_masks).parameters
    assert sig["min_object_size"].default == 400 and sig["hole_area_threshold"].default == 120
