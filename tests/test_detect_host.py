"""Cell localisation, host side: integer Gaussian taps, the numpy restatement (tests/detect_ref.py) against float64 and against
scikit-learn, the seed grid, and argument errors of cellsegmentation_amd.detect.  No GPU needed."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import detect_ref as R  # noqa: E402
from cellsegmentation_amd import detect as D  # noqa: E402
from cellsegmentation_amd import tiles  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "detect_vectors.npz")


@pytest.mark.parametrize("k,sigma", [(15, 3.0), (3, 0.5), (31, 5.0), (9, 0.0), (15, 0.0), (1, 2.0), (5, 100.0)])
def test_taps_sum_to_one_and_are_symmetric(k, sigma):
    t = D.gaussian_taps(k, sigma)
    assert t.dtype == np.int32 and len(t) == k
    assert int(t.astype(np.int64).sum()) == 1 << 14
    assert np.array_equal(t, t[::-1])
    assert (t >= 0).all()
    assert np.array_equal(t, R.taps(k, sigma))


def test_integer_blur_within_one_lsb_of_float64():
    rng = np.random.RandomState(0)
    img = rng.randint(0, 256, size=(299, 299)).astype(np.uint8)
    got = R.blur(img).astype(np.int64)
    ref = R.blur_f64(img)
    assert np.abs(got - ref).max() <= 1.0
    smooth = (np.add.outer(np.arange(64), np.arange(80)) * 2 % 256).astype(np.uint8)
    assert np.abs(R.blur(smooth, (7, 9), 1.5).astype(np.int64) - R.blur_f64(smooth, (7, 9), 1.5)).max() <= 1.0


def test_blur_of_constant_is_constant():
    img = np.full((40, 17), 201, np.uint8)
    assert (R.blur(img) == 201).all()


def _golden_sets():
    z = np.load(GOLDEN)
    o = z["offsets"]
    return [(z["points"][o[i]:o[i + 1]], float(z["eps"][i]), z["labels"][o[i]:o[i + 1]]) for i in range(len(o) - 1)]


def test_clustering_matches_the_fixture():
    for pts, eps, lab in _golden_sets():
        assert np.array_equal(R.dbscan_labels(pts, eps), lab), (pts[:6], eps)


def test_clustering_matches_sklearn():
    sk = pytest.importorskip("sklearn.cluster")
    rng = np.random.RandomState(5)
    cases = [(rng.randint(0, 300, size=(n, 2)), eps) for n, eps in ((50, 11.0), (400, 11.0), (800, 15.0), (300, 4.5), (200, 0.5))]
    cases += [(p, e) for p, e, _ in _golden_sets()]
    for pts, eps in cases:
        want = sk.DBSCAN(eps=eps, min_samples=1).fit_predict(pts.astype(np.float64))
        assert np.array_equal(R.dbscan_labels(pts, eps), want)


def test_clustering_scales_on_the_host():
    rng = np.random.RandomState(9)
    pts = rng.randint(0, 4096, size=(60000, 2))
    lab = R.dbscan_labels(pts, 11)
    assert lab.min() == 0 and len(np.unique(lab)) == lab.max() + 1


@pytest.mark.parametrize("hw", [(299, 299), (512, 512), (17, 40), (16, 16), (4096, 300)])
def test_seed_grid_matches_get_tiles(hw):
    ws, interval = 16, 10
    grid = tiles.get_tiles(hw, interval, ws)
    rows = sorted({r for r, _ in grid})
    cols = sorted({c for _, c in grid})
    assert rows[-1] == hw[0] - ws and cols[-1] == hw[1] - ws              # border-aligned last row and column
    full = np.full(hw, 255, np.uint8)
    assert R.seeds(full, 0.2, ws, interval) == grid
    from cellsegmentation_amd import kernels as K
    try:
        n = K.detect_grid_size(hw[0], hw[1], interval, ws)                # the library's count of the same grid
    except Exception:                                                     # library not built: host half only
        return
    assert n == len(grid)


def test_meanshift_restatement_fixed_point_and_zero_mass():
    img = np.zeros((64, 64), np.uint8)
    img[30:34, 40:44] = 200
    ends = R.meanshift(img, [(0, 0), (24, 30), (28, 36)], 16, 100)
    assert ends[0].tolist() == [8, 8]                                      # zero mass: the window stays
    assert ends[2].tolist() == [32, 42]                                    # moves onto the blob


def test_argument_errors():
    with pytest.raises(ValueError):
        D.gaussian_taps(14, 3.0)
    with pytest.raises(ValueError):
        D.gaussian_taps(5, 0.0)                                            # cv2's fixed tables
    with pytest.raises(ValueError):
        D._blur_taps((0, 0), 3.0)
    mask = np.zeros((64, 64), np.uint8)
    with pytest.raises(NotImplementedError, match="distancetransform"):
        D.meanshift_cluster(mask, "distancetransform", distanceType=2, maskSize=0)
    with pytest.raises(ValueError):
        D.meanshift_cluster(mask, "nosuchmethod")
    with pytest.raises(TypeError):
        D.meanshift_cluster(mask.astype(np.float32), "gaussianblur", ksize=(15, 15), sigmaX=3.)
    with pytest.raises(ValueError):
        D.meanshift_cluster(mask, "gaussianblur", ksize=(14, 15), sigmaX=3.)
    with pytest.raises(TypeError):
        D.detect_points(np.zeros((2, 64, 64), np.float64))
