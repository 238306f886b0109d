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


def test_detect_options_defaults_are_those_of_detect_points():
    import dataclasses
    import inspect
    sig = inspect.signature(D.detect_points).parameters
    fields = [f for f in dataclasses.fields(D.DetectOptions) if f.init]
    assert [f.name for f in fields] == ["thr", "window_size", "interval", "eps", "ksize", "sigmaX", "sigmaY", "max_iter", "method",
                                        "thr_for_dt"]
    for f in fields:
        assert sig[f.name].default == f.default and type(sig[f.name].default) is type(f.default), f.name
    assert set(sig) - {f.name for f in fields} == {"masks_u8", "cell_counts", "_force_global"}
    opts = D.DetectOptions()
    with pytest.raises(dataclasses.FrozenInstanceError):
        opts.eps = 3
    assert all(np.array_equal(t, D.gaussian_taps(15, 3.)) for t in opts.taps) and opts.dt_thr is None
    dt = D.DetectOptions(method="distancetransform", thr_for_dt=12.7, ksize=(0, 0), sigmaX=-1.)     # ksize / sigma: not consulted
    assert dt.taps is None and dt.dt_thr == 12
    assert D.DetectOptions(sigmaY=2.).taps[1].tolist() == D.gaussian_taps(15, 2.).tolist()


_BAD_OPTIONS = [
    (dict(method="median"), ValueError, "Smoothing method not found. "),
    (dict(ksize=(0, 0)), ValueError, r"ksize \(0, 0\) \(size derived from sigma\) is not supported: pass odd kernel sizes"),
    (dict(ksize=15), ValueError, r"ksize must be a pair \(kx, ky\), got 15"),
    (dict(ksize=(14, 15)), ValueError, "ksize must be a positive odd integer, got 14"),
    (dict(ksize=(33, 15)), ValueError, "ksize 33 > 31 is not supported"),
    (dict(ksize=(5, 5), sigmaX=0.), ValueError, "cv2's fixed kernel tables"),
    (dict(eps=-1), ValueError, "eps must be finite and non-negative"),
    (dict(eps=float("inf")), ValueError, "eps must be finite and non-negative"),
    (dict(eps=float("nan")), ValueError, "eps must be finite and non-negative"),
    (dict(max_iter=-1), ValueError, "max_iter must be non-negative"),
    (dict(method="distancetransform", thr_for_dt=float("nan")), ValueError, "thr_for_dt must be finite, got nan"),
    (dict(method="distancetransform", thr_for_dt=float("inf")), ValueError, "thr_for_dt must be finite, got inf"),
    (dict(method="distancetransform", eps=-2), ValueError, "eps must be finite and non-negative"),
]


@pytest.mark.parametrize("kw,exc,msg", _BAD_OPTIONS)
def test_invalid_options_raise_alike_everywhere(kw, exc, msg):
    """the same type and message from the record, from detect_points (before the mask is looked at) and from a driver (before the
    model or the loader is touched)"""
    from cellsegmentation_amd import inference as I
    raised = []
    for call in (lambda: D.DetectOptions(**kw), lambda: D.detect_points(None, **kw), lambda: I.detect_cells([], None, None, **kw)):
        with pytest.raises(exc, match=msg) as e:
            call()
        raised.append((type(e.value), str(e.value)))
    assert raised[0] == raised[1] == raised[2]


def test_drivers_name_themselves_and_check_before_the_model():
    from cellsegmentation_amd import inference as I
    img = np.zeros((150, 170, 3), np.uint8)
    drivers = {"detect_cells": lambda **kw: I.detect_cells([], None, None, **kw),
               "detect_slide": lambda **kw: I.detect_slide(img, None, patch_size=64, **kw),
               "evaluate_detection": lambda **kw: I.evaluate_detection([], None, None, **kw),
               "evaluate_instances": lambda **kw: I.evaluate_instances([], None, None, **kw)}
    for name, call in drivers.items():
        with pytest.raises(TypeError, match=rf"^{name}: unexpected arguments \['bogus', 'sigma'\]$"):
            call(sigma=3., bogus=1)
        with pytest.raises(ValueError, match="Smoothing method not found. "):
            call(method="median")
        with pytest.raises(ValueError, match="pass odd kernel sizes"):
            call(ksize=(0, 0))
        with pytest.raises(ValueError, match="max_iter must be non-negative"):
            call(max_iter=-5)
    # detect_slide's ``interval`` is the patch grid's, never a blur keyword: the options are fine, the grid is refused
    with pytest.raises(ValueError, match="^interval must be positive, got 0$"):
        I.detect_slide(img, None, patch_size=64, interval=0)
    with pytest.raises(ValueError, match="square"):                         # ... and a good interval reaches the next check
        I.detect_slide(img, None, patch_size=(64, 48), interval=48)
    assert I._detect_options("detect_slide", 11, "gaussianblur", 10, thr=0.3).interval == 10      # the seed grid's stays 10
    assert I._detect_options("detect_cells", 11, "gaussianblur", 10, interval=7).interval == 7
