"""CPU: the numpy restatement of the distance-transform smoothing (tests/edt_ref.py) against squared distances made with
scipy.ndimage.distance_transform_edt (tests/golden/make_edt_golden.py) and against the definition on tiny maps; the integer rounding
rule on hand-made ties; and the argument errors of cellsegmentation_amd.detect / inference, which are raised before any device
work."""
import os
import re

import numpy as np
import pytest
import torch

import edt_ref as E
from cellsegmentation_amd import _lib, detect, inference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "edt_vectors.npz"), allow_pickle=False)
NAMES = sorted(k[:-len(".mask")] for k in GOLD.files if k.endswith(".mask"))


def golden_mask(name):
    """uint8 map whose foreground at the default threshold is the stored mask: 11 on foreground, 10 on background"""
    H, W = GOLD[f"{name}.shape"]
    fg = np.unpackbits(GOLD[f"{name}.mask"], axis=1)[:, :W].astype(bool)
    return np.where(fg, 11, 10).astype(np.uint8)


def test_golden_holds_the_pinned_maps():
    assert set(NAMES) == {"rand64x80_half", "rand64x80_sparse", "rand5x3", "blobs70x90", "checker9x8", "corner40x33", "bars48x61"}
    assert np.array_equal(golden_mask("rand64x80_half") > 10, np.random.RandomState(0).rand(64, 80) > 0.5)
    d2 = GOLD["corner40x33.d2"]
    assert d2.dtype == np.int32 and d2[39, 0] == 0 and d2[0, 32] == 39 * 39 + 32 * 32 and d2[39, 5] == 25
    assert (GOLD["checker9x8.d2"] == (np.indices((9, 8)).sum(0) % 2)).all()


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_scipy_vectors(name):
    got = E.edt_sq(golden_mask(name))
    assert got.dtype == np.int32 and np.array_equal(got, GOLD[f"{name}.d2"])


def test_restatement_equals_brute_force():
    rng = np.random.RandomState(5)
    for i in range(60):
        H, W = rng.randint(1, 13, size=2)
        m = E.random_mask(H, W, rng.choice([0.02, 0.2, 0.5, 0.9]), seed=100 + i)
        thr = int(rng.choice([10, 0, 100, 254]))
        assert np.array_equal(E.edt_sq(m, thr), E.edt_sq_brute(m, thr)), (i, H, W, thr)


def tie_map_up():
    """D2 takes the values 0, 1, 4 with M = 4: 255 sqrt(1/4) = 127.5 -> 128 (even)"""
    m = np.full((5, 5), 255, np.uint8)
    m[0, :] = m[-1, :] = 0
    m[:, 0] = m[:, -1] = 0
    return m


def tie_map_down():
    """a 67 x 67 foreground square in a background frame: M = 34^2 = 1156; D2 = 3^2 gives 255 * 3 / 34 = 22.5 -> 22 (even), D2 = 5^2
    gives 37.5 -> 38, D2 = 7^2 gives 52.5 -> 52"""
    m = np.zeros((69, 69), np.uint8)
    m[1:68, 1:68] = 200
    return m


def test_rounding_rule_on_ties():
    assert E.round_scaled(1, 4) == 128                      # 127.5 -> 128
    assert E.round_scaled(9, 1156) == 22                    # 22.5 -> 22
    assert E.round_scaled(25, 1156) == 38                   # 37.5 -> 38
    assert E.round_scaled(9, 4 * 1156) == 11 and E.round_scaled(49, 1156) == 52      # 11.25, 52.5 -> 52
    assert E.round_scaled(0, 7) == 0 and E.round_scaled(7, 7) == 255
    # against exact rational arithmetic for every D2 of a few maxima
    from fractions import Fraction
    for M in (1, 2, 3, 4, 50, 1156, 2 ** 31 - 2):
        for d2 in sorted(v for v in {0, 1, 2, 3, M // 4, M // 3, M // 2, M - 1, M} if 0 <= v <= M):
            k = E.round_scaled(d2, M)
            v2 = Fraction(255 * 255 * d2, M)                 # the square of the real value
            lo, hi = Fraction(2 * k - 1, 2), Fraction(2 * k + 1, 2)
            assert (k == 0 or lo * lo <= v2) and v2 <= hi * hi
            if v2 == hi * hi:
                assert k % 2 == 0
            if k > 0 and v2 == lo * lo:
                assert k % 2 == 0
    # the vectorised int64 form used for whole maps equals the scalar rule
    for M in (1, 4, 50, 1156, 2 ** 31 - 2):
        vals = np.unique(np.concatenate([np.arange(0, min(M, 1000) + 1), M - np.arange(0, min(M, 1000) + 1),
                                         np.random.RandomState(M % 1000).randint(0, M + 1, size=300)]))
        assert np.array_equal(E.normalise(vals), [E.round_scaled(v, M) for v in vals]), M
    up = E.smooth(tie_map_up())
    assert up[2, 2] == 255 and up[1, 1] == 128 and up[1, 2] == 128 and up[0, 0] == 0
    dn = E.edt_sq(tie_map_down())
    assert dn.max() == 1156 and dn[3, 34] == 9
    s = E.smooth(tie_map_down())
    assert s[34, 34] == 255 and s[3, 34] == 22 and s[5, 34] == 38 and s[7, 34] == 52


def test_no_background_and_no_foreground():
    full = np.full((6, 9), 200, np.uint8)
    assert (E.edt_sq(full) == -1).all() and (E.edt_sq_brute(full) == -1).all()
    assert E.smooth(full).dtype == np.uint8 and not E.smooth(full).any()
    empty = np.full((6, 9), 10, np.uint8)                   # exactly the threshold: background (strict >)
    assert not E.edt_sq(empty).any() and not E.smooth(empty).any()
    assert (E.edt_sq(empty, thr=9) == -1).all()
    assert not E.edt_sq(full, thr=255).any() and (E.edt_sq(np.zeros((3, 3), np.uint8), thr=-1) == -1).all()
    (pts, rest), kept = E.detect(np.full((64, 64), 200, np.uint8), with_kept=True)
    assert pts.shape == (0, 2) and rest == [] and kept == 0


def test_argument_errors_come_before_device_work():
    m = np.zeros((32, 32), np.uint8)
    for bad in ("gaussian", "distance", None, "DistanceTransform"):
        with pytest.raises(ValueError, match="Smoothing method not found. "):
            detect.detect_points(m, method=bad)
        with pytest.raises(ValueError, match="Smoothing method not found. "):
            inference.detect_cells([], None, None, method=bad)
    for fn in (detect.distance_transform_sq, detect.distance_smooth, lambda x: detect.detect_points(x, method="distancetransform")):
        for bad in (m.astype(np.float64), m.astype(np.float32), m.astype(np.int32), torch.zeros(4, 5, dtype=torch.int64)):
            with pytest.raises(TypeError):
                fn(bad)
        with pytest.raises(TypeError):
            fn([[1, 2], [3, 4]])
        for bad in (np.zeros(5, np.uint8), np.zeros((1, 2, 3, 4), np.uint8)):
            with pytest.raises(ValueError):
                fn(bad)
        # H^2 + W^2 >= 2^31: refused on the shape alone (46341^2 = 2^31 + 4633)
        for shape in ((46341, 1), (1, 46341), (2, 32768, 32768)):
            with pytest.raises(ValueError, match="2\\^31"):
                fn(np.broadcast_to(np.zeros((1, 1), np.uint8), shape))
        with pytest.raises(ValueError, match="2\\^31"):
            fn(torch.zeros((1, 1), dtype=torch.uint8).expand(46341, 1))
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError):
            detect.distance_smooth(m, thr_for_dt=bad)
    # the blur's arguments are not consulted by the distance form, and still checked by the default form
    with pytest.raises(ValueError):
        detect.detect_points(m, ksize=(4, 4))
    assert detect._dt_threshold(10) == 10 and detect._dt_threshold(10.7) == 10 and detect._dt_threshold(-5) == -1
    assert detect._dt_threshold(1e9) == 255
    # meanshift_cluster is unchanged
    with pytest.raises(NotImplementedError):
        detect.meanshift_cluster(m, "distancetransform")


def test_library_refuses_bad_sizes_without_gpu():
    lib = _lib.load()
    assert lib.cs_detect_edt_workspace(1, 46341, 1, 0) == 0 and lib.cs_detect_edt_workspace(0, 4, 4, 1) == 0
    assert lib.cs_detect_edt_workspace(65536, 4, 4, 0) == 0
    assert lib.cs_detect_edt_workspace(3, 5, 7, 0) == 32 and lib.cs_detect_edt_workspace(3, 5, 7, 1) == 32 + 432
    assert lib.cs_detect_edt_workspace(1, 46340, 1, 0) == 16 and lib.cs_detect_edt_workspace(1, 32767, 32767, 0) == 16
    assert lib.cs_detect_edt_sq(None, 0, 1, 4, 4, 10, None, None, 0, None) == -1 and b"detect_edt_sq" in lib.cs_last_error()
    assert lib.cs_detect_edt_smooth(None, 0, 1, 4, 4, 10, None, None, 0, None) == -1 and b"detect_edt_smooth" in lib.cs_last_error()


def test_new_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "cellseg_hip.h")).read()
    lib = _lib.load()
    for name in ("cs_detect_edt_workspace", "cs_detect_edt_sq", "cs_detect_edt_smooth"):
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.exported_symbols() and hasattr(lib, name)
