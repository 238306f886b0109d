"""CPU: the Python-integer restatement of the per-label convex hull (tests/hull_ref.py) against the qhull vectors of
tests/golden/hull_vectors.npz and against closed forms (one pixel, the 5 x 5 square, lines, the diagonal, the radius-20 disc,
rectangles); the argument errors of regions.hull_labels / hull, which are raised before any device work; the two new entry points
in the header, the ctypes table and the library."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import hull_ref as HR
import shape_ref as SR
from cellsegmentation_amd import _lib, inference, kernels, regions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "hull_vectors.npz"), allow_pickle=False)
NAMES = sorted(k[:-len(".labels")] for k in GOLD.files if k.endswith(".labels"))
CLOSED_FORMS = {"pixel": (4, 2, 2, 1, 1), "square5": (4, 50, 50, 25, 25), "line7": (4, 14, 50, 7, 49),
                "diagonal6": (6, 22, 72, 10, 50), "disc20": (24, 2626, 1714, 247, 37)}


def _one_object(m):
    """bool [H, W] -> (the hull row of the one object, its float columns)"""
    t = HR.hull_labels(np.asarray(m).astype(np.int32))
    assert t["capacity"] == 1
    return tuple(t["hull"][0, 0].tolist()), {k: v[0, 0] for k, v in HR.columns(t).items()}


@pytest.mark.parametrize("name", NAMES)
def test_restatement_reproduces_the_qhull_vectors(name):
    lab = GOLD[f"{name}.labels"].astype(np.int32)
    t = HR.hull_labels(lab)
    assert max(lab.shape) <= 96 and t["capacity"] == max(1, int(lab.max()))
    assert t["hull"].dtype == np.int32 and np.array_equal(t["hull"][0], GOLD[f"{name}.hull"])
    empty = t["area"][0] == 0
    assert not t["hull"][0][empty].any() and (t["hull"][0][~empty, 0] >= 4).all()


def test_golden_covers_what_it_should():
    assert set(CLOSED_FORMS) | {"blobs", "split_discs", "random", "gap"} <= set(NAMES)
    for name, want in CLOSED_FORMS.items():
        assert GOLD[f"{name}.hull"].tolist() == [list(want)], name
    assert (GOLD["gap.hull"][3] == 0).all() and GOLD["gap.labels"].min() < 0       # a label without a pixel, labels below 0
    assert GOLD["split_discs.hull"].shape == (2, 5)                                 # two objects that touch
    lab = GOLD["random.labels"].astype(np.int32)                                    # disconnected labels, empty rows inside a box
    rows_with = np.unique(np.nonzero(lab == 1)[0])
    assert len(rows_with) < rows_with.max() - rows_with.min() + 1


def test_closed_forms():
    cases = dict(pixel=np.zeros((3, 4), bool), square5=np.zeros((9, 9), bool), line7=np.zeros((3, 9), bool),
                 diagonal6=np.zeros((8, 8), bool), disc20=SR.disc(64, 64, (32, 32), 20))
    cases["pixel"][1, 2] = True
    cases["square5"][2:7, 2:7] = True
    cases["line7"][1, 1:8] = True
    cases["diagonal6"][np.arange(1, 7), np.arange(1, 7)] = True
    for name, m in cases.items():
        row, c = _one_object(m)
        assert row == CLOSED_FORMS[name], name
        assert _one_object(m.T)[0] == row and _one_object(m[::-1])[0] == row, name   # the measures do not see a reflection
    row, c = _one_object(cases["pixel"])
    assert c["convex_area"] == 1.0 and c["solidity"] == 1.0 and c["feret_diameter_max"] == math.sqrt(2) and c["feret_diameter_min"] == 1.0
    row, c = _one_object(cases["diagonal6"])
    assert c["convex_area"] == 11.0 and c["solidity"] == pytest.approx(6 / 11) and c["feret_diameter_min"] == pytest.approx(math.sqrt(2))
    row, c = _one_object(cases["disc20"])
    assert c["feret_diameter_max"] == pytest.approx(math.sqrt(1714)) and 0.95 < c["solidity"] < 1.0 and c["n_vertices"] == 24.0


@pytest.mark.parametrize("a,b", [(1, 1), (1, 7), (4, 1), (2, 2), (5, 5), (6, 11), (13, 4)])
def test_filled_rectangles_have_solidity_one(a, b):
    m = np.zeros((a + 3, b + 5), bool)
    m[2:2 + a, 1:1 + b] = True
    row, c = _one_object(m)
    assert row == (4, 2 * a * b, a * a + b * b, a * b, max(a, b) ** 2)               # the width is taken across the longer side
    assert c["solidity"] == 1.0 and c["convex_area"] == a * b and c["feret_diameter_min"] == min(a, b)


def test_solidity_is_at_most_one_and_shapes_with_notches():
    for seed in (1, 2, 3):
        t = HR.hull_labels(SR.random_labels(2, 40, 70, seed=seed, top=6))
        s = HR.solidity(t)
        used = t["area"] > 0
        assert used.any() and (s[used] > 0).all() and (s[used] <= 1).all() and np.isnan(s[~used]).all()
        assert (HR.feret_diameter_min(t)[used] <= HR.feret_diameter_max(t)[used]).all()
    c_shape = np.zeros((9, 9), bool)
    c_shape[1:8, 1:8] = True
    c_shape[3:5, 3:8] = False                                                        # the notch's corners are no vertices
    row, c = _one_object(c_shape)
    assert row == (4, 98, 98, 49, 49) and c["solidity"] == (49 - 10) / 49
    ell = np.zeros((9, 9), bool)
    ell[1:8, 1:3] = True
    ell[6:8, 1:8] = True
    row, c = _one_object(ell)
    assert row[:2] == (5, 2 * 49 - 25) and c["solidity"] == 24 / 36.5
    # the hull is taken relative to the box: an object does not know where in the image it lies
    big = np.zeros((40, 50), np.int32)
    big[30:34, 41:48] = 1
    big[35, 44] = 1
    assert np.array_equal(HR.hull_labels(big)["hull"], HR.hull_labels(big[29:37, 40:49])["hull"])


def test_side_limit_in_the_restatement():
    for shape in ((1025, 3), (3, 1025)):
        lab = np.zeros(shape, np.int32)
        if shape[0] > 3:
            lab[:1024, 0] = 1                                                        # a line of exactly 1024 pixels: measured
        else:
            lab[0, :1024] = 1
        lab[-1, -1] = 2
        t = HR.hull_labels(lab)
        assert t["hull"][0].tolist() == [[4, 2048, 1024 ** 2 + 1, 1024, 1024 ** 2], [4, 2, 2, 1, 1]] and not HR.too_large(t).any()
        f = HR.hull_labels(np.ones(shape, np.int32))                                 # 1025 long: counted, not measured
        assert (f["hull"][0, 0] == -1).all() and HR.too_large(f)[0, 0] and f["area"][0, 0] == 3 * 1025
        assert all(np.isnan(v[0, 0]) for v in HR.columns(f).values())
    assert HR.MAX_SIDE == kernels.REGIONS_HULL_MAX_SIDE == 1024


def test_argument_errors_before_any_device_work():
    lab = np.zeros((4, 5), np.int32)
    for bad in (lab.astype(np.int64), lab.astype(np.uint8), lab.astype(np.float32), lab.astype(bool), [[0, 1]]):
        with pytest.raises(TypeError):
            regions.hull_labels(bad)
    for bad in (lab, lab.astype(np.uint8)):
        with pytest.raises(TypeError):
            regions.hull(bad)                                               # integer input is a label image: hull_labels
    with pytest.raises(TypeError):
        regions.hull_labels(lab, table={"bbox": None})
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError):
            regions.hull_labels(lab, max_regions=bad)
        with pytest.raises(ValueError):
            regions.hull(lab.astype(bool), max_regions=bad)
    with pytest.raises(ValueError):
        regions.hull(lab.astype(bool), connectivity=3)
    with pytest.raises(ValueError):
        regions.hull_labels(np.zeros((0, 5), np.int32))
    with pytest.raises(ValueError):
        regions.hull_labels(np.zeros((1, 2, 3, 4), np.int32))

    def table(n, cap, rows=None):
        return regions.RegionTable(torch.zeros(n, dtype=torch.int32), cap, torch.zeros((n, cap), dtype=torch.int32),
                                   torch.zeros((n, cap if rows is None else rows, 4), dtype=torch.int32),
                                   torch.zeros((n, cap, 2), dtype=torch.int64))
    with pytest.raises(ValueError, match="capacity"):
        regions.hull_labels(lab, table=table(1, 3), max_regions=4)
    batch = np.zeros((2, 4, 5), np.int32)
    for bad in (table(1, 3), table(3, 3), table(2, 3, rows=5)):
        with pytest.raises(ValueError, match="RegionTable"):
            regions.hull_labels(batch, table=bad)
    with pytest.raises(ValueError, match="RegionTable"):
        regions.hull_labels(lab, table=table(2, 3))
    assert inspect.signature(inference.measure_cells).parameters["hull"].default is False
    assert list(inspect.signature(regions.hull_labels).parameters) == list(inspect.signature(regions.shape_labels).parameters)
    assert list(inspect.signature(regions.hull).parameters) == ["m", "connectivity", "max_regions", "intensity"]


def test_entry_points_in_header_table_and_library():
    header = open(os.path.join(ROOT, "include", "cellseg_hip.h")).read()
    decl = re.search(r"\bint cs_regions_hull_labels\((.*?)\);", header, flags=re.S)
    assert decl is not None and len(decl.group(1).split(",")) == 8
    restype, argtypes = _lib._SIGNATURES["cs_regions_hull_labels"]
    assert restype is ctypes.c_int and len(argtypes) == 8 and argtypes[-1] is ctypes.c_void_p
    assert re.search(r"\bint cs_regions_hull_max_side\(void\);", header)
    assert _lib._SIGNATURES["cs_regions_hull_max_side"] == (ctypes.c_int, [])
    for name in ("cs_regions_hull_labels", "cs_regions_hull_max_side"):
        assert name in _lib.exported_symbols() and f" * {name}" in header       # described in the section's comment
    assert callable(kernels.regions_hull_labels) and kernels.REGIONS_HULL_MAX_SIDE == 1024


def test_library_refuses_bad_arguments():
    """argument checks of the library itself: refused with a message, nothing launched (only where the library is built)"""
    lib = _lib.load()
    assert lib.cs_regions_hull_max_side() == 1024 and lib.cs_abi_version() == 10
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    assert lib.cs_regions_hull_labels(p, 1, 4, 5, 0, p, p, None) == -1 and b"capacity" in lib.cs_last_error()
    assert lib.cs_regions_hull_labels(None, 1, 4, 5, 2, p, p, None) == -1 and b"NULL" in lib.cs_last_error()
    assert lib.cs_regions_hull_labels(p, 1, 4, 5, 2, None, p, None) == -1 and b"NULL table" in lib.cs_last_error()
    assert lib.cs_regions_hull_labels(p, 1, 4, 5, 2, p, None, None) == -1 and b"NULL table" in lib.cs_last_error()
    assert lib.cs_regions_hull_labels(p, 0, 4, 5, 2, p, p, None) == -1 and b"2^31" in lib.cs_last_error()
    assert lib.cs_regions_hull_labels(p, 1, 40000, 60000, 2, p, p, None) == -1 and b"2^31" in lib.cs_last_error()
    assert lib.cs_regions_hull_labels(p, 65535, 1, 1, 1 << 20, p, p, None) == -1 and b"N capacity" in lib.cs_last_error()
