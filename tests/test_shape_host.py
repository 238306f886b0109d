"""CPU: the numpy restatement of the shape descriptors (tests/shape_ref.py) against the scipy.ndimage vectors of
tests/golden/shape_vectors.npz and against closed forms (rectangles, the 5 x 5 square, the radius-20 disc, one- and two-pixel
objects, lines, the staircase); the argument errors of regions.shape_labels / shape / boundaries, which are raised before any device
work; the two new entry points in the header, the ctypes table and the library."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import shape_ref as SR
from cellsegmentation_amd import _lib, inference, kernels, regions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "shape_vectors.npz"), allow_pickle=False)
NAMES = sorted(k[:-len(".labels")] for k in GOLD.files if k.endswith(".labels"))


def _one_object(m):
    """bool [H, W] -> (tables of the one object, its float columns)"""
    t = SR.shape_labels(np.asarray(m).astype(np.int32))
    assert t["capacity"] == 1
    return t, {k: v[0, 0] for k, v in SR.columns(t).items()}


@pytest.mark.parametrize("name", NAMES)
def test_restatement_reproduces_the_scipy_vectors(name):
    lab = GOLD[f"{name}.labels"].astype(np.int32)
    t = SR.shape_labels(lab)
    assert max(lab.shape) <= 96 and t["capacity"] == max(1, int(lab.max()))
    assert np.array_equal(t["edges"], np.unpackbits(GOLD[f"{name}.edges"], axis=1)[:, :lab.shape[1]].astype(bool))
    assert t["tallies"].dtype == np.int32 and np.array_equal(t["tallies"][0], GOLD[f"{name}.tallies"])
    assert t["moments"].dtype == np.int64 and np.array_equal(t["moments"][0], GOLD[f"{name}.moments"])
    empty = t["area"][0] == 0
    assert not t["tallies"][0][empty].any() and not t["moments"][0][empty].any()


def test_golden_covers_what_it_should():
    assert {"square5", "disc20", "gap"} <= set(NAMES)
    assert GOLD["square5.tallies"].tolist() == [[16, 16, 0, 0]] and GOLD["disc20.tallies"].tolist() == [[112, 32, 16, 64]]
    assert (GOLD["gap.tallies"][3] == 0).all() and GOLD["gap.labels"].min() < 0    # a label without a pixel, labels below 0
    assert GOLD["split_discs.tallies"].shape == (2, 4)                              # two objects that touch


@pytest.mark.parametrize("a,b", [(1, 1), (1, 7), (4, 1), (2, 2), (5, 5), (6, 11), (13, 4)])
def test_filled_rectangle_closed_forms(a, b):
    m = np.zeros((a + 3, b + 5), bool)
    m[2:2 + a, 1:1 + b] = True
    t, c = _one_object(m)
    assert t["bbox"][0, 0].tolist() == [2, 1, 2 + a, 1 + b] and c["extent"] == 1.0
    want = [(a * a - 1) / 12, (b * b - 1) / 12, 0.0]
    assert np.allclose(c["central_moments"], want, rtol=1e-13, atol=1e-13)
    assert t["moments"][0, 0].tolist() == [b * sum(x * x for x in range(a)), a * sum(y * y for y in range(b)),
                                           sum(range(a)) * sum(range(b))]
    assert np.allclose(c["axis_lengths"], [4 * math.sqrt(max(want[:2])), 4 * math.sqrt(min(want[:2]))], rtol=1e-12, atol=1e-7)
    assert t["tallies"][0, 0, 0] == (a * b if min(a, b) <= 2 else 2 * (a + b) - 4)


def test_square_disc_and_tiny_objects():
    sq = np.zeros((9, 9), bool)
    sq[2:7, 2:7] = True
    t, c = _one_object(sq)
    assert t["tallies"][0, 0].tolist() == [16, 16, 0, 0] and c["perimeter"] == 16.0
    assert c["circularity"] == pytest.approx(4 * math.pi * 25 / 256) and c["eccentricity"] == 0.0 and c["orientation"] == 0.0
    assert c["equivalent_diameter"] == pytest.approx(math.sqrt(100 / math.pi))
    t, c = _one_object(SR.disc(64, 64, (32, 32), 20))
    assert t["tallies"][0, 0].tolist() == [112, 32, 16, 64]
    assert c["perimeter"] == pytest.approx(32 + 16 * math.sqrt(2) + 32 * (1 + math.sqrt(2)))
    assert c["eccentricity"] == pytest.approx(0.0, abs=1e-6) and 0.85 < c["circularity"] < 1.0
    one = np.zeros((3, 4), bool)
    one[1, 2] = True
    t, c = _one_object(one)
    assert t["tallies"][0, 0].tolist() == [1, 0, 0, 0] and not t["moments"].any()
    assert c["perimeter"] == 0.0 and c["axis_lengths"].tolist() == [0.0, 0.0] and c["eccentricity"] == 0.0
    assert c["circularity"] == math.inf and c["extent"] == 1.0
    two = one.copy()
    two[1, 3] = True
    t, c = _one_object(two)
    assert t["tallies"][0, 0].tolist() == [2, 0, 0, 0] and c["perimeter"] == 0.0
    assert c["axis_lengths"].tolist() == [4 * math.sqrt(0.25), 0.0] and c["eccentricity"] == 1.0


def test_lines_and_the_staircase():
    L = 9
    h = np.zeros((5, L + 4), bool)
    h[2, 2:2 + L] = True
    t, c = _one_object(h)
    assert t["tallies"][0, 0].tolist() == [L, L - 2, 0, 0] and c["perimeter"] == L - 2
    assert abs(c["orientation"]) == pytest.approx(math.pi / 2) and c["eccentricity"] == 1.0
    t, c = _one_object(h.T)
    assert t["tallies"][0, 0].tolist() == [L, L - 2, 0, 0] and c["orientation"] == 0.0
    stairs = np.zeros((8, 8), np.int32)
    for i in range(7):
        stairs[i, i] = stairs[i + 1, i] = 1                     # 4-connected, along the main diagonal
    stairs[7, 7] = 1
    for lab in (stairs, stairs[::-1].copy()):
        t = SR.shape_labels(lab)
        mu11, angle = SR.central_moments(t)[0, 0, 2], SR.orientation(t)[0, 0]
        assert mu11 != 0 and np.sign(angle) == np.sign(mu11) and abs(angle) == pytest.approx(math.pi / 4, abs=0.05)
    assert SR.central_moments(SR.shape_labels(stairs))[0, 0, 2] > 0 > SR.central_moments(SR.shape_labels(stairs[::-1].copy()))[0, 0, 2]


def test_edge_rule_between_objects_and_images():
    lab = np.asarray([[1, 1, 2, 2], [1, 1, 2, 2], [0, -3, 3, 3]], np.int32)
    assert SR.edges(lab).tolist() == [[True] * 4, [True] * 4, [False, False, True, True]]
    board = np.asarray([[1, 2], [3, 4]], np.int32)
    t = SR.shape_labels(board)
    assert t["edges"].all() and t["tallies"][0].tolist() == [[1, 0, 0, 0]] * 4   # a diagonal neighbour of another object is not counted
    both = np.zeros((2, 3, 3), np.int32)
    both[0, 2], both[1, 0] = 1, 1                                               # the same label in the last row and in the next image's first
    t = SR.shape_labels(both)
    assert t["tallies"][:, 0].tolist() == [[3, 1, 0, 0]] * 2 and t["edges"].sum() == 6
    # the moments are relative to the box: an object does not know where in the image it lies
    big = np.zeros((40, 50), np.int32)
    big[30:34, 41:48] = 1
    small = big[29:35, 40:49]
    assert np.array_equal(SR.shape_labels(big)["moments"], SR.shape_labels(small)["moments"])


def test_argument_errors_before_any_device_work():
    lab = np.zeros((4, 5), np.int32)
    for bad in (lab.astype(np.int64), lab.astype(np.uint8), lab.astype(np.float32), lab.astype(bool), [[0, 1]]):
        with pytest.raises(TypeError):
            regions.shape_labels(bad)
    for bad in (lab.astype(np.int64), lab.astype(np.float32), [[0, 1]]):
        with pytest.raises(TypeError):
            regions.boundaries(bad)
    for bad in (lab, lab.astype(np.uint8)):
        with pytest.raises(TypeError):
            regions.shape(bad)                                              # integer input is a label image: shape_labels
    with pytest.raises(TypeError):
        regions.shape_labels(lab, table={"bbox": None})
    for shape in ((32769, 1), (1, 32769), (2, 1, 32769)):
        huge = torch.zeros(1, dtype=torch.int32).expand(*shape)             # no memory behind it
        with pytest.raises(ValueError, match="32768"):
            regions.shape_labels(huge)
        with pytest.raises(ValueError, match="32768"):
            regions.shape(torch.zeros(1, dtype=torch.bool).expand(*shape))
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError):
            regions.shape_labels(lab, max_regions=bad)
        with pytest.raises(ValueError):
            regions.shape(lab.astype(bool), max_regions=bad)
    with pytest.raises(ValueError):
        regions.boundaries(lab, connectivity=3)
    with pytest.raises(ValueError):
        regions.shape_labels(np.zeros((0, 5), np.int32))
    with pytest.raises(ValueError):
        regions.shape_labels(np.zeros((1, 2, 3, 4), np.int32))
    # a table that does not fit: capacity against max_regions, and N / capacity against the images and the table's own rows
    def table(n, cap, rows=None):
        return regions.RegionTable(torch.zeros(n, dtype=torch.int32), cap, torch.zeros((n, cap), dtype=torch.int32),
                                   torch.zeros((n, cap if rows is None else rows, 4), dtype=torch.int32),
                                   torch.zeros((n, cap, 2), dtype=torch.int64))
    with pytest.raises(ValueError, match="capacity"):
        regions.shape_labels(lab, table=table(1, 3), max_regions=4)
    batch = np.zeros((2, 4, 5), np.int32)
    for bad in (table(1, 3), table(3, 3), table(2, 3, rows=5)):
        with pytest.raises(ValueError, match="RegionTable"):
            regions.shape_labels(batch, table=bad)
    with pytest.raises(ValueError, match="RegionTable"):
        regions.shape_labels(lab, table=table(2, 3))
    import inspect
    assert inspect.signature(inference.measure_cells).parameters["shape"].default is False


def test_entry_points_in_header_table_and_library():
    header = open(os.path.join(ROOT, "include", "cellseg_hip.h")).read()
    for name, n_args in (("cs_regions_edges_labels", 6), ("cs_regions_shape_labels", 10)):
        decl = re.search(rf"\bint {name}\((.*?)\);", header, flags=re.S)
        assert decl is not None and len(decl.group(1).split(",")) == n_args
        restype, argtypes = _lib._SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == n_args and argtypes[-1] is ctypes.c_void_p
        assert name in _lib.exported_symbols() and f" * {name}" in header      # described in the section's comment
    assert callable(kernels.regions_edges_labels) and callable(kernels.regions_shape_labels)
    assert kernels.REGIONS_SHAPE_MAX_SIDE == 32768


def test_library_refuses_bad_arguments():
    """argument checks of the library itself: refused with a message, nothing launched (only where the library is built)"""
    lib = _lib.load()
    assert hasattr(lib, "cs_regions_edges_labels") and hasattr(lib, "cs_regions_shape_labels")
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    assert lib.cs_regions_shape_labels(p, p, 1, 4, 5, 0, p, p, p, None) == -1 and b"capacity" in lib.cs_last_error()
    assert lib.cs_regions_shape_labels(p, p, 1, 4, 5, 2, p, None, p, None) == -1 and b"NULL table" in lib.cs_last_error()
    assert lib.cs_regions_shape_labels(p, p, 1, 4, 5, 2, None, p, p, None) == -1 and b"NULL table" in lib.cs_last_error()
    assert lib.cs_regions_shape_labels(p, p, 1, 4, 5, 2, p, p, None, None) == -1 and b"NULL table" in lib.cs_last_error()
    assert lib.cs_regions_shape_labels(None, p, 1, 4, 5, 2, p, p, p, None) == -1 and b"NULL" in lib.cs_last_error()
    assert lib.cs_regions_shape_labels(p, None, 1, 4, 5, 2, p, p, p, None) == -1 and b"NULL" in lib.cs_last_error()
    assert lib.cs_regions_shape_labels(p, p, 1, 1, 32769, 2, p, p, p, None) == -1 and b"32768" in lib.cs_last_error()
    assert lib.cs_regions_shape_labels(p, p, 1, 32769, 1, 2, p, p, p, None) == -1 and b"32768" in lib.cs_last_error()
    assert lib.cs_regions_shape_labels(p, p, 0, 4, 5, 2, p, p, p, None) == -1 and b"2^31" in lib.cs_last_error()
    assert lib.cs_regions_shape_labels(p, p, 65535, 1, 1, 1 << 20, p, p, p, None) == -1 and b"N capacity" in lib.cs_last_error()
    assert lib.cs_regions_edges_labels(None, 1, 4, 5, p, None) == -1 and b"NULL" in lib.cs_last_error()
    assert lib.cs_regions_edges_labels(p, 1, 4, 5, None, None) == -1 and b"NULL" in lib.cs_last_error()
    assert lib.cs_regions_edges_labels(p, 1, 40000, 60000, p, None) == -1 and b"2^31" in lib.cs_last_error()
