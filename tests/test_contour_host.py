"""CPU: the plain-loop restatement of the per-label contour polygons (tests/contour_ref.py) against the scipy vectors of
tests/golden/contour_vectors.npz and against hand cases with literal values; the argument errors of regions.contour_labels /
contours, which are raised before anything is copied; the two new entry points in the header, the ctypes table and the library;
``ContourTable.geojson`` and the table's columns on CPU tensors."""
import ctypes
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import contour_ref as CR
import shape_ref as SR
from cellsegmentation_amd import _lib, inference, kernels, regions
from cellsegmentation_amd.regions import ContourTable, RegionTable

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "contour_vectors.npz"), allow_pickle=False)
NAMES = sorted(k[:-len(".labels")] for k in GOLD.files if k.endswith(".labels"))
PINCH = np.array([[1, 0, 2], [0, 1, 2], [1, 1, 0]], np.int32)
PINCH_RING2 = [(0, 0), (0, 1), (1, 1), (1, 2), (3, 2), (3, 0), (2, 0), (2, 1), (1, 1), (1, 0)]


def _first_pixel(obj):
    i = int(np.flatnonzero(obj.ravel())[0])
    return divmod(i, obj.shape[1])


def check_ring(ring, row, obj):
    """the properties every ring has: the start, alternating axis-parallel edges, an even count >= 4, length and area"""
    n = len(ring)
    assert n == row[0] and n >= 4 and n % 2 == 0 and ring[0] == _first_pixel(obj)
    length = 0
    for k in range(n):
        (ra, ca), (rb, cb) = ring[k], ring[(k + 1) % n]
        assert (ra == rb) != (ca == cb)                                   # axis-parallel and not degenerate
        assert (ra == rb) == (k % 2 == 0)                                 # horizontal first, then alternating: a strict ring
        length += abs(ra - rb) + abs(ca - cb)
    assert length == row[1]
    area2 = sum(ring[k][1] * ring[(k + 1) % n][0] - ring[(k + 1) % n][1] * ring[k][0] for k in range(n))
    assert area2 == row[2] > 0


@pytest.mark.parametrize("conn", [1, 2])
@pytest.mark.parametrize("name", NAMES)
def test_restatement_reproduces_the_scipy_vectors(name, conn):
    lab = GOLD[f"{name}.labels"].astype(np.int32)
    filled = GOLD[f"{name}.filled{conn}"].astype(bool)
    t = CR.contour_labels(lab, None, conn)
    assert t["capacity"] == len(filled) == max(1, int(lab.max())) and not t["hit_bound"].any()
    assert t["contour"].dtype == np.int32 and np.array_equal(t["contour"][0, :, 3], GOLD[f"{name}.cracks_all"])
    for k in range(t["capacity"]):
        row, ring = t["contour"][0, k].tolist(), t["rings"][0][k]
        if t["area"][0, k] == 0:
            assert row == [0, 0, 0, 0] and ring is None and not filled[k].any() and (t["vertices"][0, k] == -1).all()
            continue
        check_ring(ring, row, lab == k + 1)
        assert np.array_equal(CR.fill(ring, lab.shape), filled[k]) and row[2] == 2 * int(filled[k].sum())
        assert row[1] <= row[3] and np.array_equal(t["vertices"][0, k, :row[0]], ring)
        # simple exactly where the filled first component is all of the label
        assert CR.is_simple(t)[0, k] == np.array_equal(filled[k], lab == k + 1)


def test_golden_covers_what_it_should():
    assert {"pinch", "frame3", "square5", "ring_dot", "checker", "blobs", "random", "gap"} <= set(NAMES)
    assert (GOLD["gap.filled1"][3] == 0).all() and GOLD["gap.labels"].min() < 0              # a label without a pixel, labels below 0
    assert GOLD["ring_dot.filled1"][0].sum() > (GOLD["ring_dot.labels"] == 1).sum()          # a hole, and another label inside it
    assert GOLD["checker.filled1"][0].sum() == 1 and GOLD["checker.filled2"][0].sum() > 27   # pinch points at every vertex
    differ = [n for n in NAMES if not np.array_equal(GOLD[f"{n}.filled1"], GOLD[f"{n}.filled2"])]
    assert {"pinch", "checker", "random"} <= set(differ)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "contour_vectors.npz")) < 64 * 1024


def _one(lab, conn=1, label=1):
    t = CR.contour_labels(np.asarray(lab, np.int32), None, conn)
    return tuple(t["contour"][0, label - 1].tolist()), t["rings"][0][label - 1], t


def test_hand_cases():
    for conn in (1, 2):
        row, ring, t = _one([[1]], conn)
        assert row == (4, 4, 2, 4) and ring == [(0, 0), (0, 1), (1, 1), (1, 0)] and CR.is_simple(t).all()
        sq = np.zeros((7, 7), np.int32)
        sq[1:6, 1:6] = 1
        row, ring, t = _one(sq, conn)
        assert row == (4, 20, 50, 20) and ring == [(1, 1), (1, 6), (6, 6), (6, 1)] and CR.hole_area(t)[0, 0] == 0
        frame = np.ones((3, 3), np.int32)
        frame[1, 1] = 0
        row, ring, t = _one(frame, conn)
        assert row == (4, 12, 18, 16) and CR.hole_area(t)[0, 0] == 1.0 and not CR.is_simple(t)[0, 0]
        assert CR.enclosed_area(t)[0, 0] == 9.0 and CR.crack_perimeter(t)[0, 0] == 12.0
    row, ring, t = _one(PINCH, 1)
    assert row == (4, 4, 2, 12) and ring == [(0, 0), (0, 1), (1, 1), (1, 0)] and CR.is_simple(t)[0].tolist() == [False, True]
    row, ring, t = _one(PINCH, 2)
    assert row == (10, 12, 8, 12) and ring == PINCH_RING2 and CR.is_simple(t)[0].tolist() == [True, True]
    assert ring.count((1, 1)) == 2                                        # the pinch point occurs twice
    assert _one(PINCH, 1, label=2)[0] == _one(PINCH, 2, label=2)[0] == (4, 6, 4, 6)


def test_rings_do_not_depend_on_where_the_object_lies_and_the_box_defines_it():
    big = np.zeros((40, 50), np.int32)
    big[30:34, 41:48] = 1
    big[35, 44] = 1                                                       # a second piece: counted in cracks_all only
    big[34, 48] = 1                                                       # a diagonal neighbour: joined at connectivity 2 only
    for conn in (1, 2):
        a, b = CR.contour_labels(big, None, conn), CR.contour_labels(big[29:37, 40:50], None, conn)
        assert np.array_equal(a["contour"], b["contour"])
        assert [(r - 29, c - 40) for r, c in a["rings"][0][0]] == b["rings"][0][0]
    assert _one(big, 1)[0] == (4, 22, 56, 30) and _one(big, 2)[0] == (8, 26, 58, 30)
    cut = CR.contour_labels(big, None, 2, None, bbox=np.array([[[30, 41, 34, 48]]]))      # the box without the two extra pixels
    assert cut["contour"][0, 0].tolist() == [4, 22, 56, 22] and cut["bbox"][0, 0].tolist() == [30, 41, 36, 49]
    miss = CR.contour_labels(big, None, 1, None, bbox=np.array([[[0, 0, 5, 5]]]))
    assert not miss["contour"].any() and (miss["vertices"] == -1).all()


def test_side_limit_and_capacities_in_the_restatement():
    assert CR.MAX_SIDE == kernels.REGIONS_CONTOUR_MAX_SIDE == 512
    line = np.zeros((2, 514), np.int32)
    line[0, :512] = 1
    line[1, :513] = 2
    t = CR.contour_labels(line)
    assert t["contour"][0].tolist() == [[4, 1026, 1024, 1026], [-1] * 4] and CR.too_large(t)[0].tolist() == [False, True]
    assert t["area"][0].tolist() == [512, 513] and np.isnan(CR.n_vertices(t)[0, 1]) and not CR.is_simple(t)[0, 1]
    comb = np.zeros((6, 24), np.int32)
    comb[1, 2:21] = 1
    comb[2:5, 2:21:2] = 1
    t = CR.contour_labels(comb, None, 1, 8)
    assert t["contour"][0, 0, 0] == 40 and CR.truncated(t)[0].tolist() == [True] and t["vertices"].shape == (1, 1, 8, 2)
    assert (t["vertices"] >= 0).all() and CR.contour_labels(comb)["vertices"].shape == (1, 1, 40, 2)
    assert CR.contour_labels(comb, 3, 1, 0)["vertices"].shape == (1, 3, 0, 2)
    lab = SR.random_labels(2, 30, 40, seed=4, top=6)
    full, few = CR.contour_labels(lab, None, 2), CR.contour_labels(lab, 2, 2)
    assert np.array_equal(few["contour"], full["contour"][:, :2]) and np.array_equal(few["counts"], full["counts"])


def test_argument_errors_before_any_device_work():
    lab = np.zeros((4, 5), np.int32)
    for bad in (lab.astype(np.int64), lab.astype(np.uint8), lab.astype(np.float32), lab.astype(bool), [[0, 1]]):
        with pytest.raises(TypeError):
            regions.contour_labels(bad)
    for bad in (lab, lab.astype(np.uint8)):
        with pytest.raises(TypeError):
            regions.contours(bad)                                           # integer input is a label image: contour_labels
    with pytest.raises(TypeError):
        regions.contour_labels(lab, table={"bbox": None})
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError):
            regions.contour_labels(lab, max_regions=bad)
        with pytest.raises(ValueError):
            regions.contours(lab.astype(bool), max_regions=bad)
    for bad in (0, 3, 1.5, "1"):
        with pytest.raises(ValueError, match="connectivity"):
            regions.contour_labels(lab, connectivity=bad)
        with pytest.raises(ValueError, match="connectivity"):
            regions.contours(lab.astype(bool), connectivity=bad)
    for bad in (-1, 2.5, True):
        with pytest.raises(ValueError, match="max_vertices"):
            regions.contour_labels(lab, max_vertices=bad)
        with pytest.raises(ValueError, match="max_vertices"):
            regions.contours(lab.astype(bool), max_vertices=bad)
    with pytest.raises(ValueError):
        regions.contour_labels(np.zeros((0, 5), np.int32))
    with pytest.raises(ValueError):
        regions.contour_labels(np.zeros((1, 2, 3, 4), np.int32))

    def table(n, cap, rows=None):
        return regions.RegionTable(torch.zeros(n, dtype=torch.int32), cap, torch.zeros((n, cap), dtype=torch.int32),
                                   torch.zeros((n, cap if rows is None else rows, 4), dtype=torch.int32),
                                   torch.zeros((n, cap, 2), dtype=torch.int64))
    with pytest.raises(ValueError, match="capacity"):
        regions.contour_labels(lab, table=table(1, 3), max_regions=4)
    batch = np.zeros((2, 4, 5), np.int32)
    for bad in (table(1, 3), table(3, 3), table(2, 3, rows=5)):
        with pytest.raises(ValueError, match="RegionTable"):
            regions.contour_labels(batch, table=bad)
    with pytest.raises(ValueError, match="RegionTable"):
        regions.contour_labels(lab, table=table(2, 3))
    params = inspect.signature(inference.measure_cells).parameters
    assert params["contours"].default is False and params["max_vertices"].default is None
    assert list(inspect.signature(regions.contour_labels).parameters) == \
        list(inspect.signature(regions.hull_labels).parameters) + ["connectivity", "max_vertices"]
    assert list(inspect.signature(regions.contours).parameters) == ["m", "connectivity", "max_regions", "max_vertices"]
    assert inspect.signature(regions.contour_labels).parameters["connectivity"].default == 1


def test_entry_points_in_header_table_and_library():
    header = open(os.path.join(ROOT, "include", "cellseg_hip.h")).read()
    decl = re.search(r"\bint cs_regions_contour_labels\((.*?)\);", header, flags=re.S)
    assert decl is not None and len(decl.group(1).split(",")) == 11
    restype, argtypes = _lib._SIGNATURES["cs_regions_contour_labels"]
    assert restype is ctypes.c_int and len(argtypes) == 11 and argtypes[-1] is ctypes.c_void_p
    assert [a is ctypes.c_int for a in argtypes] == [False, True, True, True, True, False, True, True, False, False, False]
    assert re.search(r"\bint cs_regions_contour_max_side\(void\);", header)
    assert _lib._SIGNATURES["cs_regions_contour_max_side"] == (ctypes.c_int, [])
    for name in ("cs_regions_contour_labels", "cs_regions_contour_max_side"):
        assert name in _lib.exported_symbols() and f" * {name}" in header       # described in the section's comment
    assert callable(kernels.regions_contour_labels) and kernels.REGIONS_CONTOUR_MAX_SIDE == 512


def test_library_refuses_bad_arguments():
    """argument checks of the library itself: refused with a message, nothing launched (only where the library is built)"""
    lib = _lib.load()
    assert lib.cs_regions_contour_max_side() == 512 and lib.cs_abi_version() == 10
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    call = lib.cs_regions_contour_labels
    assert call(p, 1, 4, 5, 0, p, 1, 4, p, p, None) == -1 and b"capacity" in lib.cs_last_error()
    assert call(None, 1, 4, 5, 2, p, 1, 4, p, p, None) == -1 and b"NULL" in lib.cs_last_error()
    assert call(p, 1, 4, 5, 2, None, 1, 4, p, p, None) == -1 and b"NULL table" in lib.cs_last_error()
    assert call(p, 1, 4, 5, 2, p, 1, 4, None, p, None) == -1 and b"NULL table" in lib.cs_last_error()
    assert call(p, 1, 4, 5, 2, p, 1, 4, p, None, None) == -1 and b"NULL vertices" in lib.cs_last_error()
    assert call(p, 0, 4, 5, 2, p, 1, 4, p, p, None) == -1 and b"2^31" in lib.cs_last_error()
    assert call(p, 1, 40000, 60000, 2, p, 1, 4, p, p, None) == -1 and b"2^31" in lib.cs_last_error()
    assert call(p, 65535, 1, 1, 1 << 20, p, 1, 4, p, p, None) == -1 and b"N capacity" in lib.cs_last_error()
    for conn in (0, 3, -1):
        assert call(p, 1, 4, 5, 2, p, conn, 4, p, p, None) == -1 and b"connectivity" in lib.cs_last_error()
    assert call(p, 1, 4, 5, 2, p, 1, -1, p, p, None) == -1 and b"max_vertices >= 0" in lib.cs_last_error()
    assert call(p, 1, 4, 5, 1 << 20, p, 2, 1 << 10, p, p, None) == -1 and b"max_vertices < 2^31" in lib.cs_last_error()


def _cpu_table(lab, conn, max_vertices=None):
    """a ContourTable of CPU tensors with the restatement's numbers"""
    t = CR.contour_labels(lab, None, conn, max_vertices)
    table = RegionTable(torch.from_numpy(t["counts"]), t["capacity"], torch.from_numpy(t["area"]), torch.from_numpy(t["bbox"]),
                        torch.from_numpy(t["sum_rc"]))
    return ContourTable(table, torch.from_numpy(t["contour"]), torch.from_numpy(t["vertices"]), conn), t


def test_columns_and_per_image_on_cpu_tensors():
    lab = SR.random_labels(2, 30, 40, seed=4, top=6)
    lab[lab == 3] = 0                                                     # an unused row
    ct, t = _cpu_table(lab, 2, 6)
    assert ct.max_vertices == 6 and CR.truncated(t).any() and not CR.truncated(t).all()
    for name in ("too_large", "truncated", "is_simple"):
        got = getattr(ct, name)()
        assert got.dtype == torch.bool and np.array_equal(got.numpy(), getattr(CR, name)(t)), name
    for name, want in CR.columns(t).items():
        got = getattr(ct, name)()
        assert got.dtype == torch.float64 and np.array_equal(got.numpy(), want, equal_nan=True), name
        assert np.isnan(got.numpy()[:, 2]).all()
    for n, d in enumerate(ct.per_image()):
        assert len(d["polygon"]) == len(d["area"]) == 6 and d["contour"].shape == (6, 4)
        for k, poly in enumerate(d["polygon"]):
            kept = min(int(t["contour"][n, k, 0]), 6)
            assert poly.dtype == np.int32 and np.array_equal(poly, t["vertices"][n, k, :kept])
        assert len(d["polygon"][2]) == 0 and np.isnan(d["hole_area"][2]) and not d["is_simple"][2]


def test_geojson():
    ct, t = _cpu_table(PINCH, 2)
    doc = ct.geojson()
    assert json.loads(json.dumps(doc)) == doc and doc["type"] == "FeatureCollection" and len(doc["features"]) == 2
    f = doc["features"][0]
    assert f["type"] == "Feature" and f["geometry"]["type"] == "Polygon" and f["properties"] == {"row": 0, "area": 4}
    ring = f["geometry"]["coordinates"][0]
    assert len(f["geometry"]["coordinates"]) == 1 and ring[0] == ring[-1] and len(ring) == 11
    assert ring == [[float(c), float(r)] for r, c in PINCH_RING2 + PINCH_RING2[:1]]            # x = col, y = row
    assert doc["features"][1]["geometry"]["coordinates"][0] == [[2, 0], [3, 0], [3, 2], [2, 2], [2, 0]]
    moved = ct.geojson(origin=(1000, -20), scale=0.25, properties={"name": np.array(["a", "b"]), "score": [0.5, 2]})
    assert moved["features"][1]["geometry"]["coordinates"][0] == [[1000.5, -20.0], [1000.75, -20.0], [1000.75, -19.5], [1000.5, -19.5],
                                                                  [1000.5, -20.0]]
    assert moved["features"][1]["properties"] == {"row": 1, "area": 2, "name": "b", "score": 2.0}
    assert json.loads(json.dumps(moved)) == moved
    # rows that are unused, truncated or too large are left out
    lab = np.zeros((3, 520), np.int32)
    lab[0, :513] = 1                                                      # too large
    lab[2, 0:5:2] = 2                                                     # three pieces: traced is the first, 4 vertices
    lab[2, 10:13] = 4                                                     # label 3 has no pixel
    lab[1, 11] = 4                                                        # 8 vertices: truncated at 6
    lab[2, 20] = 5
    ct, t = _cpu_table(lab[None], 1, 6)
    assert t["contour"][0, :, 0].tolist() == [-1, 4, 0, 8, 4]
    doc = ct.geojson(image=0)
    assert [f["properties"]["row"] for f in doc["features"]] == [1, 4]
    assert doc["features"][0]["geometry"]["coordinates"][0] == [[0, 2], [1, 2], [1, 3], [0, 3], [0, 2]]
    with pytest.raises(IndexError):
        ct.geojson(image=1)
    with pytest.raises(ValueError, match="one value per row"):
        ct.geojson(properties={"x": [1, 2]})
