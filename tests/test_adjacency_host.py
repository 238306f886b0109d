"""CPU: the numpy statement of the adjacency tables (tests/adjacency_ref.py) against answers worked by hand, against
tests/golden/adjacency_vectors.npz and against two statements that share nothing with it (scipy's dilation for the listed pairs,
tests/contour_ref.py's crack count for the boundary); the argument errors of ``regions.adjacency_labels``, ``regions.adjacency``,
``spatial.voronoi_graph`` and ``inference.slide_contacts`` (raised before any device work); ``AdjacencyTable`` on host tensors; the
new entry points in the library, their workspace formula and their refusals."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import adjacency_ref as A  # noqa: E402
from cellsegmentation_amd import _lib, inference, spatial  # noqa: E402
from cellsegmentation_amd import kernels as K  # noqa: E402
from cellsegmentation_amd import regions as G  # noqa: E402

GOLD = np.load(os.path.join(ROOT, "tests", "golden", "adjacency_vectors.npz"), allow_pickle=False)
NAMES = sorted(k[:-len(".labels")] for k in GOLD.files if k.endswith(".labels"))
TOL = 1e-12


def test_golden_file_is_what_the_maker_writes():
    import make_adjacency_golden as MG
    assert NAMES == sorted(name for name, _ in MG.cases())
    for name, (labels, cap) in MG.cases():
        assert np.array_equal(labels, GOLD[f"{name}.labels"]) and labels.dtype == np.int32
        assert cap is None or cap == int(GOLD[f"{name}.cap"][0])
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "adjacency_vectors.npz")) < 256 * 1024


@pytest.mark.parametrize("conn", (1, 2))
@pytest.mark.parametrize("name", NAMES)
def test_reference_equals_golden(name, conn):
    t = A.adjacency(GOLD[f"{name}.labels"], int(GOLD[f"{name}.cap"][0]), conn)
    for key in A.TABLES:
        assert t[key].dtype == np.int32 and np.array_equal(t[key], GOLD[f"{name}.c{conn}.{key}"]), key
    for key, col in zip(A.PAIRS, t["pairs"]):
        assert col.dtype == np.int64 and np.array_equal(col, GOLD[f"{name}.c{conn}.pair_{key}"]), key


@pytest.mark.parametrize("conn", (1, 2))
@pytest.mark.parametrize("name", NAMES)
def test_scipy_dilation_and_crack_count_pin_the_golden_tables(name, conn):
    import make_adjacency_golden as MG
    t = {k: GOLD[f"{name}.c{conn}.{k}"] for k in A.TABLES}
    t.update(cap=int(GOLD[f"{name}.cap"][0]), connectivity=conn, pairs=tuple(GOLD[f"{name}.c{conn}.pair_{k}"] for k in A.PAIRS))
    MG.pins(GOLD[f"{name}.labels"], t)


def _one(name, conn):
    lab, cap = A.hand_cases()[name]
    return A.adjacency(lab, cap, conn)


def _pairs(t):
    return [tuple(int(c[k]) for c in t["pairs"][1:]) for k in range(len(t["pairs"][0]))]


def _rows(t, *keys):
    return [t[k][0].tolist() for k in keys]


def test_hand_worked_answers():
    for conn, corners in ((1, (0, 0, 0)), (2, (1, 2, 2))):
        t = _one("three", conn)
        assert _pairs(t) == [(1, 2, 1, corners[0]), (1, 3, 2, corners[1]), (2, 3, 2, corners[2])]
        assert _rows(t, "background", "outside", "contact", "n_neighbors", "partner", "partner_sides") == \
            [[1, 0, 1], [4, 3, 3], [3, 3, 4], [2, 2, 2], [3, 3, 1], [2, 2, 2]]          # label 3: a tie at 2 sides, the lower label
        assert t["counts"].tolist() == [3] and t["n_pairs"].tolist() == [3] and t["cap"] == 3
        t = _one("one_row", conn)                                       # 1 1 2 0 2 3
        assert _pairs(t) == [(1, 2, 1, 0), (2, 3, 1, 0)]
        assert _rows(t, "background", "outside", "contact", "n_neighbors", "partner") == [[0, 2, 0], [5, 4, 3], [1, 2, 1], [1, 2, 1], [2, 1, 2]]
        t = _one("one_column", conn)                                    # 1 2 2 0 1
        assert _pairs(t) == [(1, 2, 1, 0)] and _rows(t, "background", "outside", "contact") == [[1, 1], [6, 4], [1, 1]]
        t = _one("empty", conn)
        assert t["cap"] == 1 and _pairs(t) == [] and t["counts"].tolist() == [0]
        assert all(not t[k].any() for k in A.TABLES)
        t = _one("single_pixel", conn)
        assert _rows(t, "outside", "background", "contact", "n_neighbors", "partner") == [[4], [0], [0], [0], [0]] and _pairs(t) == []
        t = _one("non_positive", conn)                                  # labels <= 0 are background: 1 and 2 never meet
        assert _pairs(t) == [] and _rows(t, "background", "outside") == [[3, 3], [3, 5]] and t["counts"].tolist() == [2]
    t = _one("corner_only", 1)
    assert _pairs(t) == [] and _rows(t, "n_neighbors", "partner", "background", "outside") == [[0, 0], [0, 0], [2, 2], [2, 2]]
    t = _one("corner_only", 2)                                          # listed by its corner, with no side at all
    assert _pairs(t) == [(1, 2, 0, 1)] and _rows(t, "n_neighbors", "partner", "partner_sides", "contact") == [[1, 1], [2, 1], [0, 0], [0, 0]]
    t = _one("disconnected", 2)                                         # label 1 in three pieces: one row, every piece counted
    assert _pairs(t) == [(1, 2, 3, 3), (2, 3, 1, 1)]
    assert _rows(t, "background", "outside", "contact", "n_neighbors", "partner") == [[3, 2, 1], [6, 2, 2], [3, 4, 1], [1, 2, 1], [2, 1, 2]]
    t = _one("above_capacity", 2)                                       # labels 4 and 5 are background at capacity 3
    assert t["counts"].tolist() == [5] and _pairs(t) == [(1, 2, 1, 1), (2, 3, 1, 1)]
    assert _rows(t, "background", "outside", "contact") == [[2, 1, 2], [3, 3, 3], [1, 2, 1]]
    names, batch = A.stacked()
    assert "above_capacity" not in names and "three" in names and batch.dtype == np.int32 and batch.shape == (len(names), 5, 6)


def test_identity_on_random_label_images():
    rng = np.random.RandomState(3)
    for shape in ((1, 1, 9), (2, 7, 1), (3, 12, 17), (2, 30, 31)):
        lab = rng.randint(-1, 7, size=shape).astype(np.int32)
        for conn in (1, 2):
            t = A.adjacency(lab, 5, conn)
            assert np.array_equal(A.boundary(t), 4 * t["area"] - 2 * t["same_sides"])
            assert t["area"].sum() > 0
            pair_sum = np.zeros_like(t["contact"])
            for n, a, b, s, _ in zip(*t["pairs"]):
                pair_sum[n, a - 1] += s
                pair_sum[n, b - 1] += s
            assert np.array_equal(pair_sum, t["contact"]) and t["n_pairs"].sum() == len(t["pairs"][0])


def test_argument_errors_before_any_device_work():
    lab = np.zeros((4, 5), np.int32)
    with pytest.raises(TypeError, match="numpy array or a torch tensor"):
        G.adjacency_labels([[1]])
    with pytest.raises(TypeError, match="int32 label image"):
        G.adjacency_labels(lab.astype(np.int64))
    with pytest.raises(TypeError, match="int32 label image"):
        G.adjacency_labels(lab > 0)
    with pytest.raises(ValueError, match=r"\[H, W\] or \[N, H, W\]"):
        G.adjacency_labels(lab[0])
    with pytest.raises(ValueError, match="empty label image"):
        G.adjacency_labels(lab[:0])
    with pytest.raises(ValueError, match="2\\^31 pixels"):
        G.adjacency_labels(torch.zeros((1, 1), dtype=torch.int32).expand(1 << 16, 1 << 15))
    for bad in (0, 3, "1", None):
        with pytest.raises(ValueError, match="connectivity"):
            G.adjacency_labels(lab, connectivity=bad)
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match="max_regions"):
            G.adjacency_labels(lab, max_regions=bad)
    for bad in (0, -1, 1.5, True, (1 << 29) + 1):
        with pytest.raises(ValueError, match="max_pairs"):
            G.adjacency_labels(lab, max_regions=4, max_pairs=bad)
    for kw in ({"counts": torch.zeros(2, dtype=torch.int32)}, {"counts": torch.zeros(1, dtype=torch.int64)}, {"counts": np.zeros(1, np.int32)}):
        with pytest.raises(TypeError, match="counts must be an int32 tensor of shape"):
            G.adjacency_labels(lab, **kw)
    with pytest.raises(ValueError, match="either distance or radius_sq"):
        G.adjacency_labels(lab, distance=2, radius_sq=4)
    with pytest.raises((TypeError, ValueError)):
        G.adjacency_labels(lab, distance=-1)
    with pytest.raises(TypeError, match="radius_sq must be an integer"):
        G.adjacency_labels(lab, radius_sq=2.0)
    with pytest.raises(ValueError, match="H\\^2 \\+ W\\^2"):
        G.adjacency_labels(torch.zeros((1, 1), dtype=torch.int32).expand(40000, 30000), distance=1)
    # the mask counterpart
    with pytest.raises(TypeError, match="boolean mask"):
        G.adjacency(lab)
    with pytest.raises(ValueError, match="connectivity"):
        G.adjacency(lab > 0, connectivity=3)
    with pytest.raises(ValueError, match="max_pairs"):
        G.adjacency(lab > 0, max_pairs=0)
    with pytest.raises(ValueError, match="either distance or radius_sq"):
        G.adjacency(lab > 0, distance=1, radius_sq=1)


def test_voronoi_graph_and_slide_contacts_argument_errors():
    pts = np.asarray([[1, 2], [3, 4]], np.int64)
    with pytest.raises(TypeError, match="image_hw"):
        spatial.voronoi_graph(pts, 7)
    with pytest.raises(ValueError, match="image_hw"):
        spatial.voronoi_graph(pts, (0, 4))
    with pytest.raises(ValueError, match="2\\^31"):
        spatial.voronoi_graph(pts, (40000, 30000))
    with pytest.raises(ValueError, match="wider than"):
        spatial.voronoi_graph(pts, (4, 41000))
    with pytest.raises(ValueError, match="connectivity"):
        spatial.voronoi_graph(pts, (8, 8), connectivity=0)
    with pytest.raises(ValueError, match="max_pairs"):
        spatial.voronoi_graph(pts, (8, 8), max_pairs=0)
    with pytest.raises((TypeError, ValueError)):
        spatial.voronoi_graph(pts, (8, 8), max_distance=-2)
    with pytest.raises(ValueError, match="shaped \\[n, 2\\]"):
        spatial.voronoi_graph(np.zeros((3, 3), np.int64), (8, 8))
    with pytest.raises(TypeError, match="integer coordinates"):
        spatial.voronoi_graph(pts.astype(np.float32), (8, 8))
    with pytest.raises(ValueError, match="offsets must rise"):
        spatial.voronoi_graph(pts, (8, 8), offsets=[0, 1])
    with pytest.raises(ValueError, match="fewer than 2\\^31 pixels"):
        spatial.voronoi_graph(np.zeros((0, 2), np.int64), (30000, 30000), offsets=np.zeros(4, np.int64))

    with pytest.raises(TypeError, match="SlideResult"):
        inference.slide_contacts(object())
    res = inference.SlideResult(pts, [], 2, torch.zeros((8, 8), dtype=torch.uint8))
    with pytest.raises(ValueError, match="connectivity"):
        inference.slide_contacts(res, connectivity=4)
    with pytest.raises(ValueError, match="max_pairs"):
        inference.slide_contacts(res, max_pairs=-1)
    with pytest.raises((TypeError, ValueError)):
        inference.slide_contacts(res, distance="far")
    with pytest.raises(TypeError, match="bogus"):
        inference.slide_contacts(res, bogus=1)
    with pytest.raises(ValueError, match="thr_u8"):
        inference.slide_contacts(res, thr_u8=300)


def _host_table(t, cap, conn, keys, sides, corners, dropped=0):
    i32 = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32))  # noqa: E731
    return G.AdjacencyTable(i32(t["counts"]), cap, conn, i32(t["n_pairs"]), torch.full((len(t["counts"]),), dropped, dtype=torch.int32),
                            *(i32(t[k]) for k in A.TABLES[2:]), keys, sides, corners)


def test_adjacency_table_on_host_tensors():
    """the table's tensors may live anywhere: pairs() and edge_index() sort the raw slots, the floats are plain quotients"""
    t = _one("three", 2)
    keys = torch.tensor([[0, (2 << 32) | 3, 0, (1 << 32) | 3, (1 << 32) | 2, 0, 0, 0]], dtype=torch.int64)   # out of order, with gaps
    sides = torch.tensor([[0, 2, 0, 2, 1, 0, 0, 0]], dtype=torch.int32)
    corners = torch.tensor([[0, 2, 0, 2, 1, 0, 0, 0]], dtype=torch.int32)
    table = _host_table(t, 3, 2, keys, sides, corners)
    got = table.pairs()
    assert len(got) == 5
    for a, b in zip(got, t["pairs"]):
        assert a.dtype == np.int64 and np.array_equal(a, b)
    edges, image, s, c = table.edge_index()
    assert edges.dtype == torch.int64 and edges.tolist() == [[0, 0, 1], [1, 2, 2]] and image.tolist() == [0, 0, 0]
    assert s.tolist() == [1, 2, 2] and c.tolist() == [1, 2, 2]
    assert table.boundary().dtype == torch.int32 and table.boundary().tolist() == [[8, 6, 8]]
    f = table.touching_fraction()
    assert f.dtype == torch.float64 and np.abs(f.numpy() - np.asarray([[3 / 8, 3 / 6, 4 / 8]])).max() <= TOL
    assert table.overflowed().tolist() == [False]
    table.dropped = torch.ones(1, dtype=torch.int32)
    assert table.overflowed().tolist() == [True]
    table.dropped, table.capacity = torch.zeros(1, dtype=torch.int32), 2
    assert table.overflowed().tolist() == [True]
    table.capacity = 3
    per = table.per_image()
    assert len(per) == 1 and per[0]["pairs"].tolist() == [[1, 2, 1, 1], [1, 3, 2, 2], [2, 3, 2, 2]] and per[0]["boundary"].tolist() == [8, 6, 8]
    # a label without pixels: boundary 0 -> NaN; two images keep their own pairs apart
    names, batch = A.stacked()
    t = A.adjacency(batch, None, 1)
    keys = torch.zeros((len(names), 4), dtype=torch.int64)
    sides = torch.zeros((len(names), 4), dtype=torch.int32)
    for n, a, b, s_, _ in zip(*t["pairs"]):
        slot = int((keys[n] != 0).sum())
        keys[n, 3 - slot], sides[n, 3 - slot] = (int(a) << 32) | int(b), int(s_)
    table = _host_table(t, t["cap"], 1, keys, sides, torch.zeros_like(sides))
    for a, b in zip(table.pairs(), t["pairs"]):
        assert np.array_equal(a, b)
    edges, image, s, c = table.edge_index()
    assert np.array_equal(image.numpy(), t["pairs"][0]) and np.array_equal(edges.numpy() + 1, np.stack(t["pairs"][1:3]))
    assert np.array_equal(s.numpy(), t["pairs"][3]) and not c.any()
    f = table.touching_fraction().numpy()
    b = A.boundary(t).astype(np.float64)
    assert np.array_equal(np.isnan(f), b == 0) and (b == 0).any()
    with np.errstate(invalid="ignore", divide="ignore"):
        want = t["contact"].astype(np.float64) / b
    assert np.nanmax(np.abs(f - want)) <= TOL
    assert [len(d["pairs"]) for d in table.per_image()] == t["n_pairs"].tolist()


def test_library_has_the_entry_points():
    lib = _lib.load()
    P, I = ctypes.c_void_p, ctypes.c_int
    assert _lib._SIGNATURES["cs_regions_adjacency_workspace"] == (ctypes.c_size_t, [I, I, I])
    restype, argtypes = _lib._SIGNATURES["cs_regions_adjacency_labels"]
    assert restype is I and len(argtypes) == 19 and argtypes[:7] == [P] + [I] * 6 and argtypes[-2:] == [ctypes.c_size_t, P]
    restype, argtypes = _lib._SIGNATURES["cs_regions_seed_labels"]
    assert restype is I and len(argtypes) == 9 and argtypes[3] is ctypes.c_longlong
    for name in ("cs_regions_adjacency_workspace", "cs_regions_adjacency_labels", "cs_regions_seed_labels"):
        assert hasattr(lib, name) and name in _lib.exported_symbols()
    assert lib.cs_abi_version() == 10
    with open(os.path.join(ROOT, "include", "cellseg_hip.h")) as f:
        header = f.read()
    for name in ("cs_regions_adjacency_workspace(", "cs_regions_adjacency_labels(", "cs_regions_seed_labels("):
        assert name in header
    # 16 N slots + 8 N capacity bytes, slots = the power of two >= 2 max_pairs; every part 16-byte aligned
    ws = lib.cs_regions_adjacency_workspace
    assert ws(1, 1, 1) == 16 * 2 + 16 and ws(1, 4, 1) == 16 * 2 + 32 and ws(1, 3, 3) == 16 * 8 + 32
    assert ws(3, 1000, 5000) == 16 * 3 * 16384 + 8 * 3 * 1000
    assert ws(2, 10000, 30000) == 16 * 2 * 65536 + 8 * 2 * 10000        # far from 2 x 10^4 x 10^4 x 4
    for bad in ((0, 1, 1), (65536, 1, 1), (1, 0, 1), (1, -1, 1), (1, 1, 0), (1, 1, -1), (1, 1, (1 << 29) + 1), (4, 1, 1 << 28), (2, 1 << 30, 1)):
        assert ws(*bad) == 0, bad
    # the call refuses what the workspace function refuses, before anything is launched
    buf = ctypes.create_string_buffer(64)
    ptr = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    args = lambda N, H, W, cap, mp, conn=1: (ptr, N, H, W, cap, mp, conn, None) + (ptr,) * 9 + (1 << 20, None)  # noqa: E731
    call = lib.cs_regions_adjacency_labels
    assert call(*args(1, 4, 4, 0, 1)) == -1 and b"capacity" in lib.cs_last_error()
    assert call(*args(2, 4, 4, 1 << 30, 1)) == -1 and b"capacity" in lib.cs_last_error()
    assert call(*args(1, 4, 4, 1, 0)) == -1 and b"max_pairs" in lib.cs_last_error()
    assert call(*args(1, 4, 4, 1, (1 << 29) + 1)) == -1 and b"max_pairs" in lib.cs_last_error()
    assert call(*args(0, 4, 4, 1, 1)) == -1 and b"N H W" in lib.cs_last_error()
    assert call(*args(1, 0, 4, 1, 1)) == -1 and b"N H W" in lib.cs_last_error()
    assert call(*args(1, 4, 4, 1, 1, 3)) == -1 and b"connectivity" in lib.cs_last_error()
    small = list(args(1, 4, 4, 8, 8))
    small[17] = 16
    assert call(*small) == -1 and b"workspace too small" in lib.cs_last_error()
    odd = list(args(1, 4, 4, 1, 1))
    odd[16] = ctypes.c_void_p(ptr.value + 4)
    assert call(*odd) == -1 and b"misaligned" in lib.cs_last_error()
    for at in (0, 8, 9, 15, 16):                                        # labels, n_pairs, dropped, partner_sides, the workspace
        missing = list(args(1, 4, 4, 8, 8))
        missing[at] = None
        assert call(*missing) == -1 and b"NULL" in lib.cs_last_error(), at
    seed = lib.cs_regions_seed_labels
    assert seed(ptr, ptr, None, 1, 0, 4, 4, ptr, None) == -1 and b"N H W" in lib.cs_last_error()
    assert seed(ptr, ptr, None, -1, 1, 4, 4, ptr, None) == -1 and b"P" in lib.cs_last_error()
    assert seed(None, ptr, None, 1, 1, 4, 4, ptr, None) == -1 and b"NULL" in lib.cs_last_error()
    assert seed(ptr, ptr, None, 1, 1, 4, 4, None, None) == -1 and b"NULL" in lib.cs_last_error()
    assert seed(ptr, None, None, 0, 1, 4, 4, ptr, None) == -1 and b"NULL" in lib.cs_last_error()
    with pytest.raises(ValueError, match="max_pairs"):
        K.regions_adjacency_workspace(1, 1, 0, "cpu")
    assert K._ADJACENCY_TABLES == A.TABLES[2:]
