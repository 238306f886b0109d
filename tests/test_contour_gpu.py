"""The per-label contour polygons on the GPU (contour_kernel of csrc/regions.hip through cellsegmentation_amd.regions.contour_labels
and contours) against the plain-loop restatement tests/contour_ref.py, the scipy vectors of tests/golden/contour_vectors.npz and
scipy.ndimage.binary_fill_holes of the device's own labelling.  Everything is compared by value, on the whole ``contour`` and
``vertices`` tensors.  The float64 columns are compared by value too: each is an int32 converted (exact), halved (exact) or the
difference of two such numbers below 2^53 (exact), so there is no rounding to allow for."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import contour_ref as CR  # noqa: E402
import shape_ref as SR  # noqa: E402
from cellsegmentation_amd import kernels as K  # noqa: E402
from cellsegmentation_amd import regions as G  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "contour_vectors.npz"), allow_pickle=False)
NAMES = sorted(k[:-len(".labels")] for k in GOLD.files if k.endswith(".labels"))
INT_TABLES = {"area": torch.int32, "bbox": torch.int32, "sum_rc": torch.int64}
BOOLS = ("too_large", "truncated", "is_simple")
PINCH = np.array([[1, 0, 2], [0, 1, 2], [1, 1, 0]], np.int32)
PINCH_RING2 = [(0, 0), (0, 1), (1, 1), (1, 2), (3, 2), (3, 0), (2, 0), (2, 1), (1, 1), (1, 0)]


def _np(t):
    return t.cpu().numpy()


def assert_contour(ct, ref):
    """a ContourTable against the restatement's dict: every integer and every column by value, per_image trimmed"""
    assert isinstance(ct, G.ContourTable) and isinstance(ct.table, G.RegionTable) and ct.table.capacity == ref["capacity"]
    assert ct.connectivity == ref["connectivity"] and not ref["hit_bound"].any()
    assert np.array_equal(_np(ct.table.counts), ref["counts"])
    for name, dtype in INT_TABLES.items():
        got = getattr(ct.table, name)
        assert got.dtype == dtype and got.is_cuda and np.array_equal(_np(got), ref[name]), name
    assert ct.contour.dtype == torch.int32 and ct.contour.is_cuda and tuple(ct.contour.shape) == ref["contour"].shape
    assert np.array_equal(_np(ct.contour), ref["contour"])
    assert ct.vertices.dtype == torch.int32 and ct.vertices.is_cuda and tuple(ct.vertices.shape) == ref["vertices"].shape
    assert ct.max_vertices == ref["vertices"].shape[2] and np.array_equal(_np(ct.vertices), ref["vertices"])
    for name in BOOLS:
        got = getattr(ct, name)()
        assert got.dtype == torch.bool and got.is_cuda and np.array_equal(_np(got), getattr(CR, name)(ref)), name
    want = CR.columns(ref)
    unmeasured = (ref["area"] == 0) | (ref["contour"][..., 0] <= 0)
    for name in CR.COLUMNS:
        got = getattr(ct, name)()
        assert got.dtype == torch.float64 and got.is_cuda, name
        got = _np(got)
        assert np.isnan(got[unmeasured]).all() and not np.isnan(got[~unmeasured]).any(), name
        assert np.array_equal(got, want[name], equal_nan=True), name
    nv = ref["contour"][..., 0][~unmeasured]
    assert (nv >= 4).all() and (nv % 2 == 0).all()
    per = ct.per_image()
    assert len(per) == len(ref["counts"])
    for n, d in enumerate(per):
        k = min(int(ref["counts"][n]), ref["capacity"])
        assert {"area", "bbox", "centroid", "contour", "polygon", *BOOLS, *CR.COLUMNS} <= set(d)
        assert np.array_equal(d["area"], ref["area"][n, :k]) and np.array_equal(d["contour"], ref["contour"][n, :k])
        for name in BOOLS:
            assert np.array_equal(d[name], getattr(CR, name)(ref)[n, :k]), name
        for name in CR.COLUMNS:
            assert np.array_equal(d[name], want[name][n, :k], equal_nan=True), name
        assert len(d["polygon"]) == k
        for i, poly in enumerate(d["polygon"]):
            kept = min(max(int(ref["contour"][n, i, 0]), 0), ref["vertices"].shape[2])
            assert poly.dtype == np.int32 and poly.shape == (kept, 2) and np.array_equal(poly, ref["vertices"][n, i, :kept])


def check_labels(lab, max_regions=None, max_vertices=None):
    out = []
    for conn in (1, 2):
        ct = G.contour_labels(lab, max_regions=max_regions, connectivity=conn, max_vertices=max_vertices)
        ref = CR.contour_labels(lab, max_regions, conn, max_vertices)
        assert_contour(ct, ref)
        out.append((ct, ref))
    return out


def rows_of(ct, image=0):
    return [tuple(r) for r in _np(ct.contour)[image].tolist()]


def ring_of(ct, k, image=0):
    n = int(ct.contour[image, k, 0])
    return [tuple(v) for v in _np(ct.vertices)[image, k, :n].tolist()]


def test_hand_cases(dev):
    one = np.ones((1, 1), np.int32)
    sq = np.zeros((7, 7), np.int32)
    sq[1:6, 1:6] = 1
    frame = np.ones((3, 3), np.int32)
    frame[1, 1] = 0
    for (ct, _) in check_labels(one):
        assert rows_of(ct) == [(4, 4, 2, 4)] and ring_of(ct, 0) == [(0, 0), (0, 1), (1, 1), (1, 0)] and bool(ct.is_simple()[0, 0])
    for (ct, _) in check_labels(sq):
        assert rows_of(ct) == [(4, 20, 50, 20)] and ring_of(ct, 0) == [(1, 1), (1, 6), (6, 6), (6, 1)]
        assert float(ct.enclosed_area()[0, 0]) == 25.0 and float(ct.hole_area()[0, 0]) == 0.0
    for (ct, _) in check_labels(frame):
        assert rows_of(ct) == [(4, 12, 18, 16)] and float(ct.hole_area()[0, 0]) == 1.0 and not bool(ct.is_simple()[0, 0])
    (c1, _), (c2, _) = check_labels(PINCH)
    assert rows_of(c1)[0] == (4, 4, 2, 12) and ring_of(c1, 0) == [(0, 0), (0, 1), (1, 1), (1, 0)]
    assert rows_of(c2)[0] == (10, 12, 8, 12) and ring_of(c2, 0) == PINCH_RING2
    assert _np(c1.is_simple())[0].tolist() == [False, True] and _np(c2.is_simple())[0].tolist() == [True, True]
    assert rows_of(c1)[1] == rows_of(c2)[1] == (4, 6, 4, 6) and ring_of(c1, 1) == [(0, 2), (0, 3), (2, 3), (2, 2)]


@pytest.mark.parametrize("hw", [(1, 1), (1, 64), (2, 63), (3, 65), (5, 129), (70, 90)])
def test_random_disconnected_labels(dev, hw):
    lab = SR.random_labels(2, hw[0], hw[1], seed=hw[0] * 131 + hw[1])
    got = check_labels(lab)
    if hw == (70, 90):                                                    # pieces and holes are there, and boxes wider than 64
        ref = got[0][1]
        assert not CR.is_simple(ref).all() and (ref["bbox"][:, :, 3] - ref["bbox"][:, :, 1]).max() > 64
        assert (CR.hole_area(ref)[ref["area"] > 0] < 0).any()
    check_labels(lab[0])
    check_labels(np.zeros(hw, np.int32))


def _comb_and_staircase(width, transpose):
    """label 1: a comb whose box is `width` columns wide (a bar with a tooth under every other pixel); label 2: a staircase of
    two-pixel steps whose box is `width` columns wide; label 3: a dot.  Transposed, the same in rows."""
    lab = np.zeros((width + 7, width + 2), np.int32)
    lab[1, 1:1 + width] = 1
    lab[2:4, 1:1 + width:2] = 1
    for i in range(width - 1):
        lab[5 + i, 1 + i:3 + i] = 2
    lab[-1, 0] = 3
    return np.ascontiguousarray(lab.T) if transpose else lab


@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("width", [31, 32, 33, 63, 64, 65])
def test_bit_word_edges(dev, width, transpose):
    lab = _comb_and_staircase(width, transpose)
    for ct, ref in check_labels(lab):
        side = 2 if transpose else 3
        assert (ref["bbox"][0, :2, side] - ref["bbox"][0, :2, side - 2]).tolist() == [width, width]
        assert rows_of(ct)[0][0] == 2 * width + 2 and rows_of(ct)[1][0] == 4 * (width - 1) and _np(ct.is_simple()).all()


@pytest.mark.parametrize("hw", [(1, 64), (64, 1), (2, 64), (64, 64)])
def test_objects_that_fill_the_image(dev, hw):
    for ct, _ in check_labels(np.ones(hw, np.int32)):
        h, w = hw
        assert rows_of(ct) == [(4, 2 * (h + w), 2 * h * w, 2 * (h + w))] and ring_of(ct, 0) == [(0, 0), (0, w), (h, w), (h, 0)]


def _frame(side, pad=1):
    lab = np.zeros((side + 2 * pad, side + 2 * pad), np.int32)
    lab[pad:pad + side, pad:pad + side] = 1
    lab[pad + 1:pad + side - 1, pad + 1:pad + side - 1] = 0
    lab[0, 0] = 2
    return lab


def test_side_limit(dev):
    assert K.REGIONS_CONTOUR_MAX_SIDE == CR.MAX_SIDE == 512
    for ct, _ in check_labels(_frame(512)):
        assert rows_of(ct) == [(4, 4 * 512, 2 * 512 * 512, 8 * 512 - 8), (4, 4, 2, 4)] and not bool(ct.too_large().any())
        assert ring_of(ct, 0) == [(1, 1), (1, 513), (513, 513), (513, 1)] and float(ct.hole_area()[0, 0]) == 510.0 ** 2
    for ct, _ in check_labels(_frame(513)):
        assert rows_of(ct) == [(-1,) * 4, (4, 4, 2, 4)] and _np(ct.too_large()).tolist() == [[True, False]]
        assert int(ct.table.area[0, 0]) == 4 * 512 and _np(ct.table.bbox)[0, 0].tolist() == [1, 1, 514, 514]
        assert bool((ct.vertices[0, 0] == -1).all()) and np.isnan(_np(ct.n_vertices())[0, 0]) and not bool(ct.is_simple()[0, 0])
        assert ct.per_image()[0]["too_large"].tolist() == [True, False] and len(ct.per_image()[0]["polygon"][0]) == 0


def test_vertex_capacity_and_region_capacity(dev):
    comb = np.zeros((6, 24), np.int32)
    comb[1, 2:21] = 1
    comb[2:5, 2:21:2] = 1                                                 # 10 teeth: 4 + 4 * 9 = 40 vertices
    comb[5, 23] = 2
    for ct, ref in check_labels(comb, max_vertices=8):
        assert rows_of(ct)[0][0] == 40 and _np(ct.truncated()).tolist() == [[True, False]]
        assert np.array_equal(_np(ct.vertices)[0, 0], np.asarray(ref["rings"][0][0][:8]))
        assert np.array_equal(_np(ct.vertices)[0, 1], [[5, 23], [5, 24], [6, 24], [6, 23]] + [[-1, -1]] * 4)
        assert len(ct.per_image()[0]["polygon"][0]) == 8
    for ct, ref in check_labels(comb):                                    # max_vertices=None: exactly the largest count
        assert ct.max_vertices == 40 and not bool(ct.truncated().any()) and ring_of(ct, 0) == ref["rings"][0][0]
    for ct, _ in check_labels(comb, max_vertices=0):                      # counting only
        assert tuple(ct.vertices.shape) == (1, 2, 0, 2) and rows_of(ct)[0][0] == 40
    for ct, _ in check_labels(np.zeros((1, 2, 3), np.int32)):             # nothing to trace: still 4 slots
        assert ct.max_vertices == 4
    lab = SR.random_labels(2, 40, 70, seed=8, top=9)
    lab[lab == 4] = 0                                                     # a label without a pixel inside the range
    fulls = {conn: CR.contour_labels(lab, None, conn) for conn in (1, 2)}
    assert fulls[1]["capacity"] == 9 and not fulls[1]["contour"][:, 3].any()
    for cap in (1, 3, 14):
        for ct, ref in check_labels(lab, max_regions=cap, max_vertices=12):
            k, full = min(cap, 9), fulls[ct.connectivity]
            assert np.array_equal(_np(ct.contour)[:, :k], full["contour"][:, :k]) and not _np(ct.contour)[:, k:].any()
            assert np.array_equal(_np(ct.table.counts), full["counts"]) and bool((ct.vertices[:, k:] == -1).all())


def test_the_box_defines_the_object(dev):
    """a table whose box for label 1 is one row and one column smaller than the object: the object is what lies in the box"""
    lab = np.zeros((20, 30), np.int32)
    lab[SR.disc(20, 30, (9, 12), 7)] = 1
    lab[2:8, 10:13] = 0                                                   # a notch from the top
    lab[15:19, 22:28] = 2
    t = torch.from_numpy(lab).to(dev)
    table = G.measure_labels(t)
    bbox = table.bbox.clone()
    bbox[0, 0, 2] -= 1
    bbox[0, 0, 3] -= 1
    cut = G.RegionTable(table.counts, table.capacity, table.area, bbox, table.sum_rc)
    for conn in (1, 2):
        ref = CR.contour_labels(lab, None, conn, None, bbox=_np(bbox))
        own = CR.contour_labels(lab, None, conn, None)
        ct = G.contour_labels(t, table=cut, connectivity=conn)
        ref["bbox"] = _np(bbox)                                           # the table handed in is the table handed back
        assert_contour(ct, ref)
        rows, cols = int(bbox[0, 0, 2] - bbox[0, 0, 0]), int(bbox[0, 0, 3] - bbox[0, 0, 1])
        assert not ref["hit_bound"].any() and int(ct.contour[0, 0, 1]) == int(ref["contour"][0, 0, 1]) < 2 * rows * cols + rows + cols
        assert ref["contour"][0, 0].tolist() != own["contour"][0, 0].tolist() and ref["contour"][0, 1].tolist() == own["contour"][0, 1].tolist()
        inside = [(r, c) for r, c in ring_of(ct, 0)]
        assert max(r for r, _ in inside) <= int(bbox[0, 0, 2]) and max(c for _, c in inside) <= int(bbox[0, 0, 3])
        # a box that reaches over the image is cut to it; one that misses the label gives an all-zero row
        wild = table.bbox.clone()
        wild[0, 0] = torch.tensor([-5, -7, 99, 99], dtype=torch.int32)
        wild[0, 1] = torch.tensor([0, 0, 3, 3], dtype=torch.int32)
        got = G.contour_labels(t, table=G.RegionTable(table.counts, table.capacity, table.area, wild, table.sum_rc), connectivity=conn)
        assert np.array_equal(_np(got.contour)[0, 0], own["contour"][0, 0]) and not _np(got.contour)[0, 1].any()
        assert bool((got.vertices[0, 1] == -1).all())


@pytest.mark.parametrize("conn", [1, 2])
def test_round_trip_against_scipy_fill(dev, conn):
    from scipy import ndimage
    cross, full = ndimage.generate_binary_structure(2, 1), ndimage.generate_binary_structure(2, 2)
    own, other = (cross, full) if conn == 1 else (full, cross)
    m = SR.random_labels(2, 70, 90, seed=21 + conn) > 1
    lab = G.label(m, conn)
    ct = G.contour_labels(lab, connectivity=conn)
    labels, contour, simple = _np(lab), _np(ct.contour), _np(ct.is_simple())
    seen = 0
    for n in range(2):
        assert np.array_equal(labels[n], ndimage.label(m[n], structure=own)[0])
        for k in range(int(ct.table.counts[n])):
            comp = labels[n] == k + 1
            filled = ndimage.binary_fill_holes(comp, structure=other)
            assert np.array_equal(CR.fill(ring_of(ct, k, n), comp.shape), filled), (n, k)
            assert contour[n, k, 2] == 2 * filled.sum() and simple[n, k] == np.array_equal(filled, comp)
            seen += 1
    assert seen > 20 and simple.any() and not simple[_np(ct.table.area) > 0].all()
    # labels in several pieces: simple exactly where the label is its first component and that component has no hole
    lab = SR.random_labels(1, 70, 90, seed=31)[0]
    ct = G.contour_labels(lab, connectivity=conn)
    for k in range(ct.table.capacity):
        comp, _ = ndimage.label(lab == k + 1, structure=own)
        first = comp == comp.ravel()[np.flatnonzero((lab == k + 1).ravel())[0]]
        filled = ndimage.binary_fill_holes(first, structure=other)
        assert np.array_equal(CR.fill(ring_of(ct, k), lab.shape), filled)
        assert bool(ct.is_simple()[0, k]) == (np.array_equal(filled, first) and np.array_equal(first, lab == k + 1))


@pytest.mark.parametrize("name", NAMES)
def test_golden_scipy_vectors(dev, name):
    lab = GOLD[f"{name}.labels"].astype(np.int32)
    for conn in (1, 2):
        ct = G.contour_labels(lab, connectivity=conn)
        filled = GOLD[f"{name}.filled{conn}"].astype(bool)
        assert ct.table.capacity == len(filled) and np.array_equal(_np(ct.contour)[0, :, 3], GOLD[f"{name}.cracks_all"])
        for k in range(len(filled)):
            assert int(ct.contour[0, k, 2]) == 2 * filled[k].sum()
            if filled[k].any():
                assert np.array_equal(CR.fill(ring_of(ct, k), lab.shape), filled[k])


def test_masks_tables_chunks_and_buffers(dev, monkeypatch):
    m = SR.random_labels(3, 40, 70, seed=9) > 1
    for conn in (1, 2):
        ct = G.contours(m, connectivity=conn)
        assert_contour(ct, CR.contours(m, conn))
        plain = G.measure(m, connectivity=conn)                          # row k is row k of measure(m)
        for name in INT_TABLES:
            assert torch.equal(getattr(ct.table, name), getattr(plain, name)), name
        assert torch.equal(ct.table.counts, plain.counts)
    assert_contour(G.contours(m, max_regions=5, max_vertices=6), CR.contours(m, 1, 5, 6))
    lab = torch.from_numpy(SR.random_labels(3, 40, 70, seed=9)).to(dev)
    lab[1] = 0                                                            # an image without objects inside the batch
    table = G.measure_labels(lab, max_regions=7)
    ct = G.contour_labels(lab, table=table, connectivity=2, max_vertices=10)
    ref = CR.contour_labels(_np(lab), 7, 2, 10)
    assert ct.table is table
    assert_contour(ct, ref)
    monkeypatch.setattr(G, "_MAX_PIXELS", 2 * 40 * 70 + 5)                # two images per call: 2 + 1
    assert [b - a for a, b in G._chunks(torch.empty(3, 40, 70))] == [2, 1]
    assert_contour(G.contour_labels(lab, table=table, connectivity=2, max_vertices=10), ref)
    assert_contour(G.contour_labels(lab, max_regions=7, connectivity=2), CR.contour_labels(_np(lab), 7, 2))
    with pytest.raises(ValueError):
        G.contour_labels(lab, table=table, max_regions=8)
    with pytest.raises(ValueError):
        G.contour_labels(lab[:1], table=table)
    # a caller's buffers: written inside their views only
    cap, maxv, pad = 3, 5, 16
    ref = CR.contour_labels(_np(lab), cap, 1, maxv)
    nc, nv = 3 * cap * 4, 3 * cap * maxv * 2
    bc = torch.full((nc + 2 * pad,), 77, dtype=torch.int32, device=dev)
    bv = torch.full((nv + 2 * pad,), 77, dtype=torch.int32, device=dev)
    vc, vv = bc[pad:pad + nc].view(3, cap, 4), bv[pad:pad + nv].view(3, cap, maxv, 2)
    bbox = torch.from_numpy(ref["bbox"]).to(dev)
    got = K.regions_contour_labels(lab, cap, bbox, 1, maxv, contour=vc, vertices=vv)
    assert got[0] is vc and got[1] is vv
    for buf, n in ((bc, nc), (bv, nv)):
        assert bool((buf[:pad] == 77).all()) and bool((buf[pad + n:] == 77).all())
    assert np.array_equal(_np(vc), ref["contour"]) and np.array_equal(_np(vv), ref["vertices"])
    only, none = K.regions_contour_labels(lab, cap, bbox, 1, 0)
    assert none is None and np.array_equal(_np(only), ref["contour"])
    with pytest.raises(RuntimeError):
        K.regions_contour_labels(lab, cap, bbox, 3, maxv)                 # connectivity: refused, nothing launched
    with pytest.raises(TypeError):
        K.regions_contour_labels(lab, cap, bbox[:, :2], 1, maxv)          # a table of another capacity
    with pytest.raises(TypeError):
        K.regions_contour_labels(lab, cap, bbox, 1, maxv, vertices=vv[:, :, :4])
    with pytest.raises(ValueError):
        K.regions_contour_labels(lab, cap, bbox, 1, -1)


def test_negative_labels_are_background(dev):
    lab = SR.random_labels(1, 20, 70, seed=3)[0]
    lab[lab <= 0] = np.where(np.indices(lab.shape).sum(0) % 2, 0, -3)[lab <= 0]
    (ct, ref), _ = check_labels(lab)
    assert (lab == -3).any() and (lab == 0).any()
    assert_contour(G.contour_labels(np.maximum(lab, 0)), ref)


def test_graph_replay(dev):
    lab = SR.random_labels(3, 70, 90, seed=12, top=20)
    other = SR.random_labels(3, 70, 90, seed=13, top=20)
    cap, maxv = 18, 8                                                   # below the largest label and the longest ring
    static = torch.zeros((3, 70, 90), dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        G.contour_labels(static, max_regions=cap, connectivity=2, max_vertices=maxv)   # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ct = G.contour_labels(static, max_regions=cap, connectivity=2, max_vertices=maxv)
    for contents in (lab, other):
        static.copy_(torch.from_numpy(contents).to(dev))
        graph.replay()
        eager = G.contour_labels(contents, max_regions=cap, connectivity=2, max_vertices=maxv)
        assert _np(ct.contour).tobytes() == _np(eager.contour).tobytes() and _np(ct.vertices).tobytes() == _np(eager.vertices).tobytes()
        ref = CR.contour_labels(contents, cap, 2, maxv)
        assert CR.truncated(ref).any()
        assert_contour(ct, ref)


def test_geojson_of_device_tables(dev):
    ct = G.contour_labels(PINCH, connectivity=2)
    doc = ct.geojson(origin=(100, 200), scale=0.5, properties={"solidity": torch.tensor([0.25, 1.0], device=dev)})
    assert doc["type"] == "FeatureCollection" and [f["properties"] for f in doc["features"]] == [
        {"row": 0, "area": 4, "solidity": 0.25}, {"row": 1, "area": 2, "solidity": 1.0}]
    ring = doc["features"][0]["geometry"]["coordinates"][0]
    assert ring == [[100 + 0.5 * c, 200 + 0.5 * r] for r, c in PINCH_RING2 + PINCH_RING2[:1]]


def test_measure_cells_with_contours_end_to_end_resnet18(dev):
    from cellsegmentation_amd import inference, synth
    from cellsegmentation_amd.model import resnet as RN
    m = RN.MILresnet18()
    sd = m.state_dict()
    synth.fill_state_dict(sd)
    m.load_state_dict(sd)
    m = m.to(dev).set_compute_dtype(torch.float32)
    m.setmode("segment")
    x = synth.normalise(synth.ihc_tiles(4, 299, seed=23))
    loader = [x[:3], x[3:]]
    probs = inference.inference_seg(loader, m, dev, mode="test")
    thr = float(np.median(probs))                                        # a threshold that splits this model's output
    classes = _np(inference.segment_classes(loader, m, dev, thr, 40, 15))
    assert classes.any()
    batches = (classes[:3], classes[3:])
    keys = {"contour", "polygon", *BOOLS, *CR.COLUMNS}
    renamed = (keys - {"n_vertices", "too_large"}) | {"contour_n_vertices", "contour_too_large"}
    for kw, maxv in (({}, None), ({"max_regions": 3}, 6)):
        refs = [CR.contours(b, 1, kw.get("max_regions"), maxv) for b in batches]     # every batch sizes its own tables
        plain = inference.measure_cells(loader, m, dev, thr, 40, 15, **kw)
        got = inference.measure_cells(loader, m, dev, thr, 40, 15, contours=True, max_vertices=maxv, **kw)
        hulled = inference.measure_cells(loader, m, dev, thr, 40, 15, hull=True, **kw)
        both = inference.measure_cells(loader, m, dev, thr, 40, 15, hull=True, contours=True, max_vertices=maxv, **kw)
        assert len(got) == len(plain) == len(both) == 4
        for n, (g, p, h, b) in enumerate(zip(got, plain, hulled, both)):
            assert set(g) == set(p) | keys and set(b) == set(h) | renamed
            for k in p:                                                   # the old keys: bit for bit
                assert g[k].dtype == p[k].dtype and g[k].shape == p[k].shape and g[k].tobytes() == p[k].tobytes(), k
            for k in h:                                                   # the hull keeps n_vertices and too_large
                assert b[k].tobytes() == h[k].tobytes(), k
            assert b["contour_n_vertices"].tobytes() == g["n_vertices"].tobytes()
            assert b["contour_too_large"].tobytes() == g["too_large"].tobytes()
            ref, i, rows = refs[n // 3], n % 3, len(p["area"])
            assert rows == min(int(ref["counts"][i]), ref["capacity"])
            assert np.array_equal(g["area"], ref["area"][i, :rows]) and np.array_equal(g["contour"], ref["contour"][i, :rows])
            for name, col in CR.columns(ref).items():
                assert np.array_equal(g[name], col[i, :rows], equal_nan=True), name
            for k in range(rows):
                kept = min(int(ref["contour"][i, k, 0]), ref["vertices"].shape[2])
                assert np.array_equal(g["polygon"][k], ref["vertices"][i, k, :kept]) and np.array_equal(b["polygon"][k], g["polygon"][k])
    assert sum(len(g["area"]) for g in got) >= 1 and m.mode == "segment"
