"""The per-label convex hull on the GPU (hull_kernel of csrc/regions.hip through cellsegmentation_amd.regions.hull_labels and hull)
against the Python-integer restatement tests/hull_ref.py and the qhull vectors of tests/golden/hull_vectors.npz.  The integer table
is compared by value.  The float64 columns are compared at rtol = 1e-13: each is at most three float64 operations (a conversion is
exact, the integers are below 2^53) of at most 1 ulp each, so the error is <= 3 * 2^-52 ~ 7e-16; the tolerance leaves two orders
over that for a device sqrt or division that is not correctly rounded.  The worst difference seen is printed."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import hull_ref as HR  # noqa: E402
import shape_ref as SR  # noqa: E402
from cellsegmentation_amd import kernels as K  # noqa: E402
from cellsegmentation_amd import regions as G  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "hull_vectors.npz"), allow_pickle=False)
NAMES = sorted(k[:-len(".labels")] for k in GOLD.files if k.endswith(".labels"))
INT_TABLES = {"area": torch.int32, "bbox": torch.int32, "sum_rc": torch.int64}
RTOL = 1e-13


def _np(t):
    return t.cpu().numpy()


def assert_close(got, want, what):
    """float64 columns: NaN in the same places, everything else within RTOL"""
    assert got.shape == want.shape and got.dtype == np.float64, what
    worst = 0.0
    both = np.isfinite(got) & np.isfinite(want) & (want != 0)
    if both.any():
        worst = float(np.max(np.abs(got[both] - want[both]) / np.abs(want[both])))
    print(f"{what}: worst relative difference {worst:.3e}")
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=0, equal_nan=True, err_msg=what)


def assert_hull(ht, ref):
    """a HullTable against the restatement's dict: integers by value, floats at RTOL, per_image trimmed"""
    assert isinstance(ht, G.HullTable) and isinstance(ht.table, G.RegionTable) and ht.table.capacity == ref["capacity"]
    assert np.array_equal(_np(ht.table.counts), ref["counts"])
    for name, dtype in INT_TABLES.items():
        got = getattr(ht.table, name)
        assert got.dtype == dtype and got.is_cuda and np.array_equal(_np(got), ref[name]), name
    assert ht.hull.dtype == torch.int32 and ht.hull.is_cuda and tuple(ht.hull.shape) == ref["hull"].shape
    assert np.array_equal(_np(ht.hull), ref["hull"])
    big = ht.too_large()
    assert big.dtype == torch.bool and big.is_cuda and np.array_equal(_np(big), HR.too_large(ref))
    want = HR.columns(ref)
    unmeasured = (ref["area"] == 0) | HR.too_large(ref)
    for name in HR.COLUMNS:
        got = getattr(ht, name)()
        assert got.dtype == torch.float64 and got.is_cuda, name
        got = _np(got)
        assert np.isnan(got[unmeasured]).all() and not np.isnan(got[~unmeasured]).any(), name
        assert_close(got, want[name], name)
    s = _np(ht.solidity())[~unmeasured]
    assert (s > 0).all() and (s <= 1).all()
    per = ht.per_image()
    assert len(per) == len(ref["counts"])
    for n, d in enumerate(per):
        k = min(int(ref["counts"][n]), ref["capacity"])
        assert {"area", "bbox", "centroid", "hull", "too_large", *HR.COLUMNS} <= set(d)
        assert np.array_equal(d["area"], ref["area"][n, :k]) and np.array_equal(d["hull"], ref["hull"][n, :k])
        assert np.array_equal(d["too_large"], HR.too_large(ref)[n, :k])
        for name in HR.COLUMNS:
            assert_close(d[name], want[name][n, :k], f"per_image {name}")


def check_labels(lab, max_regions=None):
    ht = G.hull_labels(lab, max_regions=max_regions)
    ref = HR.hull_labels(lab, max_regions)
    assert_hull(ht, ref)
    return ht, ref


def rows_of(ht, image=0):
    return [tuple(r) for r in _np(ht.hull)[image].tolist()]


@pytest.mark.parametrize("hw", [(1, 1), (1, 64), (2, 63), (3, 65), (5, 129), (70, 90)])
def test_wide_boxes_and_disconnected_labels(dev, hw):
    lab = SR.random_labels(2, hw[0], hw[1], seed=hw[0] * 131 + hw[1])
    _, ref = check_labels(lab)
    if hw[0] * hw[1] > 64:
        assert (ref["counts"] >= 2).all()
    if hw == (70, 90):                                                    # empty rows inside a box, boxes wider than a wave's stride
        rows = np.unique(np.nonzero(lab[0] == 1)[0])
        assert len(rows) < rows.max() - rows.min() + 1 and (ref["bbox"][:, :, 3] - ref["bbox"][:, :, 1]).max() > 64
    check_labels(lab[0])
    check_labels(np.ones((1,) + hw, np.int32))
    check_labels(np.zeros(hw, np.int32))


def test_ring_round_a_dot_and_notched_shapes(dev):
    ring = np.zeros((24, 26), np.int32)
    ring[SR.disc(24, 26, (12, 13), 10)] = 1
    ring[SR.disc(24, 26, (12, 13), 6)] = 0
    ring[11:14, 12:15] = 2                                                # nested boxes: the dot lies inside the ring's
    ht, ref = check_labels(ring)
    filled = HR.hull_labels(SR.disc(24, 26, (12, 13), 10).astype(np.int32))
    assert rows_of(ht) == [tuple(filled["hull"][0, 0]), (4, 18, 18, 9, 9)]  # the ring's hull is the disc's: the hole plays no part
    shapes = np.zeros((12, 150), np.int32)
    shapes[1:8, 1:8] = 1
    shapes[3:5, 3:8] = 0                                                  # a C: the notch's corners are no vertices
    shapes[1:8, 60:62] = 2
    shapes[6:8, 60:67] = 2                                                # an L across column 64
    shapes[1:8, 100:107] = 3
    shapes[3:5, 100:105] = 0                                              # a C open to the left
    ht, _ = check_labels(shapes)
    assert rows_of(ht) == [(4, 98, 98, 49, 49), (5, 73, 98, 45, 50), (4, 98, 98, 49, 49)]
    assert _np(ht.solidity())[0].tolist() == [39 / 49, 24 / 36.5, 39 / 49]


def test_collinear_candidates(dev):
    lab = np.zeros((70, 80), np.int32)
    for i in range(30):
        lab[2 + i, 3 + 2 * i:5 + 2 * i] = 1                              # a staircase of slope 2: every step's corners are collinear
    lab[40:44, :] = 2                                                     # full-width rectangles
    lab[50:70, :] = 3
    lab[np.arange(33, 39), np.arange(70, 76)] = 4                         # the 6-pixel diagonal
    ht, _ = check_labels(lab)
    rows = rows_of(ht)
    assert rows[0][0] == 6 and rows[1] == (4, 2 * 4 * 80, 16 + 6400, 320, 6400) and rows[2] == (4, 2 * 20 * 80, 400 + 6400, 1600, 6400)
    assert rows[3] == (6, 22, 72, 10, 50)
    assert _np(ht.solidity())[0, 1:3].tolist() == [1.0, 1.0]
    for a, b in [(1, 1), (1, 7), (4, 1), (6, 11), (3, 70)]:
        m = np.zeros((a + 3, b + 5), np.int32)
        m[2:2 + a, 1:1 + b] = 1
        ht, _ = check_labels(m)
        assert rows_of(ht) == [(4, 2 * a * b, a * a + b * b, a * b, max(a, b) ** 2)] and float(ht.solidity()[0, 0]) == 1.0


def test_borders_abutting_labels_and_images(dev):
    lab = np.zeros((3, 20, 140), np.int32)
    lab[0, 0, 5:9] = 1                                                    # objects on all four borders of the image
    lab[0, 0:3, 6] = 1
    lab[0, 17:20, 100:139] = 2
    lab[0, 19, 90:140] = 2
    lab[0, 4:15, 0] = 3
    lab[0, 8, 0:4] = 3
    lab[0, 3:9, 139] = 4
    lab[0, 6, 130:140] = 4
    lab[0, 5:12, 30:64] = 5                                               # two labels abut at column 64
    lab[0, 5:12, 64:99] = 6
    lab[1] = lab[0]                                                       # identical labels in different images
    lab[2, 19, 5:9] = 1                                                   # the same label in the last row of one image ...
    lab[2, 2:4, 64:70] = 6
    ht, ref = check_labels(lab)
    assert rows_of(ht, 0) == rows_of(ht, 1) and rows_of(ht, 0)[4] == (4, 2 * 7 * 34, 49 + 34 * 34, 7 * 34, 34 * 34)
    assert rows_of(ht, 2)[0] == (4, 8, 17, 4, 16) and rows_of(ht, 2)[1:5] == [(0,) * 5] * 4   # labels without a pixel
    for i in range(3):
        one = G.hull_labels(lab[i], max_regions=ht.table.capacity)
        assert torch.equal(one.hull[0], ht.hull[i])


def test_negative_labels_are_background(dev):
    lab = SR.random_labels(1, 20, 70, seed=3)[0]
    lab[lab <= 0] = np.where(np.indices(lab.shape).sum(0) % 2, 0, -3)[lab <= 0]
    lab[5:15, 20:40] = -3
    _, ref = check_labels(lab)
    assert (lab == -3).any() and (lab == 0).any()
    assert_hull(G.hull_labels(np.maximum(lab, 0)), ref)


def test_capacity_below_the_labels_and_empty_rows(dev):
    lab = SR.random_labels(2, 40, 70, seed=8, top=9)
    lab[lab == 4] = 0                                                     # a label without a pixel inside the range
    full = HR.hull_labels(lab)
    assert full["capacity"] == 9 and (full["area"][:, 3] == 0).all() and not full["hull"][:, 3].any()
    for cap in (1, 3, 9, 14):
        ht, ref = check_labels(lab, max_regions=cap)
        k = min(cap, 9)
        assert np.array_equal(_np(ht.hull)[:, :k], full["hull"][:, :k]) and not _np(ht.hull)[:, k:].any()
        assert np.array_equal(_np(ht.table.overflowed()), full["counts"] > cap)
        assert np.array_equal(_np(ht.table.counts), full["counts"])     # counts reports the labels that have no row


def test_many_vertices_radius_500(dev):
    """a digital disc of radius 500 in a 1024 x 1024 image: 1001 row extents, 232 vertices.  The pixel squares hold the circle of
    radius 500 round the centre pixel's centre and lie inside the one of radius 500 + sqrt(1 / 2), which bounds both diameters."""
    lab = SR.disc(1024, 1024, (511, 512), 500).astype(np.int32)
    ht, ref = check_labels(lab, max_regions=1)
    n, area2, far2, cross, len2 = rows_of(ht)[0]
    assert n > 200 and n % 4 == 0 and far2 >= 1001 ** 2 and 0.99 < float(ht.solidity()[0, 0]) < 1.0
    assert 1000.0 < float(ht.feret_diameter_min()[0, 0]) <= 1001.0 <= float(ht.feret_diameter_max()[0, 0]) < 1001.5


@pytest.mark.parametrize("shape", [(1025, 3), (3, 1025)])
def test_side_limit(dev, shape):
    long = 0 if shape[0] > 3 else 1
    lab = np.zeros(shape, np.int32)
    sl = [slice(0, 1), slice(0, 1)]
    sl[long] = slice(0, 1024)
    lab[tuple(sl)] = 1                                                    # a line of exactly 1024 pixels: measured
    lab[-1, -1] = 2
    ht, _ = check_labels(lab)
    assert rows_of(ht) == [(4, 2048, 1024 ** 2 + 1, 1024, 1024 ** 2), (4, 2, 2, 1, 1)] and not bool(ht.too_large().any())
    whole = np.ones(shape, np.int32)                                      # 1025 long: counted, not measured
    whole[1, 1] = 2
    ht, ref = check_labels(whole)
    assert rows_of(ht) == [(-1,) * 5, (4, 2, 2, 1, 1)] and _np(ht.too_large()).tolist() == [[True, False]]
    assert int(ht.table.area[0, 0]) == 3 * 1025 - 1 and np.isnan(_np(ht.solidity())[0, 0]) and np.isnan(_np(ht.n_vertices())[0, 0])
    assert ht.per_image()[0]["too_large"].tolist() == [True, False]


def test_masks_tables_and_buffers_handed_in(dev):
    m = SR.random_labels(2, 40, 70, seed=9) > 1
    for conn in (1, 2):
        ht = G.hull(m, connectivity=conn)
        assert_hull(ht, HR.hull(m, conn))
        lab = G.label(m, conn)
        assert torch.equal(ht.hull, G.hull_labels(lab).hull)
    assert_hull(G.hull(m, max_regions=5), HR.hull(m, 1, 5))
    lab = torch.from_numpy(SR.random_labels(2, 40, 70, seed=9)).to(dev)
    table = G.measure_labels(lab, max_regions=7)
    ht = G.hull_labels(lab, table=table)
    assert ht.table is table
    assert_hull(ht, HR.hull_labels(_np(lab), 7))
    assert torch.equal(ht.hull, G.hull_labels(lab, max_regions=7).hull)
    assert_hull(G.hull_labels(lab, table=table, max_regions=7), HR.hull_labels(_np(lab), 7))
    host = G.RegionTable(table.counts.cpu(), 7, table.area.cpu(), table.bbox.cpu(), table.sum_rc.cpu())
    with pytest.raises(ValueError, match="RegionTable"):
        G.hull_labels(lab, table=host)
    with pytest.raises(ValueError):
        G.hull_labels(lab, table=table, max_regions=8)
    with pytest.raises(ValueError):
        G.hull_labels(lab[:1], table=table)
    # a caller's buffer: written inside its view only
    cap, pad = 3, 16                                                      # below the largest label: its rows exist nowhere
    ref = HR.hull_labels(_np(lab), cap)
    assert (ref["counts"] > cap).all()
    n = 2 * cap * 5
    buf = torch.full((n + 2 * pad,), 77, dtype=torch.int32, device=dev)
    view = buf[pad:pad + n].view(2, cap, 5)
    bbox = torch.from_numpy(ref["bbox"]).to(dev)
    assert K.regions_hull_labels(lab, cap, bbox, hull=view) is view
    assert bool((buf[:pad] == 77).all()) and bool((buf[pad + n:] == 77).all()) and np.array_equal(_np(view), ref["hull"])
    with pytest.raises(RuntimeError):
        K.regions_hull_labels(lab, 0, bbox[:, :0])                        # capacity < 1: refused, nothing launched
    with pytest.raises(TypeError):
        K.regions_hull_labels(lab, cap, bbox[:, :2])                      # a table of another capacity
    with pytest.raises(TypeError):
        K.regions_hull_labels(lab, cap, bbox, hull=view.to(torch.int64))
    with pytest.raises(TypeError):
        K.regions_hull_labels(lab.to(torch.int64), cap, bbox)


def test_batches_and_chunks(dev, monkeypatch):
    lab = SR.random_labels(5, 40, 70, seed=11)
    lab[1] = 0                                                            # an image without objects inside the batch
    ref = HR.hull_labels(lab)
    assert_hull(G.hull_labels(lab), ref)
    monkeypatch.setattr(G, "_MAX_PIXELS", 2 * 40 * 70 + 5)                # two images per call: 2 + 2 + 1
    assert [b - a for a, b in G._chunks(torch.empty(5, 40, 70))] == [2, 2, 1]
    assert_hull(G.hull_labels(lab), ref)
    assert_hull(G.hull_labels(lab, max_regions=3), HR.hull_labels(lab, 3))


def test_graph_replay(dev):
    lab = SR.random_labels(3, 70, 90, seed=12, top=20)
    other = SR.random_labels(3, 70, 90, seed=13, top=20)
    cap = 18                                                              # below the largest label
    static = torch.zeros((3, 70, 90), dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        G.hull_labels(static, max_regions=cap)                            # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ht = G.hull_labels(static, max_regions=cap)
    for contents in (lab, other):
        static.copy_(torch.from_numpy(contents).to(dev))
        graph.replay()
        eager = G.hull_labels(contents, max_regions=cap)
        assert _np(ht.hull).tobytes() == _np(eager.hull).tobytes()
        assert_hull(ht, HR.hull_labels(contents, cap))


@pytest.mark.parametrize("name", NAMES)
def test_golden_qhull_vectors(dev, name):
    lab = GOLD[f"{name}.labels"].astype(np.int32)
    ht = G.hull_labels(lab)
    assert ht.table.capacity == len(GOLD[f"{name}.hull"]) and np.array_equal(_np(ht.hull)[0], GOLD[f"{name}.hull"])
    if name in ("blobs", "square5", "disc20", "pixel", "line7"):          # label images that are scipy's labelling of their foreground
        assert np.array_equal(_np(G.hull(lab > 0).hull)[0], GOLD[f"{name}.hull"])


def test_measure_cells_with_hull_end_to_end_resnet18(dev):
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
    hull_keys = {"hull", "too_large", *HR.COLUMNS}
    for kw in ({}, {"max_regions": 3}):
        refs = [HR.hull(b, 1, kw.get("max_regions")) for b in batches]     # every batch sizes its own tables
        plain = inference.measure_cells(loader, m, dev, thr, 40, 15, **kw)
        shaped = inference.measure_cells(loader, m, dev, thr, 40, 15, shape=True, **kw)
        got = inference.measure_cells(loader, m, dev, thr, 40, 15, hull=True, **kw)
        both = inference.measure_cells(loader, m, dev, thr, 40, 15, shape=True, hull=True, **kw)
        off = inference.measure_cells(loader, m, dev, thr, 40, 15, hull=False, **kw)
        assert len(got) == len(plain) == len(both) == len(off) == 4
        for n, (g, p, s, b, o) in enumerate(zip(got, plain, shaped, both, off)):
            assert set(g) == set(p) | hull_keys and set(b) == set(s) | hull_keys and set(o) == set(p)
            for k in p:                                                   # the old keys: bit for bit
                assert g[k].dtype == p[k].dtype and g[k].shape == p[k].shape and g[k].tobytes() == p[k].tobytes(), k
                assert o[k].tobytes() == p[k].tobytes(), k
            for k in s:
                assert b[k].dtype == s[k].dtype and b[k].tobytes() == s[k].tobytes(), k
            for k in hull_keys:
                assert b[k].tobytes() == g[k].tobytes(), k
            ref, i, rows = refs[n // 3], n % 3, len(p["area"])
            assert rows == min(int(ref["counts"][i]), ref["capacity"])
            assert np.array_equal(g["area"], ref["area"][i, :rows]) and np.array_equal(g["hull"], ref["hull"][i, :rows])
            for name, col in HR.columns(ref).items():
                assert_close(g[name], col[i, :rows], name)
    assert sum(len(g["area"]) for g in got) >= 1 and m.mode == "segment"
