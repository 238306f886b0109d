"""Shape descriptors on the GPU (edge_kernel / shape_kernel of csrc/regions.hip through cellsegmentation_amd.regions.shape_labels,
shape and boundaries) against the numpy restatement tests/shape_ref.py and the scipy.ndimage vectors of
tests/golden/shape_vectors.npz.  The integer tables and the edge map are compared by value.  The float64 columns are compared at
rtol = 1e-9: for the shapes used here (boxes <= 96 but for exact closed-form cases, areas < 2^14) every integer and every product
formed is below 2^53, so the only loss is the cancellation in S / A - (S / A)^2, bounded by box^2 / variance * 2^-52 < 1e-11; the
tolerance leaves a factor of 100 over that."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import shape_ref as SR  # noqa: E402
from cellsegmentation_amd import kernels as K  # noqa: E402
from cellsegmentation_amd import regions as G  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "shape_vectors.npz"), allow_pickle=False)
NAMES = sorted(k[:-len(".labels")] for k in GOLD.files if k.endswith(".labels"))
INT_TABLES = {"area": torch.int32, "bbox": torch.int32, "sum_rc": torch.int64}
RTOL = 1e-9


def _np(t):
    return t.cpu().numpy()


def assert_close(got, want, what):
    """float64 columns: NaN and inf in the same places, everything else within RTOL"""
    assert got.shape == want.shape and got.dtype == np.float64, what
    worst = 0.0
    both = np.isfinite(got) & np.isfinite(want) & (want != 0)
    if both.any():
        worst = float(np.max(np.abs(got[both] - want[both]) / np.abs(want[both])))
    print(f"{what}: worst relative difference {worst:.3e}")
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=0, equal_nan=True, err_msg=what)


def assert_shape(st, ref):
    """a ShapeTable against the restatement's dict: integers by value, the edge map by value, floats at RTOL, per_image trimmed"""
    assert isinstance(st, G.ShapeTable) and isinstance(st.table, G.RegionTable) and st.table.capacity == ref["capacity"]
    assert np.array_equal(_np(st.table.counts), ref["counts"])
    for name, dtype in INT_TABLES.items():
        got = getattr(st.table, name)
        assert got.dtype == dtype and got.is_cuda and np.array_equal(_np(got), ref[name]), name
    for name, dtype in (("moments", torch.int64), ("tallies", torch.int32)):
        got = getattr(st, name)
        assert got.dtype == dtype and got.is_cuda and tuple(got.shape) == ref[name].shape, name
        assert np.array_equal(_np(got), ref[name]), name
    assert st.edges.dtype == torch.bool and st.edges.is_cuda and tuple(st.edges.shape) == ref["edges"].shape
    assert np.array_equal(_np(st.edges), ref["edges"])
    want = SR.columns(ref)
    unused = ref["area"] == 0
    for name in SR.COLUMNS:
        got = getattr(st, name)()
        assert got.dtype == torch.float64 and got.is_cuda, name
        got = _np(got)
        assert np.isnan(got[unused]).all(), name
        assert_close(got, want[name], name)
    per = st.per_image()
    assert len(per) == len(ref["counts"])
    for n, d in enumerate(per):
        k = min(int(ref["counts"][n]), ref["capacity"])
        assert {"area", "bbox", "centroid", "moments", "tallies", *SR.COLUMNS} <= set(d)
        assert np.array_equal(d["area"], ref["area"][n, :k]) and np.array_equal(d["moments"], ref["moments"][n, :k])
        assert np.array_equal(d["tallies"], ref["tallies"][n, :k])
        for name in SR.COLUMNS:
            assert_close(d[name], want[name][n, :k], f"per_image {name}")


def check_labels(lab, max_regions=None):
    st = G.shape_labels(lab, max_regions=max_regions)
    ref = SR.shape_labels(lab, max_regions)
    assert_shape(st, ref)
    assert torch.equal(G.boundaries(lab), st.edges)
    return st, ref


@pytest.mark.parametrize("hw", [(1, 1), (1, 64), (2, 63), (3, 65), (5, 129), (70, 90)])
def test_segment_ends_borders_and_runs_across_segments(dev, hw):
    lab = SR.random_labels(2, hw[0], hw[1], seed=hw[0] * 131 + hw[1])
    _, ref = check_labels(lab)
    if hw[0] * hw[1] > 64:
        assert ref["edges"].any() and (ref["counts"] >= 2).all()
    check_labels(lab[0])                                                  # [H, W]: the edge map comes back two-dimensional
    check_labels(np.ones((1,) + hw, np.int32))
    check_labels(np.zeros(hw, np.int32))


def test_abutting_labels_and_checkerboards(dev):
    side = np.zeros((6, 140), np.int32)
    side[1:5, 3:64] = 1
    side[1:5, 64:130] = 2                                                 # abut horizontally, at a segment end
    _, ref = check_labels(side)
    assert ref["edges"][2, 63] and ref["edges"][2, 64] and not ref["edges"][2, 62]
    above = np.zeros((8, 9), np.int32)
    above[1:4, 2:7] = 1
    above[4:7, 2:7] = 2                                                   # abut vertically
    _, ref = check_labels(above)
    assert ref["edges"][3, 4] and ref["edges"][4, 4] and ref["tallies"][0, :, 0].tolist() == [12, 12]
    corner = np.zeros((6, 6), np.int32)
    corner[1:3, 1:3] = 1
    corner[3:5, 3:5] = 2                                                  # touch diagonally
    _, ref = check_labels(corner)
    assert ref["tallies"][0].tolist() == [[4, 4, 0, 0]] * 2
    # a diagonal neighbour of another object is not counted: (1, 1) has one diagonal neighbour of its own, code 11, not 21
    _, ref = check_labels(np.asarray([[1, 0, 0], [0, 1, 0], [0, 0, 2]], np.int32))
    assert ref["tallies"][0].tolist() == [[2, 0, 0, 0], [1, 0, 0, 0]]
    st, ref = check_labels(np.asarray([[1, 2], [3, 4]], np.int32))
    assert ref["edges"].all() and _np(st.tallies)[0].tolist() == [[1, 0, 0, 0]] * 4
    board = (np.indices((8, 70)).sum(0) % 2).astype(bool)
    for conn in (1, 2):
        st = G.shape(board, connectivity=conn)
        assert_shape(st, SR.shape(board, conn))
        assert torch.equal(G.boundaries(board, connectivity=conn), st.edges) and bool(st.edges.cpu().numpy()[board].all())
    assert G.shape(board, connectivity=1).table.capacity == 280 and G.shape(board, connectivity=2).table.capacity == 1
    assert _np(G.shape(board, connectivity=1).tallies)[0].tolist() == [[1, 0, 0, 0]] * 280


def test_no_neighbours_across_images(dev):
    lab = np.zeros((3, 4, 70), np.int32)
    lab[0, 3, 5:69] = 1
    lab[1, 0, 5:69] = 1                                                   # the last row of image 0 and the first row of image 1
    lab[1, 3, :] = 2
    lab[2, 0, :] = 2
    st, ref = check_labels(lab)
    assert _np(st.tallies)[0, 0].tolist() == [64, 62, 0, 0] == _np(st.tallies)[1, 0].tolist()
    assert _np(st.tallies)[1, 1].tolist() == [70, 68, 0, 0] == _np(st.tallies)[2, 1].tolist()


def test_labels_of_zero_and_below_are_one_background(dev):
    lab = SR.random_labels(1, 20, 70, seed=3)[0]
    lab[lab <= 0] = np.where(np.indices(lab.shape).sum(0) % 2, 0, -3)[lab <= 0]
    lab[5:15, 20:40] = -3
    lab[8:12, 25:35] = 0
    st, ref = check_labels(lab)
    assert not _np(st.edges)[lab <= 0].any() and (lab == -3).any() and (lab == 0).any()
    assert_shape(G.shape_labels(np.maximum(lab, 0)), ref)


def test_one_object_fills_the_image(dev):
    lab = np.ones((70, 90), np.int32)
    st, ref = check_labels(lab)
    frame = np.ones((70, 90), bool)
    frame[1:-1, 1:-1] = False
    assert np.array_equal(_np(st.edges), frame) and _np(st.tallies)[0, 0].tolist() == [316, 316, 0, 0]
    assert float(st.extent()[0, 0]) == 1.0 and float(st.perimeter()[0, 0]) == 316.0


def test_sums_need_64_bits(dev):
    """a 2 x 3000 stripe: Syy = 2 * sum of y^2 below 3000 = 17 991 001 000 > 2^32; expected values in closed form"""
    W = 3000
    lab = np.zeros((4, W + 7), np.int32)
    lab[1:3, 5:5 + W] = 1
    st = G.shape_labels(lab, max_regions=2)
    syy = 2 * (W - 1) * W * (2 * W - 1) // 6
    assert syy > 2 ** 32
    assert _np(st.moments)[0].tolist() == [[W, syy, W * (W - 1) // 2], [0, 0, 0]]
    assert _np(st.tallies)[0].tolist() == [[2 * W, 2 * W, 0, 0], [0, 0, 0, 0]]     # two rows thick: every pixel is an edge pixel
    mu = _np(st.central_moments())[0, 0]
    np.testing.assert_allclose(mu, [0.25, (W * W - 1) / 12, 0.0], rtol=RTOL, atol=0)
    assert abs(float(st.orientation()[0, 0])) == pytest.approx(np.pi / 2, rel=RTOL)
    ref = SR.shape_labels(lab, 2)
    assert np.array_equal(_np(st.moments), ref["moments"]) and np.array_equal(_np(st.edges), ref["edges"])
    assert np.array_equal(_np(st.tallies), ref["tallies"])


def test_capacity_below_the_labels_and_empty_rows(dev):
    lab = SR.random_labels(2, 40, 70, seed=8, top=9)
    lab[lab == 4] = 0                                                     # a label without a pixel inside the range
    full = SR.shape_labels(lab)
    assert full["capacity"] == 9 and (full["area"][:, 3] == 0).all()
    for cap in (1, 3, 9, 14):
        st, ref = check_labels(lab, max_regions=cap)
        k = min(cap, 9)
        assert np.array_equal(_np(st.moments)[:, :k], full["moments"][:, :k]) and np.array_equal(_np(st.tallies)[:, :k], full["tallies"][:, :k])
        assert not _np(st.moments)[:, k:].any() and not _np(st.tallies)[:, k:].any()
        assert np.array_equal(_np(st.edges), full["edges"])               # the capacity plays no part in the edge rule
        assert np.array_equal(_np(st.table.overflowed()), full["counts"] > cap)
    st = G.shape_labels(lab)
    assert not _np(st.moments)[:, 3].any() and not _np(st.tallies)[:, 3].any() and np.isnan(_np(st.perimeter())[:, 3]).all()


def test_table_handed_in(dev):
    lab = torch.from_numpy(SR.random_labels(2, 40, 70, seed=9)).to(dev)
    table = G.measure_labels(lab, max_regions=7)
    st = G.shape_labels(lab, table=table)
    assert st.table is table
    assert_shape(st, SR.shape_labels(_np(lab), 7))
    assert_shape(G.shape_labels(lab, table=table, max_regions=7), SR.shape_labels(_np(lab), 7))
    host = G.RegionTable(table.counts.cpu(), 7, table.area.cpu(), table.bbox.cpu(), table.sum_rc.cpu())
    with pytest.raises(ValueError, match="RegionTable"):
        G.shape_labels(lab, table=host)
    with pytest.raises(ValueError):
        G.shape_labels(lab, table=table, max_regions=8)
    with pytest.raises(ValueError):
        G.shape_labels(lab[:1], table=table)


def test_tables_are_written_inside_their_views_only(dev):
    lab = SR.random_labels(2, 40, 70, seed=10, top=9)
    d = torch.from_numpy(lab).to(dev)
    N, H, W, cap, pad = 2, 40, 70, 5, 16
    ref = SR.shape_labels(lab, cap)
    assert (ref["counts"] > cap).all()
    shapes = {"edges": ((N, H, W), torch.uint8), "moments": ((N, cap, 3), torch.int64), "tallies": ((N, cap, 4), torch.int32)}
    bufs, views = {}, {}
    for name, (shape, dtype) in shapes.items():
        n = int(np.prod(shape))
        bufs[name] = torch.full((n + 2 * pad,), 77, dtype=dtype, device=dev)
        views[name] = bufs[name][pad:pad + n].view(shape)
    bbox = torch.from_numpy(ref["bbox"]).to(dev)
    assert K.regions_edges_labels(d, edges=views["edges"]) is views["edges"]
    out = K.regions_shape_labels(d, views["edges"], cap, bbox, moments=views["moments"], tallies=views["tallies"])
    assert out[0] is views["moments"] and out[1] is views["tallies"]
    for name, b in bufs.items():
        n = int(np.prod(shapes[name][0]))
        assert bool((b[:pad] == 77).all()) and bool((b[pad + n:] == 77).all()), name
    assert np.array_equal(_np(views["edges"]).astype(bool), ref["edges"])
    assert np.array_equal(_np(views["moments"]), ref["moments"]) and np.array_equal(_np(views["tallies"]), ref["tallies"])
    with pytest.raises(RuntimeError):
        K.regions_shape_labels(d, views["edges"], 0, bbox[:, :0])          # capacity < 1: refused, nothing launched
    with pytest.raises(TypeError):
        K.regions_shape_labels(d, views["edges"], cap, bbox[:, :4])
    with pytest.raises(TypeError):
        K.regions_shape_labels(d, views["edges"].to(torch.int32), cap, bbox)
    with pytest.raises(TypeError):
        K.regions_edges_labels(d.to(torch.int64))


def test_batches_and_chunks(dev, monkeypatch):
    lab = SR.random_labels(5, 40, 70, seed=11)
    lab[1] = 0                                                            # an image without objects inside the batch
    ref = SR.shape_labels(lab)
    whole = G.shape_labels(lab)
    assert_shape(whole, ref)
    for i in range(5):
        one = G.shape_labels(lab[i], max_regions=whole.table.capacity)
        assert torch.equal(one.moments[0], whole.moments[i]) and torch.equal(one.tallies[0], whole.tallies[i])
        assert torch.equal(one.edges, whole.edges[i])
    monkeypatch.setattr(G, "_MAX_PIXELS", 2 * 40 * 70 + 5)                # two images per call: 2 + 2 + 1
    assert [b - a for a, b in G._chunks(torch.empty(5, 40, 70))] == [2, 2, 1]
    assert_shape(G.shape_labels(lab), ref)
    assert_shape(G.shape_labels(lab, max_regions=3), SR.shape_labels(lab, 3))
    assert np.array_equal(_np(G.boundaries(lab)), ref["edges"])
    m = lab > 0
    assert_shape(G.shape(m, connectivity=2), SR.shape(m, 2))


def test_two_runs_identical_and_graph_replay(dev):
    lab = SR.random_labels(3, 70, 90, seed=12, top=20)
    other = SR.random_labels(3, 70, 90, seed=13, top=20)
    cap = 18                                                              # below the largest label
    d = torch.from_numpy(lab).to(dev)
    a, b = G.shape_labels(d, max_regions=cap), G.shape_labels(d, max_regions=cap)
    for name in ("moments", "tallies", "edges"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    static = torch.zeros_like(d)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        G.shape_labels(static, max_regions=cap)                           # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st = G.shape_labels(static, max_regions=cap)
    for contents in (lab, other):
        static.copy_(torch.from_numpy(contents).to(dev))
        graph.replay()
        assert_shape(st, SR.shape_labels(contents, cap))
        eager = G.shape_labels(contents, max_regions=cap)
        assert torch.equal(st.moments, eager.moments) and torch.equal(st.tallies, eager.tallies) and torch.equal(st.edges, eager.edges)


@pytest.mark.parametrize("name", NAMES)
def test_golden_scipy_vectors(dev, name):
    lab = GOLD[f"{name}.labels"].astype(np.int32)
    edges = np.unpackbits(GOLD[f"{name}.edges"], axis=1)[:, :lab.shape[1]].astype(bool)
    st = G.shape_labels(lab)
    n = len(GOLD[f"{name}.tallies"])
    assert st.table.capacity == n
    assert np.array_equal(_np(st.tallies)[0], GOLD[f"{name}.tallies"]) and np.array_equal(_np(st.moments)[0], GOLD[f"{name}.moments"])
    assert np.array_equal(_np(st.edges), edges) and np.array_equal(_np(G.boundaries(lab)), edges)
    if name in ("blobs", "square5", "disc20"):                            # label images that are scipy's labelling of their foreground
        st = G.shape(lab > 0)
        assert np.array_equal(_np(st.tallies)[0], GOLD[f"{name}.tallies"]) and np.array_equal(_np(st.moments)[0], GOLD[f"{name}.moments"])
        assert np.array_equal(_np(st.edges), edges) and np.array_equal(_np(G.boundaries(lab > 0)), edges)


def test_measure_cells_with_shape_end_to_end_resnet18(dev):
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
    for kw in ({}, {"max_regions": 3}):
        refs = [SR.shape(b, 1, kw.get("max_regions")) for b in batches]    # every batch sizes its own tables
        plain = inference.measure_cells(loader, m, dev, thr, 40, 15, **kw)
        got = inference.measure_cells(loader, m, dev, thr, 40, 15, shape=True, **kw)
        assert len(got) == len(plain) == 4
        assert sorted(inference.measure_cells(loader, m, dev, thr, 40, 15, shape=False, **kw)[0]) == sorted(plain[0])
        for n, (g, p) in enumerate(zip(got, plain)):
            assert set(g) == set(p) | {"moments", "tallies", *SR.COLUMNS}
            for k in p:                                                   # the old keys: bit for bit
                assert g[k].dtype == p[k].dtype and g[k].shape == p[k].shape and g[k].tobytes() == p[k].tobytes(), k
            ref, i, rows = refs[n // 3], n % 3, len(p["area"])
            assert rows == min(int(ref["counts"][i]), ref["capacity"])
            assert np.array_equal(g["area"], ref["area"][i, :rows]) and np.array_equal(g["bbox"], ref["bbox"][i, :rows])
            assert np.array_equal(g["moments"], ref["moments"][i, :rows]) and np.array_equal(g["tallies"], ref["tallies"][i, :rows])
            for name, col in SR.columns(ref).items():
                assert_close(g[name], col[i, :rows], name)
    assert sum(len(g["area"]) for g in got) >= 1 and m.mode == "segment"
