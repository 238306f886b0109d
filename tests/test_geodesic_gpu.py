"""The geodesic seeded split on the GPU (csrc/regions.hip through cellsegmentation_amd.regions.split_geodesic), exact against the
plain-loop statement tests/geodesic_ref.py (a heap Dijkstra) and the vectors of tests/golden/geodesic_vectors.npz.  Shapes: 70 x 90
and 130 x 67 cross the 64 x 64 tiles in both directions with a ragged last tile, 37 x 130 has three tiles in a row and an odd
height.  Every comparison is exact."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import geodesic_ref as GR  # noqa: E402
import regions_ref as R  # noqa: E402
import split_ref as S  # noqa: E402
from cellsegmentation_amd import detect, inference  # noqa: E402
from cellsegmentation_amd import regions as G  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "geodesic_vectors.npz"), allow_pickle=False)
NAMES = sorted(k[:-len(".labels")] for k in GOLD.files if k.endswith(".labels"))
KEYS = ("labels", "counts", "n_seeds", "live", "distance")
TABLES = ("area", "bbox", "sum_rc", "intensity_sum", "intensity_max")


def _np(t):
    return t.cpu().numpy()


def assert_geodesic(got, ref, mask, converged=True):
    assert isinstance(got, G.GeodesicSplitResult) and isinstance(got, G.SplitResult)
    assert got.labels.dtype == torch.int32 and got.labels.is_cuda and tuple(got.labels.shape) == ref["labels"].shape
    assert got.counts.dtype == torch.int32 and got.n_seeds.dtype == torch.int32 and got.live.dtype == torch.bool
    assert got.converged.dtype == torch.bool and got.converged.is_cuda and tuple(got.converged.shape) == tuple(got.counts.shape)
    assert np.array_equal(_np(got.labels), ref["labels"])
    assert np.array_equal(_np(got.counts), ref["counts"]) and np.array_equal(_np(got.n_seeds), ref["n_seeds"])
    assert np.array_equal(_np(got.live), ref["live"])
    assert np.array_equal(_np(got.labels) > 0, np.asarray(mask))
    if got.distance is not None:
        assert got.distance.dtype == torch.int32 and np.array_equal(_np(got.distance), ref["distance"])
    if converged:
        assert bool(got.converged.all())


def check(m, pts, off=None, lim=None, conn=1, device_points=None, **kw):
    """split_geodesic on the GPU, with the distance map, against the reference; returns (GeodesicSplitResult, reference)"""
    ref = GR.split(m, pts, off, lim, conn)
    got = G.split_geodesic(m, pts if device_points is None else device_points, off, lim, conn, want_distance=True, **kw)
    assert got.distance is not None
    assert_geodesic(got, ref, m)
    return got, ref


@functools.lru_cache(maxsize=None)
def _golden(name):
    shape = tuple(GOLD[f"{name}.shape"])
    m = np.unpackbits(GOLD[f"{name}.mask"], axis=1)[:, :shape[2]].astype(bool).reshape(shape)
    lim = GOLD[f"{name}.limits"]
    return m, GOLD[f"{name}.points"], GOLD[f"{name}.offsets"], lim if len(lim) else None, int(GOLD[f"{name}.connectivity"])


@pytest.mark.parametrize("name", NAMES)
def test_golden_vectors_and_their_tables(dev, name):
    m, pts, off, lim, conn = _golden(name)
    ref = {k: GOLD[f"{name}.{k}"] for k in KEYS}
    got = G.split_geodesic(m, pts, off, lim, conn, want_distance=True)
    assert_geodesic(got, ref, m)
    assert G.split_geodesic(m, pts, off, lim, conn).distance is None
    v = np.random.RandomState(len(name)).randint(0, 256, size=m.shape).astype(np.uint8)
    t = G.measure_labels(got.labels, intensity=v, counts=got.counts)     # a GeodesicSplitResult is a SplitResult to its users
    want = S.tables(ref["labels"], v, counts=ref["counts"])
    assert t.capacity == want["capacity"] and np.array_equal(_np(t.counts), want["counts"])
    for key in TABLES:
        assert np.array_equal(_np(getattr(t, key)), want[key]), key
    assert int(t.area.sum()) == int(m.sum())


def test_horseshoe_is_torn_by_split_and_whole_after_split_geodesic(dev):
    m, pts = GR.horseshoe()
    euclid = _np(G.split(m, pts).labels)
    assert GR.disconnected_labels(euclid) == [1]                        # the device result itself: a cell in two pieces
    got, ref = check(m, pts)
    assert GR.disconnected_labels(_np(got.labels)) == [] and _np(got.counts).tolist() == [2]
    lab = _np(got.labels)
    for k, (r, c) in enumerate(pts):
        assert lab[r, c] == k + 1 and _np(got.distance)[r, c] == 0
    check(m, pts, conn=2)


def test_tie_column_goes_to_the_lower_index(dev):
    m, pts = GR.two_discs()
    mid = int(pts[:, 1].sum()) // 2
    assert m[:, mid].any()
    lab = _np(check(m, pts)[0].labels)
    assert (lab[:, :mid + 1][m[:, :mid + 1]] == 1).all() and (lab[:, mid + 1:][m[:, mid + 1:]] == 2).all()
    lab = _np(check(m, pts[::-1].copy())[0].labels)
    assert (lab[:, :mid][m[:, :mid]] == 2).all() and (lab[:, mid:][m[:, mid:]] == 1).all()      # the tie column changed owner


@pytest.mark.parametrize("connectivity", [1, 2])
def test_a_nearer_seed_of_another_component_does_not_win(dev, connectivity):
    m, pts = GR.foreign_seed()
    b = np.zeros_like(m)
    b[8:28, 42:100] = True
    lab = _np(check(m, pts, conn=connectivity)[0].labels)
    assert (lab[b] == 2).all() and (lab[m & ~b] == 1).all()
    lab = _np(check(m, pts[::-1].copy(), conn=connectivity)[0].labels)
    assert (lab[b] == 1).all() and (lab[m & ~b] == 2).all()
    corner = np.zeros((70, 90), bool)
    corner[40:64, 40:64] = True
    corner[64:69, 64:88] = True                                         # touches the first square at the corner of four tiles
    seeds = np.asarray([[63, 63], [66, 80]], np.int64)
    got, _ = check(corner, seeds[:1], conn=connectivity)                # one seed: it crosses the corner only with connectivity 2
    assert _np(got.counts).tolist() == [3 - connectivity] and (_np(got.labels)[64:69, 64:88] == 3 - connectivity).all()
    check(corner, seeds, conn=connectivity)


def test_two_calls_device_points_and_single_images_give_the_same_bits(dev):
    m, pts, off, lim, conn = _golden("batch2")
    a, _ = check(m, pts, off, lim, conn)
    b, _ = check(m, pts, off, lim, conn)
    d, _ = check(m, pts, off, lim, conn, device_points=torch.from_numpy(pts).to(dev))
    longer = torch.from_numpy(np.concatenate([pts, pts[:4]])).to(dev)   # a buffer longer than offsets[-1], device offsets
    e = G.split_geodesic(m, longer, torch.from_numpy(off).to(dev), lim, conn, want_distance=True)
    for other in (b, d, e):
        assert torch.equal(a.labels, other.labels) and torch.equal(a.distance, other.distance) and torch.equal(a.counts, other.counts)
        assert torch.equal(a.live, other.live[:len(pts)]) and not bool(other.live[len(pts):].any())
    for n in range(len(m)):
        one = G.split_geodesic(m[n], pts[off[n]:off[n + 1]], limits=None if lim is None else int(lim[n]), connectivity=conn,
                               want_distance=True)
        assert torch.equal(one.labels, a.labels[n]) and torch.equal(one.distance, a.distance[n])
        assert _np(one.counts).tolist() == [int(_np(a.counts)[n])]


def _rounds_batch():
    snake, seed = GR.serpentine()
    easy = S.discs(37, 130, [(18, 60), (18, 100)], 14)                  # the first across the tile edge, the second inside a tile
    easy_pts = np.asarray([[18, 50], [10, 95], [25, 108]], np.int64)
    m = np.stack([snake, easy])
    pts, off = np.concatenate([seed, easy_pts]), np.asarray([0, 1, 4], np.int64)
    return m, pts, off


def test_rounds_convergence_flags_and_skipped_rounds(dev):
    m, pts, off = _rounds_batch()
    ref = GR.split(m, pts, off)
    assert GR.jacobi_rounds(m[0], pts[:1]) == 19 and GR.jacobi_rounds(m[1], pts[1:]) <= 3
    short = G.split_geodesic(m, pts, off, max_rounds=4, want_distance=True)
    assert _np(short.converged).tolist() == [False, True]
    assert np.array_equal(_np(short.labels)[1], ref["labels"][1]) and np.array_equal(_np(short.distance)[1], ref["distance"][1])
    lab0, d0 = _np(short.labels)[0], _np(short.distance)[0]              # what is promised of the image that did not converge
    assert np.array_equal(lab0 > 0, m[0]) and (lab0[m[0]] == 1).all()
    reached = d0 >= 0
    assert np.array_equal(d0[reached], ref["distance"][0][reached]) and (d0[~reached] == -1).all() and (~reached).any()
    assert np.array_equal(_np(short.counts), ref["counts"]) and np.array_equal(_np(short.live), ref["live"])
    bound = G.split_geodesic(m, pts, off, max_rounds=19, want_distance=True)      # the model's bound
    assert_geodesic(bound, ref, m)
    exact = G.split_geodesic(m, pts, off, want_distance=True)            # batches of rounds until converged
    assert_geodesic(exact, ref, m)
    many = G.split_geodesic(m, pts, off, max_rounds=40, want_distance=True)       # rounds after convergence are skipped tile by tile
    assert_geodesic(many, ref, m)
    assert torch.equal(many.labels, bound.labels) and torch.equal(many.distance, bound.distance)
    one = G.split_geodesic(m[1], pts[1:], max_rounds=1)                  # a single round never sees itself settle
    assert _np(one.converged).tolist() == [False] and np.array_equal(_np(one.labels), ref["labels"][1])


def _dead_seed_mask():
    m = S.discs(70, 90, [(20, 20)], 12) & ~S.discs(70, 90, [(20, 20)], 3)          # A: a ring, its hole at the centre
    m[40:60, 10:40] = True                                                          # B
    m[5:25, 50:85] = True                                                           # C: its first pixel precedes A's and B's
    pts = np.asarray([[20, 20], [20, 14], [20, 14], [0, 0], [50, 20], [10, 60]], np.int64)
    return m, pts


def test_dead_duplicate_and_limited_seeds(dev):
    m, pts = _dead_seed_mask()
    got, _ = check(m, pts, lim=5)                                       # in the hole, live, its duplicate, on the background, live | cut
    assert _np(got.live).tolist() == [False, True, True, False, True, False] and _np(got.n_seeds).tolist() == [5]
    lab = _np(got.labels)
    assert (lab[:40, :45][m[:40, :45]] == 2).all()                      # the lower of two seeds on one pixel owns the ring
    assert (lab[40:60, 10:40] == 5).all() and (lab[5:25, 50:85] == 6).all() and _np(got.counts).tolist() == [6]
    assert (_np(got.distance)[5:25, 50:85] == -1).all()                 # seedless: numbered after the seeds, no distance
    got, _ = check(m, pts, lim=4)                                       # B loses its seed too: seedless, numbered after C
    assert (_np(got.labels)[5:25, 50:85] == 5).all() and (_np(got.labels)[40:60, 10:40] == 6).all()
    got, _ = check(m, pts)
    assert (_np(got.labels)[5:25, 50:85] == 6).all() and _np(got.counts).tolist() == [6] and _np(got.live)[5]
    check(m, pts, lim=-2)
    check(m, pts, lim=-9)
    check(m, pts, lim=0)
    assert torch.equal(G.split_geodesic(m, pts, limits=0).labels, G.label(m))


@pytest.mark.parametrize("connectivity", [1, 2])
def test_without_points_it_is_label(dev, connectivity):
    m = R.blobs(3, 70, 90, seed=70 + connectivity, density=1 / 120.0)
    m[1] = False
    want = G.label(m, connectivity)
    none = np.zeros((0, 2), np.int64)
    for rounds in (None, 3):
        got = G.split_geodesic(m, [none, none, none], connectivity=connectivity, max_rounds=rounds, want_distance=True)
        assert torch.equal(got.labels, want) and got.live.numel() == 0 and _np(got.n_seeds).tolist() == [0, 0, 0]
        assert np.array_equal(_np(got.counts), _np(want.view(3, -1).max(dim=1).values)) and bool(got.converged.all())
        assert np.array_equal(_np(got.distance), np.where(m, -1, 0))


def test_batches_cut_into_chunks(dev, monkeypatch):
    m, pts, off, lim, conn = _golden("batch1")
    whole, _ = check(m, pts, off, lim, conn)
    monkeypatch.setattr(G, "_MAX_PIXELS", 2 * 130 * 67 + 40)            # two images per call: 2 + 1
    assert [b - a for a, b in G._chunks(torch.empty(3, 130, 67))] == [2, 1]
    got, _ = check(m, pts, off, lim, conn)
    assert torch.equal(got.labels, whole.labels) and torch.equal(got.live, whole.live) and torch.equal(got.distance, whole.distance)


def test_graph_replay_of_a_fixed_number_of_rounds(dev):
    """the pattern of tests/test_split_gpu.py: warm up on a side stream, capture, then replay on two inputs"""
    m, pts, off, _, _ = _golden("batch1")
    other = GR.noise_masks(3, 130, 67, seed=11, density=0.8)
    pts2 = S.random_seeds(other, 14, seed=2)[0][:len(pts)]
    rounds = 0                                                          # the model's bound for both inputs
    for masks, points in ((m, pts), (other, pts2)):
        for n, x in enumerate(masks):
            rounds = max(rounds, GR.jacobi_rounds(x, points[off[n]:off[n + 1]]))
    assert 2 <= rounds <= 8
    doff = torch.from_numpy(off).to(dev)
    static_m = torch.zeros(m.shape, dtype=torch.bool, device=dev)
    static_p = torch.zeros(pts.shape, dtype=torch.int64, device=dev)

    def run():
        return G.split_geodesic(static_m, static_p, doff, max_rounds=rounds, want_distance=True)

    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        run()                                                           # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s = run()
    for mask, points in ((m, pts), (other, pts2)):
        static_m.copy_(torch.from_numpy(mask).to(dev))
        static_p.copy_(torch.from_numpy(points).to(dev))
        graph.replay()
        assert_geodesic(s, GR.split(mask, points, off), mask)


def test_detect_result_split_and_the_drivers_take_geodesic(dev):
    H, W = 300, 420
    blobs = R.blobs(1, H, W, seed=21)[0]
    rng = np.random.RandomState(17)
    u8 = np.where(blobs, rng.randint(128, 256, (H, W)), rng.randint(0, 11, (H, W))).astype(np.uint8)
    clean = R.remove_small_regions(u8 > 127, 300, 100)
    res = detect.detect_points(u8, method="distancetransform")
    assert res.device_points is not None and len(res.points) >= 3
    got = res.split(clean, geodesic=True)
    want = G.split_geodesic(clean, res.device_points, res.device_offsets, limits=None)
    assert isinstance(got, G.GeodesicSplitResult) and torch.equal(got.labels, want.labels) and torch.equal(got.counts, want.counts)
    assert np.array_equal(_np(got.labels), GR.split(clean, _np(res.device_points), res.offsets)["labels"])
    assert type(res.split(clean)) is G.SplitResult                      # the default stays the Euclidean split
    kept, discarded = res.per_image()[0]
    slide = inference.SlideResult(kept, discarded, len(kept), torch.from_numpy(u8).to(dev))
    table, parts = inference.measure_slide_cells(slide, geodesic=True)
    assert isinstance(parts, G.GeodesicSplitResult) and np.array_equal(_np(parts.labels), GR.split(clean, kept)["labels"])
    assert int(table.area.sum()) == int(clean.sum())
    assert type(inference.measure_slide_cells(slide)[1]) is G.SplitResult


def test_evaluate_instances_returns_the_same_keys_with_geodesic(dev):
    import detect_ref
    from cellsegmentation_amd import synth
    from cellsegmentation_amd.model import resnet as RN
    net = RN.MILresnet18()
    sd = net.state_dict()
    synth.fill_state_dict(sd)
    net.load_state_dict(sd)
    net = net.to(dev).set_compute_dtype(torch.float32)
    net.setmode("segment")
    x = synth.normalise(synth.ihc_tiles(1, 299, seed=21))
    probs = inference.inference_seg([x], net, dev, mode="test")
    thr = float(np.median(probs))
    kw = dict(threshold=thr, eps=11, method="distancetransform", thr_for_dt=int(np.median(detect_ref.quantize(probs))))
    truth = torch.from_numpy(_np(inference.segment_classes([x], net, dev, thr)).astype(np.uint8) * 255)
    plain = inference.evaluate_instances([(x, truth)], net, dev, **kw)
    geo = inference.evaluate_instances([(x, truth)], net, dev, geodesic=True, **kw)
    assert sorted(geo) == sorted(plain)
    assert np.array_equal(geo["n_truth"], plain["n_truth"]) and np.array_equal(geo["n_pred"], plain["n_pred"])      # the same seeds
