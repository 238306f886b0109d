"""Polygons to pixels on the GPU (csrc/polygons.hip through cellsegmentation_amd.polygons.rasterize) against the plain-loop
restatement tests/polygon_ref.py, bit for bit: hand cases, odd sizes, shapes outside the image, degenerate rings, holes and
batches, overlaps, more edges than an LDS chunk, more spanning edges than a wave's list, forced banding, the fan-of-triangles
partition, the round trip through regions.contour_labels (eager and as a replayed graph) and detect_slide(roi=...)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import contour_ref as CR  # noqa: E402
import polygon_ref as PR  # noqa: E402
from cellsegmentation_amd import polygons as P  # noqa: E402
from cellsegmentation_amd import regions as G  # noqa: E402
from test_polygon_host import TRIANGLE, TRIANGLE_WANT, UNIT, fan, pentagram, random_polygon  # noqa: E402

pytestmark = pytest.mark.gpu
RULES = ("evenodd", "nonzero")
MODES = ("labels", "mask")


def _np(t):
    return t.cpu().numpy()


def make_set(per_image, sub):
    """per_image: images -> shapes -> rings of integer (row, col) in units of 1/2**sub pixel -> a host PolygonSet"""
    ps = P.from_rings([[[np.asarray(r, np.int64).reshape(-1, 2) for r in rings] for rings in shapes] for shapes in per_image], sub=0)
    ps.sub = sub
    return ps


def check(per_image, hw, sub, dev, rules=RULES, modes=MODES, **kw):
    """device == restatement for every rule and mode; returns the even-odd labels"""
    ps = make_set(per_image, sub)
    first = None
    for rule in rules:
        for mode in modes:
            got = P.rasterize(ps, hw, mode=mode, rule=rule, device=dev, **kw)
            want = PR.rasterize(per_image, hw, sub, rule, mode)
            assert got.is_cuda and got.dtype == (torch.int32 if mode == "labels" else torch.uint8) and tuple(got.shape) == want.shape
            assert _np(got).tobytes() == want.tobytes(), (rule, mode, hw)
            first = got if first is None else first
    return first


def test_hand_cases(dev):
    assert _np(check([[[UNIT]]], (3, 3), 0, dev))[0].tolist() == [[1, 0, 0], [0, 0, 0], [0, 0, 0]]
    for ring in (TRIANGLE, TRIANGLE[::-1]):
        assert np.array_equal(_np(check([[[ring]]], (4, 4), 1, dev))[0] != 0, TRIANGLE_WANT)
    check([[[pentagram()]]], (40, 40), 0, dev)
    ps = make_set([[[pentagram()]]], 0)
    assert int(P.rasterize(ps, (40, 40), rule="evenodd", device=dev)[0, 20, 20]) == 0
    assert int(P.rasterize(ps, (40, 40), rule="nonzero", device=dev)[0, 20, 20]) == 1
    # two squares that share a half-pixel edge: no overlap, no gap
    a, b = [(0, 0), (0, 5), (8, 5), (8, 0)], [(0, 5), (0, 12), (8, 12), (8, 5)]
    assert _np(check([[[a], [b]]], (4, 6), 1, dev))[0].tolist() == [[1, 1, 2, 2, 2, 2]] * 4


@pytest.mark.parametrize("hw", [(1, 1), (1, 64), (2, 63), (3, 65), (5, 129), (70, 90)])
def test_random_polygons_on_odd_sizes(dev, hw):
    rng = np.random.default_rng(hw[0] * 1000 + hw[1])
    shapes = [[random_polygon(rng, *hw, 4).tolist()] for _ in range(6)]
    check([shapes], hw, 4, dev)


def test_outside_the_image(dev):
    H, W, big = 9, 70, 1 << 28
    partly = [[(-40, -30), (-20, 500), (90, 300), (70, -100)]]
    left, right = [[(2, -50), (2, -10), (7, -10), (7, -50)]], [[(2, 80), (7, 120), (7, 80)]]
    above, below = [[(-9, 3), (-2, 30), (-5, 60)]], [[(10, 3), (12, 30), (30, 60)]]
    cover = [[(-5, -5), (-5, 100), (20, 100), (20, -5)]]
    spike = [[(-big, -big), (4, big), (big, -big)]]
    far = [[(big, big), (big - 5, big), (big, big - 7)]]
    for shapes in ([partly], [left, right, above, below], [cover], [spike], [far], [partly, left, cover, spike, far, above]):
        check([shapes], (H, W), 0, dev)
    assert (_np(check([[cover]], (H, W), 0, dev)) == 1).all()
    assert not _np(check([[left, right, above, below, far]], (H, W), 0, dev)).any()
    s = 3                                                                  # the same at sub = 3, the largest coordinate again 2^28
    check([[[[(-big, -big), (4 << s, big), (big, -big)]], [[(r << s, c << s) for r, c in partly[0]]]]], (H, W), s, dev)


def test_degenerate_rings(dev):
    rings = [[], [(1, 1)], [(0, 0), (3, 3)], [(0, 0), (2, 2), (4, 4)], [(1, 0), (1, 5), (1, 2)], [(0, 2), (4, 2), (2, 2)]]
    assert not _np(check([[[r] for r in rings] + [rings]], (5, 6), 0, dev)).any()
    doubled = [(0, 0), (0, 0), (0, 1), (1, 1), (1, 1), (1, 1), (1, 0), (0, 0)]
    assert _np(check([[[[]], [doubled, [(2, 2)]]]], (3, 3), 0, dev))[0].tolist() == [[2, 0, 0], [0, 0, 0], [0, 0, 0]]
    assert not _np(check([[]], (3, 3), 0, dev)).any() and not _np(check([[[]]], (3, 3), 0, dev)).any()   # no shape; a shape of no ring


def test_holes_parts_and_a_ragged_batch(dev):
    outer, hole = [(1, 1), (1, 30), (20, 30), (20, 1)], [(5, 5), (5, 20), (15, 20), (15, 5)]
    island, part = [(8, 8), (8, 12), (12, 12), (12, 8)], [(22, 40), (22, 60), (30, 50)]
    rng = np.random.default_rng(5)
    images = [[[outer, hole, island], [part]], [], [[random_polygon(rng, 33, 65, 2).tolist()] for _ in range(3)] + [[outer, part]]]
    images = [[[[(r << 2, c << 2) for r, c in ring] for ring in rings] for rings in shapes] for shapes in images[:1]] + images[1:]
    images[2][3] = [[(r << 2, c << 2) for r, c in ring] for ring in images[2][3]]
    lab = _np(check(images, (33, 65), 2, dev))
    assert lab[0, 3, 3] == 1 and lab[0, 6, 6] == 0 and lab[0, 9, 9] == 1 and not lab[1].any() and lab[2].max() == 4
    nz = P.rasterize(make_set(images, 2), (33, 65), rule="nonzero", device=dev)
    assert int(nz[0, 6, 6]) == 1                                           # the hole runs the same way as the outline here


def test_overlaps_values_and_buffers(dev):
    rng = np.random.default_rng(9)
    H, W = 30, 41
    images = [[[random_polygon(rng, H, W, 4, margin=2.0).tolist()] for _ in range(k)] for k in (5, 0, 3)]
    ps = make_set(images, 4)
    lab = check(images, (H, W), 4, dev)
    want = PR.rasterize(images, (H, W), 4)
    assert (np.bincount(want.ravel()) > 0).sum() > 3                       # several labels survive, some pixels hold a covered shape
    mask = P.rasterize(ps, (H, W), mode="mask", device=dev)
    assert torch.equal(mask, (lab > 0).to(torch.uint8))
    values = np.array([7, -3, 900, 2, 5, 11, 11, 1 << 30], np.int32)
    got = P.rasterize(ps, (H, W), values=values, device=dev)
    per = [values[:5].tolist(), [], values[5:].tolist()]
    assert _np(got).tobytes() == PR.rasterize(images, (H, W), 4, values=per).tobytes()
    assert _np(P.rasterize(ps, (H, W), values=torch.from_numpy(values).to(dev), device=dev)).tobytes() == _np(got).tobytes()
    # onto a buffer that already holds labels: the larger stays
    held = rng.integers(0, 4, (3, H, W)).astype(np.int32)
    buf = torch.from_numpy(held).to(dev)
    assert P.rasterize(ps, (H, W), out=buf, clear=False) is buf
    assert _np(buf).tobytes() == PR.rasterize(images, (H, W), 4, base=held).tobytes() == np.maximum(held, want).tobytes()
    buf = torch.from_numpy(held).to(dev)
    P.rasterize(ps, (H, W), out=buf, clear=False, values=values)
    assert _np(buf).tobytes() == PR.rasterize(images, (H, W), 4, values=per, base=held).tobytes()
    m = torch.from_numpy((held == 3).astype(np.uint8)).to(dev)
    P.rasterize(ps, (H, W), mode="mask", out=m, clear=False)
    assert _np(m).tobytes() == ((held == 3) | (want > 0)).astype(np.uint8).tobytes()
    # out= as a non-first slice of a larger buffer; clear=True clears the slice only
    big = torch.full((5, H, W), 77, dtype=torch.int32, device=dev)
    P.rasterize(ps, (H, W), out=big[1:4], rule="nonzero")
    assert _np(big[1:4]).tobytes() == PR.rasterize(images, (H, W), 4, "nonzero").tobytes() and (big[0] == 77).all() and (big[4] == 77).all()


def test_more_edges_than_a_chunk(dev):
    n, H, W, S = 5000, 96, 96, 16
    rng = np.random.default_rng(21)
    ang = np.arange(n) * (2 * math.pi / n)
    rad = 40 + rng.uniform(-1.5, 1.5, n)
    ring = np.rint(np.stack([48.3 + rad * np.sin(ang), 47.6 + rad * np.cos(ang)], 1) * S).astype(np.int64).tolist()
    hole = [(30 * S, 30 * S), (30 * S, 60 * S), (60 * S, 60 * S), (60 * S, 30 * S)]
    lab = _np(check([[[ring, hole], [ring[::-1]]]], (H, W), 4, dev, rules=("evenodd",), modes=("labels",)))
    assert lab[0, 48, 48] == 2 and lab[0, 10, 48] == 2 and lab[0, 0, 0] == 0
    check([[[ring, hole]]], (H, W), 4, dev, rules=("nonzero",), modes=("mask",), _band_rows=7)


def comb(teeth, pitch, top, base, bottom):
    ring = []
    for t in range(teeth):
        ring += [(base, pitch * t), (top, pitch * t), (top, pitch * t + 2), (base, pitch * t + 2)]
    return ring + [(bottom, pitch * (teeth - 1) + 2), (bottom, 0)]


def test_more_spanning_edges_than_a_list(dev):
    ring = comb(650, 6, 4, 40, 56)                                         # sub = 4: teeth 1/8 pixel wide from row 0.25 to row 2.5
    Y = 8                                                                  # the centre line of row 0 in units of 1/16
    assert sum((a[0] <= Y) != (b[0] <= Y) for a, b in zip(ring, ring[1:] + ring[:1])) == 1300
    lab = _np(check([[[ring]]], (4, 200), 4, dev, modes=("labels",)))
    assert lab[0, 0, :6].tolist() == [0, 1, 0, 0, 1, 0] and lab[0, 2].all() and not lab[0, 3].any()
    check([[[ring], [comb(650, 4, 4, 40, 56)]]], (4, 200), 4, dev, rules=("nonzero",), _band_rows=1)
    # 200 and 256 spanning edges: a full list, read in several steps, over several segments and with a hole ring besides
    for teeth in (100, 128):
        wide = comb(teeth, 22, 4, 40, 56)
        assert sum((a[0] <= Y) != (b[0] <= Y) for a, b in zip(wide, wide[1:] + wide[:1])) == 2 * teeth
        check([[[wide, [(6, 30), (30, 30), (30, 2000), (6, 2000)]]]], (4, 200), 4, dev)


@pytest.mark.parametrize("band", [1, 3, 64])
def test_forced_banding(dev, band):
    rng = np.random.default_rng(33)
    H, W = 44, 70
    tall = [[(2 * 16, 5 * 16), (42 * 16, 30 * 16), (30 * 16, 66 * 16), (10 * 16, 40 * 16)]]       # 40 rows
    on_centres = [[(r * 16 + 8, c * 16 + 8) for r, c in ((1, 3), (4, 60), (7, 20), (10, 64), (13, 8), (40, 33))]]
    shapes = [tall, on_centres] + [[random_polygon(rng, H, W, 4, margin=20.0).tolist()] for _ in range(4)]
    ps = make_set([shapes, shapes[::-1]], 4)
    for rule in RULES:
        for mode in MODES:
            whole = P.rasterize(ps, (H, W), mode=mode, rule=rule, device=dev, _band_rows=1 << 20)
            cut = P.rasterize(ps, (H, W), mode=mode, rule=rule, device=dev, _band_rows=band)
            assert torch.equal(whole, cut)
            assert _np(cut).tobytes() == PR.rasterize([shapes, shapes[::-1]], (H, W), 4, rule, mode).tobytes()
    assert len(P.plan(ps, (H, W), band)) > len(P.plan(ps, (H, W), 1 << 20)) or band == 64


def test_fan_of_triangles_partition(dev):
    rng = np.random.default_rng(17)
    H, W = 20, 24
    for case in range(12):
        ring, parts = fan(rng, H, W, 4, snap=case % 3 == 0)
        whole = P.rasterize(make_set([[[ring]]], 4), (H, W), mode="mask", device=dev)
        each = P.rasterize(make_set([[[p]] for p in parts], 4), (H, W), mode="mask", device=dev)
        assert torch.equal(each.sum(0, dtype=torch.int32), whole[0].to(torch.int32)) and whole.any()
        lab = P.rasterize(make_set([[[p] for p in parts]], 4), (H, W), device=dev)
        assert torch.equal(lab > 0, whole > 0)


@pytest.mark.parametrize("conn,density", [(1, 0.45), (2, 0.3)])
def test_round_trip_through_contour_labels(dev, conn, density):
    import regions_ref as R
    rng = np.random.default_rng(40 + conn)
    H, W, maxv = 40, 50, 48
    lab = np.stack([R.label(rng.random((H, W)) < density, conn)[0] for _ in range(3)]).astype(np.int32)   # one piece per label
    ct = G.contour_labels(lab, connectivity=conn, max_vertices=maxv)
    ps = P.from_contours(ct)
    assert ps.sub == 0 and ps.vertices.is_cuda and ps.n_images == 3 and ps.n_shapes == 3 * ct.table.capacity
    ref = CR.contour_labels(lab, None, conn, maxv)
    traced, cut = ref["contour"][..., 0] > 0, CR.truncated(ref)
    simple = CR.is_simple(ref) & ~cut
    assert simple.any() and (traced & ~CR.is_simple(ref)).any() and cut.any()      # labels with holes and rings too long for the table
    got = _np(P.rasterize(ps, (H, W)))
    assert _np(P.rasterize(ps, (H, W), rule="nonzero")).tobytes() == got.tobytes()
    for n in range(3):
        for k in np.flatnonzero(simple[n]):
            assert np.array_equal(got[n] == k + 1, lab[n] == k + 1), (n, k)
    # every ring, simple or not: the device's fill of it is the restatement's; truncated rows draw nothing
    rings = [[[r] if r is not None and len(r) <= maxv else [[]] for r in ref["rings"][n]] for n in range(3)]
    assert got.tobytes() == PR.rasterize(rings, (H, W), 0).tobytes()
    assert _np(P.rasterize(ps, (H, W), mode="mask")).tobytes() == (got > 0).astype(np.uint8).tobytes()


def test_graph_replay(dev):
    import regions_ref as R
    H, W, cap, maxv = 40, 50, 60, 24                                       # below the largest label and the longest ring
    lab, other = (np.stack([R.label(np.random.default_rng(seed + n).random((H, W)) < 0.3, 2)[0] for n in range(3)]).astype(np.int32)
                  for seed in (50, 60))

    def chain(x):
        return P.rasterize(P.from_contours(G.contour_labels(x, max_regions=cap, connectivity=2, max_vertices=maxv)), (H, W))
    static = torch.zeros((3, H, W), dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        chain(static)                                                      # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = chain(static)
    for contents in (lab, other):
        static.copy_(torch.from_numpy(contents).to(dev))
        graph.replay()
        assert _np(out).tobytes() == _np(chain(torch.from_numpy(contents).to(dev))).tobytes()
        ref = CR.contour_labels(contents, cap, 2, maxv)
        assert CR.truncated(ref).any()
        rings = [[[r] if r is not None and len(r) <= maxv else [[]] for r in ref["rings"][n]] for n in range(3)]
        assert max(int(c.max()) for c in contents) > cap and len(rings[0]) == cap
        assert _np(out).tobytes() == PR.rasterize(rings, (H, W), 0).tobytes() and out.any()


def test_detect_slide_roi_resnet18(dev):
    from cellsegmentation_amd import inference, synth
    from cellsegmentation_amd.model import resnet as RN
    from test_slide_gpu import _blob_slide
    m = RN.MILresnet18()
    sd = m.state_dict()
    synth.fill_state_dict(sd)
    m.load_state_dict(sd)
    m = m.to(dev).set_compute_dtype(torch.float32)
    H, W = 150, 170
    img = _blob_slide(H, W, 31)
    kw = dict(batch_size=5, patch_size=64, interval=48, eps=11, thr=-0.01)
    everything = P.from_rings([[np.array([[0, 0], [0, W], [H, W], [H, 0]])]], sub=0)
    drawn = {"type": "Feature", "properties": {"name": "roi"},                # (x, y), convex
             "geometry": {"type": "Polygon", "coordinates": [[[20.5, 10.25], [120.0, 14.0], [124.75, 60.5], [30.0, 70.0], [20.5, 10.25]]]}}
    for blend in (None, True):
        plain = inference.detect_slide(img, m, dev, blend=blend, **kw)
        assert plain.roi is None and len(plain.points) + len(plain.discarded) > 0
        full = inference.detect_slide(img, m, dev, blend=blend, roi=everything, **kw)
        assert torch.equal(full.mask, plain.mask) and full.cell_count == plain.cell_count and bool(full.roi.all())
        assert np.array_equal(full.points, plain.points) and np.array_equal(full.discarded, plain.discarded)
        got = inference.detect_slide(img, m, dev, blend=blend, roi=drawn, **kw)
        roi = got.roi
        assert roi.dtype == torch.uint8 and tuple(roi.shape) == (H, W) and 0 < int(roi.sum()) < H * W // 4
        assert _np(roi).tobytes() == PR.rasterize([[[[(int(y * 16), int(x * 16)) for x, y in drawn["geometry"]["coordinates"][0][:-1]]]]],
                                                  (H, W), 4, mode="mask")[0].tobytes()
        assert torch.equal(got.mask, plain.mask * roi)
        # seeds only where the blurred mask is above 0 (thr < 0 above keeps the seed windows of an empty mask where they are)
        seeded = inference.detect_slide(img, m, dev, blend=blend, roi=drawn, **{**kw, "thr": 0.0})
        pts = np.concatenate([seeded.points.reshape(-1, 2), np.asarray(seeded.discarded).reshape(-1, 2)]).astype(np.int64)
        assert torch.equal(seeded.mask, got.mask) and len(pts) > 0 and _np(roi)[pts[:, 0], pts[:, 1]].all()   # none outside the ROI
        same = inference.detect_slide(img, m, dev, blend=blend, roi=_np(roi).astype(bool), **kw)
        assert torch.equal(same.mask, got.mask) and same.cell_count == got.cell_count and torch.equal(same.roi, roi)
        assert np.array_equal(same.points, got.points) and np.array_equal(same.discarded, got.discarded)
    both = list(inference.detect_slides([img], m, dev, roi=P.from_geojson(drawn), **kw))
    assert torch.equal(both[0].roi, roi) and m.mode == "segment"


def test_host_roi_reaches_the_kernel_with_an_item_table(dev, monkeypatch):
    from cellsegmentation_amd import kernels as K
    real, seen = K.polygons_rasterize, []

    def spy(*args):
        seen.append(args[-1])
        return real(*args)
    monkeypatch.setattr(K, "polygons_rasterize", spy)
    ring = np.array([[10.25, 20.5], [14.0, 120.0], [60.5, 124.75], [70.0, 30.0]])
    host = P.from_rings([[ring]])
    mask = P.roi_mask(host, (150, 170))(dev)
    items = seen.pop()
    assert items is not None and items.is_cuda and np.array_equal(_np(items), P.plan(host, (150, 170))) and len(items) == 4
    again = P.roi_mask(host.to(dev), (150, 170))(dev)                      # a set that lives on the device goes without a plan
    assert seen.pop() is None and torch.equal(again, mask) and 0 < int(mask.sum()) < 150 * 170
    doc = {"type": "Polygon", "coordinates": [ring[:, ::-1].tolist()]}
    assert torch.equal(P.roi_mask(doc, (150, 170))(dev), mask) and seen.pop() is not None


def test_detect_slide_roi_with_tissue_resnet18(dev):
    from cellsegmentation_amd import inference, synth, tiles, tissue
    from cellsegmentation_amd import kernels as K
    from cellsegmentation_amd.model import resnet as RN
    from test_slide_gpu import _blob_slide
    m = RN.MILresnet18()
    sd = m.state_dict()
    synth.fill_state_dict(sd)
    m.load_state_dict(sd)
    m = m.to(dev).set_compute_dtype(torch.float32)
    H, W = 150, 170
    img = _blob_slide(H, W, 31)
    kw = dict(batch_size=5, patch_size=64, interval=48, eps=11, tissue=tissue.TissueOptions(min_pixels=20))
    roi = P.from_rings([[np.array([[10.25, 20.5], [14.0, 120.0], [60.5, 124.75], [70.0, 30.0]])]])
    whole = inference.detect_slide(img, m, dev, **kw)
    got = inference.detect_slide(img, m, dev, roi=roi, **kw)
    cut = whole.tissue.mask & got.roi                                      # the tissue decision itself is taken on the slide as scanned
    assert got.tissue.threshold == whole.tissue.threshold and torch.equal(got.tissue.mask, cut) and 0 < int(cut.sum()) < int(whole.tissue.mask.sum())
    rc = torch.from_numpy(np.asarray(tiles.sample_patches((H, W), 64, 48), dtype=np.int32)).to(dev)
    cover = K.tissue_coverage(cut[None].contiguous(), torch.zeros(len(rc), dtype=torch.int32, device=dev), rc, 64, 64)
    keep = torch.nonzero(cover >= 20).reshape(-1).to(torch.int32)
    assert torch.equal(got.tissue.coverage, cover) and torch.equal(got.tissue.selected, keep)
    assert 0 < got.tissue.n_selected == len(keep) < whole.tissue.n_selected
    assert not (got.mask * (1 - got.roi)).any()
    # the same patches in the same order as a run over them alone: the stitched bytes inside the ROI
    covered = torch.zeros((H, W), dtype=torch.bool, device=dev)
    for r, c in rc[keep.long()].tolist():
        covered[r:r + 64, c:c + 64] = True
    assert not got.mask[~covered].any()
