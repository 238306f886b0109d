"""CPU: the plain-loop restatement of polygons to pixels (tests/polygon_ref.py) against hand cases, against tests/contour_ref.py
(``fill`` and the labels of simple rings), against its own fan-of-triangles partition and against matplotlib; the host half of
cellsegmentation_amd.polygons -- ``from_rings``, ``from_geojson``, quantisation, the planner -- and its argument errors, which are
raised before the library is loaded."""
import math

import numpy as np
import pytest
import torch

import contour_ref as CR
import polygon_ref as PR
import regions_ref as R
from cellsegmentation_amd import _lib, polygons as P
from cellsegmentation_amd.regions import ContourTable, RegionTable

UNIT = [(0, 0), (0, 1), (1, 1), (1, 0)]
# sub = 1, units of half a pixel: (row, col) = (0.5, 0.5), (0.5, 3.5), (3.5, 0.5); the three edges pass through pixel centres
TRIANGLE = [(1, 1), (1, 7), (7, 1)]
TRIANGLE_WANT = np.array([[1, 1, 1, 0], [1, 1, 0, 0], [1, 0, 0, 0], [0, 0, 0, 0]], bool)


def pentagram(cy=20, cx=20, r=18, sub=0):
    pts = [(cy - r * math.cos(2 * math.pi * k / 5), cx + r * math.sin(2 * math.pi * k / 5)) for k in range(5)]
    return [(int(round(y * (1 << sub))), int(round(x * (1 << sub)))) for y, x in (pts[(2 * k) % 5] for k in range(5))]


def random_polygon(rng, H, W, sub, lo=3, hi=11, margin=5.0):
    n = int(rng.integers(lo, hi + 1))
    v = np.stack([rng.uniform(-margin, H + margin, n), rng.uniform(-margin, W + margin, n)], 1)
    return np.rint(v * (1 << sub)).astype(np.int64)


def fan(rng, H, W, sub, snap):
    """a star-shaped polygon round a centre and the triangles (centre, v_k, v_k+1) that partition it"""
    S = 1 << sub
    q = (lambda x: int(round(x * 2)) * S // 2) if snap else (lambda x: int(round(x * S)))
    cy, cx = q(rng.uniform(0.3, 0.7) * H), q(rng.uniform(0.3, 0.7) * W)
    n = int(rng.integers(3, 9))
    ang = np.sort(rng.uniform(0, 2 * math.pi, n))
    while np.diff(np.concatenate([ang, [ang[0] + 2 * math.pi]])).max() >= math.pi:      # the centre must see every edge from inside
        n += 1
        ang = np.sort(rng.uniform(0, 2 * math.pi, n))
    rad = rng.uniform(0.15, 0.6, n) * min(H, W)
    ring = [(cy + q(r * math.sin(a)), cx + q(r * math.cos(a))) for a, r in zip(ang, rad)]
    turn = [(ring[k][0] - cy) * (ring[(k + 1) % n][1] - cx) - (ring[k][1] - cx) * (ring[(k + 1) % n][0] - cy) for k in range(n)]
    if not (all(t > 0 for t in turn) or all(t < 0 for t in turn)):         # rounding flipped a thin triangle: no partition
        return fan(rng, H, W, sub, snap)
    parts = [[(cy, cx), ring[k], ring[(k + 1) % n]] for k in range(n)]
    return ring, parts


def test_hand_cases():
    assert np.array_equal(PR.winding([UNIT], (3, 3)) != 0, np.array([[1, 0, 0], [0, 0, 0], [0, 0, 0]], bool))
    for rule in ("evenodd", "nonzero"):
        assert np.array_equal(PR.taken(PR.winding([TRIANGLE], (4, 4), 1), rule), TRIANGLE_WANT)
        assert np.array_equal(PR.taken(PR.winding([TRIANGLE[::-1]], (4, 4), 1), rule), TRIANGLE_WANT)
    w = PR.winding([pentagram()], (40, 40))
    assert abs(w[20, 20]) == 2 and not PR.taken(w, "evenodd")[20, 20] and PR.taken(w, "nonzero")[20, 20]
    assert abs(w[8, 20]) == 1 and PR.taken(w, "evenodd")[8, 20]            # inside a point of the star
    # degenerate rings contribute nothing
    for ring in ([], [(1, 1)], [(0, 0), (3, 3)], [(0, 0), (2, 2), (4, 4)], [(1, 0), (1, 5), (1, 2)]):
        assert not PR.winding([ring], (5, 5)).any()
    assert np.array_equal(PR.winding([[(0, 0), (0, 0), (0, 1), (1, 1), (1, 1), (1, 0)]], (3, 3)), PR.winding([UNIT], (3, 3)))
    # two squares that share an edge neither overlap nor leave a gap, at a half-pixel edge too
    a, b = [(0, 0), (0, 5), (8, 5), (8, 0)], [(0, 5), (0, 12), (8, 12), (8, 5)]
    wa, wb = PR.winding([a], (4, 6), 1) != 0, PR.winding([b], (4, 6), 1) != 0
    assert not (wa & wb).any() and (wa | wb).all() and wa[:, :2].all() and not wa[:, 2:].any()


@pytest.mark.parametrize("conn", [1, 2])
def test_restatement_against_contour_ref(conn):
    rings = simple = 0
    for seed in range(8):
        rng = np.random.default_rng(100 + seed)
        mask = rng.random((20, 26)) < (0.3 + 0.05 * seed)
        t = CR.contours(mask[None], conn)
        lab = R.label(mask, conn)[0]
        for k, ring in enumerate(t["rings"][0]):
            if ring is None:
                continue
            w = PR.winding([ring], mask.shape)
            for rule in ("evenodd", "nonzero"):
                assert np.array_equal(PR.taken(w, rule), CR.fill(ring, mask.shape))
            rings += 1
            if CR.is_simple(t)[0, k]:
                assert np.array_equal(w != 0, lab == k + 1)
                simple += 1
    assert rings > 40 and 0 < simple < rings


def test_fan_of_triangles_partition():
    rng = np.random.default_rng(7)
    for case in range(30):
        ring, parts = fan(rng, 20, 24, 4, snap=case % 3 == 0)
        whole = PR.winding([ring], (20, 24), 4)
        total = sum(PR.winding([p], (20, 24), 4) for p in parts)
        assert np.array_equal(total, whole) and set(np.unique(np.abs(whole))) == {0, 1}
        for rule in ("evenodd", "nonzero"):                                # every pixel of the whole lies in exactly one part
            assert np.array_equal(sum(PR.taken(PR.winding([p], (20, 24), 4), rule).astype(int) for p in parts), PR.taken(whole, rule))


def test_evenodd_against_matplotlib():
    mpath = pytest.importorskip("matplotlib.path")
    H, W, sub = 40, 50, 4
    rng = np.random.default_rng(11)
    jj, ii = np.meshgrid(np.arange(W), np.arange(H))
    centres = np.stack([jj.ravel() + 0.5, ii.ravel() + 0.5], 1)             # (x, y)
    checked = left_out = 0
    for _ in range(100):
        ring = random_polygon(rng, H, W, sub)
        xy = ring[:, ::-1] / float(1 << sub)
        path = mpath.Path(np.concatenate([xy, xy[:1]]), closed=True)
        votes = [path.contains_points(centres, radius=r) for r in (1e-6, 0.0, -1e-6)]
        stable = (votes[0] == votes[1]) & (votes[1] == votes[2])
        got = PR.taken(PR.winding([ring.tolist()], (H, W), sub), "evenodd").ravel()
        assert np.array_equal(got[stable], votes[1][stable])
        checked += int(stable.sum())
        left_out += int((~stable).sum())
    assert left_out <= 0.01 * (checked + left_out)


def _cpu_contours(lab, conn=1):
    t = CR.contour_labels(lab, None, conn)
    table = RegionTable(torch.from_numpy(t["counts"]), t["capacity"], torch.from_numpy(t["area"]), torch.from_numpy(t["bbox"]),
                        torch.from_numpy(t["sum_rc"]))
    return ContourTable(table, torch.from_numpy(t["contour"]), torch.from_numpy(t["vertices"]), conn), t


@pytest.mark.parametrize("origin,scale,sub", [((0, 0), 1.0, 4), ((1000, -20), 0.25, 0), ((-3, 7), 2.0, 2), ((64, 64), 0.5, 8)])
def test_from_geojson_inverts_contour_geojson(origin, scale, sub):
    lab = np.array([[1, 0, 2], [0, 1, 2], [1, 1, 0]], np.int32)
    ct, t = _cpu_contours(lab, 2)
    ps = P.from_geojson(ct.geojson(origin=origin, scale=scale), origin=origin, scale=scale, sub=sub)
    assert ps.n_images == 1 and ps.n_shapes == 2 and ps.sub == sub and [p["row"] for p in ps.properties] == [0, 1]
    assert ps.shape_rings.tolist() == [0, 1, 2] and ps.image_shapes.tolist() == [0, 2] and ps.vertices.dtype == torch.int32
    for k in range(2):
        a, n = int(ps.ring_start[k]), int(ps.ring_count[k])
        assert n == len(t["rings"][0][k])                                  # the repeated closing point is dropped
        assert np.array_equal(ps.vertices[a:a + n].numpy(), np.asarray(t["rings"][0][k]) << sub)


def test_from_geojson_kinds():
    sq = [[0, 0], [4, 0], [4, 4], [0, 4], [0, 0]]
    hole = [[1, 1], [2, 1], [2, 2], [1, 2], [1, 1]]
    far = [[10, 10], [12, 10], [12, 12], [10, 10]]
    poly = {"type": "Polygon", "coordinates": [sq, hole]}
    multi = {"type": "MultiPolygon", "coordinates": [[sq, hole], [far]]}
    feat = {"type": "Feature", "properties": {"name": "roi"}, "geometry": poly}
    point = {"type": "Point", "coordinates": [1, 2]}
    ps = P.from_geojson(poly, sub=0)
    assert ps.n_shapes == 1 and ps.ring_count.tolist() == [4, 4] and ps.properties == [None]
    assert ps.vertices[:4].tolist() == [[0, 0], [0, 4], [4, 4], [4, 0]]    # (row, col) = (y, x)
    ps = P.from_geojson(multi, sub=0)
    assert ps.n_shapes == 1 and ps.ring_count.tolist() == [4, 4, 3] and ps.shape_rings.tolist() == [0, 3]
    ps = P.from_geojson(feat)
    assert ps.properties == [{"name": "roi"}] and ps.sub == 4 and ps.vertices[1].tolist() == [0, 64]
    ps = P.from_geojson([feat, multi, {"type": "FeatureCollection", "features": [feat, feat]}])
    assert ps.n_shapes == 4 and ps.n_images == 1 and ps.properties == [{"name": "roi"}, None, {"name": "roi"}, {"name": "roi"}]
    with pytest.raises(ValueError, match="Point"):
        P.from_geojson({"type": "FeatureCollection", "features": [feat, {"type": "Feature", "properties": {}, "geometry": point}]})
    with pytest.raises(ValueError, match="LineString"):
        P.from_geojson({"type": "LineString", "coordinates": [[0, 0], [1, 1]]})
    ps = P.from_geojson([point, feat, {"type": "Feature", "properties": {}, "geometry": point}], ignore_other=True)
    assert ps.n_shapes == 1
    assert P.from_geojson({"type": "FeatureCollection", "features": []}).n_shapes == 0


def test_from_rings_layout_and_quantisation():
    assert P.quantize(np.array([0.03125, 0.09375, 0.15625, -0.03125, -0.09375, 2.5]), 4).tolist() == [0, 2, 2, 0, -2, 40]   # ties to even
    assert P.quantize(np.array([0.5, 1.5, 2.5, -0.5]), 0).tolist() == [0, 2, 2, 0]
    ring = np.array([[0, 0], [0, 3], [2, 3]], np.int32)
    ps = P.from_rings([[ring, [ring, ring + 1]], [], [ring.astype(np.float64) / 2]], sub=0)
    assert ps.n_images == 3 and ps.n_shapes == 3 and ps.image_shapes.tolist() == [0, 2, 2, 3] and ps.shape_rings.tolist() == [0, 1, 3, 4]
    assert ps.ring_start.tolist() == [0, 3, 6, 9] and ps.ring_count.tolist() == [3, 3, 3, 3]
    assert np.array_equal(ps.vertices[:3].numpy(), ring) and ps.vertices[9:].tolist() == [[0, 0], [0, 2], [1, 2]]
    assert all(getattr(ps, k).dtype == torch.int32 for k in P._TABLES)
    assert P.from_rings([[ring]], sub=3).vertices.tolist() == (ring << 3).tolist()
    assert P.from_rings([[ring[:, ::-1]]], sub=0, xy=True).vertices.tolist() == ring.tolist()
    assert P.from_rings([[np.concatenate([ring, ring[:1]])]], sub=0).ring_count.tolist() == [3]
    assert P.from_rings([[torch.from_numpy(ring)]], sub=0).vertices.tolist() == ring.tolist()
    # a list of rings is told from a ring by its first element that is not empty
    ps = P.from_rings([[[[], ring.tolist()], [[], []], [np.zeros((0, 2)), ring], ring.tolist(), []]], sub=0)
    assert ps.shape_rings.tolist() == [0, 2, 4, 6, 7, 7] and ps.ring_count.tolist() == [0, 3, 0, 0, 0, 3, 3]
    assert P.from_rings([[np.array([[0.0, 0.0], [0.0, 2.0 ** 27 + 0.2], [1.0, 1.0]])]], sub=1).vertices[1].tolist() == [0, 1 << 28]
    with pytest.raises(ValueError, match="image 0 shape 0.*2\\^28"):
        P.from_rings([[np.array([[0, 0], [0, (1 << 27) + 1], [1, 1]])]], sub=1)
    with pytest.raises(ValueError, match="2\\^28"):
        P.from_rings([[np.array([[0.0, 0.0], [0.0, 2.0 ** 28], [1.0, 1.0]])]], sub=1)
    with pytest.raises(ValueError, match="sub"):
        P.from_rings([[ring]], sub=9)


@pytest.mark.parametrize("band", [1, 3, 64, None])
def test_planner_tiles_every_shape_once(band):
    rng = np.random.default_rng(3)
    H, W, sub = 70, 90, 4
    shapes = [[random_polygon(rng, H, W, sub, margin=30.0)] for _ in range(40)]
    shapes += [[np.zeros((0, 2), np.int64)], [np.array([[5, 5]])], [np.array([[-900, 3], [-800, 40], [-850, 9]])],
               [np.array([[8, 0], [8, 64], [24, 64]])]]                     # empty, one vertex, wholly above, centre lines on vertices
    ps = P.from_rings([shapes[:20], shapes[20:]], sub=0)
    ps.sub = sub                                                           # the integers above are units of 1/16 pixel already
    items = P.plan(ps, (H, W), band)
    assert items.dtype == np.int32 and items.shape[1] == 3 and (items[:, 2] >= 1).all() and (items[:, 2] <= (band or P.BAND_ROWS)).all()
    S = 1 << sub
    for s, (ring,) in enumerate(shapes):
        mine = items[items[:, 0] == s]
        rows = np.concatenate([np.arange(a, a + n) for _, a, n in mine]) if len(mine) else np.zeros(0, int)
        want = [i for i in range(H) if len(ring) and 2 * int(ring[:, 0].min()) <= (2 * i + 1) * S < 2 * int(ring[:, 0].max())]
        assert rows.tolist() == want, s                                    # in order, each exactly once
    assert (np.diff(items[:, 0]) >= 0).all()
    with pytest.raises(ValueError, match="band_rows"):
        P.plan(ps, (H, W), 0)


def test_argument_errors_come_before_the_library(monkeypatch):
    def no_load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_load)
    ring = np.array([[0, 0], [0, 3], [2, 3]], np.int32)
    ps = P.from_rings([[ring, ring + 1]], sub=0)
    with pytest.raises(ValueError, match="rule"):
        P.rasterize(ps, (4, 4), rule="winding")
    with pytest.raises(ValueError, match="mode"):
        P.rasterize(ps, (4, 4), mode="image")
    with pytest.raises(TypeError, match="PolygonSet"):
        P.rasterize([ring], (4, 4))
    with pytest.raises(TypeError, match="image_hw"):
        P.rasterize(ps, 4)
    for name in P._TABLES:
        bad = P.PolygonSet(**{**{k: getattr(ps, k) for k in P._TABLES}, name: getattr(ps, name).long()}, sub=0)
        with pytest.raises(TypeError, match=name):
            P.rasterize(bad, (4, 4))
    tabs = {k: getattr(ps, k) for k in P._TABLES}
    ragged = [{"ring_count": torch.tensor([3, 4], dtype=torch.int32)}, {"ring_start": torch.tensor([-1, 3], dtype=torch.int32)},
              {"ring_count": torch.tensor([3, -1], dtype=torch.int32)}, {"shape_rings": torch.tensor([0, 2, 1], dtype=torch.int32)},
              {"shape_rings": torch.tensor([0, 1, 3], dtype=torch.int32)}, {"image_shapes": torch.tensor([0, 3], dtype=torch.int32)},
              {"image_shapes": torch.tensor([1, 2], dtype=torch.int32)}, {"ring_count": torch.tensor([3], dtype=torch.int32)},
              {"vertices": ps.vertices.reshape(-1)}, {"image_shapes": torch.tensor([2], dtype=torch.int32)}]
    for change in ragged:
        with pytest.raises(ValueError):
            P.rasterize(P.PolygonSet(**{**tabs, **change}, sub=0), (4, 4))
    far = P.PolygonSet(**{**tabs, "vertices": ps.vertices * (1 << 27)}, sub=0)
    with pytest.raises(ValueError, match="2\\^28"):
        P.rasterize(far, (4, 4))
    with pytest.raises(ValueError, match="sub"):
        P.rasterize(P.PolygonSet(**tabs, sub=9), (4, 4))
    with pytest.raises(ValueError, match="2\\^31"):
        P.rasterize(ps, (1 << 16, 1 << 15))
    with pytest.raises(ValueError, match="2\\^30"):
        P.rasterize(P.PolygonSet(**tabs, sub=8), (1 << 21, 4))
    with pytest.raises(ValueError, match="65535"):
        P.rasterize(P.PolygonSet(ps.vertices, ps.ring_start, ps.ring_count, ps.shape_rings,
                                 torch.cat([torch.zeros(65535, dtype=torch.int32), ps.image_shapes]), 0), (4, 4))
    with pytest.raises(ValueError, match="values"):
        P.rasterize(ps, (4, 4), values=np.array([1, 2, 3], np.int32))
    with pytest.raises(TypeError, match="values"):
        P.rasterize(ps, (4, 4), values=np.array([1.0, 2.0]))
    with pytest.raises(ValueError, match="values"):
        P.rasterize(ps, (4, 4), mode="mask", values=np.array([1, 2], np.int32))
    with pytest.raises(TypeError, match="out"):
        P.rasterize(ps, (4, 4), out=torch.zeros((1, 4, 4), dtype=torch.uint8))
    with pytest.raises(TypeError, match="out"):
        P.rasterize(ps, (4, 4), out=torch.zeros((1, 4, 5), dtype=torch.int32))
    with pytest.raises(ValueError, match="device"):
        P.rasterize(ps, (4, 4), out=torch.zeros((1, 4, 4), dtype=torch.int32))
    with pytest.raises(ValueError, match="GPU"):
        P.rasterize(ps, (4, 4), device="cpu")
    with pytest.raises(ValueError, match="band_rows"):
        P.rasterize(ps, (4, 4), _band_rows=0)


def test_detect_slide_roi_errors_come_first(monkeypatch):
    from cellsegmentation_amd import inference

    def no_load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_load)
    img = np.zeros((40, 50, 3), np.uint8)
    ring = np.array([[0, 0], [0, 3], [2, 3]], np.int32)
    for bad, err in ((np.zeros((40, 51), np.uint8), TypeError), (np.zeros((40, 50), np.float32), TypeError), ("roi.json", TypeError),
                     (P.from_rings([[ring], [ring]], sub=0), ValueError), ({"type": "Point", "coordinates": [0, 0]}, ValueError)):
        with pytest.raises(err):
            inference.detect_slide(img, None, patch_size=32, roi=bad)
    import inspect
    assert inspect.signature(inference.detect_slide).parameters["roi"].default is None
    assert [f for f in inference.SlideResult.__dataclass_fields__] == ["points", "discarded", "cell_count", "mask", "tissue"]
    assert inference.SlideResult.roi is None


def test_a_host_roi_is_planned(monkeypatch):
    """detect_slide's ROI: a host-side set (GeoJSON, from_rings) reaches rasterize on the host, where it is planned and cut into
    bands; nothing is moved to the device first"""
    seen = []
    monkeypatch.setattr(P, "rasterize", lambda pset, hw, **kw: seen.append((pset, hw, kw)) or torch.zeros((1,) + tuple(hw), dtype=torch.uint8))
    ring = [[20.5, 10.25], [120.0, 14.0], [124.75, 60.5], [30.0, 70.0], [20.5, 10.25]]
    dev = torch.device("cuda:0")
    for roi in ({"type": "Polygon", "coordinates": [ring]}, P.from_rings([[np.array(ring)]], xy=True)):
        out = P.roi_mask(roi, (150, 170))(dev)
        pset, hw, kw = seen.pop()
        assert tuple(out.shape) == (150, 170) and hw == (150, 170) and kw == {"mode": "mask", "device": dev}
        assert not pset.vertices.is_cuda and len(P.plan(pset, hw)) == -(-60 // P.BAND_ROWS)     # rows 10 .. 69
