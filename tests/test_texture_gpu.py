"""Per-cell texture tables on the GPU (csrc/regions.hip, texture_kernel, through cellsegmentation_amd.kernels.texture_labels,
regions.texture_labels, stain.texture_labels, ``TextureTable`` and inference.slide_texture), exact against the numpy restatement
tests/texture_ref.py and the vectors of tests/golden/texture_vectors.npz: every integer table by value, the float64 methods within
1e-12 max(1, |want|) of numpy on the same integers (sums of at most 2L - 1 = 63 non-negative terms, ``variance`` and
``correlation`` from exact integers at these sizes).  Shapes are the smallest at which each mechanism can go wrong: the 3 x 4 hand
case, widths either side of the 64-lane steps with one to three rows, labels at the image's sides and thinner than the distance,
and one 256 x 300 image under a single label for the contention on one counter and the int64 sums.

The hand case: labels [[1,1,1,2],[1,1,2,2],[0,1,2,-3]] over the plane [[0,40,40,255],[100,40,255,200],[7,250,31,9]] with L = 8 and
d = 1 have the grey levels [[0,1,1,7],[3,1,7,6],[0,7,0,0]].

The rows of ``pattern`` (before their shift):  1 1 1 1 1 2 2 2 2 2 . -5 4 4 4 4 4 4 4 4 4 . . .   label 3 owns nothing, label 5
covers columns 58 .. 70: two labels side by side, a label below zero and a run across the 64-lane boundary."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import quantify_ref as Q  # noqa: E402
import regions_ref as R  # noqa: E402
import split_ref as SR  # noqa: E402
import stain_ref  # noqa: E402
import texture_ref as T  # noqa: E402
from cellsegmentation_amd import inference, stain  # noqa: E402
from cellsegmentation_amd import kernels as K  # noqa: E402
from cellsegmentation_amd import regions as G  # noqa: E402
from shifted import guards_intact, shifted  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "texture_vectors.npz"), allow_pickle=False)
NAMES = [str(n) for n in GOLD["names"]]
TABLES = ("pairs", "diff", "sum", "marg", "sq", "cross", "matrix")
TOL = 1e-12


def _np(t):
    return None if t is None else t.cpu().numpy()


def up(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def raw(dev, labels, cap, plane=None, images=None, Mq=None, levels=16, distance=1, want_matrix=False):
    """the kernel wrapper on numpy operands, the boxes from measure_labels -> the dict of device tensors"""
    lab = up(labels, dev)
    bbox = G.measure_labels(lab, max_regions=cap).bbox
    od = None if images is None else torch.from_numpy(stain.od_table(240)).to(dev)
    return K.texture_labels(lab, cap, bbox, up(plane, dev), up(images, dev), od, up(None if Mq is None else np.asarray(Mq, np.int32), dev),
                            levels, distance, want_matrix)


def assert_tables(got, want):
    """got: a TextureTable or the wrapper's dict; want: the reference's dict"""
    get = (lambda k: got.get(k)) if isinstance(got, dict) else (lambda k: getattr(got, k))
    for k in TABLES:
        if k == "matrix" and "matrix" not in want:
            assert get("matrix") is None
        else:
            g = _np(get(k))
            assert g.shape == want[k].shape and g.dtype == (np.int64 if k in ("sq", "cross") else np.int32), k
            assert np.array_equal(g.astype(np.int64), want[k]), k


def close(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and \
        bool((np.abs(got[~nan] - want[~nan]) <= TOL * np.maximum(1.0, np.abs(want[~nan]))).all())


def assert_methods(table, ref):
    for m in T.METHODS + (("entropy",) if "matrix" in ref else ()):
        want = T.method(ref, m)
        got, avg = getattr(table, m)(), getattr(table, m)(average=True)
        assert got.is_cuda and got.dtype == torch.float64
        assert close(_np(got), want), m
        assert close(_np(avg), T.averaged(want)), m


def pattern(rows, W):
    lab = np.zeros((rows, W), np.int32)
    base = np.zeros(max(W, 80), np.int32)
    base[0:5], base[5:10], base[11], base[12:21], base[58:71] = 1, 2, -5, 4, 5
    for r in range(rows):
        lab[r] = np.roll(base, 7 * r)[:W]
    return lab[None]


def test_hand_case(dev):
    t = raw(dev, T.HAND_LABELS, 2, T.HAND_PLANE, levels=8, distance=1, want_matrix=True)
    assert _np(t["pairs"])[0].tolist() == [[3, 2, 3, 2], [1, 0, 2, 2]]
    assert _np(t["diff"])[0, 0, 0, :5].tolist() == [2, 2, 2, 0, 0] and _np(t["marg"])[0, 0, 0].tolist() == [1, 4, 0, 1, 0, 0, 0, 0]
    assert (int(t["sq"][0, 0, 0]), int(t["cross"][0, 0, 0])) == (8, 8)
    assert _np(t["diff"])[0, 0, 1, :5].tolist() == [0, 2, 0, 0, 2] and (int(t["sq"][0, 0, 1]), int(t["cross"][0, 0, 1])) == (4, 42)
    assert (int(t["sq"][0, 1, 0]), int(t["cross"][0, 1, 0])) == (2, 84)
    assert all(int(t[k][0, 1, 1].abs().sum()) == 0 for k in TABLES)
    assert _np(t["marg"])[0, 1, 3].tolist() == [1, 0, 0, 0, 0, 0, 1, 2] and (int(t["sq"][0, 1, 3]), int(t["cross"][0, 1, 3])) == (6, 98)
    assert_tables(t, T.texture(T.HAND_PLANE, T.HAND_LABELS, 2, 8, 1, want_matrix=True))
    assert_tables(raw(dev, T.HAND_LABELS, 1, T.HAND_PLANE, levels=8), T.texture(T.HAND_PLANE, T.HAND_LABELS, 1, 8, 1))


@pytest.mark.parametrize("W", [63, 64, 65, 129])
def test_widths_around_the_lane_steps(dev, W):
    rng = np.random.RandomState(W)
    for rows, (L, d) in ((1, (8, 1)), (2, (16, 2)), (3, (32, 3)), (3, (8, 1)), (2, (32, 1))):
        lab = pattern(rows, W)
        plane = rng.randint(0, 256, size=(1, rows, W)).astype(np.uint8)
        want = T.texture(plane, lab, 5, L, d, want_matrix=True)
        got = G.texture_labels(lab, plane, levels=L, distance=d, max_regions=5, want_matrix=True)
        assert got.levels == L and got.distance == d and got.table.capacity == 5 and got.Mq is None
        assert_tables(got, want)
        assert want["pairs"][0, 2].sum() == 0 and want["pairs"][0, 3, 0] > 0                        # label 3 owns nothing
        assert_methods(got, want)
        short = G.texture_labels(lab[0], plane[0], levels=L, distance=d, max_regions=3)
        assert_tables(short, T.texture(plane, lab, 3, L, d))                                         # labels 4 and 5: counted, not measured
        assert _np(short.overflowed()).tolist() == [True] and _np(short.table.counts).tolist() == [5]


def test_edges_of_the_image_and_of_a_label(dev):
    rng = np.random.RandomState(11)
    # a label that touches all four borders, with a hole of another label and of background
    lab = np.ones((1, 9, 11), np.int32)
    lab[0, 3:5, 4:8], lab[0, 6, 2] = 2, 0
    plane = rng.randint(0, 256, size=(1, 9, 11)).astype(np.uint8)
    for L, d in ((8, 1), (16, 3), (32, 8)):
        want = T.texture(plane, lab, 2, L, d, want_matrix=True)
        assert want["pairs"][0, 0].min() > 0
        assert_tables(raw(dev, lab, 2, plane, levels=L, distance=d, want_matrix=True), want)
    # a label narrower and lower than d: no direction has a pair and every method is NaN
    small = np.zeros((1, 7, 9), np.int32)
    small[0, 2:4, 3:5] = 1
    plane = rng.randint(0, 256, size=(1, 7, 9)).astype(np.uint8)
    got = G.texture_labels(small, plane, levels=8, distance=2, max_regions=1, want_matrix=True)
    want = T.texture(plane, small, 1, 8, 2, want_matrix=True)
    assert int(np.abs(want["pairs"]).sum()) == 0 and all(int(_np(getattr(got, k)).any()) == 0 for k in TABLES)
    assert_tables(got, want)
    for m in T.METHODS + ("entropy",):
        assert np.isnan(_np(getattr(got, m)())).all() and np.isnan(_np(getattr(got, m)(average=True))).all()
    # a label in column 0 (the (d, -d) partner would lie at column -d) and one in the last column and row
    side = np.zeros((1, 6, 8), np.int32)
    side[0, :, 0:2], side[0, 3:, 6:] = 1, 2
    plane = rng.randint(0, 256, size=(1, 6, 8)).astype(np.uint8)
    for d in (1, 2):
        want = T.texture(plane, side, 2, 16, d)
        assert want["pairs"][0, 0, 3] == (6 - d) * (2 - d) and want["pairs"][0, 0, 2] == 2 * (6 - d)
        assert_tables(raw(dev, side, 2, plane, levels=16, distance=d), want)
    # two pieces of label 1 exactly d apart with label 2 between them: the pieces pair, label 2 pairs with neither
    apart = np.asarray([[[1, 2, 1, 0], [1, 2, 1, 0], [0, 0, 0, 0], [1, 0, 1, 0]]], np.int32)
    plane = np.asarray([[[10, 90, 200, 0], [50, 90, 250, 0], [0, 0, 0, 0], [130, 0, 70, 0]]], np.uint8)
    want = T.texture(plane, apart, 2, 8, 2, want_matrix=True)
    assert want["pairs"][0].tolist() == [[3, 1, 2, 1], [0, 0, 0, 0]]
    assert_tables(raw(dev, apart, 2, plane, levels=8, distance=2, want_matrix=True), want)


def test_one_label_over_one_value(dev):
    """76 800 pixels of one grey level under one label: every add of a direction goes to one counter, sq = (2 pairs)^2 > 2^32"""
    H, W, d, L, value = 256, 300, 2, 16, 200
    g = value * L >> 8
    plane, lab = np.full((1, H, W), value, np.uint8), np.ones((1, H, W), np.int32)
    a, b = (raw(dev, lab, 1, plane, levels=L, distance=d, want_matrix=True) for _ in range(2))
    pairs = [H * (W - d), (H - d) * (W - d), (H - d) * W, (H - d) * (W - d)]
    assert _np(a["pairs"])[0, 0].tolist() == pairs
    for k, p in enumerate(pairs):
        assert int(a["diff"][0, 0, k, 0]) == int(a["sum"][0, 0, k, 2 * g]) == int(a["marg"][0, 0, k, g]) == int(a["matrix"][0, 0, k, g, g]) == 2 * p
        assert int(a["sq"][0, 0, k]) == (2 * p) ** 2 > 1 << 32 and int(a["cross"][0, 0, k]) == g * g * 2 * p
        assert int(a["diff"][0, 0, k].sum()) == int(a["sum"][0, 0, k].sum()) == int(a["marg"][0, 0, k].sum()) == int(a["matrix"][0, 0, k].sum()) == 2 * p
    assert all(torch.equal(a[k], b[k]) for k in a)
    noise = np.random.RandomState(9).randint(0, 256, size=(1, H, W)).astype(np.uint8)
    blocks = T.blocks(H, W, seed=2, n_labels=40)[None]
    assert_tables(raw(dev, blocks, 40, noise, levels=32, distance=1, want_matrix=True), T.texture_fast(noise, blocks, 40, 32, 1, want_matrix=True))


def test_stain_route(dev):
    rng = np.random.RandomState(5)
    lab = np.stack([T.blocks(20, 70, seed=s, n_labels=4 + s) for s in range(2)])
    img = rng.randint(0, 256, size=(2, 20, 70, 3)).astype(np.uint8)
    for s, residual, L, d in ((0, False, 16, 1), (1, False, 32, 2), (2, True, 8, 1)):
        Mq = Q.quantised_matrix(Q.HDAB, residual, 2.5)[s]
        levels = Q.levels(img, Mq[None])[..., 0].astype(np.uint8)             # the reference's own levels of that stain
        got = stain.texture_labels(img, lab, stain=s, residual=residual, levels=L, distance=d, max_regions=5, want_matrix=True,
                                   options=stain.StainOptions(conc_max=2.5))
        assert np.array_equal(got.Mq, np.stack([Mq, Mq])) and got.Mq.dtype == np.int32 and got.options.conc_max == 2.5
        assert_tables(got, T.texture_fast(levels, lab, 5, L, d, want_matrix=True))
        assert_tables(G.texture_labels(lab, levels, levels=L, distance=d, max_regions=5, want_matrix=True),
                      T.texture_fast(levels, lab, 5, L, d, want_matrix=True))


def test_stain_route_clamps_and_a_matrix_per_image(dev):
    lab = np.concatenate([pattern(2, 65)] * 3)
    img = np.random.RandomState(3).randint(0, 256, size=(3, 2, 65, 3)).astype(np.uint8)
    img[1] = 0                                                             # od_q[0] 2^24 >> 24 = 22449: clamps to 255
    Mq = np.stack([Q.quantised_matrix(Q.HDAB, False, 0.7)[0], [1 << 24, 0, 0], [-(1 << 24), 3, 0]])
    acc = Q.od_table(240)[img[0]] @ Mq[0] + (1 << 23)
    assert (acc < 0).any() and ((acc >> 24) > 255).any()                   # both clamps bite under Ruifrok's vectors
    levels = np.stack([Q.levels(img[n], Mq[n][None])[..., 0] for n in range(3)]).astype(np.uint8)
    assert (levels[1] == 255).all() and (levels[2] == 0).all()
    for L, d in ((16, 1), (8, 2)):
        assert_tables(raw(dev, lab, 5, images=img, Mq=Mq, levels=L, distance=d, want_matrix=True),
                      T.texture(levels, lab, 5, L, d, want_matrix=True))


@pytest.mark.parametrize("shift_img,shift_lab", [(1, 4), (2, 8), (3, 12), (5, 0), (7, 4)])
def test_misaligned_plane_image_and_labels(dev, shift_img, shift_lab):
    rng = np.random.RandomState(shift_img)
    lab = pattern(3, 129)
    plane = rng.randint(0, 256, size=(1, 3, 129)).astype(np.uint8)
    img = rng.randint(0, 256, size=(1, 3, 129, 3)).astype(np.uint8)
    Mq = Q.quantised_matrix(Q.HDAB, False, 8.0)[:1]
    bbox = G.measure_labels(lab, max_regions=5).bbox
    p, fp, sp = shifted(plane, shift_img, dev)
    x, fx, sx = shifted(img, shift_img, dev)
    l, fl, sl = shifted(lab, shift_lab, dev)
    assert_tables(K.texture_labels(l, 5, bbox, plane=p, levels=16, distance=1), T.texture(plane, lab, 5, 16, 1))
    od = torch.from_numpy(stain.od_table(240)).to(dev)
    got = K.texture_labels(l, 5, bbox, images_u8=x, od_q=od, Mq=torch.from_numpy(Mq.astype(np.int32)).to(dev), levels=8, distance=2)
    assert_tables(got, T.texture(Q.levels(img, Mq)[..., 0], lab, 5, 8, 2))
    assert guards_intact(fp, sp) and guards_intact(fx, sx) and guards_intact(fl, sl)


def test_front_end_modes_and_given_tables(dev):
    rng = np.random.RandomState(12)
    lab = np.stack([T.blocks(20, 70, seed=s, n_labels=4 + s) for s in range(2)])
    plane = rng.randint(0, 256, size=(2, 20, 70)).astype(np.uint8)
    region = G.measure_labels(lab)
    cap = region.capacity
    want = T.texture_fast(plane, lab, cap, 16, 1, want_matrix=True)
    with_table = G.texture_labels(torch.from_numpy(lab).to(dev), torch.from_numpy(plane).to(dev), table=region, want_matrix=True)
    assert with_table.table is region and with_table.pairs.is_cuda and with_table.sq.dtype == torch.int64
    assert_tables(with_table, want)
    fixed = G.texture_labels(lab, plane, max_regions=cap, want_matrix=True)
    found = G.texture_labels(lab, plane, want_matrix=True)
    given = G.texture_labels(lab, plane, counts=region.counts.cpu(), want_matrix=True)
    for t in (fixed, found, given):
        assert t.table.capacity == cap and _np(t.table.counts).tolist() == _np(region.counts).tolist() and not _np(t.overflowed()).any()
        assert_tables(t, want)
    bare = G.texture_labels(lab, plane, table=region)
    assert bare.matrix is None
    assert_tables(bare, {k: v for k, v in want.items() if k != "matrix"})
    with pytest.raises(ValueError, match="without the matrix"):
        bare.entropy()
    per = found.per_image()
    assert [len(p["pairs"]) for p in per] == _np(region.counts).tolist() and np.array_equal(per[1]["sum"], want["sum"][1, :len(per[1]["pairs"])])
    # tables that the caller passes are the ones written
    mine = {"pairs": torch.full((2, cap, 4), -7, dtype=torch.int32, device=dev), "sq": torch.full((2, cap, 4), -7, dtype=torch.int64, device=dev)}
    out = K.texture_labels(torch.from_numpy(lab).to(dev), cap, region.bbox, plane=torch.from_numpy(plane).to(dev), **mine)
    assert out["pairs"] is mine["pairs"] and out["sq"] is mine["sq"] and "matrix" not in out
    assert_tables(out, {k: v for k, v in want.items() if k != "matrix"})


def test_batches_in_chunks_of_whole_images(dev, monkeypatch):
    rng = np.random.RandomState(21)
    lab = np.stack([T.blocks(12, 40, seed=s, n_labels=3 + s % 3) for s in range(5)])
    plane = rng.randint(0, 256, size=(5, 12, 40)).astype(np.uint8)
    img = rng.randint(0, 256, size=(5, 12, 40, 3)).astype(np.uint8)
    stains = [Q.HDAB, Q.HDAB[:, ::-1]] * 2 + [Q.HDAB]                       # a matrix per image goes with its chunk
    Mq = np.stack([Q.quantised_matrix(s)[1] for s in stains])
    levels = np.stack([Q.levels(img[n], Mq[n][None])[..., 0] for n in range(5)])
    want, want_rgb = T.texture_fast(plane, lab, 5, 16, 1, want_matrix=True), T.texture_fast(levels, lab, 5, 8, 2)
    monkeypatch.setattr(G, "_MAX_PIXELS", 2 * 12 * 40 + 5)                 # two images per call: 2 + 2 + 1
    assert [b - a for a, b in G._chunks(torch.empty(5, 12, 40))] == [2, 2, 1]
    assert_tables(G.texture_labels(lab, plane, max_regions=5, want_matrix=True), want)
    got = stain.texture_labels(img, lab, stains, stain=1, levels=8, distance=2, max_regions=5)
    assert np.array_equal(got.Mq, Mq)
    assert_tables(got, want_rgb)


def test_graph_replay(dev):
    rng = np.random.RandomState(14)
    cap = 4                                                                # below the largest label
    static_lab = torch.zeros((2, 30, 70), dtype=torch.int32, device=dev)
    static_plane = torch.zeros((2, 30, 70), dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        G.texture_labels(static_lab, static_plane, levels=32, distance=2, max_regions=cap, want_matrix=True)    # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tt = G.texture_labels(static_lab, static_plane, levels=32, distance=2, max_regions=cap, want_matrix=True)
    for seed in (12, 13):
        lab = np.stack([T.blocks(30, 70, seed=seed + s, n_labels=6) for s in range(2)])
        plane = rng.randint(0, 256, size=(2, 30, 70)).astype(np.uint8)
        static_lab.copy_(torch.from_numpy(lab).to(dev))
        static_plane.copy_(torch.from_numpy(plane).to(dev))
        graph.replay()
        assert_tables(tt, T.texture_fast(plane, lab, cap, 32, 2, want_matrix=True))
        assert _np(tt.table.counts).tolist() == [int(x.max()) for x in lab]


@pytest.mark.parametrize("name", NAMES)
def test_golden_vectors(dev, name):
    g = lambda k: GOLD[f"{name}.{k}"]  # noqa: E731
    want = {k: g(k) for k in TABLES if f"{name}.{k}" in GOLD.files}
    got = G.texture_labels(g("labels"), g("plane"), levels=int(g("levels")), distance=int(g("distance")), max_regions=int(g("capacity")),
                           want_matrix=bool(g("want_matrix")))
    assert_tables(got, want)
    assert_methods(got, want)
    assert _np(got.overflowed()).any() == (name == "wide_40x130_short")


def test_slide_texture(dev):
    centres = np.asarray([(30, 20), (30, 42), (30, 64), (52, 31), (12, 86)], np.int64)
    mask = SR.discs(72, 100, centres, 13)
    pts = np.concatenate([centres, [[2, 2]]])                           # a detection on the background: an all-zero row, all NaN
    result = inference.SlideResult(pts, [], len(pts), torch.from_numpy(mask.astype(np.uint8) * 255).to(dev))
    img = stain_ref.synth_hdab(72, 100, seed=5)
    cells, table, parts = inference.slide_texture(result, img, stains=stain.HDAB)
    assert isinstance(cells, G.TextureTable) and isinstance(table, G.RegionTable) and isinstance(parts, G.SplitResult)
    labels = _np(parts.labels).reshape(1, 72, 100)
    assert np.array_equal(labels[0], SR.split(R.remove_small_regions(mask, 300, 100, 1), pts)["labels"])
    Mq = Q.quantised_matrix()
    want = T.texture_fast(Q.levels(img[None], Mq[:1])[..., 0], labels, table.capacity, 16, 1)
    assert cells.table is table and table.capacity == len(pts) and cells.levels == 16 and cells.distance == 1
    assert np.array_equal(cells.Mq, Mq[:1]) and (want["pairs"][0, :5] > 0).all()
    assert_tables(cells, want)
    assert_methods(cells, want)
    assert all(int(_np(getattr(cells, k))[0, 5].any()) == 0 for k in TABLES[:-1])                    # row k is point k: the dead point
    assert all(np.isnan(_np(getattr(cells, m)())[0, 5]).all() and np.isnan(_np(getattr(cells, m)(average=True))[0, 5]) for m in T.METHODS)
    assert np.isfinite(_np(cells.contrast(average=True))[0, :5]).all()
    # the DAB plane at another resolution, a device image and a fixed capacity
    cells, table, _ = inference.slide_texture(result, torch.from_numpy(img).to(dev), stains=stain.HDAB, stain=1, levels=32, distance=2,
                                              max_regions=8)
    assert_tables(cells, T.texture_fast(Q.levels(img[None], Mq[1:])[..., 0], labels, 8, 32, 2))
    assert table.capacity == 8 and np.array_equal(cells.Mq, Mq[1:])
    # stains=None: the slide's own estimate
    cells, _, _ = inference.slide_texture(result, img)
    est = stain.estimate(img)
    assert np.array_equal(cells.Mq[0], stain.quantised_matrix(est)[0])
    assert_tables(cells, T.texture_fast(Q.levels(img[None], cells.Mq)[..., 0], labels, 6, 16, 1))
