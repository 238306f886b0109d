"""DBSCAN clustering on the GPU (csrc/spatial.hip through cellsegmentation_amd.spatial.cluster), bit-exact against the brute-force
numpy restatement tests/cluster_ref.py: the vectors scikit-learn wrote, every bucket side on a lattice full of d2 == r2 ties, chains
across many workgroups in every row order, border semantics, a bucket that overflows the LDS chunk and the workgroup with every
union on one root, live rules, ragged batches, repeatability, graph replay, DetectResult.cluster and inference.slide_clusters.
Every comparison is exact integer equality over every row of every column."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cluster_ref as C  # noqa: E402
from cellsegmentation_amd import detect as D  # noqa: E402
from cellsegmentation_amd import spatial as S  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "cluster_vectors.npz"), allow_pickle=False)
NAMES = [str(n) for n in GOLD["names"]]
HW = (61, 45)
COLUMNS = ("labels", "core", "n_clusters", "size", "n_core", "sums", "bbox")


def same(got, want, what):
    got = got.cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    bad = np.argwhere(got != want)
    assert not len(bad), (what, bad[:5].tolist(), [got[tuple(b)] for b in bad[:5]], [want[tuple(b)] for b in bad[:5]])


def check(pts, hw, eps, min_samples, off=None, limits=None, buckets=(None,), want=None):
    """spatial.cluster at every bucket side of ``buckets`` against the restatement (computed once), every column"""
    want = want or C.cluster(pts, hw, eps, min_samples, off, limits)
    for b in buckets:
        t = S.cluster(pts, hw, eps, min_samples, offsets=off, limits=limits, _bucket=b)
        assert t.radius2 == C.radius_squared(eps) and t.min_samples == min_samples
        for k in COLUMNS:
            same(getattr(t, k), want[k], (k, b))
    return want


def test_golden_cases_as_one_batch_and_one_by_one(dev):
    by_rule = {}
    for n in NAMES:
        by_rule.setdefault((float(GOLD[f"{n}.eps"]), int(GOLD[f"{n}.min_samples"])), []).append(n)
    assert len(by_rule) >= 8
    for n in NAMES:
        check(GOLD[f"{n}.pts"], HW, float(GOLD[f"{n}.eps"]), int(GOLD[f"{n}.min_samples"]), buckets=(None, 5),
              want={k: GOLD[f"{n}.{k}"] for k in COLUMNS})
    # one ragged batch per rule, each padded with every other case's points: images share nothing, and the tables of image n start
    # at its own offset
    for (eps, ms), mine in by_rule.items():
        names = mine + [n for n in NAMES if n not in mine]
        pts, off = C.ragged([GOLD[f"{n}.pts"] for n in names])
        want = check(pts, HW, eps, ms, off, buckets=(None, 5))
        for i, n in enumerate(mine):
            rows = slice(off[i], off[i + 1])
            for k in COLUMNS[:2] + COLUMNS[3:]:
                assert np.array_equal(want[k][rows], GOLD[f"{n}.{k}"]), (n, k)
            assert want["n_clusters"][i] == GOLD[f"{n}.n_clusters"][0]


def test_bucket_side_independence_on_a_lattice_of_ties(dev):
    lattice = np.stack(np.meshgrid(np.arange(8), np.arange(8), indexing="ij"), axis=-1).reshape(-1, 2) * 3 + 2
    pts = np.concatenate([lattice, lattice[[0, 9, 9, 27, 63]]])                               # distance 0 between distinct rows
    pts = pts[(pts[:, 0] + pts[:, 1]) % 7 != 0]                                               # holes: core, border and noise all occur
    H, W = 29, 31
    for eps, ms in ((3, 3), (3, 4), (3, 5), (4.5, 6), (2.5, 2), (0, 2), (3, 1)):             # d2 == 9 == r2 between lattice neighbours
        want = check(pts, (H, W), eps, ms, buckets=(None, 1, 3, 4, max(H, W)))
        if (eps, ms) == (3, 4):
            live = want["labels"] >= -1
            assert (want["labels"] == -1).any() and ((want["labels"] >= 0) & (want["core"] == 0)).any() and want["core"].any() and live.all()


@pytest.mark.parametrize("order", ["forward", "reversed", "shuffled"])
def test_chain_across_many_workgroups(dev, order):
    eps, n = 4, 200
    idx = {"forward": np.arange(n), "reversed": np.arange(n)[::-1], "shuffled": np.random.RandomState(5).permutation(n)}[order]
    line = np.stack([np.full(n, 1), idx * eps], axis=1)                                       # every point in a bucket of its own
    want = check(line, (4, 1024), eps, 2, buckets=(4, None))
    assert want["n_clusters"].tolist() == [1] and (want["labels"] == 0).all() and want["size"][0] == n and want["core"].all()
    assert want["bbox"][0].tolist() == [1, 0, 2, (n - 1) * eps + 1]
    # two chains and a loner in between: the numbers follow the smallest core row, whichever end of the line it lies at
    cut = np.delete(line, np.nonzero((idx >= 90) & (idx < 93) & (idx != 91))[0], axis=0)
    want = check(cut, (4, 1024), eps, 2, buckets=(4, None))
    first = want["labels"][np.argmax(want["core"])]
    assert want["n_clusters"].tolist() == [2] and first == 0 and (want["labels"] == -1).sum() == 1
    assert sorted(want["size"][:2].tolist()) == [90, 107]
    apart = np.stack([np.full(n, 1), idx * (eps + 1)], axis=1)
    want = check(apart, (4, 1024), eps, 2, buckets=(4, None))
    assert want["n_clusters"].tolist() == [0] and (want["labels"] == -1).all() and not want["size"].any()


def test_border_semantics(dev):
    left = np.asarray([(20, 18), (19, 18), (21, 18), (20, 17), (19, 17), (21, 17), (20, 16)])
    right = left * (1, -1) + (0, 44)
    bridge = np.asarray([(20, 22)])                                                           # 4 from (20, 18) and from (20, 26)
    for pts, at, label in ((np.concatenate([bridge, left, right]), 0, 0), (np.concatenate([right, left, bridge]), 14, 0),
                           (np.concatenate([right, bridge, left]), 7, 0)):
        want = check(pts, (48, 48), 4, 5, buckets=(None, 1, 4, 48))
        assert want["n_clusters"].tolist() == [2] and want["core"][at] == 0 and want["labels"][at] == label
        assert want["size"][:2].tolist() == [8, 7] and want["n_core"][:2].tolist() == [7, 7]
    # the lower NUMBER wins, not the nearer clump or the lower row: here `right` holds the smallest core row
    assert want["labels"][0] == 0 and want["labels"][8] == 1
    # a point that reaches only a border point is noise
    tail = np.concatenate([left, [(20, 22)], [(20, 26)]])
    want = check(tail, (48, 48), 4, 5, buckets=(None, 2))
    assert want["labels"][7] == 0 and want["core"][7] == 0 and want["labels"][8] == -1 and want["n_clusters"].tolist() == [1]


def test_contention_in_one_bucket(dev):
    n = 2000
    assert n > 3 * S.CHUNK and n > 7 * S.THREADS
    pts = np.concatenate([np.full((n, 2), 9), [(9, 10)]])
    for b in (None, 16, 4):
        t = S.cluster(pts, (16, 16), 0, 5, _bucket=b)
        assert t.n_clusters.tolist() == [1] and t.labels.tolist() == [0] * n + [-1] and t.core.tolist() == [1] * n + [0]
        assert t.size[:2].tolist() == [n, 0] and t.n_core[0].item() == n and t.sums[0].tolist() == [9 * n, 9 * n]
        assert t.bbox[:2].tolist() == [[9, 9, 10, 10], [0, 0, 0, 0]] and t.n_noise.tolist() == [1]
    mixed = pts[np.random.RandomState(2).permutation(n + 1)]
    check(mixed, (16, 16), 0, 5, buckets=(None, 16))
    assert check(mixed, (16, 16), 1, n + 1, buckets=(16,))["core"].all()                      # 2001 points within a pixel of each other
    assert not check(mixed, (16, 16), 1, n + 2, buckets=(16,))["core"].any()


def test_live_rules(dev):
    rng = np.random.RandomState(29)
    H, W = 40, 56
    per = [np.stack([rng.randint(-3, H + 3, n), rng.randint(-3, W + 3, n)], axis=1) for n in (160, 0, 120)]
    per[0][:4] = [(-1, 5), (H, 5), (5, W), (5, -1)]
    pts, off = C.ragged(per)
    for lim in (None, 90, [150, 3, -40], np.asarray([-170, 0, 1]), [0, 0, -1]):
        want = check(pts, (H, W), 4.5, 4, off, lim, buckets=(None, 6))
        live = C.live_mask(pts, off, lim, (H, W))
        assert (want["labels"][~live] == -2).all() and (want["labels"][live] >= -1).all() and not want["core"][~live].any()
        assert not live[:4].any()
    assert (check(pts, (H, W), 4.5, 4, off)["labels"] >= 0).sum() > 30
    # a point that would be core only thanks to a dead row is not core: dead by the limit, and dead by lying outside
    trio = np.asarray([(5, 5), (5, 6), (5, 7), (0, 0)])
    assert check(trio, (8, 8), 1, 3)["core"].tolist() == [0, 1, 0, 0]
    assert check(trio, (8, 8), 1, 3, limits=2)["labels"].tolist() == [-1, -1, -2, -2]
    assert check(np.asarray([(5, 6), (5, 7), (5, 8), (0, 0)]), (8, 8), 1, 3)["labels"].tolist() == [-1, -1, -2, -1]
    # device operands of other integer types, and spare rows after the last image
    t = S.cluster(torch.from_numpy(pts).to(dev).int(), (H, W), 4.5, 4, offsets=torch.from_numpy(off[:3]).to(dev),
                  limits=torch.tensor([150, 3], device=dev))
    want = C.cluster(pts[:off[2]], (H, W), 4.5, 4, off[:3], [150, 3])
    for k in COLUMNS:
        same(getattr(t, k)[:len(want[k])], want[k], ("spare", k))
    assert (t.labels[off[2]:] == -2).all() and not t.core[off[2]:].any() and not t.size[off[2]:].any() and not t.bbox[off[2]:].any()


def test_ragged_batches_and_tables(dev):
    rng = np.random.RandomState(3)
    for ms in (1, 3, 5):
        per = [rng.randint(0, 6, size=(n, 2)) for n in (0, 1, max(ms - 1, 0), ms, 0, ms + 3)]
        pts, off = C.ragged(per)
        want = check(pts, (20, 20), 10, ms, off, buckets=(None, 2))                           # everybody within eps of everybody
        assert want["n_clusters"].tolist() == [0, int(ms == 1), 0, 1, 0, 1]                   # a cluster needs min_samples points
    per = [np.stack([rng.randint(0, 37, n), rng.randint(0, 33, n)], axis=1) for n in rng.randint(0, 40, size=300)]
    pts, off = C.ragged(per)
    lim = rng.randint(-3, 40, size=300)
    want = check(pts, (37, 33), 4, 3, off, lim, buckets=(None, 7))
    assert want["n_clusters"].max() >= 3 and (want["n_clusters"] == 0).any()
    for n in np.nonzero(want["n_clusters"])[0][:40]:                                          # the numbering restarts at 0 in every image
        lab, core = want["labels"][off[n]:off[n + 1]], want["core"][off[n]:off[n + 1]]
        assert lab[core == 1][0] == 0 and lab.max() + 1 == want["n_clusters"][n]
    t = S.cluster(pts, (37, 33), 4, 3, offsets=off, limits=lim)
    used = np.zeros(len(pts), bool)
    for n in range(300):
        used[off[n]:off[n] + want["n_clusters"][n]] = True
    assert used.any() and not want["size"][~used].any() and not want["bbox"][~used].any() and (want["size"][used] >= 3).all()
    cen = t.centroid.cpu().numpy()
    assert cen.dtype == np.float64 and np.array_equal(np.isnan(cen[:, 0]), ~used)
    assert np.array_equal(cen[used], want["sums"][used] / want["size"][used, None].astype(np.float64))
    noise = np.asarray([(want["labels"][off[n]:off[n + 1]] == -1).sum() for n in range(300)])
    assert t.n_noise.dtype == torch.int64 and t.n_noise.is_cuda and np.array_equal(t.n_noise.cpu().numpy(), noise)
    images = t.per_image()
    assert len(images) == 300
    for n in (0, 7, 150, 299):
        d = images[n]
        assert len(d["labels"]) == off[n + 1] - off[n] and len(d["size"]) == len(d["bbox"]) == len(d["centroid"]) == want["n_clusters"][n]
        assert np.array_equal(d["size"], want["size"][off[n]:off[n] + len(d["size"])])
    check(pts, (37, 33), 6.5, 5, off, 25)


def test_two_runs_identical_and_graph_replay(dev):
    H, W, sizes = 64, 61, (300, 0, 900, 33)

    def batch(seed):
        r = np.random.RandomState(seed)
        return C.ragged([np.stack([r.randint(-1, H + 1, n), r.randint(-1, W + 1, n)], axis=1) for n in sizes])

    def up(x):
        return torch.from_numpy(x).to(dev)

    lim = torch.tensor([250, 5, -50, 33], dtype=torch.int32, device=dev)

    def run(a):
        t = S.cluster(a[0], (H, W), 2.5, 4, offsets=a[1], limits=lim, _bucket=6)
        return [getattr(t, k) for k in COLUMNS]

    data = batch(1)
    first, second = run([up(a) for a in data]), run([up(a) for a in data])
    assert all(torch.equal(x, y) for x, y in zip(first, second))
    want = C.cluster(data[0], (H, W), 2.5, 4, data[1], [250, 5, -50, 33])
    assert want["n_clusters"].max() > 5
    for g, k in zip(first, COLUMNS):
        same(g, want[k], ("eager", k))
    static = [torch.zeros_like(up(a)) for a in data]
    static[1].copy_(up(data[1]))
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        run(static)                                                        # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run(static)
    for seed in (1, 2):                                                    # same sizes, other points: overwritten in place
        new = batch(seed)
        static[0].copy_(up(new[0]))
        graph.replay()
        eager = run([up(a) for a in new])
        assert all(torch.equal(x, y) for x, y in zip(captured, eager))
    assert not torch.equal(captured[0], first[0])
    want = C.cluster(new[0], (H, W), 2.5, 4, new[1], [250, 5, -50, 33])
    for g, k in zip(captured, COLUMNS):
        same(g, want[k], ("replayed", k))


def test_detect_result_cluster(dev):
    from test_edt_gpu import mixed_batch
    maps = mixed_batch(299, 299)
    hw = maps.shape[1:]
    for cc in (None, [3, 0, 5, 5, 1], np.asarray([-1, 100, 0, 1, -5])):
        res = D.detect_points(torch.from_numpy(maps).to(dev), cell_counts=cc, eps=11, method="distancetransform")
        assert res.device_points.is_cuda
        t = res.cluster(hw, 40, min_samples=2)
        host = D.DetectResult(res.points, res.weights, res.offsets, res.n_kept, res.cell_counts)          # no device copy kept
        off = np.asarray(res.offsets)
        pts = np.asarray(res.points, np.int64).reshape(-1, 2)
        direct = S.cluster(pts, hw, 40, 2, offsets=off, limits=cc)
        again = host.cluster(hw, 40, min_samples=2)
        want = C.cluster(pts, hw, 40, 2, off, cc)
        for k in COLUMNS:
            assert len(getattr(t, k)) == (len(off) - 1 if k == "n_clusters" else off[-1])
            assert torch.equal(getattr(t, k), getattr(direct, k)) and torch.equal(getattr(t, k), getattr(again, k)), (cc, k)
            same(getattr(t, k), want[k], (cc, k))
        if cc is None:
            assert want["n_clusters"].sum() > 0
        assert np.array_equal(t.n_noise.cpu().numpy(), [(want["labels"][off[i]:off[i + 1]] == -1).sum() for i in range(len(off) - 1)])


def test_slide_clusters(dev):
    from cellsegmentation_amd import inference as I
    rng = np.random.RandomState(37)
    H, W = 301, 517
    centres = np.stack([rng.randint(20, H - 20, 12), rng.randint(20, W - 20, 12)], axis=1)
    pts = np.concatenate([np.clip(centres[rng.randint(0, 12, 300)] + rng.randint(-12, 13, size=(300, 2)), 0, (H - 1, W - 1)),
                          np.stack([rng.randint(0, H, 100), rng.randint(0, W, 100)], axis=1)])
    slide = I.SlideResult(pts, [], 400, torch.zeros((H, W), dtype=torch.uint8, device=dev))
    t = I.slide_clusters(slide, 8.5, min_samples=4)
    assert t.labels.is_cuda and t.size.is_cuda
    want = C.cluster(pts, (H, W), 8.5, 4)
    assert want["n_clusters"][0] >= 5 and (want["labels"] == -1).any()
    direct = S.cluster(pts, (H, W), 8.5, 4)
    for k in COLUMNS:
        same(getattr(t, k), want[k], ("slide", k))
        assert torch.equal(getattr(t, k), getattr(direct, k))
    assert I.slide_clusters(slide, 8.5).min_samples == 5
    empty = I.slide_clusters(I.SlideResult(np.zeros((0, 2), np.int64), [], 0, slide.mask), 5)
    assert empty.labels.shape == (0,) and empty.n_clusters.tolist() == [0] and empty.bbox.shape == (0, 4) and empty.n_noise.tolist() == [0]
    with pytest.raises(TypeError):
        I.slide_clusters(pts, 5)
