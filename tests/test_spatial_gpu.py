"""Neighbourhood queries on the GPU (csrc/spatial.hip through cellsegmentation_amd.spatial), bit-exact against the brute-force numpy
restatement tests/spatial_ref.py: the pinned vectors, lattices full of ties, duplicates, images with fewer than k points, every
bucket side from one pixel to one bucket, buckets that overflow the LDS chunk and the workgroup, long ring walks and the strict
settling rule, radii on the d2 == r^2 edge, live rules, a second point set, bin counts, repeatability, graph replay,
DetectResult.nearest / .count_within and inference.slide_neighbors."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import spatial_ref as R  # noqa: E402
from cellsegmentation_amd import detect as D  # noqa: E402
from cellsegmentation_amd import kernels as K  # noqa: E402
from cellsegmentation_amd import spatial as S  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "spatial_vectors.npz"), allow_pickle=False)
NAMES = [str(n) for n in GOLD["names"]]
HW, RADII = (61, 45), (0, 4.99, 5, 16)


def same(got, want, what):
    got = got.cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert not len(bad), (what, bad[:5].tolist(), [got[tuple(b)] for b in bad[:5]], [want[tuple(b)] for b in bad[:5]])


def check(pts, hw, k=None, radii=None, off=None, limits=None, buckets=(None,), want=None, **other):
    """nearest and / or count_within at every bucket side of ``buckets`` against the restatement (computed once); ``other`` holds the
    second point set under the restatement's names"""
    kw = {"offsets": off, "limits": limits}
    for name, theirs in (("other", "other"), ("other_off", "other_offsets"), ("other_limits", "other_limits"), ("other_xy", "other_xy")):
        if name in other:
            kw[theirs] = other[name]
    want = dict(want or {})
    if k is not None and "near" not in want:
        want["near"] = R.nearest(pts, hw, k, off, limits, **other)
    if radii is not None and "within" not in want:
        want["within"] = R.count_within(pts, hw, radii, off, limits, **other)
    for b in buckets:
        if k is not None:
            t = S.nearest(pts, hw, k, _bucket=b, **kw)
            same(t.index, want["near"][0], ("index", b))
            same(t.d2, want["near"][1], ("d2", b))
        if radii is not None:
            w = S.count_within(pts, hw, radii, _bucket=b, **kw)
            same(w.counts, want["within"][0], ("counts", b))
            same(w.pair_counts, want["within"][1], ("pair_counts", b))
            live = want["within"][0][:, :1] >= 0
            assert np.array_equal(np.where(live, want["within"][0], 0).astype(np.int64).sum(axis=0), want["within"][1].sum(axis=0))
    return want


def test_golden_cases_as_one_batch_and_one_by_one(dev):
    per = [GOLD[f"{n}.pts"] for n in NAMES]
    pts, off = R.ragged(per)
    want_i = np.concatenate([GOLD[f"{n}.index"] for n in NAMES])
    want_d = np.concatenate([GOLD[f"{n}.d2"] for n in NAMES])
    want_c = np.concatenate([GOLD[f"{n}.counts"] for n in NAMES])
    want_p = np.concatenate([GOLD[f"{n}.pairs"] for n in NAMES])
    check(pts, HW, 8, RADII, off, buckets=(None, 5), want={"near": (want_i, want_d), "within": (want_c, want_p)})
    same(S.bin_counts(pts, HW, 7, offsets=off), np.concatenate([GOLD[f"{n}.bins"] for n in NAMES]), "bins")
    for k in (1, 3):
        check(pts, HW, k, off=off, want={"near": (want_i[:, :k].copy(), want_d[:, :k].copy())})
    for n, p in zip(NAMES, per):
        check(p, HW, 8, RADII, want={"near": (GOLD[f"{n}.index"], GOLD[f"{n}.d2"]), "within": (GOLD[f"{n}.counts"], GOLD[f"{n}.pairs"])})
    # the cases with a second set, as one batch (the others get an empty one) and one by one
    others = [GOLD[f"{n}.other"] if f"{n}.other" in GOLD.files else np.zeros((0, 2), np.int64) for n in NAMES]
    o, o_off = R.ragged(others)
    check(pts, HW, 8, RADII, off, buckets=(None, 3), other=o, other_off=o_off)
    for n, p, q in zip(NAMES, per, others):
        if f"{n}.other" in GOLD.files:
            check(p, HW, 8, RADII, other=q, want={"near": (GOLD[f"{n}.x_index"], GOLD[f"{n}.x_d2"]),
                                                 "within": (GOLD[f"{n}.x_counts"], GOLD[f"{n}.x_pairs"])})


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 8])
def test_lattice_ties_and_duplicates(dev, k):
    lattice = np.stack(np.meshgrid(np.arange(8), np.arange(8), indexing="ij"), axis=-1).reshape(-1, 2) * 3 + 2
    pts = np.concatenate([lattice, lattice[[0, 9, 9, 27, 63]]])                               # distance 0 between distinct rows
    want = check(pts, (29, 31), k, buckets=(None, 1, 3, 4, 31))
    idx, d2 = want["near"]
    assert d2[64, 0] == 0 and idx[64, 0] == 0 and idx[0, 0] == 64 and not (idx == np.arange(len(pts))[:, None]).any()
    assert (np.diff(d2.astype(np.int64), axis=1) >= 0).all() and (d2[:64, 0] <= 9).all()
    if k >= 2:
        assert idx[9, :2].tolist() == [65, 66] and d2[9, :2].tolist() == [0, 0]               # the two copies, the lower index first


def test_fewer_than_k_candidates_and_many_ragged_images(dev):
    rng = np.random.RandomState(3)
    for k in (1, 4, 8):
        per = [rng.randint(0, 20, size=(n, 2)) for n in (0, 1, 2, k, k + 1, 0, 3)]
        pts, off = R.ragged(per)
        want = check(pts, (20, 20), k, [2, 30], off, buckets=(None, 2))
        assert (want["near"][0][off[1]] == -1).all() and (want["near"][0][off[3]:off[4], -1] == -1).all()
        assert (want["near"][0][off[4]:off[5], -1] >= 0).all()
    per = [rng.randint(0, 37, size=(rng.randint(0, 12), 2)) for _ in range(300)]
    pts, off = R.ragged(per)
    lim = rng.randint(-3, 12, size=300)
    check(pts, (37, 33), 4, [0, 3, 9.5], off, lim, buckets=(None, 7))
    check(pts, (37, 33), 2, [6], off, 5)


def test_grid_independence(dev):
    H, W = 67, 45
    rng = np.random.RandomState(11)
    edge = [(0, 0), (H - 1, W - 1), (H - 1, 0), (0, W - 1), (16, 16), (32, 32), (64, 16), (48, 3), (3, 3), (6, 9), (63, 44), (64, 44), (15, 15)]
    pts = np.concatenate([np.asarray(edge), np.stack([rng.randint(0, H, 150), rng.randint(0, W, 150)], axis=1)])
    other = np.stack([rng.randint(0, H, 40), rng.randint(0, W, 40)], axis=1)
    sides = (None, 1, 3, 16, 64, max(H, W), 1000)
    check(pts, (H, W), 8, [0, 2, 5, 16, 200], buckets=sides)
    check(pts, (H, W), 3, [3, 17.2], buckets=sides, other=other)
    two, off = R.ragged([pts[:90], pts[90:]])
    check(two, (H, W), 5, [4, 33], off, [80, -7], buckets=sides)
    for b in (1, 3, 16, 64, 67):
        same(S.bin_counts(pts, (H, W), b), R.bin_counts(pts, (H, W), b), ("bins", b))


def test_buckets_that_overflow_the_chunk_and_the_workgroup(dev):
    lib_threads, lib_chunk = S.THREADS, S.CHUNK
    n_patch = max(5000, 5 * max(lib_threads, lib_chunk))                                      # about ten chunks of 512 records
    assert n_patch > 4 * lib_chunk and n_patch > 4 * lib_threads
    rng = np.random.RandomState(17)
    patch = np.stack([rng.randint(40, 48, n_patch), rng.randint(72, 80, n_patch)], axis=1)   # 64 pixels: duplicates by construction
    spread = np.stack([rng.randint(0, 128, 300), rng.randint(0, 160, 300)], axis=1)
    pts = np.concatenate([patch, spread])[rng.permutation(n_patch + 300)]
    assert 40 // 8 == 47 // 8 and 72 // 8 == 79 // 8                                          # one bucket of side 8 holds the patch
    check(pts, (128, 160), 8, [0, 1, 3, 200], buckets=(8, None))
    check(spread, (128, 160), 2, [2.5], buckets=(8,), other=pts)
    check(pts, (128, 160), 1, None, buckets=(160,))                                           # everything in one bucket


def test_long_ring_walk_and_the_strict_settling_rule(dev):
    corner = np.asarray([(0, 0)] + [(63 - i, 63 - j) for i in range(3) for j in range(3)])
    want = check(corner, (64, 64), 4, [80, 90], buckets=(1, 2, 64))
    assert want["near"][0][0].tolist() == [9, 6, 8, 5] and want["near"][1][0, 0] == 2 * 61 * 61
    check(corner[:1], (64, 64), 8, [100], buckets=(1,), other=corner[1:])
    # two targets at distance 5 of the query at (20, 20).  Rings are squares: with 1-pixel buckets (23, 24), index 1, is met in ring 4,
    # where the region's edge is exactly 5 away, and (20, 25), index 0, only in ring 5 -- the later ring holds the winner of the tie
    pts = np.asarray([(20, 25), (23, 24), (20, 20)])
    for b in (1, 2, 3, 4, 5):
        want = check(pts, (64, 64), 1, buckets=(b,))
        assert want["near"][0][2, 0] == 0 and want["near"][1][2, 0] == 25
    tgt = np.asarray([(10, 15), (13, 14), (10, 5), (6, 7)])                                   # all at d2 = 25 of (10, 10)
    want = check(np.asarray([(10, 10)]), (32, 32), 3, buckets=(1, 2, 3, 4, 8), other=tgt)
    assert want["near"][0][0].tolist() == [0, 1, 2]


def test_radii(dev):
    pts = np.asarray([(20, 20), (23, 24), (20, 25), (25, 25), (20, 26), (20, 20), (17, 16), (15, 20)])
    want = check(pts, (40, 50), None, [5, 0, 4.99, 100, 5.01, 1, 6, 7.08], buckets=(None, 1, 2, 5, 50))
    assert want["within"][0][0].tolist() == [5, 1, 1, 7, 5, 1, 6, 7]                          # d2 == 25 counts at r = 5, not at 4.99
    assert want["within"][1][0].tolist()[1] == 2                                              # the coincident pair, both ways round
    rng = np.random.RandomState(23)
    cloud = np.stack([rng.randint(0, 90, 400), rng.randint(0, 70, 400)], axis=1)
    check(cloud, (90, 70), None, [0, 1, 2, 4, 8, 16, 32, 64], buckets=(None, 4, 90))
    check(cloud, (90, 70), None, [46340], buckets=(None, 9))                                  # larger than the image: everybody


def test_live_rules_and_xy(dev):
    rng = np.random.RandomState(29)
    H, W = 40, 56
    per = [np.stack([rng.randint(-3, H + 3, n), rng.randint(-3, W + 3, n)], axis=1) for n in (60, 0, 45)]
    per[0][:4] = [(-1, 5), (H, 5), (5, W), (5, -1)]
    pts, off = R.ragged(per)
    for lim in (None, 30, [50, 3, -40], np.asarray([-60, 0, 1])):
        want = check(pts, (H, W), 4, [3, 12], off, lim, buckets=(None, 6))
        live = R.live_mask(pts, off, lim, (H, W))
        idx = want["near"][0]
        assert (idx[~live] == -2).all() and (idx[live] >= -1).all() and not live[:4].any()
        for n in range(3):                                                                    # a dead point is nobody's neighbour
            rows = np.arange(off[n], off[n + 1])
            dead = set((rows[~live[rows]] - off[n]).tolist())
            assert not dead & set(idx[rows][idx[rows] >= 0].tolist())
    others = [np.stack([rng.randint(-2, H + 2, n), rng.randint(-2, W + 2, n)], axis=1) for n in (20, 9, 30)]
    o, o_off = R.ragged(others)
    want = check(pts, (H, W), 3, [5, 20], off, [50, 3, -40], buckets=(None, 4), other=o, other_off=o_off, other_limits=[10, -1, 25])
    swapped = np.ascontiguousarray(o[:, ::-1])
    check(pts, (H, W), 3, [5, 20], off, [50, 3, -40], buckets=(None, 4), other=swapped, other_off=o_off, other_limits=[10, -1, 25],
          other_xy=True, want=want)
    # device operands of other integer types, and spare rows after the last image
    t = S.nearest(torch.from_numpy(pts).to(dev).int(), (H, W), 2, offsets=torch.from_numpy(off[:3]).to(dev), limits=torch.tensor([50, 3], device=dev))
    idx2, d22 = R.nearest(pts[:off[2]], (H, W), 2, off[:3], [50, 3])
    same(t.index[:off[2]], idx2, "spare index")
    same(t.d2[:off[2]], d22, "spare d2")
    assert (t.index[off[2]:] == -2).all() and (t.d2[off[2]:] == -1).all()
    dist = t.distance().cpu().numpy()
    assert dist.dtype == np.float64 and np.array_equal(np.isnan(dist[:off[2]]), d22 < 0)
    # the one float of the module: a float64 square root of an exact integer, so within one ulp of numpy's correctly rounded one
    root = np.sqrt(d22[d22 >= 0].astype(np.float64))
    assert (np.abs(dist[:off[2]][d22 >= 0] - root) <= np.spacing(root)).all()


def test_cross_mode_has_no_self_exclusion(dev):
    pts = np.asarray([(5, 5), (9, 9), (30, 2)])
    want = check(pts, (32, 32), 2, [0, 6], buckets=(None, 1, 4), other=pts)
    assert want["near"][0][:, 0].tolist() == [0, 1, 2] and want["near"][1][:, 0].tolist() == [0, 0, 0]
    assert want["within"][0][:, 0].tolist() == [1, 1, 1]
    me = check(pts, (32, 32), 2, [0, 6], buckets=(None, 1, 4))
    assert me["near"][0][:, 0].tolist() == [1, 0, 1] and me["within"][0][:, 0].tolist() == [0, 0, 0]


def test_bin_counts(dev):
    rng = np.random.RandomState(31)
    H, W = 50, 38
    per = [np.stack([rng.randint(-2, H + 2, n), rng.randint(-2, W + 2, n)], axis=1) for n in (500, 0, 70)]
    pts, off = R.ragged(per)
    for b in (1, 7, 16, 50, 64):
        for lim in (None, [300, 1, -10]):
            got = S.bin_counts(pts, (H, W), b, offsets=off, limits=lim)
            same(got, R.bin_counts(pts, (H, W), b, off, lim), ("bins", b))
    p = per[0][(per[0][:, 0] >= 0) & (per[0][:, 0] < H) & (per[0][:, 1] >= 0) & (per[0][:, 1] < W)]
    hist = np.histogram2d(p[:, 0], p[:, 1], bins=[np.arange(0, H + 7, 7), np.arange(0, W + 7, 7)])[0]
    same(S.bin_counts(per[0], (H, W), 7)[0], hist.astype(np.int32), "histogram2d")


def test_two_runs_identical_and_graph_replay(dev):
    H, W, sizes = 83, 71, (120, 0, 700, 33)

    def batch(seed):
        r = np.random.RandomState(seed)
        pts, off = R.ragged([np.stack([r.randint(-1, H + 1, n), r.randint(-1, W + 1, n)], axis=1) for n in sizes])
        o, o_off = R.ragged([np.stack([r.randint(0, H, n), r.randint(0, W, n)], axis=1) for n in sizes[::-1]])
        return pts, off, o, o_off

    def up(x):
        return torch.from_numpy(x).to(dev)

    lim = torch.tensor([100, 5, -50, 33], dtype=torch.int32, device=dev)
    r2 = (9, 256)

    def run(a, b=6):
        near = K.spatial_nearest(a[0], a[1], H, W, b, 4, limits=lim)
        cross = K.spatial_count_within(a[0], a[1], H, W, b, r2, limits=lim, other=a[2], other_off=a[3])
        return near + cross

    data = batch(1)
    first, second = run([up(a) for a in data]), run([up(a) for a in data])
    assert all(torch.equal(x, y) for x, y in zip(first, second))
    want = R.nearest(data[0], (H, W), 4, data[1], [100, 5, -50, 33]) + R.count_within(data[0], (H, W), [3, 16], data[1], [100, 5, -50, 33],
                                                                                    other=data[2], other_off=data[3])
    for g, w in zip(first, want):
        same(g, w, "eager")
    static = [torch.zeros_like(up(a)) for a in data]
    static[1].copy_(up(data[1]))
    static[3].copy_(up(data[3]))
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
        for s, a in zip(static, new):
            s.copy_(up(a))
        graph.replay()
        eager = run([up(a) for a in new])
        assert all(torch.equal(x, y) for x, y in zip(captured, eager))
    assert not torch.equal(captured[0], first[0])
    want = R.nearest(new[0], (H, W), 4, new[1], [100, 5, -50, 33])
    same(captured[0], want[0], "replayed index")


def test_detect_result_neighbours(dev):
    from test_edt_gpu import mixed_batch
    maps = mixed_batch(299, 299)
    hw = maps.shape[1:]
    rng = np.random.RandomState(8)
    free = D.detect_points(torch.from_numpy(maps).to(dev), eps=11, method="distancetransform")
    assert sum(len(p[0]) for p in free.per_image()) > 20
    gts = [np.concatenate([p[0][::2] + rng.randint(-9, 10, size=p[0][::2].shape), rng.randint(0, 299, size=(3, 2))]) for p in free.per_image()]
    for cc in (None, [3, 0, 5, 5, 1], 2, np.asarray([-1, 100, 0, 1, -5])):
        res = D.detect_points(torch.from_numpy(maps).to(dev), cell_counts=cc, eps=11, method="distancetransform")
        assert res.device_points.is_cuda
        near, within = res.nearest(hw, k=3), res.count_within(hw, [16, 40])
        x_near, x_within = res.nearest(hw, k=2, other=gts), res.count_within(hw, 16, other=[g[:, ::-1] for g in gts], other_xy=True)
        host = D.DetectResult(res.points, res.weights, res.offsets, res.n_kept, res.cell_counts)      # no device copy kept
        off = res.offsets
        assert len(near.index) == len(within.counts) == len(x_near.d2) == off[-1]
        assert torch.equal(host.nearest(hw, k=3).index, near.index) and torch.equal(host.count_within(hw, [16, 40]).counts, within.counts)
        for i, (kept, _) in enumerate(res.per_image()):
            rows = slice(off[i], off[i] + len(kept))
            idx, d2 = R.nearest(kept, hw, 3)
            same(near.index[rows], idx, ("index", cc, i))
            same(near.d2[rows], d2, ("d2", cc, i))
            cnt, pairs = R.count_within(kept, hw, [16, 40])
            same(within.counts[rows], cnt, ("counts", cc, i))
            same(within.pair_counts[i], pairs[0], ("pairs", cc, i))
            xi, xd = R.nearest(kept, hw, 2, other=gts[i])
            same(x_near.index[rows], xi, ("x index", cc, i))
            same(x_near.d2[rows], xd, ("x d2", cc, i))
            same(x_within.counts[rows], R.count_within(kept, hw, 16, other=gts[i])[0], ("x counts", cc, i))
            assert (near.index[off[i] + len(kept):off[i + 1]] == -2).all() and (within.counts[off[i] + len(kept):off[i + 1]] == -1).all()
    one = D.detect_points(maps[0], eps=11, method="distancetransform")
    assert torch.equal(one.nearest(hw).index, free.nearest(hw).index[:free.offsets[1]])
    assert torch.equal(one.nearest(hw, other=gts[0]).d2, free.nearest(hw, other=gts).d2[:free.offsets[1]])


def test_slide_neighbors(dev):
    from cellsegmentation_amd import inference as I
    rng = np.random.RandomState(37)
    H, W = 301, 517
    pts = np.stack([rng.randint(0, H, 400), rng.randint(0, W, 400)], axis=1)
    other = np.stack([rng.randint(0, W, 90), rng.randint(0, H, 90)], axis=1)                  # (x, y)
    slide = I.SlideResult(pts, [], 400, torch.zeros((H, W), dtype=torch.uint8, device=dev))
    near, within = I.slide_neighbors(slide, k=2, radii=[16, 40.5])
    assert near.index.is_cuda and within.counts.is_cuda
    for g, w in zip((near.index, near.d2, within.counts, within.pair_counts), R.nearest(pts, (H, W), 2) + R.count_within(pts, (H, W), [16, 40.5])):
        same(g, w, "slide")
    near, within = I.slide_neighbors(slide, k=1, radii=16, other=other, other_xy=True)
    for g, w in zip((near.index, near.d2, within.counts), R.nearest(pts, (H, W), 1, other=other, other_xy=True)
                    + R.count_within(pts, (H, W), 16, other=other, other_xy=True)[:1]):
        same(g, w, "slide against a second set")
    assert I.slide_neighbors(slide, k=0) == (None, None) and I.slide_neighbors(slide, radii=[3])[0].index.shape == (400, 1)
    empty = I.SlideResult(np.zeros((0, 2), np.int64), [], 0, slide.mask)
    near, within = I.slide_neighbors(empty, radii=5)
    assert near.index.shape == (0, 1) and within.counts.shape == (0, 1) and within.pair_counts.tolist() == [[0]]
    with pytest.raises(TypeError):
        I.slide_neighbors(pts)
