"""CPU: the brute-force restatement of the neighbourhood queries (tests/spatial_ref.py) against its pinned vectors
(tests/golden/make_spatial_golden.py) and against scipy's KD-tree, the argument errors of cellsegmentation_amd.spatial, which are
raised before the library is loaded, the bucket rule, and the ABI additions with their refusals (no GPU needed)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import spatial_ref as R
from cellsegmentation_amd import _lib, detect, kernels, spatial

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "spatial_vectors.npz"), allow_pickle=False)
NAMES = [str(n) for n in GOLD["names"]]
HW, K, RADII, BIN = (61, 45), 8, (0, 4.99, 5, 16), 7


def test_golden_holds_the_pinned_cases():
    assert len(NAMES) == 24 and NAMES[0] == "random_00" and NAMES[11] == "random_11"
    assert set(NAMES) >= {"empty", "one_point", "tie_goes_to_the_lower_index", "radius_5_edge_3_4_and_0_5", "duplicates_are_neighbours_at_0",
                          "corners_and_borders", "outside_points_are_not_live", "lattice_8x8", "cross_same_coordinates", "cross_empty_targets"}
    assert GOLD["tie_goes_to_the_lower_index.index"][0].tolist() == [1, 2, 3, 4, -1, -1, -1, -1]
    assert GOLD["tie_goes_to_the_lower_index.d2"][0].tolist() == [25, 25, 25, 25, -1, -1, -1, -1]
    assert GOLD["radius_5_edge_3_4_and_0_5.counts"][0].tolist() == [0, 0, 2, 4]
    assert GOLD["one_point.index"].tolist() == [[-1] * 8] and GOLD["one_point.counts"].tolist() == [[0] * 4]
    assert GOLD["outside_points_are_not_live.index"][1].tolist() == [-2] * 8 and GOLD["outside_points_are_not_live.counts"][2].tolist() == [-1] * 4
    assert GOLD["outside_points_are_not_live.index"][0].tolist() == [4] + [-1] * 7           # the dead rows are no neighbours
    assert GOLD["cross_same_coordinates.x_d2"][:, 0].tolist() == [0, 0] and GOLD["cross_same_coordinates.x_index"][:, 0].tolist() == [1, 0]
    assert GOLD["lattice_8x8.d2"][0].tolist() == [1, 1, 2, 4, 4, 5, 5, 8] and GOLD["lattice_8x8.index"][0].tolist() == [1, 8, 9, 2, 16, 10, 17, 18]
    assert sum(int(GOLD[f"{n}.pairs"][0, 3]) for n in NAMES[:12]) > 500                       # the random cases have neighbours


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_vectors(name):
    pts = GOLD[f"{name}.pts"]
    idx, d2 = R.nearest(pts, HW, K)
    cnt, pairs = R.count_within(pts, HW, RADII)
    assert idx.dtype == d2.dtype == cnt.dtype == np.int32 and pairs.dtype == np.int64
    assert np.array_equal(idx, GOLD[f"{name}.index"]) and np.array_equal(d2, GOLD[f"{name}.d2"])
    assert np.array_equal(cnt, GOLD[f"{name}.counts"]) and np.array_equal(pairs, GOLD[f"{name}.pairs"])
    assert np.array_equal(R.bin_counts(pts, HW, BIN), GOLD[f"{name}.bins"])
    live = R.live_mask(pts, [0, len(pts)], None, HW)
    assert GOLD[f"{name}.bins"].sum() == live.sum() and np.array_equal(pairs[0], np.where(live[:, None], cnt, 0).sum(axis=0))
    assert np.all(idx[~live] == -2) and np.all(d2[~live] == -1) and np.all(cnt[~live] == -1)
    assert np.all(np.diff(cnt[live], axis=1) >= 0)                                            # the radii rise
    if f"{name}.other" in GOLD.files:
        other = GOLD[f"{name}.other"]
        xi, xd = R.nearest(pts, HW, K, other=other)
        xc, xp = R.count_within(pts, HW, RADII, other=other)
        assert np.array_equal(xi, GOLD[f"{name}.x_index"]) and np.array_equal(xd, GOLD[f"{name}.x_d2"])
        assert np.array_equal(xc, GOLD[f"{name}.x_counts"]) and np.array_equal(xp, GOLD[f"{name}.x_pairs"])
        # (x, y) targets are the same targets with their columns swapped
        si, sd = R.nearest(pts, HW, K, other=other[:, ::-1], other_xy=True)
        assert np.array_equal(si, xi) and np.array_equal(sd, xd)


def test_restatement_limits_and_batches():
    pts, off = R.ragged([[(1, 1), (1, 2), (1, 4)], [], [(3, 3)], [(0, 0), (0, 3)]])
    idx, d2 = R.nearest(pts, (8, 8), 2, off, limits=[2, 5, -1, -1])
    assert idx.tolist() == [[1, -1], [0, -1], [-2, -2], [-2, -2], [-1, -1], [-2, -2]]
    assert d2.tolist() == [[1, -1], [1, -1], [-1, -1], [-1, -1], [-1, -1], [-1, -1]]
    cnt, pairs = R.count_within(pts, (8, 8), [1, 3], off)
    assert cnt.tolist() == [[1, 2], [1, 2], [0, 2], [0, 0], [0, 1], [0, 1]] and pairs.tolist() == [[2, 6], [0, 0], [0, 0], [0, 2]]
    idx, _ = R.nearest(pts, (8, 8), 1, off, other=[(1, 3), (9, 9), (3, 3), (0, 0)], other_off=[0, 2, 2, 3, 4])
    assert idx[:, 0].tolist() == [0, 0, 0, 0, 0, 0]
    idx, _ = R.nearest(pts, (8, 8), 1, off, other=[(1, 3), (9, 9), (3, 3), (0, 0)], other_off=[0, 2, 2, 3, 4], other_limits=[0, 1, 1, 1])
    assert idx[:, 0].tolist() == [-1, -1, -1, 0, 0, 0]


def test_restatement_against_the_kd_tree():
    """distances and counts only: the tree breaks ties its own way.  Integers below 2^31 are exact in float64."""
    cKDTree = pytest.importorskip("scipy.spatial").cKDTree
    rng = np.random.RandomState(5)
    for n, side in ((1, 10), (2, 10), (40, 12), (300, 200), (500, 64)):
        pts = np.stack([rng.randint(0, side, n), rng.randint(0, side, n)], axis=1)
        other = np.stack([rng.randint(0, side, 50), rng.randint(0, side, 50)], axis=1)
        _, d2 = R.nearest(pts, (side, side), 8)
        tree = cKDTree(pts.astype(np.float64))
        dist, _ = tree.query(pts.astype(np.float64), k=min(9, n))
        dist = np.asarray(dist).reshape(n, -1)[:, 1:]                                         # the first hit is the point itself
        want = np.full((n, 8), -1, np.int64)
        want[:, :dist.shape[1]] = np.rint(dist * dist).astype(np.int64)
        assert np.array_equal(d2, want)
        _, xd2 = R.nearest(pts, (side, side), 4, other=other)
        xdist, _ = cKDTree(other.astype(np.float64)).query(pts.astype(np.float64), k=4)
        assert np.array_equal(xd2, np.rint(xdist * xdist).astype(np.int64))
        for radii in ((0, 1, 5, 7.5), (side * 2,)):
            cnt, _ = R.count_within(pts, (side, side), radii)
            xcnt, _ = R.count_within(pts, (side, side), radii, other=other)
            for j, r in enumerate(radii):
                # the ball of the integer floor(r^2): sqrt of it, nudged up within the gap to the next integer's root
                rr = np.sqrt(R.radius_squared(r) + 0.5)
                assert cnt[:, j].tolist() == [len(b) - 1 for b in tree.query_ball_point(pts.astype(np.float64), rr)]
                assert xcnt[:, j].tolist() == [len(b) for b in cKDTree(other.astype(np.float64)).query_ball_point(pts.astype(np.float64), rr)]


def test_bucket_rule():
    assert spatial.choose_bucket(299, 299, 128, 128 * 80) == 95 and spatial.choose_bucket(4096, 4096, 1, 100000) == 37
    assert spatial.choose_bucket(4096, 4096, 1, 100000, reach=64) == 37 and spatial.choose_bucket(4096, 4096, 1, 100000, reach=200) == 100
    assert spatial.choose_bucket(64, 48, 1, 0) == 64 and spatial.choose_bucket(64, 48, 1, 10 ** 9) == 1
    b = spatial.choose_bucket(299, 299, 65535, 1 << 30)                                       # the cap on the buckets of one call
    fits = min(s for s in range(1, 300) if 65535 * spatial.n_buckets(299, 299, s) <= spatial.MAX_BUCKETS)
    assert 65535 * spatial.n_buckets(299, 299, b) <= spatial.MAX_BUCKETS and fits <= b <= fits + fits // 8 + 1    # raised by eighths
    for H, W, N, P, reach in ((1, 1, 1, 5, 0), (7, 5000, 3, 10, 46340), (32767, 32767, 1, 10 ** 6, 3)):
        b = spatial.choose_bucket(H, W, N, P, reach)
        assert 1 <= b <= max(H, W) and N * spatial.n_buckets(H, W, b) <= spatial.MAX_BUCKETS


def test_argument_errors_come_before_the_library_is_loaded(monkeypatch):
    def no_load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_load)
    monkeypatch.setattr(spatial, "_device", no_load)
    pts = np.asarray([(0, 0), (5, 5), (3, 4)])
    calls = (lambda p, **kw: spatial.nearest(p, kw.pop("hw", (16, 16)), **kw),
             lambda p, **kw: spatial.count_within(p, kw.pop("hw", (16, 16)), kw.pop("radii", 3), **kw),
             lambda p, **kw: spatial.bin_counts(p, kw.pop("hw", (16, 16)), kw.pop("bin", 4), **kw))
    for call in calls:
        for bad in (pts.astype(np.float64), pts.astype(np.float32), torch.zeros(2, 2), torch.zeros(2, 2, dtype=torch.bool)):
            with pytest.raises(TypeError):
                call(bad)
        for bad in (np.zeros((2, 3), np.int64), np.zeros(4, np.int64), np.zeros((1, 2, 2), np.int64), torch.zeros(2, 3, dtype=torch.int64)):
            with pytest.raises(ValueError):
                call(bad)
        for bad in ([0, 1], [0, 4], [1, 3], [0, 2, 1, 3], [0], np.asarray([0.0, 3.0])):
            with pytest.raises(ValueError):
                call(pts, offsets=bad)
        for bad in ((46341, 1), (32768, 32768), (0, 5), (5, -1)):
            with pytest.raises(ValueError):
                call(pts, hw=bad)
        for bad in ((16.0, 16), (16,), 16, None, (True, 4)):
            with pytest.raises(TypeError):
                call(pts, hw=bad)
        with pytest.raises(TypeError):
            call(pts, limits=1.5)
        with pytest.raises(ValueError):
            call(pts, limits=[1, 2])
    assert spatial.check_image_hw((46340, 1)) == (46340, 1) and spatial.check_image_hw((np.int64(32767), 32767)) == (32767, 32767)
    for call in calls[:2]:
        for bad in (0, -3, 1.5, True, "4"):
            with pytest.raises(ValueError):
                call(pts, _bucket=bad)
        with pytest.raises(ValueError, match="exceed"):
            call(pts, hw=(4096, 4096), _bucket=1)
        for bad in (pts.astype(np.float32), np.zeros((2, 3), np.int64)):
            with pytest.raises((TypeError, ValueError)):
                call(pts, other=bad)
        with pytest.raises(ValueError):
            call(pts, offsets=[0, 1, 3], other=pts, other_offsets=[0, 3])               # two images of points, one of targets
        with pytest.raises(ValueError):
            call(pts, other=pts, other_offsets=[0, 2])
        with pytest.raises(ValueError):
            call(pts, other_offsets=[0, 3])                                              # describes a set that was not given
        with pytest.raises(ValueError):
            call(pts, other_xy=True)
    for bad in (0, 9, -1, 1.0, True, "1", None):
        with pytest.raises(ValueError):
            spatial.nearest(pts, (16, 16), k=bad)
    for bad in ([], list(range(9)), [-1], [3, float("nan")], [float("inf")], -0.5, [46341]):
        with pytest.raises(ValueError):
            spatial.count_within(pts, (16, 16), bad)
    for bad in ("3", [None], None, [True]):
        with pytest.raises(TypeError):
            spatial.count_within(pts, (16, 16), bad)
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError):
            spatial.bin_counts(pts, (16, 16), bad)
    with pytest.raises(ValueError, match="exceed"):
        spatial.bin_counts(pts, (4096, 4096), 1)
    # the raw bindings refuse host tensors, wrong dtypes and wrong shapes before they load anything either
    t, off = torch.zeros(2, 2, dtype=torch.int64), torch.tensor([0, 2])
    with pytest.raises(ValueError):
        kernels.spatial_nearest(t, off, 16, 16, 4)
    with pytest.raises(ValueError):
        kernels.spatial_count_within(t, off, 16, 16, 4, [9])
    with pytest.raises(ValueError):
        kernels.spatial_bin_counts(t, off, 16, 16, 4)
    # DetectResult: the second point set must say which map it belongs to
    res = detect.DetectResult(np.zeros((3, 2), np.int64), np.zeros(3, np.int64), np.asarray([0, 1, 3]), np.asarray([1, 2]))
    for bad in (pts, [pts], [pts, pts, pts], np.zeros((3, 4, 2), np.int64)):
        with pytest.raises(ValueError):
            res.nearest((16, 16), other=bad)
        with pytest.raises(ValueError):
            res.count_within((16, 16), 3, other=bad)
    with pytest.raises(ValueError):
        res.nearest((16, 16), k=9)
    with pytest.raises(ValueError):
        res.count_within((16, 16), -2)
    with pytest.raises(ValueError):
        res.nearest((40000, 40000))


def test_new_symbols_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "cellseg_hip.h")).read()
    names = ("cs_spatial_threads", "cs_spatial_chunk", "cs_spatial_max_buckets", "cs_spatial_workspace", "cs_spatial_nearest",
             "cs_spatial_count_within", "cs_spatial_bin_counts")
    for name in names:
        assert re.search(rf"^(size_t|int|long long) {name}\(", header, re.M), name
        assert name in _lib._SIGNATURES and name in _lib.exported_symbols()
    assert len(_lib._SIGNATURES["cs_spatial_nearest"][1]) == 19 and len(_lib._SIGNATURES["cs_spatial_count_within"][1]) == 20
    assert len(_lib._SIGNATURES["cs_spatial_bin_counts"][1]) == 10 and _lib._SIGNATURES["cs_spatial_workspace"][0] is _lib.c_size_t
    lib = _lib.load()
    assert lib.cs_abi_version() == 10
    # the constants the Python layer and the tests size things by
    assert (lib.cs_spatial_threads(), lib.cs_spatial_chunk(), lib.cs_spatial_max_buckets()) == (spatial.THREADS, spatial.CHUNK, spatial.MAX_BUCKETS)
    src = open(os.path.join(ROOT, "cellsegmentation_amd", "csrc", "spatial.hip")).read()
    assert "asm" not in re.sub(r"//.*", "", src), "plain C++ only"
    assert "spatial.hip" in open(os.path.join(ROOT, "cellsegmentation_amd", "csrc", "Makefile")).read()


def test_workspace_size():
    ws = _lib.load().cs_spatial_workspace
    for bad in ((0, 8, 8, 4, 1, -1), (65536, 8, 8, 4, 1, -1), (1, 0, 8, 4, 1, -1), (1, 8, 0, 4, 1, -1), (1, 8, 8, 0, 1, -1), (1, 8, 8, 4, -1, -1),
                (1, 46341, 1, 4, 1, -1), (1, 32768, 32768, 64, 1, -1), (1, 4096, 4096, 1, 1, -1), (1, 8, 8, 4, 1 << 31, -1), (1, 8, 8, 4, 1, 1 << 31)):
        assert ws(*bad) == 0, bad
    one = ws(1, 8, 8, 4, 10, -1)
    assert one >= 4 * 4 + 5 * 4 + 16 * 10 and one % 16 == 0
    assert ws(1, 8, 8, 4, 10, 0) > one and ws(1, 8, 8, 4, 10, 7) == ws(1, 8, 8, 4, 10, 0) + 6 * 16
    assert ws(1, 8, 8, 100, 0, -1) == ws(1, 8, 8, 8, 0, -1) == 16 + 16 + 16                  # one bucket, room for one record
    assert ws(128, 299, 299, 1, 0, -1) == 0 and ws(46, 299, 299, 1, 0, -1) > 0               # 2^22 buckets in one call


def test_entry_points_refuse_bad_calls_without_a_gpu():
    lib = _lib.load()
    buf = (ctypes.c_int64 * 64)()                                                             # host memory: nothing is launched
    base = ctypes.addressof(buf)
    base += -base % 16
    P = ctypes.c_void_p
    ws_bytes = lib.cs_spatial_workspace(1, 8, 8, 4, 2, -1)

    def nearest(pts=base, off=base, other=None, other_off=None, other_limit=None, P_o=0, N=1, H=8, W=8, b=4, k=1, flags=0, index=base, d2=base,
                ws=base, ws_b=ws_bytes, rows=2):
        return lib.cs_spatial_nearest(P(pts), P(off), None, rows, P(other), P(other_off), P(other_limit), P_o, N, H, W, b, k, flags, P(index), P(d2),
                                      P(ws), ws_b, None)

    def within(pts=base, off=base, other=None, other_off=None, N=1, H=8, W=8, b=4, radii=(4,), n_r=None, flags=0, counts=base, pairs=base,
               ws=base, ws_b=ws_bytes, rows=2):
        arr = (ctypes.c_int32 * max(len(radii), 1))(*radii)
        return lib.cs_spatial_count_within(P(pts), P(off), None, rows, P(other), P(other_off), None, 0, N, H, W, b, arr if radii else None,
                                           len(radii) if n_r is None else n_r, flags, P(counts), P(pairs), P(ws), ws_b, None)

    def bins(pts=base, off=base, N=1, H=8, W=8, b=4, out=base, rows=2):
        return lib.cs_spatial_bin_counts(P(pts), P(off), None, rows, N, H, W, b, P(out), None)

    for what, fn, cases in (
        ("spatial_nearest", nearest, (dict(N=0), dict(N=65536), dict(H=0), dict(W=-1), dict(b=0), dict(H=46341), dict(H=4096, W=4096, b=1),
                                      dict(rows=-1), dict(rows=1 << 31), dict(pts=None), dict(off=None), dict(ws=None), dict(index=None), dict(d2=None),
                                      dict(k=0), dict(k=9), dict(flags=2), dict(ws_b=ws_bytes - 1), dict(ws_b=0), dict(ws=base + 8), dict(pts=base + 4),
                                      dict(off=base + 4), dict(index=base + 2), dict(d2=base + 1), dict(other=base), dict(other_limit=base), dict(P_o=3),
                                      dict(other_off=base, P_o=2), dict(other_off=base, other=base + 4, P_o=1, ws_b=4096),
                                      dict(other_off=base + 4, other=base, P_o=1, ws_b=4096), dict(other_off=base, other=base, P_o=1))),
        ("spatial_count_within", within, (dict(N=0), dict(b=0), dict(H=46341), dict(pts=None), dict(off=None), dict(ws=None), dict(counts=None),
                                          dict(pairs=None), dict(radii=()), dict(radii=(1,) * 9), dict(radii=(4, -1)), dict(n_r=0), dict(flags=4),
                                          dict(ws_b=ws_bytes - 16), dict(ws=base + 4), dict(counts=base + 2), dict(pairs=base + 4), dict(other=base))),
        ("spatial_bin_counts", bins, (dict(N=0), dict(N=65536), dict(H=0), dict(b=0), dict(H=46341), dict(H=4096, W=4096, b=1), dict(rows=-1),
                                      dict(pts=None), dict(off=None), dict(out=None), dict(pts=base + 4), dict(off=base + 2), dict(out=base + 1))),
    ):
        for kw in cases:
            assert fn(**kw) == -1, (what, kw)
            assert what.encode() in lib.cs_last_error(), (what, kw, lib.cs_last_error())
    assert b"workspace too small" in (nearest(ws_b=ws_bytes - 1), lib.cs_last_error())[1]
    assert b"misaligned" in (nearest(ws=base + 8), lib.cs_last_error())[1]
    assert b"NULL" in (within(pairs=None), lib.cs_last_error())[1]
    assert b"1 <= k <= 8" in (nearest(k=9), lib.cs_last_error())[1]
