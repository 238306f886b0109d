"""The ragged point set of csrc/cs_points.h through every kernel that reads it: one small batch -- four images of 24 x 31, one of them
empty, some points just outside the image, four spare rows after the last image's, int32 device offsets -- and the rows that score,
the spatial queries, the clustering, the point raster and the two splits treat as kept (and inside) against a numpy restatement of
``list[:c]``.  Then offsets that do not describe rows of the buffer, in the first or the last image so that the others keep their
rows: the image has no live point and no seed, or -- score, which knows no row count and so cannot see offsets beyond the buffer --
the call is refused."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import spatial_ref as SR  # noqa: E402
from cellsegmentation_amd import regions, render, score, spatial  # noqa: E402

pytestmark = pytest.mark.gpu

N, H, W = 4, 24, 31
COUNTS = (14, 0, 11, 13)
SPARE = 4
LIMITS = (None, 3, [50, 0, -2, 1])


def _batch():
    rng = np.random.RandomState(7)
    P = sum(COUNTS) + SPARE
    pts = np.stack([rng.randint(0, H, size=P), rng.randint(0, W, size=P)], axis=1).astype(np.int64)
    pts[[1, 9, 16, 27]] = [(-1, 5), (H, 0), (3, -1), (7, W)]              # just outside, one on every side
    pts[2] = pts[0]                                                        # two rows at one place
    off = np.zeros(N + 1, np.int64)
    np.cumsum(COUNTS, out=off[1:])
    return pts, off


PTS, OFF = _batch()
P = len(PTS)
INSIDE = (PTS[:, 0] >= 0) & (PTS[:, 0] < H) & (PTS[:, 1] >= 0) & (PTS[:, 1] < W)


def _kept(off, limits):
    """bool [P]: the rows that ``rows_of_image_n[:c]`` keeps, image by image"""
    kept = np.zeros(P, bool)
    for n in range(N):
        rows = list(range(off[n], off[n + 1]))
        c = None if limits is None else int(limits) if np.ndim(limits) == 0 else int(limits[n])
        kept[rows[:c]] = True
    return kept


def _image_of(off):
    image = np.full(P, -1)
    for n in range(N):
        image[off[n]:off[n + 1]] = n
    return image


def _dev(dev, off=OFF):
    return torch.from_numpy(PTS).to(dev), torch.from_numpy(np.asarray(off)).to(device=dev, dtype=torch.int32)


def _np(t):
    return t.cpu().numpy()


def _painted(canvas, color):
    """the set of (image, row, col) that hold ``color``; everything else must still be zero"""
    c = _np(canvas)
    hit = (c == np.asarray(color, np.uint8)).all(axis=-1)
    assert not c[~hit].any()
    return set(zip(*np.nonzero(hit)))


def test_the_batch_is_what_the_docstring_says():
    assert P == 42 and OFF.tolist() == [0, 14, 14, 25, 38] and (~INSIDE[:OFF[-1]]).sum() == 4 and INSIDE[OFF[-1]:].all()
    assert {_image_of(OFF)[i] for i in np.nonzero(~INSIDE)[0]} == {0, 2, 3}
    for limits in LIMITS:
        assert np.array_equal(SR.live_mask(PTS, OFF, limits, (H, W)), _kept(OFF, limits) & INSIDE)
    assert _kept(OFF, LIMITS[2]).sum() == 14 + 0 + 9 + 1 and _kept(OFF, 3).sum() == 9


@pytest.mark.parametrize("limits", LIMITS)
def test_every_consumer_keeps_the_same_rows(dev, limits):
    pts, off = _dev(dev)
    kept = _kept(OFF, limits)
    live = kept & INSIDE
    image = _image_of(OFF)
    gt = np.asarray([(5, 5), (20, 20)])
    res = score.score_points(pts, gt, hat_offsets=off, offsets=[0, 1, 1, 2, 2], limits=limits, return_match=True)
    assert np.array_equal(res.match != -2, kept)                           # score has no image to be inside of
    assert np.array_equal(res.tp + res.fp, np.bincount(image[kept], minlength=N))
    assert np.array_equal(_np(spatial.nearest(pts, (H, W), offsets=off, limits=limits).index[:, 0]) != -2, live)
    assert np.array_equal(_np(spatial.count_within(pts, (H, W), 5, offsets=off, limits=limits).counts[:, 0]) != -1, live)
    bins = _np(spatial.bin_counts(pts, (H, W), 8, offsets=off, limits=limits))
    assert np.array_equal(bins.sum(axis=(1, 2)), np.bincount(image[live], minlength=N))
    assert np.array_equal(_np(spatial.cluster(pts, (H, W), 6, 2, offsets=off, limits=limits).labels) != -2, live)
    canvas = render.draw_points(torch.zeros((N, H, W, 3), dtype=torch.uint8, device=dev), pts, off, limits, radius=0, color=(9, 8, 7))
    assert _painted(canvas, (9, 8, 7)) == {(image[i], PTS[i, 0], PTS[i, 1]) for i in np.nonzero(live)[0]}
    if limits is not None:
        tail = (image >= 0) & ~kept & INSIDE
        canvas = render.draw_points(torch.zeros((N, H, W, 3), dtype=torch.uint8, device=dev), pts, off, limits, radius=0,
                                    color=(1, 2, 3), tail=True)
        assert _painted(canvas, (1, 2, 3)) == {(image[i], PTS[i, 0], PTS[i, 1]) for i in np.nonzero(tail)[0]}
    m = torch.ones((N, H, W), dtype=torch.bool, device=dev)
    for got in (regions.split(m, pts, off, limits), regions.split_geodesic(m, pts, off, limits)):
        assert np.array_equal(_np(got.live), live)
        assert np.array_equal(_np(got.n_seeds), np.bincount(image[kept], minlength=N))


# one image whose offsets do not describe rows of the buffer: (the offsets, the image, the offsets with that image emptied)
MALFORMED = {
    "descending": ([0, 14, 14, 25, 20], 3, [0, 14, 14, 25, 25]),
    "below_zero": ([-3, 14, 14, 25, 38], 0, [14, 14, 14, 25, 38]),
    "above_rows": ([0, 14, 14, 25, P + 5], 3, [0, 14, 14, 25, 25]),
}


@pytest.mark.parametrize("case", sorted(MALFORMED))
def test_an_image_with_malformed_offsets_has_no_rows(dev, case):
    bad_off, bad, emptied = MALFORMED[case]
    limits = [50, 5, -2, 6]
    pts, off = _dev(dev, bad_off)
    live = SR.live_mask(PTS, emptied, limits, (H, W))
    kept = _kept(emptied, limits)
    image = _image_of(emptied)
    assert live.any() and not (image == bad).any() and sorted(set(image[live])) == [n for n in (0, 2, 3) if n != bad]
    if case != "above_rows":                                               # score is given no row count to hold the offsets against
        with pytest.raises(ValueError, match="offsets do not describe"):
            score.score_points(pts, np.asarray([(5, 5)]), hat_offsets=off, offsets=[0, 1, 1, 1, 1], limits=limits)
    near = spatial.nearest(pts, (H, W), k=2, offsets=off, limits=limits)
    want = SR.nearest(PTS, (H, W), 2, emptied, limits)
    assert np.array_equal(_np(near.index), want[0]) and np.array_equal(_np(near.d2), want[1])
    within = spatial.count_within(pts, (H, W), [3, 9], offsets=off, limits=limits)
    want = SR.count_within(PTS, (H, W), [3, 9], emptied, limits)
    assert np.array_equal(_np(within.counts), want[0]) and np.array_equal(_np(within.pair_counts), want[1])
    assert not _np(within.pair_counts)[bad].any()
    bins = _np(spatial.bin_counts(pts, (H, W), 8, offsets=off, limits=limits))
    assert np.array_equal(bins.sum(axis=(1, 2)), np.bincount(image[live], minlength=N)) and not bins[bad].any()
    got = spatial.cluster(pts, (H, W), 6, 2, offsets=off, limits=limits)
    well = spatial.cluster(pts, (H, W), 6, 2, offsets=torch.tensor(emptied, device=dev), limits=limits)
    assert np.array_equal(_np(got.labels) != -2, live) and torch.equal(got.labels, well.labels) and torch.equal(got.core, well.core)
    assert torch.equal(got.n_clusters, well.n_clusters) and int(got.n_clusters[bad]) == 0
    for tail in (False, True):
        rows = (image >= 0) & INSIDE & (~kept if tail else kept)
        canvas = render.draw_points(torch.zeros((N, H, W, 3), dtype=torch.uint8, device=dev), pts, off, limits, radius=0, color=(9, 8, 7),
                                    tail=tail)
        assert _painted(canvas, (9, 8, 7)) == {(image[i], PTS[i, 0], PTS[i, 1]) for i in np.nonzero(rows)[0]}
    m = np.zeros((N, H, W), bool)
    m[:, 2:10, 3:20] = m[:, 14:22, 8:29] = True
    m = torch.from_numpy(m).to(dev)
    plain = regions.label(m)
    for fn in (regions.split, regions.split_geodesic):
        got, well = fn(m, pts, off, limits), fn(m, pts, torch.tensor(emptied, device=dev), limits)
        assert np.array_equal(_np(got.n_seeds), np.bincount(image[kept], minlength=N)) and int(got.n_seeds[bad]) == 0
        assert torch.equal(got.labels[bad], plain[bad]) and int(got.counts[bad]) == 2
        assert torch.equal(got.labels, well.labels) and torch.equal(got.counts, well.counts) and torch.equal(got.live, well.live)
        assert np.array_equal(_np(got.live), live & _np(m)[image, PTS[:, 0].clip(0, H - 1), PTS[:, 1].clip(0, W - 1)])
