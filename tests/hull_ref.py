"""Pure numpy / Python-int restatement of the per-label convex hull (cellsegmentation_amd.regions.hull_labels / HullTable), the
reference of tests/test_hull_gpu.py.  The rules, as the docstring of ``regions.hull_labels`` states them:

* a pixel's object id is max(label, 0); images of a batch are independent; a label need not be connected;
* an object is the union of the closed unit squares of its pixels: pixel (r, c) gives the lattice points (r, c), (r + 1, c),
  (r, c + 1), (r + 1, c + 1), and the hull is the convex hull of those points;
* only the corners of the leftmost and the rightmost pixel of every pixel row are candidates;
* per label: n_vertices (strict vertices), area2 (shoelace, twice the area), feret_max2 (the largest squared distance of two
  vertices), and (width_cross, width_len2) of the hull edge that minimises (cross^2 / len2, len2), cross(e) being the largest
  |(b - a) x (v - a)| over the vertices v and len2(e) = |b - a|^2, the fractions compared by cross-multiplication;
* a bounding box of more than MAX_SIDE rows or columns: all five entries -1; a label without a pixel: all zero.

Here: Andrew's monotone chain over the sorted candidates, Python ints throughout.  Pinned to scipy.spatial.ConvexHull (qhull) over
ALL corners of all pixels by tests/golden/hull_vectors.npz (tests/test_hull_host.py); scipy is not imported here.  Row k of image n
is label k + 1; rows of labels above the capacity do not exist.
"""
import numpy as np

MAX_SIDE = 1024
COLUMNS = ("convex_area", "solidity", "feret_diameter_max", "feret_diameter_min", "n_vertices")


def candidates(rr, cc):
    """pixel coordinates of one object -> the sorted lattice corners of the leftmost and rightmost pixel of every pixel row"""
    pts = set()
    order = np.lexsort((cc, rr))
    rr, cc = rr[order], cc[order]
    starts = np.flatnonzero(np.r_[True, rr[1:] != rr[:-1]])
    ends = np.r_[starts[1:], len(rr)] - 1
    for r, lo, hi in zip(rr[starts].tolist(), cc[starts].tolist(), cc[ends].tolist()):
        pts.update(((r, lo), (r + 1, lo), (r, hi + 1), (r + 1, hi + 1)))
    return sorted(pts)


def _cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def convex_hull(pts):
    """sorted distinct lattice points -> the strict vertices of their hull, in order round it (Andrew's monotone chain)"""
    def half(seq):
        out = []
        for p in seq:
            while len(out) >= 2 and _cross(out[-2], out[-1], p) <= 0:
                out.pop()
            out.append(p)
        return out
    lower, upper = half(pts), half(pts[::-1])
    return lower[:-1] + upper[:-1]


def narrower(a, b):
    """of two (cross, len2) the one with the smaller (cross^2 / len2, len2)"""
    wa, wb = a[0] * a[0] * b[1], b[0] * b[0] * a[1]
    assert max(wa, wb) < 2 ** 64
    if wa != wb:
        return a if wa < wb else b
    return a if a[1] <= b[1] else b


def measures(v):
    """hull vertices in order -> (n_vertices, area2, feret_max2, width_cross, width_len2)"""
    n = len(v)
    area2 = abs(sum(v[k][0] * v[(k + 1) % n][1] - v[(k + 1) % n][0] * v[k][1] for k in range(n)))
    far2 = max((p[0] - q[0]) ** 2 + (p[1] - q[1]) ** 2 for p in v for q in v)
    best = None
    for k in range(n):
        a, b = v[k], v[(k + 1) % n]
        edge = (max(abs(_cross(a, b, p)) for p in v), (b[0] - a[0]) ** 2 + (b[1] - a[1]) ** 2)
        best = edge if best is None else narrower(best, edge)
    return (n, area2, far2) + best


def _one(lab, cap):
    """one [H, W] label image -> (area, bbox, sum_rc, hull) with cap rows"""
    ids = np.maximum(lab, 0).astype(np.int64)
    rr, cc = np.nonzero((ids > 0) & (ids <= cap))
    k = ids[rr, cc] - 1
    area = np.bincount(k, minlength=cap).astype(np.int32)
    bbox = np.zeros((cap, 4), np.int32)
    bbox[:, :2] = np.iinfo(np.int32).max
    np.minimum.at(bbox[:, 0], k, rr)
    np.minimum.at(bbox[:, 1], k, cc)
    np.maximum.at(bbox[:, 2], k, rr + 1)
    np.maximum.at(bbox[:, 3], k, cc + 1)
    bbox[area == 0] = 0
    sums = np.zeros((cap, 2), np.int64)
    np.add.at(sums[:, 0], k, rr)
    np.add.at(sums[:, 1], k, cc)
    hull = np.zeros((cap, 5), np.int32)
    order = np.argsort(k, kind="stable")                                  # the pixels of label 1, then of 2, ...
    start = np.concatenate([[0], np.cumsum(area)])
    for i in np.flatnonzero(area):
        if max(bbox[i, 2] - bbox[i, 0], bbox[i, 3] - bbox[i, 1]) > MAX_SIDE:
            hull[i] = -1
            continue
        mine = order[start[i]:start[i + 1]]
        hull[i] = measures(convex_hull(candidates(rr[mine], cc[mine])))
    return area, bbox, sums, hull


def hull_labels(labels, max_regions=None):
    """labels int [H, W] or [N, H, W] -> dict: counts int32 [N] (the largest label of every image), capacity (max_regions, or the
    largest count, at least 1), area int32 [N, cap], bbox int32 [N, cap, 4], sum_rc int64 [N, cap, 2], hull int32 [N, cap, 5]."""
    labels = np.asarray(labels)
    ls = labels[None] if labels.ndim == 2 else labels
    counts = np.asarray([max(int(x.max()), 0) for x in ls], np.int32)
    cap = max(1, int(counts.max())) if max_regions is None else int(max_regions)
    per = [_one(x, cap) for x in ls]
    out = {"counts": counts, "capacity": cap}
    for j, key in enumerate(("area", "bbox", "sum_rc", "hull")):
        out[key] = np.stack([p[j] for p in per])
    return out


def hull(m, connectivity=1, max_regions=None):
    """``hull_labels`` of the components of a boolean mask, numbered as scipy.ndimage.label (regions_ref.label)"""
    import regions_ref as R
    m = np.asarray(m)
    lab = np.stack([R.label(x, connectivity)[0] for x in m]) if m.ndim == 3 else R.label(m, connectivity)[0]
    return hull_labels(lab.astype(np.int32), max_regions)


# ---- the float64 columns of HullTable, from the integer tables only --------------------------------------------------------------
def too_large(t):
    return t["hull"][..., 0] < 0


def _measured(t, x):
    """x where the row holds a measured object, else NaN"""
    return np.where((t["area"] > 0) & ~too_large(t), x, np.nan)


def convex_area(t):
    return _measured(t, t["hull"][..., 1].astype(np.float64) / 2)


def solidity(t):
    with np.errstate(invalid="ignore", divide="ignore"):
        return t["area"].astype(np.float64) / convex_area(t)


def feret_diameter_max(t):
    with np.errstate(invalid="ignore"):
        return _measured(t, np.sqrt(t["hull"][..., 2].astype(np.float64)))


def feret_diameter_min(t):
    with np.errstate(invalid="ignore", divide="ignore"):
        return _measured(t, t["hull"][..., 3].astype(np.float64) / np.sqrt(t["hull"][..., 4].astype(np.float64)))


def n_vertices(t):
    return _measured(t, t["hull"][..., 0].astype(np.float64))


def columns(t):
    """name -> float64 array, one per float method of HullTable"""
    return {k: globals()[k](t) for k in COLUMNS}
