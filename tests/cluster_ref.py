"""Brute-force numpy restatement of cellsegmentation_amd.spatial.cluster (csrc/spatial.hip): DBSCAN as the kernels are held to it,
all pairs, image by image, with the per-cluster tables.  (tests/golden/make_cluster_golden.py pins it to scikit-learn.)

Image n owns rows off[n]:off[n + 1]; LIVE as in tests/spatial_ref.py.  With r2 = floor(eps^2):
  core     a live point with 1 + #(other live rows of the image with d2 <= r2) >= min_samples
  cluster  core points joined by a chain of core points with steps of d2 <= r2; numbered from 0 in increasing order of the smallest
           index within the image that a core point of the cluster has
  border   a live point that is not core with a core point within r2: the lowest cluster number among those core points'
  labels   the cluster number, -1 noise, -2 in the rows that are not live
Cluster c of image n is row off[n] + c of the tables (size, n_core, sums, bbox half-open); every other table row is zero."""
import numpy as np

from spatial_ref import live_mask, radius_squared, ragged  # noqa: F401


def image_labels(p, r2, min_samples):
    """the live points [m, 2] of one image in row order -> (labels int [m], core bool [m])"""
    m = len(p)
    d2 = (p[:, None, 0] - p[None, :, 0]) ** 2 + (p[:, None, 1] - p[None, :, 1]) ** 2
    near = d2 <= r2                                                        # the diagonal: the point counts itself
    core = near.sum(axis=1) >= min_samples
    labels = np.full(m, -1, np.int64)
    c = 0
    for i in range(m):                                                     # in increasing order of the smallest core index
        if not core[i] or labels[i] >= 0:
            continue
        labels[i] = c
        stack = [i]
        while stack:
            a = stack.pop()
            for j in np.nonzero(near[a] & core & (labels < 0))[0]:
                labels[j] = c
                stack.append(j)
        c += 1
    for i in np.nonzero(~core)[0]:
        reach = near[i] & core
        if reach.any():
            labels[i] = labels[reach].min()
    return labels, core


def cluster(pts, hw, eps, min_samples, off=None, limits=None):
    """-> dict: labels int32 [P], core uint8 [P], n_clusters int32 [N], size int32 [P], n_core int32 [P], sums int64 [P, 2],
    bbox int32 [P, 4]"""
    pts = np.asarray(pts, np.int64).reshape(-1, 2)
    off = np.asarray([0, len(pts)] if off is None else off, np.int64)
    live = live_mask(pts, off, limits, hw)
    r2 = radius_squared(eps)
    P, N = len(pts), len(off) - 1
    out = {"labels": np.full(P, -2, np.int32), "core": np.zeros(P, np.uint8), "n_clusters": np.zeros(N, np.int32),
           "size": np.zeros(P, np.int32), "n_core": np.zeros(P, np.int32), "sums": np.zeros((P, 2), np.int64),
           "bbox": np.zeros((P, 4), np.int32)}
    for n in range(N):
        rows = np.arange(off[n], off[n + 1])
        rows = rows[live[rows]]
        labels, core = image_labels(pts[rows], r2, min_samples)
        out["labels"][rows] = labels
        out["core"][rows] = core
        out["n_clusters"][n] = labels.max() + 1 if len(labels) else 0
        for c in range(int(out["n_clusters"][n])):
            mine = rows[labels == c]
            t = off[n] + c
            out["size"][t] = len(mine)
            out["n_core"][t] = out["core"][mine].sum()
            out["sums"][t] = pts[mine].sum(axis=0)
            out["bbox"][t] = (*pts[mine].min(axis=0), *(pts[mine].max(axis=0) + 1))
    return out
