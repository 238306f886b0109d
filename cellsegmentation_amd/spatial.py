"""Neighbourhood statistics of detected cells on the HIP path (csrc/spatial.hip): the nearest neighbours of every point, the number
of points within a radius of it, the density map, and the density-based clusters (DBSCAN) of the points with their per-cluster
tables -- exact integer work on a bucket grid, for a ragged batch of images at once.

Points are integer (row, col) rows; image n owns ``points[offsets[n]:offsets[n + 1]]`` (``offsets=None``: one image), numpy or
torch, on the host or the device, as ``score.score_points`` takes them.  ``limits`` (None, one count or one per image) applies
Python's slice ``[:c]`` to every image's points, which is what ``DetectResult.per_image`` does with a regression count.  A point
is *live* when it is within its image's limit and inside ``[0, H) x [0, W)`` of ``image_hw = (H, W)``; ``H^2 + W^2 < 2^31``, so every
squared distance fits an int32.  A point that is not live neither asks nor answers: its output rows hold -2 (index) and -1 (squared
distance, count), the convention of ``ScoreResult.match``.

The targets are the points themselves, or a second set ``other`` / ``other_offsets`` / ``other_limits`` per image (``other_xy``:
its rows are (x, y), as ``gt_xy`` of ``score_points``).  Among themselves a point is never its own neighbour -- the same row of the
buffer -- but another point at the same coordinates is a neighbour at distance 0; against a second set nothing is excluded.  Images
share nothing.  An index is the target's index within its image.

Every result is decided by integer comparisons: neighbours are ordered by the key (d2, index), so equal distances go to the lower
index, and the counts are sums of integers.  Nothing depends on the bucket side, which is chosen on the host from the sizes alone
(``choose_bucket``): launch grids and the workspace are independent of the data, nothing synchronises, and a call can be captured
under ``torch.cuda.graph``.

``voronoi_graph`` is the one function here that works on pixels: it paints the live points into a seed label image
(``cs_regions_seed_labels``), lets every pixel take its nearest seed (``morph.nearest_sites``, or ``morph.expand_labels`` for
territories bounded by a distance) and reads the neighbour graph off that label image with ``regions.adjacency_labels`` -- the raster
Voronoi graph of the detections, row k = point k.  Exact integers again, but its launches and read-backs are those of the functions
it is made of (its docstring says which).
"""
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import kernels as K
from ._args import _device
from ._points import PointSet
from .score import radius_squared

THREADS = 256                  # workgroup width of the query kernels           (cs_spatial_threads)
CHUNK = 512                    # candidate records staged in LDS at a time       (cs_spatial_chunk)
MAX_BUCKETS = 1 << 22          # buckets of one call, all images together        (cs_spatial_max_buckets)
MAX_K = 8
MAX_RADII = 8
OCCUPANCY = 8                  # targets per bucket that choose_bucket aims at


@dataclass
class NeighborTable:
    """``index``, ``d2`` int32 [P, k] on the device: column j of a live row holds the (j + 1)-th smallest key (d2, index within the
    image) among the live targets of the row's image, (-1, -1) beyond their number; rows that are not live hold (-2, -1)."""
    index: torch.Tensor
    d2: torch.Tensor

    def distance(self):
        """float64 [P, k] on the device: sqrt(d2) in pixels, NaN where there is no neighbour"""
        d = self.d2.to(torch.float64)
        return torch.where(self.d2 >= 0, d.clamp(min=0).sqrt(), torch.full_like(d, float("nan")))


@dataclass
class WithinCounts:
    """``counts`` int32 [P, R]: the live targets within each radius of every live point (-1 in the rows that are not live);
    ``pair_counts`` int64 [N, R]: their per-image sums.  ``radii2``: the integer ``floor(r^2)`` the kernel compared against."""
    counts: torch.Tensor
    pair_counts: torch.Tensor
    radii2: tuple


@dataclass
class ClusterTable:
    """The DBSCAN clusters of every image's live points (``cluster``), all device tensors.  Per row of ``points``: ``labels`` int32
    [P], the cluster number within the row's image, -1 for noise, -2 in the rows that are not live; ``core`` uint8 [P], 1 on core
    points.  ``n_clusters`` int32 [N].  The cluster tables have P rows too and use the points' own ``offsets``: cluster c of image n
    is row ``offsets[n] + c`` -- an image never has more clusters than points, so nothing overflows.  ``size`` int32 [P] (core plus
    border points), ``n_core`` int32 [P], ``sums`` int64 [P, 2] (sum of rows, sum of columns), ``bbox`` int32 [P, 4] = r0, c0, r1, c1
    half-open, as ``RegionTable.bbox``; every other table row is all zero.  ``radius2``, ``min_samples``: the integers the kernels
    compared against."""
    labels: torch.Tensor
    core: torch.Tensor
    n_clusters: torch.Tensor
    size: torch.Tensor
    n_core: torch.Tensor
    sums: torch.Tensor
    bbox: torch.Tensor
    radius2: int
    min_samples: int
    offsets: torch.Tensor

    @property
    def centroid(self):
        """float64 [P, 2] on the device: (row, col) = sums / size, NaN in the table rows that no cluster owns"""
        return self.sums.to(torch.float64) / self.size.to(torch.float64)[:, None]

    @property
    def n_noise(self):
        """int64 [N] on the device: the live points of every image that belong to no cluster; nothing synchronises"""
        seen = torch.cat([self.labels.new_zeros(1, dtype=torch.int64), (self.labels == -1).to(torch.int64).cumsum(0)])
        at = self.offsets.clamp(0, self.labels.numel())
        return seen[at[1:]] - seen[at[:-1]]

    def per_image(self):
        """A host list of N dicts of numpy arrays: ``labels`` and ``core`` of the image's rows, and ``size``, ``n_core``, ``bbox``,
        ``centroid`` trimmed to its ``n_clusters`` rows.  The one method that synchronises."""
        cols = {"size": self.size, "n_core": self.n_core, "bbox": self.bbox, "centroid": self.centroid}
        cols = {k: v.cpu().numpy() for k, v in cols.items()}
        labels, core = self.labels.cpu().numpy(), self.core.cpu().numpy()
        off, counts = self.offsets.cpu().numpy(), self.n_clusters.cpu().numpy()
        out = []
        for n, c in enumerate(counts):
            d = {"labels": labels[off[n]:off[n + 1]], "core": core[off[n]:off[n + 1]]}
            d.update({k: v[off[n]:off[n] + int(c)] for k, v in cols.items()})
            out.append(d)
        return out


def check_image_hw(image_hw):
    """(H, W) positive integers with H^2 + W^2 < 2^31 (the rule of ``detect._check_dt_shape``) -> (H, W)"""
    try:
        H, W = image_hw
    except (TypeError, ValueError):
        raise TypeError(f"image_hw: expected (H, W), got {image_hw!r}") from None
    for v in (H, W):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise TypeError(f"image_hw: expected two integers, got {image_hw!r}")
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError(f"image_hw: expected positive sizes, got {(H, W)}")
    if H * H + W * W >= 1 << 31:
        raise ValueError(f"image_hw: H^2 + W^2 must stay below 2^31 (squared distances are int32), got {(H, W)}")
    return H, W


def n_buckets(H, W, b):
    return -(-H // b) * -(-W // b)


def choose_bucket(H, W, n_images, n_targets, reach=0):
    """The side b of the square buckets, from sizes known on the host only: about ``OCCUPANCY`` targets per bucket were they spread
    evenly (b = ceil(sqrt(OCCUPANCY N H W / n_targets))), at least half the largest radius ``reach`` (so that the box of a radius
    query spans a handful of bucket rows, not dozens), at most max(H, W), then raised until the call's N ceil(H / b) ceil(W / b)
    buckets fit ``MAX_BUCKETS``."""
    b = math.isqrt(max(OCCUPANCY * n_images * H * W // max(int(n_targets), 1) - 1, 0)) + 1
    b = max(b, -(-int(reach) // 2), 1)
    b = min(b, max(H, W))
    while n_images * n_buckets(H, W, b) > MAX_BUCKETS:
        b += max(1, b // 8)
    return min(b, max(H, W))


def _check_bucket(_bucket, H, W, n_images):
    if isinstance(_bucket, bool) or not isinstance(_bucket, (int, np.integer)) or _bucket < 1:
        raise ValueError(f"_bucket must be a positive integer, got {_bucket!r}")
    b = min(int(_bucket), max(H, W))
    if n_images * n_buckets(H, W, b) > MAX_BUCKETS:
        raise ValueError(f"_bucket={_bucket}: {n_images} images of {n_buckets(H, W, b)} buckets exceed the {MAX_BUCKETS} of one call")
    return b


def _sets(what, points, offsets, limits, other, other_offsets, other_limits, other_xy):
    q = PointSet(points, offsets, limits, None, f"{what}: points")
    if other is None:
        if other_offsets is not None or other_limits is not None or other_xy:
            raise ValueError(f"{what}: other_offsets, other_limits and other_xy describe `other`, which was not given")
        return q, None
    return q, PointSet(other, other_offsets, other_limits, q.n_images, f"{what}: other")


def _bucket_for(_bucket, H, W, q, t, reach=0):
    if _bucket is not None:
        return _check_bucket(_bucket, H, W, q.n_images)
    return choose_bucket(H, W, q.n_images, (t or q).rows, reach)


def _upload(q, t, *args):
    dev = _device(*args)
    q.upload(dev)
    if t is None:
        return {}
    t.upload(dev)
    return {"other": t.pts_dev, "other_off": t.off_dev, "other_limits": t.lim_dev}


def nearest(points, image_hw, k=1, offsets=None, limits=None, other=None, other_offsets=None, other_limits=None, other_xy=False,
            _bucket=None):
    """The k nearest live targets of every live point -> ``NeighborTable`` (module docstring: inputs, live points, targets).
    Column j holds the (j + 1)-th smallest key (d2, index); equal distances go to the lower index; columns beyond the number of
    candidates hold (-1, -1).  ``1 <= k <= 8``.  ``_bucket`` (tests, tools/spatial_microbench.py): the bucket side instead of
    ``choose_bucket``'s; the result does not depend on it."""
    H, W = check_image_hw(image_hw)
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= MAX_K:
        raise ValueError(f"nearest: k must be an integer in 1..{MAX_K}, got {k!r}")
    q, t = _sets("nearest", points, offsets, limits, other, other_offsets, other_limits, other_xy)
    b = _bucket_for(_bucket, H, W, q, t)
    kw = _upload(q, t, points, offsets, other, other_offsets)
    index, d2 = K.spatial_nearest(q.pts_dev, q.off_dev, H, W, b, int(k), limits=q.lim_dev, other_xy=other_xy, **kw)
    return NeighborTable(index, d2)


def count_within(points, image_hw, radii, offsets=None, limits=None, other=None, other_offsets=None, other_limits=None,
                 other_xy=False, _bucket=None):
    """The number of live targets within each radius of every live point -> ``WithinCounts``.  ``radii``: one non-negative number
    or up to 8; a target counts when its integer ``d2 <= floor(r^2)`` (``score.radius_squared``), i.e. exactly where ``sqrt(d2) <=
    r``, so radius 0 counts coincident points only.  Among the points themselves a point does not count itself and the counts
    are ORDERED pairs: a pair of points within r of each other adds one to each of the two rows and two to ``pair_counts`` -- the
    raw ingredient of Ripley's K, without edge correction.  All radii are served by one pass over the box of the largest."""
    H, W = check_image_hw(image_hw)
    rs = [radii] if isinstance(radii, (int, float, np.integer, np.floating)) and not isinstance(radii, bool) else radii
    try:
        rs = list(rs)
    except TypeError:
        raise TypeError(f"count_within: radii must be a number or a sequence of numbers, got {radii!r}") from None
    if not 1 <= len(rs) <= MAX_RADII:
        raise ValueError(f"count_within: 1 to {MAX_RADII} radii in one call, got {len(rs)}")
    r2 = tuple(radius_squared(r) for r in rs)
    q, t = _sets("count_within", points, offsets, limits, other, other_offsets, other_limits, other_xy)
    b = _bucket_for(_bucket, H, W, q, t, reach=min(math.isqrt(max(r2)), max(H, W)))
    kw = _upload(q, t, points, offsets, other, other_offsets)
    counts, pairs = K.spatial_count_within(q.pts_dev, q.off_dev, H, W, b, r2, limits=q.lim_dev, other_xy=other_xy, **kw)
    return WithinCounts(counts, pairs, r2)


def cluster(points, image_hw, eps, min_samples=5, offsets=None, limits=None, _bucket=None):
    """Density-based clustering (DBSCAN) of every image's live points -> ``ClusterTable``: which cells form an aggregate, how many
    aggregates there are, how large each one is and where it lies.  The labels and core flags equal
    ``sklearn.cluster.DBSCAN(eps, min_samples)`` image by image, with ``d2 <= floor(eps^2)`` (``score.radius_squared``) for
    ``distance <= eps``:

    * a live point is a *core point* when at least ``min_samples`` live points of its image lie within ``eps`` of it, itself
      included; another row at the same coordinates is a neighbour at distance 0;
    * two core points share a cluster when a chain of core points joins them whose steps are all within ``eps``; an image's
      clusters are numbered from 0 in increasing order of the smallest index that a core point of the cluster has;
    * a live point that is not core but has a core point within ``eps`` is a *border point* of the lowest-numbered cluster among
      those core points' -- it never joins two clusters; every other live point is noise, label -1; rows that are not live hold -2.

    ``min_samples`` is an integer >= 1.  ``min_samples=1`` makes every live point a core point: single-linkage ("friends of
    friends") grouping at distance ``eps``, the connected components of the graph of pairs within ``eps``.  Nothing depends on the
    bucket side, the launch order or thread timing; the launches follow from the sizes alone, so a call can be captured."""
    H, W = check_image_hw(image_hw)
    r2 = radius_squared(eps)
    if isinstance(min_samples, bool) or not isinstance(min_samples, (int, np.integer)) or not 1 <= min_samples < 1 << 31:
        raise ValueError(f"cluster: min_samples must be an integer in 1..2^31 - 1, got {min_samples!r}")
    q = PointSet(points, offsets, limits, None, "cluster: points")
    b = _bucket_for(_bucket, H, W, q, None, reach=min(math.isqrt(r2), max(H, W)))
    _upload(q, None, points, offsets)
    out = K.spatial_cluster(q.pts_dev, q.off_dev, H, W, b, r2, int(min_samples), limits=q.lim_dev)
    return ClusterTable(*out, r2, int(min_samples), q.off_dev)


def voronoi_graph(points, image_hw, offsets=None, limits=None, max_distance=None, connectivity=1, max_pairs=None):
    """The raster Voronoi neighbour graph of every image's live points -> ``(regions.AdjacencyTable, labels)``: which detections
    are neighbours, the cell graph that graph-based tissue analysis starts from.

    Point k of an image is label k + 1.  The seed label image holds k + 1 at the pixel of live point k (of several live points on
    one pixel the lowest k owns it; the others own nothing and have no neighbours) and 0 elsewhere.  With ``max_distance=None``
    every pixel takes the label of its nearest seed, among equally near seeds the one with the lowest row-major pixel index
    (``morph.nearest_sites``): the raster Voronoi diagram.  With a number, ``morph.expand_labels(seeds, max_distance)``: the
    territories are bounded by that distance, and two points are neighbours only if their territories meet.  ``labels`` is that
    int32 [N, H, W] device image, and the table is ``regions.adjacency_labels(labels, connectivity)`` with capacity = the largest
    point count of an image, so that row k of image n is point k: ``sides`` is the length in pixel sides of the border two
    territories share.  ``max_pairs`` as in ``adjacency_labels``: None reads a counter back and doubles the pair table until every
    pair fits.  Offsets given as a device tensor cost one more read-back, for the capacity.

    This is the RASTER Voronoi graph.  Parity with ``scipy.spatial.Delaunay`` is not claimed: a thin raster cell can be cut where
    the exact one is connected, and co-circular integer points, whose exact Voronoi cells meet in a single vertex, come out as
    neighbours by a pixel side or corner or not at all.  Memory on a whole slide: the seed image and the label image, two int32
    images of N H W pixels, are held at once; ``max_distance=None`` holds two more (the squared distances and the site indices)
    during the call, and its search is as far as the nearest seed lies -- bound it with ``max_distance`` where seeds are sparse."""
    from . import morph as M
    from . import regions as Rg
    H, W = check_image_hw(image_hw)
    conn = Rg._check_connectivity(connectivity)
    Rg._check_max_pairs(max_pairs)
    r2 = None if max_distance is None else radius_squared(max_distance)
    if W > M.MAX_SITE_WIDTH:
        raise ValueError(f"voronoi_graph: rows wider than {M.MAX_SITE_WIDTH} pixels are not supported, got {H}x{W}")
    q = PointSet(points, offsets, limits, None, "voronoi_graph: points")
    if q.n_images * H * W >= 1 << 31:
        raise ValueError(f"voronoi_graph: a call takes fewer than 2^31 pixels, got {q.n_images} images of {H}x{W}")
    _upload(q, None, points, offsets)
    seeds = K.regions_seed_labels(q.pts_dev, q.off_dev, H, W, limits=q.lim_dev)
    if r2 is None:
        _, site = M.nearest_sites(seeds)
        flat = seeds.flatten(-2).gather(-1, site.flatten(-2).clamp(min=0).to(torch.int64)).view_as(seeds)
        labels = torch.where(site >= 0, flat, torch.zeros_like(flat))    # an image without a seed has no site
    else:
        labels = M.expand_labels(seeds, radius_sq=r2)
    per_image = np.diff(q.off) if q.off is not None else (q.off_dev[1:] - q.off_dev[:-1]).cpu().numpy()
    cap = max(1, int(per_image.max()))
    return Rg.adjacency_labels(labels, conn, max_regions=cap, max_pairs=max_pairs), labels


def bin_counts(points, image_hw, bin, offsets=None, limits=None):
    """The number of live points per square bin of side ``bin`` pixels -> int32 [N, ceil(H / bin), ceil(W / bin)] on the device: the
    density map, and the grid's own count pass.  At most ``MAX_BUCKETS`` bins in one call."""
    H, W = check_image_hw(image_hw)
    if isinstance(bin, bool) or not isinstance(bin, (int, np.integer)) or bin < 1:
        raise ValueError(f"bin_counts: bin must be a positive integer, got {bin!r}")
    q = PointSet(points, offsets, limits, None, "bin_counts: points")
    if q.n_images * n_buckets(H, W, int(bin)) > MAX_BUCKETS:
        raise ValueError(f"bin_counts: {q.n_images} images of {n_buckets(H, W, int(bin))} bins exceed the {MAX_BUCKETS} of one call")
    _upload(q, None, points, offsets)
    return K.spatial_bin_counts(q.pts_dev, q.off_dev, H, W, int(bin), limits=q.lim_dev)
