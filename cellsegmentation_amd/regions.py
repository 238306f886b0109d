"""Small-region clean-up of segmentation masks: the reference's ``remove_small_regions`` (utils/image_processing.py:14-17), i.e.
``skimage.morphology.remove_small_objects`` followed by ``remove_small_holes``, on the HIP path (csrc/regions.hip).

Semantics, restated from scikit-image (which labels with ``scipy.ndimage.label``):

* ``connectivity`` 1 is the 4-neighbourhood (the default, and the only one the reference uses), 2 the 8-neighbourhood; the
  background is labelled with the same connectivity as the foreground.
* ``remove_small_objects`` clears every ``True`` component with fewer than ``min_size`` pixels (strict); ``min_size=0`` copies.
* ``remove_small_holes`` is ``~remove_small_objects(~m, area_threshold)``: every ``False`` component below the threshold becomes
  ``True``, the ones that touch the image border included.
* ``remove_small_regions`` removes objects first and takes the holes of the result.
* ``label`` numbers components by their lowest row-major pixel index, as ``scipy.ndimage.label``.

All of it is integer work: bit-exact and independent of launch order.  The labelling is pinned to ``scipy.ndimage.label``
(tests/golden/regions_vectors.npz); parity with scikit-image itself is NOT pinned (it is not a dependency of this project): its
two wrappers are restated.  Only boolean input is taken: scikit-image treats an integer array as a label image, which is a
different operation, and that raises ``TypeError`` here.

Every function takes ``[H, W]`` or ``[N, H, W]`` (numpy or torch; N independent images) and returns a device tensor of the same
shape.  A call enqueues a number of launches fixed by the shape and never synchronises, so it can be captured into a graph.

``measure`` turns the same labelling into one table row per foreground component (``RegionTable``: count, area, bounding box,
centroid, intensity sum / mean / maximum), pinned to ``scipy.ndimage`` (sum, mean, maximum, center_of_mass, find_objects;
tests/golden/props_vectors.npz).  With a fixed ``max_regions`` it keeps the contract above; with ``max_regions=None`` it reads the
largest component count back once to size the tables.

``split`` cuts the components at seed points (one per cell, ``detect.detect_points``): every foreground pixel goes to the nearest
seed of its own component and label k + 1 is point k, so that ``measure_labels`` -- the same tables for a label image -- gives one
row per detection.  Exact integer rules, stated once in ``split``'s docstring and restated in numpy by tests/split_ref.py.

``split_geodesic`` is the same split with the distance measured along paths that stay inside the component (5-7 chamfer steps), so
that every cell comes out connected, which ``measure_labels``, ``shape_labels``, ``hull_labels`` and the matching functions assume:
exact integers again, the rule stated once in ``split_geodesic``'s docstring and restated in plain loops by tests/geodesic_ref.py
(``GeodesicSplitResult``).  With a fixed ``max_rounds`` it keeps the contract above; with ``max_rounds=None`` it reads a flag per
image back between batches of rounds until every image has converged.

``match_labels`` scores one label image against another at the object level: the partner of every label at IoU > 1/2, in exact
integers (``MatchTable``; the rule is in ``match_labels``'s docstring, restated in numpy by tests/match_ref.py), from which
``MatchTable.score`` forms TP / FP / FN, segmentation quality and panoptic quality on the host (``score.label_score``).

``overlap_labels`` lists every (pred, truth) pair of labels that shares a pixel, with the count, and gives every label its best
partner by IoU and by intersection, however small the overlap (``OverlapTable``; restated in numpy by tests/overlap_ref.py), from
which ``OverlapTable.score`` forms AJI and object-level Dice on the host (``score.overlap_score``).

``hausdorff_labels`` holds every object against its partner on the other side -- ``overlap_labels``' best-intersection partner, or
the nearest object where it overlaps nothing -- by the squared Hausdorff distance of the two pixel sets, in exact integers
(``HausdorffTable``; restated in numpy by tests/hausdorff_ref.py), from which ``HausdorffTable.score`` forms the object-level
Hausdorff distance on the host (``score.hausdorff_score``).

``shape_labels`` (``shape`` for a boolean mask) adds what says how a cell is shaped to the table that says where it is: int64 second
moments about the corner of the bounding box and four tallies of boundary pixels per label, in exact integers (``ShapeTable``; the
rules are in ``shape_labels``'s docstring, restated in numpy by tests/shape_ref.py), from which ``ShapeTable`` forms central moments,
axis lengths, eccentricity, orientation, perimeter, circularity, extent and equivalent diameter in float64 on the device.
``boundaries`` gives the inner-boundary map alone, e.g. as outlines for an overlay.

``hull_labels`` (``hull`` for a boolean mask) adds the convex hull of every label's pixel squares: vertex count, twice the area,
the largest squared vertex distance and the smallest width as an exact fraction, in exact integers (``HullTable``; the rules are in
``hull_labels``'s docstring, restated in Python integers by tests/hull_ref.py), from which ``HullTable`` forms convex area, solidity
and the largest and smallest Feret diameter in float64 on the device.  Objects whose bounding box exceeds 1024 rows or columns are
counted, not measured.

``contour_labels`` (``contours`` for a boolean mask) adds the outline of every label as an ordered polygon: the ring of lattice
vertices round the component of the label's first pixel, walked along the pixel sides with the object on the right hand, with its
vertex count, length, enclosed area and the length of all of the label's boundary, in exact integers (``ContourTable``; the rule is
in ``contour_labels``'s docstring, restated in plain loops by tests/contour_ref.py), from which ``ContourTable`` tells one-piece
labels without holes from the others and writes GeoJSON polygons for QuPath or shapely on the host.  Holes are not traced, and
objects whose bounding box exceeds 512 rows or columns are counted, not traced.

``adjacency_labels`` (``adjacency`` for a boolean mask) relates the cells of ONE label image to each other: every pair of labels
that shares a pixel side (with ``connectivity=2`` also a pixel corner) with the number of shared sides and corners, and per label the
number of neighbours, the sides shared with other cells, with the background and with the image edge, and the neighbour of longest
contact, in exact integers (``AdjacencyTable``; the rules are in ``adjacency_labels``'s docstring, restated in numpy by
tests/adjacency_ref.py), from which ``AdjacencyTable`` forms the touching fraction in float64 and the cell graph as a COO edge list
on the device.  ``distance=`` expands the labels first (``morph.expand_labels``), so that cells within a gap count as neighbours.

``texture_labels`` adds how the grey values of a uint8 plane are arranged inside every label: the grey-level co-occurrence matrix of
the pixel pairs inside the label at one distance in four directions, folded to its pair count, its difference, sum and marginal
histograms, its sum of squares and its cross moment, in exact integers (``TextureTable``; the rules are in ``texture_labels``'s
docstring, restated in numpy by tests/texture_ref.py), from which ``TextureTable`` forms Haralick's features -- contrast,
homogeneity, energy, correlation, the entropies -- in float64 on the device.  ``stain.texture_labels`` is the same over one stain
of an RGB image.
"""
import dataclasses
import functools
import typing

import numpy as np
import torch

from . import kernels as K
from ._args import MAX_PIXELS as _MAX_PIXELS          # per kernel call; larger batches are cut into chunks of whole images
from ._args import _device, _images, _tensor

_MAX_IMAGES = 65535


def _check_connectivity(connectivity):
    if connectivity not in (1, 2):
        raise ValueError(f"connectivity must be 1 (4-neighbourhood) or 2 (8-neighbourhood), got {connectivity!r}")
    return int(connectivity)


def _check_size(value, name):
    if isinstance(value, bool) or int(value) != value or value < 0:
        raise ValueError(f"{name} must be a non-negative integer, got {value!r}")
    return min(int(value), _MAX_PIXELS)           # no component has more pixels than a call


def _as_masks(m, what):
    """boolean numpy / torch [H,W] or [N,H,W] -> (uint8 device view [N,H,W], was_2d); argument errors before any device work."""
    t = _images(m, what, torch.bool, "a boolean mask, got {} (an integer array is a label image in scikit-image: not supported)",
                noun="mask", lift=True, to_device=True)
    return t.contiguous().view(torch.uint8), m.ndim == 2


def _chunks(t):
    """whole images per kernel call"""
    N, H, W = t.shape
    per = max(1, min(_MAX_IMAGES, _MAX_PIXELS // (H * W)))
    return [(i, min(i + per, N)) for i in range(0, N, per)]


# the workspace of the kernel calls of one batch: ``_Workspace(make)(n)`` is ``make(n)``, the workspace of a chunk of n images, kept
# for as long as n stays the same (the chunks of a batch are equal but for the last)
_Workspace = functools.lru_cache(maxsize=1)


def _run(t, fn, out):
    """fn(chunk, out_chunk, workspace) over the chunks of t [N,H,W]; out: a tensor of t's shape"""
    workspace = _Workspace(lambda n: K.regions_workspace(n, t.shape[1], t.shape[2], t.device))
    for a, b in _chunks(t):
        fn(t[a:b], out[a:b], workspace(b - a))
    return out


def _int32_like(t):
    return torch.empty(t.shape, dtype=torch.int32, device=t.device)


def label(m, connectivity=1):
    """``scipy.ndimage.label`` of every image: int32 device tensor, 0 = background, components numbered from 1 by their lowest
    row-major pixel index."""
    conn = _check_connectivity(connectivity)
    t, two_d = _as_masks(m, "label")
    out = _run(t, lambda x, o, ws: K.regions_label(x, conn, out=o, ws=ws), _int32_like(t))
    return out[0] if two_d else out


def component_areas(m, connectivity=1):
    """int32 device tensor: under every pixel, the pixel count of the connected component of equal-valued pixels it lies in
    (foreground components under ``True`` pixels, background components under ``False`` pixels)."""
    conn = _check_connectivity(connectivity)
    t, two_d = _as_masks(m, "component_areas")
    out = _run(t, lambda x, o, ws: K.regions_areas(x, conn, out=o, ws=ws), _int32_like(t))
    return out[0] if two_d else out


def _filtered(t, two_d, fn):
    out = _run(t, fn, torch.empty_like(t)).view(torch.bool)
    return out[0] if two_d else out


def remove_small_objects(m, min_size=64, connectivity=1):
    """``skimage.morphology.remove_small_objects`` of a boolean mask -> device ``torch.bool``."""
    size, conn = _check_size(min_size, "min_size"), _check_connectivity(connectivity)
    t, two_d = _as_masks(m, "remove_small_objects")
    return _filtered(t, two_d, lambda x, o, ws: K.regions_filter(x, 1, size, conn, out=o, ws=ws))


def remove_small_holes(m, area_threshold=64, connectivity=1):
    """``skimage.morphology.remove_small_holes`` of a boolean mask -> device ``torch.bool``."""
    size, conn = _check_size(area_threshold, "area_threshold"), _check_connectivity(connectivity)
    t, two_d = _as_masks(m, "remove_small_holes")
    return _filtered(t, two_d, lambda x, o, ws: K.regions_filter(x, 0, size, conn, out=o, ws=ws))


def remove_small_regions(img_bin, min_object_size, hole_area_threshold, connectivity=1, out=None):
    """utils/image_processing.py:14-17 -> device ``torch.bool``.  ``out``: a device ``torch.bool`` tensor of the input's shape to
    write into (it may be ``img_bin`` itself: in place); with it and a device input nothing is allocated but the workspace."""
    mo, ho = _check_size(min_object_size, "min_object_size"), _check_size(hole_area_threshold, "hole_area_threshold")
    conn = _check_connectivity(connectivity)
    if out is not None and not (torch.is_tensor(out) and out.is_cuda and out.dtype == torch.bool and out.is_contiguous()
                                and tuple(out.shape) == tuple(getattr(img_bin, "shape", ()))):
        raise ValueError("remove_small_regions: out must be a contiguous device torch.bool tensor of the input's shape")
    t, two_d = _as_masks(img_bin, "remove_small_regions")
    if out is None:
        return _filtered(t, two_d, lambda x, o, ws: K.regions_remove_small(x, mo, ho, conn, out=o, ws=ws))
    o8 = out.view(torch.uint8)
    _run(t, lambda x, o, ws: K.regions_remove_small(x, mo, ho, conn, out=o, ws=ws), o8.unsqueeze(0) if two_d else o8)
    return out


def threshold(probs, thr):
    """``probs > thr`` as numpy evaluates it for a float32 array and a Python float (``thr`` rounded to float32 first) -> device
    ``torch.bool``, same shape."""
    t = _tensor(probs)
    if not torch.is_tensor(t) or t.dtype != torch.float32:
        raise TypeError(f"threshold expects float32 probabilities, got {getattr(t, 'dtype', type(t))}")
    if not t.is_cuda:
        t = t.to(_device())
    return K.regions_threshold(t.contiguous(), float(thr)).view(torch.bool)


@dataclasses.dataclass
class RegionTable:
    """Per-component measurements of N masks as device tensors; row k of image n is scipy label k + 1 and rows from
    min(count, capacity) on are zero.  ``counts`` int32 [N] is the true component count, also above the capacity; ``area`` int32
    [N, cap]; ``bbox`` int32 [N, cap, 4] = (r0, c0, r1, c1), half-open (the ``find_objects`` slices); ``sum_rc`` int64 [N, cap, 2];
    ``intensity_sum`` int64 [N, cap] and ``intensity_max`` int32 [N, cap], or None without an intensity image."""
    counts: torch.Tensor
    capacity: int
    area: torch.Tensor
    bbox: torch.Tensor
    sum_rc: torch.Tensor
    intensity_sum: typing.Optional[torch.Tensor] = None
    intensity_max: typing.Optional[torch.Tensor] = None

    def centroid(self):
        """float64 [N, cap, 2] = ``scipy.ndimage.center_of_mass`` (sum_rc / area), NaN in unused rows; on the device."""
        return self.sum_rc.to(torch.float64) / self.area.to(torch.float64).unsqueeze(-1)

    def mean_intensity(self):
        """float64 [N, cap] = ``scipy.ndimage.mean`` of the intensity (intensity_sum / area), NaN in unused rows; on the device."""
        if self.intensity_sum is None:
            raise ValueError("mean_intensity: the table was measured without an intensity image")
        return self.intensity_sum.to(torch.float64) / self.area.to(torch.float64)

    def overflowed(self):
        """device bool [N]: the image has more components than the table has rows"""
        return self.counts > self.capacity

    def per_image(self):
        """A host list of N dicts of numpy arrays trimmed to min(count, capacity) rows: ``area``, ``bbox``, ``centroid`` and, with
        an intensity image, ``intensity_sum``, ``intensity_mean``, ``intensity_max``.  The one method that synchronises."""
        cols = {"area": self.area, "bbox": self.bbox, "centroid": self.centroid()}
        if self.intensity_sum is not None:
            cols.update(intensity_sum=self.intensity_sum, intensity_mean=self.mean_intensity(), intensity_max=self.intensity_max)
        cols = {k: v.cpu().numpy() for k, v in cols.items()}
        counts = self.counts.cpu().numpy()
        return [{k: v[n, :min(int(c), self.capacity)] for k, v in cols.items()} for n, c in enumerate(counts)]


def _as_intensity(v, shape):
    """uint8 numpy / torch of the mask's shape -> the tensor (not yet on the device); argument errors only"""
    t = _images(v, "measure", torch.uint8, "uint8, got {}", ranks=None, subject="intensity must be")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"measure: intensity of shape {tuple(t.shape)} for a mask of shape {tuple(shape)}")
    return t


def _tables(N, cap, with_intensity, dev):
    """the five tensors of a ``RegionTable`` with ``cap`` rows per image: area, bbox, sums, isum, imax (the last two None without an
    intensity image)"""
    area = torch.empty((N, cap), dtype=torch.int32, device=dev)
    bbox = torch.empty((N, cap, 4), dtype=torch.int32, device=dev)
    sums = torch.empty((N, cap, 2), dtype=torch.int64, device=dev)
    isum = torch.empty((N, cap), dtype=torch.int64, device=dev) if with_intensity else None
    imax = torch.empty((N, cap), dtype=torch.int32, device=dev) if with_intensity else None
    return area, bbox, sums, isum, imax


def measure(m, intensity=None, connectivity=1, max_regions=None):
    """One row per connected foreground component of every image -> ``RegionTable``.  ``intensity``: uint8 of the mask's shape, or
    None.  ``max_regions=int`` fixes the rows per image (capped at H W; components numbered above it are counted, not measured):
    nothing synchronises and the call can be captured into a graph.  ``max_regions=None`` numbers first, reads the largest count
    back (the one synchronisation) and measures with exactly that capacity (1 when there is no component)."""
    conn = _check_connectivity(connectivity)
    _check_max_regions(max_regions)
    v = None if intensity is None else _as_intensity(intensity, getattr(m, "shape", ()))
    t, two_d = _as_masks(m, "measure")
    N, H, W = t.shape
    if v is not None:
        v = v.to(t.device).contiguous().view(N, H, W)
    chunks = _chunks(t)
    counts = torch.empty((N,), dtype=torch.int32, device=t.device)
    workspace, numbered = _Workspace(lambda n: K.regions_workspace(n, H, W, t.device)), False
    if max_regions is None:
        for a, b in chunks:
            K.regions_number(t[a:b], conn, counts=counts[a:b], ws=workspace(b - a))
        cap = max(1, int(counts.max()))                                  # the one synchronisation
        numbered = len(chunks) == 1                                      # one call: its workspace still holds the numbering
    else:
        cap = min(int(max_regions), H * W)
    area, bbox, sums, isum, imax = _tables(N, cap, v is not None, t.device)
    for a, b in chunks:
        K.regions_measure(t[a:b], cap, None if v is None else v[a:b], conn, numbered, counts[a:b], area[a:b], bbox[a:b], sums[a:b],
                          None if v is None else isum[a:b], None if v is None else imax[a:b], ws=workspace(b - a))
    return RegionTable(counts, cap, area, bbox, sums, isum, imax)


@dataclasses.dataclass
class SplitResult:
    """``split`` of N masks, device tensors: ``labels`` int32 of the mask's shape (0 = background; label k + 1 = seed k of the
    image; labels above ``n_seeds[n]`` = components that hold no live seed); ``counts`` int32 [N] = n_seeds + the number of such
    components, i.e. the rows ``measure_labels`` fills; ``n_seeds`` int32 [N] = the points of image n within its limit; ``live``
    bool [P], one per row of the points buffer: the point is a seed that lies inside its image on a foreground pixel."""
    labels: torch.Tensor
    counts: torch.Tensor
    n_seeds: torch.Tensor
    live: torch.Tensor


def _seeds(points, offsets, limits, N, H, W):
    """the seed arguments of ``split`` -> their PointSet; argument errors only, no device work.  Host points are checked against the
    image, device points cannot be."""
    from ._points import PointSet
    seeds = PointSet(points, offsets, limits, N, "split", per_image=isinstance(points, (list, tuple)) and offsets is None,
                     max_images=N)                                        # any N: split serves the batch in chunks
    pts = seeds.pts
    if seeds.rows + H * W > _MAX_PIXELS:
        raise ValueError(f"split: {seeds.rows} points and {H}x{W} pixels do not leave room for int32 labels")
    if not seeds.on_device and pts.size:
        if int(pts[:, 0].min()) < 0 or int(pts[:, 0].max()) >= H or int(pts[:, 1].min()) < 0 or int(pts[:, 1].max()) >= W:
            raise ValueError(f"split: a point lies outside the {H}x{W} image")
    return seeds


def split(m, points, offsets=None, limits=None, connectivity=1):
    """Split the connected components of boolean masks at seed points -> ``SplitResult``.

    ``m``: bool [H, W] or [N, H, W] with ``H^2 + W^2 < 2^31``.  ``points``: integer (row, col) pairs -- one ``[k, 2]`` array for a
    2-D mask, a list of N per-image arrays, or one concatenated ``[P, 2]`` array with ``offsets`` [N + 1] (image n owns
    ``points[offsets[n]:offsets[n + 1]]``; with device offsets the buffer may be longer than ``offsets[-1]``: this is the layout of
    ``DetectResult.device_points`` / ``device_offsets``).  ``limits``: None, one count or one per image, Python's ``[:c]`` of every
    image's points as in ``score.score_points``: the S' points it keeps are the seeds.

    * Seed k (0-based within its image) is live iff it lies inside the image and on a foreground pixel.  Dead seeds own nothing and
      are reported in ``live``, not raised: device points cannot be checked without a synchronisation.  Host points outside the
      image raise ``ValueError`` before any device work.
    * A foreground pixel (r, c) of a component that holds a live seed gets label ``1 + k``, k minimising ``((r - r_k)^2 +
      (c - c_k)^2, k)`` over the live seeds OF THAT COMPONENT: a nearer seed of another component never wins, ties go to the lower
      index, and of two seeds on one pixel the lower owns everything (the other's cell is empty).
    * The pixels of a component without a live seed get ``S' + 1 + j``, j = the component's rank among the image's seedless
      components in ``label``'s order; the background is 0; ``counts = S' +`` the number of seedless components.

    Without points the labels are ``label(m)`` bit for bit.  All of it is integer work: exact and independent of launch order, a
    fixed number of launches, no synchronisation.  This is a Euclidean partition inside each component, NOT a watershed: a cell of
    a strongly non-convex clump may come out in two pieces (``split_geodesic`` measures the distance inside the component instead
    and leaves every cell connected), and no parity with any watershed implementation is claimed.  Cost: the
    labelling plus (foreground pixels) x (live seeds of their component) distance evaluations."""
    conn, t, two_d, pts, off, lim, n_seeds = _split_args(m, points, offsets, limits, connectivity, "split")
    N, P, dev = t.shape[0], pts.shape[0], t.device
    labels = _int32_like(t)
    counts = torch.empty((N,), dtype=torch.int32, device=dev)
    live = None
    for a, b in _chunks(t):
        # every call looks at the whole points buffer: the points of the other chunks' images come out dead in this one
        part = torch.empty((P,), dtype=torch.uint8, device=dev)
        K.regions_split(t[a:b], pts, off[a:b + 1], None if lim is None else lim[a:b], conn, labels=labels[a:b], counts=counts[a:b], live=part)
        live = part if live is None else live | part
    return SplitResult(labels[0] if two_d else labels, counts, n_seeds, live.view(torch.bool))


def _split_args(m, points, offsets, limits, connectivity, what):
    """the arguments of ``split`` / ``split_geodesic``, argument errors before any device work -> (connectivity, uint8 masks [N,H,W],
    was_2d, points int64 [P,2], offsets int64 [N+1], limits int32 [N] | None, n_seeds int32 [N]), all on the device"""
    from . import detect as D
    conn = _check_connectivity(connectivity)
    shape = tuple(getattr(m, "shape", ()))
    if len(shape) in (2, 3) and min(shape) > 0:
        D._check_dt_shape(shape)                                         # before the mask is copied anywhere
        seeds = _seeds(points, offsets, limits, 1 if len(shape) == 2 else shape[0], shape[-2], shape[-1])
    t, two_d = _as_masks(m, what)
    seeds.upload(t.device)
    pts, off, lim = seeds.pts_dev, seeds.off_dev, seeds.lim_dev
    # S' as the kernel forms it (point_window of csrc/cs_points.h): offsets that do not describe rows of the buffer leave no seeds
    lo, hi = off[:-1], off[1:]
    n_seeds = hi - lo
    n_seeds = n_seeds.masked_fill((lo | n_seeds | (pts.shape[0] - hi)) < 0, 0)     # any of lo, hi - lo, P - hi negative: none
    if lim is not None:
        n_seeds = torch.where(lim >= 0, torch.minimum(lim.to(torch.int64), n_seeds), (n_seeds + lim).clamp(min=0))
    return conn, t, two_d, pts, off, lim, n_seeds.to(torch.int32)


@dataclasses.dataclass
class GeodesicSplitResult(SplitResult):
    """``split_geodesic`` of N masks: a ``SplitResult`` plus ``converged`` bool [N] (device): the labels of image n are the rule's
    (always true in the exact mode), and ``distance``: int32 of the mask's shape, the chamfer cost from every pixel to the seed that
    owns it (0 on the background, -1 in a component without a live seed and on a pixel not reached yet), or None."""
    converged: torch.Tensor
    distance: typing.Optional[torch.Tensor] = None


# The rounds of one batch in the exact mode.  A round after convergence costs one flag read per tile, a read-back costs a drained
# queue and a resumed batch starts with one round over every tile, so a batch should nearly always be the only one.  The tiled
# relaxation needs about one round per tile edge that the longest shortest path crosses, plus the quiet last one: 2 to 4 on clumps
# a tile or two across (tests/geodesic_ref.py's model on the test masks), 6 to 10 on the two mask sets of
# tools/regions_microbench.py, whose components wind through several tiles (measured).  12 covers those in one batch; a
# maze takes more batches.
_GEODESIC_BATCH = 12


def split_geodesic(m, points, offsets=None, limits=None, connectivity=1, max_rounds=None, want_distance=False):
    """``split`` with the distance measured inside the component, so that every cell is connected -> ``GeodesicSplitResult``.

    The arguments, the seeds, ``live``, the components without a live seed, ``counts``, ``n_seeds``, limits, offsets, device points
    and dead seeds are ``split``'s, unchanged.  Only the distance differs:

    * A step goes from a foreground pixel to a foreground pixel of its 8-neighbourhood.  An axial step costs 5, a diagonal step 7
      (the 5-7 chamfer).  With ``connectivity=2`` every such step is allowed; with ``connectivity=1`` a diagonal step from (r, c)
      to (r + dr, c + dc) only if at least one of (r + dr, c) and (r, c + dc) is foreground.  So a step never leaves the component
      of the chosen connectivity, and every pixel of a component that holds a live seed is reached.
    * ``dist(p, k)`` is the cheapest path from the pixel of live seed k to p, and p gets label ``1 + k`` for the k that minimises
      ``(dist(p, k), k)`` over the live seeds of its component.  Of two seeds on one pixel the lower index owns everything.
    * ``7 H W < 2^31`` is required (a path visits a pixel at most once, so every distance fits int32); larger images raise
      ``ValueError`` before any device work.

    Every cell with a live seed is connected in the 8-neighbourhood and contains its seed pixel: for a pixel q on a shortest path
    from p to its owner k, an owner j <= k of q at equal or smaller distance would reach p at most as far as k does.  This is NOT a
    watershed either: the cut between two seeds lies where the geodesic distances are equal, not at the neck of the clump.  Nor is
    it a refinement of ``split``: the chamfer bisector differs slightly from the Euclidean one even in a convex clump.

    The keys (dist, k) are lowered to their fixpoint in rounds of one launch each (csrc/regions.hip).  ``max_rounds=int``: exactly
    that many rounds, a fixed sequence of launches with no synchronisation, capturable into a graph; ``converged[n]`` says whether
    image n reached the fixpoint, and of one that did not only this is promised: every label is 0, a live seed of that pixel's
    component or a seedless number.  ``max_rounds=None`` (the default) is exact: it runs a batch of rounds, reads ``converged``
    back, and resumes until every image has converged, as ``measure(max_regions=None)`` reads its count back.
    ``want_distance``: also return the distance map.  Without points the labels are ``label(m)`` bit for bit.  Integer work only:
    the converged result is exact and independent of launch order."""
    if max_rounds is not None and (isinstance(max_rounds, bool) or int(max_rounds) != max_rounds or max_rounds < 1):
        raise ValueError(f"max_rounds must be a positive integer or None, got {max_rounds!r}")
    shape = tuple(getattr(m, "shape", ()))
    if len(shape) in (2, 3) and 7 * shape[-2] * shape[-1] >= 1 << 31:
        raise ValueError(f"split_geodesic: a {shape[-2]}x{shape[-1]} image does not keep 7 H W below 2^31")
    conn, t, two_d, pts, off, lim, n_seeds = _split_args(m, points, offsets, limits, connectivity, "split_geodesic")
    N, P, dev = t.shape[0], pts.shape[0], t.device
    labels = _int32_like(t)
    distance = _int32_like(t) if want_distance else None
    counts = torch.empty((N,), dtype=torch.int32, device=dev)
    converged = torch.empty((N,), dtype=torch.uint8, device=dev)
    live = None
    for a, b in _chunks(t):
        part = torch.empty((P,), dtype=torch.uint8, device=dev)         # as in split: the other chunks' points come out dead
        args = (t[a:b], pts, off[a:b + 1], None if lim is None else lim[a:b], conn)
        out = dict(labels=labels[a:b], counts=counts[a:b], live=part, distance=None if distance is None else distance[a:b],
                   converged=converged[a:b])
        ws = K.regions_split_geodesic(*args, rounds=_GEODESIC_BATCH if max_rounds is None else int(max_rounds), **out)[-1]
        while max_rounds is None and not bool(converged[a:b].all()):    # the synchronisation of the exact mode
            K.regions_split_geodesic(*args, rounds=_GEODESIC_BATCH, resume=True, ws=ws, **out)
        live = part if live is None else live | part
    return GeodesicSplitResult(labels[0] if two_d else labels, counts, n_seeds, live.view(torch.bool), converged.view(torch.bool),
                               None if distance is None else (distance[0] if two_d else distance))


def _check_max_regions(max_regions):
    if max_regions is not None and (isinstance(max_regions, bool) or int(max_regions) != max_regions or max_regions < 1):
        raise ValueError(f"max_regions must be a positive integer or None, got {max_regions!r}")


def _as_labels(x, what, masks_go_to="label first"):
    """int32 numpy / torch [H, W] or [N, H, W] -> the tensor (not yet on the device); argument errors only.  ``masks_go_to``: where
    the message sends a caller who passed a boolean mask."""
    return _images(x, what, torch.int32, f"an int32 label image, got {{}} (boolean masks go to {masks_go_to})", noun="label image")


class _LabelImage:
    """The front end of one label-image argument of the call ``what``, in two phases so that every argument error of a call can
    come before its first copy.  The check, on the host: ``_as_labels``, then ``check_size(what, shape)`` where given, ``two_d`` =
    the argument was [H, W], ``N``, and in ``with_counts`` the check of the caller's ``counts``.  ``place``: ``labels`` as
    contiguous int32 [N, H, W] on a device, the ``chunks`` of whole images per kernel call, and for a call with counts ``own`` = the
    device has to find them and ``counts`` = the int32 [N] tensor (the caller's where given)."""
    own = counts = None

    def __init__(self, what, x, masks_go_to="label first", check_size=None):
        self.what, self.labels = what, _as_labels(x, what, masks_go_to)
        if check_size is not None:
            check_size(what, tuple(self.labels.shape))
        self.two_d = self.labels.dim() == 2
        self.N = 1 if self.two_d else self.labels.shape[0]

    def with_counts(self, counts, name="counts", what=None):
        """``what``: the call the message names, where it is not this one's"""
        if counts is not None and not (torch.is_tensor(counts) and counts.dtype == torch.int32 and tuple(counts.shape) == (self.N,)):
            raise TypeError(f"{what or self.what}: {name} must be an int32 tensor of shape ({self.N},)")
        self.own, self.counts = counts is None, counts
        return self

    @functools.cached_property
    def chunks(self):
        return _chunks(self.labels)                                      # (of the placed labels)

    def place(self, dev=None):
        """``dev``: None = the labels' own device, for host labels the current one -> (labels, counts)"""
        t = self.labels.unsqueeze(0) if self.two_d else self.labels
        dev = dev or (t.device if t.is_cuda else _device())
        self.labels = (t if t.device == dev else t.to(dev)).contiguous()
        if self.own is not None:
            self.counts = torch.empty((self.N,), dtype=torch.int32, device=dev) if self.own else self.counts.to(dev).contiguous()
        return self.labels, self.counts


def _largest_labels(probe, *sides):
    """The capacities that hold every label of the batch, one per placed ``_LabelImage`` of ``sides`` (1 where a side has no label).
    ``probe``: the caller's run at capacity 1, which leaves the largest labels in the sides' ``counts``; made only if a side's counts
    were not given.  One synchronisation."""
    if any(s.own for s in sides):
        probe()
    top = [s.counts.max() for s in sides]
    top = (top[0] if len(top) == 1 else torch.stack(top)).cpu().reshape(-1)
    return tuple(max(1, int(x)) for x in top)


def measure_labels(labels, intensity=None, max_regions=None, counts=None):
    """``measure`` for a label image: int32 [H, W] or [N, H, W] (numpy or torch; 0 and below = background) -> ``RegionTable`` whose
    row k belongs to label k + 1.  A label that owns no pixel (an empty cell of ``split``) leaves an all-zero row, its bounding box
    (0, 0, 0, 0) included: the row where ``scipy.ndimage.find_objects`` gives ``None``.  ``counts``: int32 [N], the labels in use per
    image (``SplitResult.counts``); None = the largest label of every image, found on the device.  ``max_regions=int`` fixes the
    rows per image (larger labels are counted, not measured): nothing synchronises and the call can be captured into a graph.
    ``max_regions=None`` reads the largest count back (the one synchronisation; without ``counts`` after a pass that finds them)
    and measures with exactly that capacity (1 when there is no label).  Only int32 is taken; boolean masks go to ``measure``."""
    _check_max_regions(max_regions)
    img = _LabelImage("measure_labels", labels, masks_go_to="measure")
    v = None if intensity is None else _as_intensity(intensity, img.labels.shape)
    t, counts = img.with_counts(counts).place()
    N, H, W = t.shape
    dev = t.device
    if v is not None:
        v = v.to(dev).contiguous().view(N, H, W)

    def run(cap, want_counts):
        area, bbox, sums, isum, imax = _tables(N, cap, v is not None, dev)
        for a, b in img.chunks:
            K.regions_measure_labels(t[a:b], cap, None if v is None else v[a:b], counts[a:b] if want_counts else None, area[a:b], bbox[a:b],
                                     sums[a:b], None if v is None else isum[a:b], None if v is None else imax[a:b], want_counts=want_counts)
        return RegionTable(counts, cap, area, bbox, sums, isum, imax)

    if max_regions is not None:
        return run(int(max_regions), img.own)
    return run(*_largest_labels(lambda: run(1, True), img), False)      # (the pass that finds the largest labels; one synchronisation)


def _host_tables(table, names):
    """the named device tables of a result as int64 numpy arrays: copied once, then kept in the result's ``_host``"""
    if table._host is None:
        table._host = tuple(getattr(table, k).cpu().numpy().astype(np.int64) for k in names)
    return table._host


def _grow_pairs(run, start, most):
    """``run(pairs)`` -> a table, from ``min(start, most)`` pairs on and with twice as many (at most ``most``) for as long as the
    table's ``dropped.max()``, read back after every run (a synchronisation per turn), is non-zero: with a ``most`` that holds every
    pair the table returned has lost none."""
    pairs = min(start, most)
    while True:
        table = run(pairs)
        if int(table.dropped.max()) == 0 or pairs >= most:
            return table
        pairs = min(2 * pairs, most)


def _gather_slots(calls, names):
    """the results of the chunks' kernel calls -> name: the raw pair table's [N, slots] array of that name for the batch; one chunk:
    the call's own views, which go on viewing its workspace"""
    return {k: calls[0][k] if len(calls) == 1 else torch.cat([r[k] for r in calls]) for k in names}


def _read_pairs(slot_keys, *columns):
    """A raw pair table (``slot_keys`` int64 [N, slots], 0 = empty, and int32 count ``columns`` of that shape) -> the int64 host
    arrays ``(image, hi, lo, *columns)`` of the occupied slots, sorted by (image, hi, lo).  One copy from the device."""
    flat = torch.cat([slot_keys.reshape(-1), *(c.reshape(-1).to(torch.int64) for c in columns)]).cpu().numpy()
    keys, *columns = flat.reshape(1 + len(columns), -1)
    at = np.nonzero(keys)[0]
    image, keys = at // slot_keys.shape[1], keys[at]
    order = np.lexsort((keys, image))                                    # a key orders by its high, then its low label
    return (image[order], keys[order] >> 32, keys[order] & 0xFFFFFFFF, *(c[at][order] for c in columns))


@dataclasses.dataclass
class MatchTable:
    """``match_labels`` of N image pairs as device tensors.  ``counts_pred`` / ``counts_truth`` int32 [N]: the largest label of
    every image, also above the capacity; ``area_pred`` int32 [N, cap_pred] and ``area_truth`` int32 [N, cap_truth]: the pixel
    count of label k + 1 in row k (0 = the label owns nothing: no object); ``match`` int32 [N, cap_pred]: the truth label matched,
    0 = none; ``inter`` int32 [N, cap_pred]: the pixels shared with it, 0 where unmatched; ``match_truth`` int32 [N, cap_truth]:
    the inverse, the pred label or 0."""
    counts_pred: torch.Tensor
    counts_truth: torch.Tensor
    cap_pred: int
    cap_truth: int
    area_pred: torch.Tensor
    area_truth: torch.Tensor
    match: torch.Tensor
    inter: torch.Tensor
    match_truth: torch.Tensor
    _host: typing.Optional[tuple] = dataclasses.field(default=None, repr=False, compare=False)

    def overflowed(self):
        """device bool [N]: a side of the image has labels above its capacity (they were taken for background)"""
        return (self.counts_pred > self.cap_pred) | (self.counts_truth > self.cap_truth)

    def iou(self):
        """float64 [N, cap_pred] = inter / (area_pred + area_truth[match] - inter) where matched, 0 elsewhere; on the device."""
        matched = self.match > 0
        at = torch.gather(self.area_truth, 1, (self.match - 1).clamp(min=0).to(torch.int64))
        union = self.area_pred.to(torch.int64) + at - self.inter
        q = self.inter.to(torch.float64) / union.clamp(min=1).to(torch.float64)
        return torch.where(matched, q, torch.zeros_like(q))

    def score(self, iou_threshold=0.5):
        """TP / FP / FN, precision, recall, F1, SQ and PQ per image -> ``score.LabelScore`` (``score.label_score`` has the
        formulas).  The one method that synchronises: the integer tables are copied to the host once and kept, so a sweep over
        thresholds costs no further transfer.  ``iou_threshold``: a float in [0.5, 1]."""
        from . import score as S
        S.check_iou_threshold(iou_threshold)                              # before any transfer
        return S.label_score(*_host_tables(self, ("area_pred", "area_truth", "match", "inter")), iou_threshold=iou_threshold)


def _match_capacities(max_regions):
    """None, one capacity or a (pred, truth) pair -> None or the pair"""
    if max_regions is None:
        return None
    pair = tuple(max_regions) if isinstance(max_regions, (tuple, list)) else (max_regions, max_regions)
    if len(pair) != 2:
        raise ValueError(f"max_regions must be a positive integer, a (pred, truth) pair of them or None, got {max_regions!r}")
    for c in pair:
        _check_max_regions(c)
        if c is None:
            raise ValueError(f"max_regions must be a positive integer, a (pred, truth) pair of them or None, got {max_regions!r}")
    return int(pair[0]), int(pair[1])


class _LabelPair:
    """The front end that ``match_labels``, ``overlap_labels`` and ``hausdorff_labels`` share, two ``_LabelImage`` (``sides``) that
    agree in shape: argument errors first, then ``pred`` / ``truth`` as int32 [N, H, W] on one device (pred's if it is on one, else
    truth's, else the current one), the ``chunks`` of whole images per kernel call, ``own`` = which side's counts the device has to
    find, and ``counts`` = the two int32 [N] tensors (the caller's where given)."""

    def __init__(self, what, pred, truth, pred_counts, truth_counts):
        self.sides = p, t = _LabelImage(what, pred), _LabelImage(what, truth)
        if tuple(p.labels.shape) != tuple(t.labels.shape):
            raise ValueError(f"{what}: pred of shape {tuple(p.labels.shape)} against truth of shape {tuple(t.labels.shape)}")
        p.with_counts(pred_counts, "pred_counts"), t.with_counts(truth_counts, "truth_counts")
        dev = p.labels.device if p.labels.is_cuda else t.labels.device if t.labels.is_cuda else _device()
        (self.pred, _), (self.truth, _) = p.place(dev), t.place(dev)
        self.N, self.dev, self.chunks = p.N, dev, p.chunks
        self.own, self.counts = (p.own, t.own), (p.counts, t.counts)

    def calls(self, want):
        """per chunk: (slice of the images, pred, truth, counts_pred | None, counts_truth | None) as a kernel call takes them"""
        for a, b in self.chunks:
            yield slice(a, b), self.pred[a:b], self.truth[a:b], *(c[a:b] if w else None for c, w in zip(self.counts, want))


def match_labels(pred, truth, max_regions=None, pred_counts=None, truth_counts=None):
    """Match the objects of two label images by intersection over union -> ``MatchTable``.

    ``pred``, ``truth``: int32 [H, W] or [N, H, W] of one shape (numpy or torch; 0 and below = background), e.g. ``split(...).labels``
    against ``label(truth_mask)``.  Per image, with Ap[p] / At[g] the pixel counts of pred label p / truth label g, I(p, g) the
    pixels that carry both and U = Ap[p] + At[g] - I:

    * p and g are matched iff ``2 I(p, g) > U``, strictly, in 64-bit integers: IoU > 1/2, the panoptic-quality condition.  Then a
      label has at most one partner on the other side: there is no assignment problem and no float decides a match.  IoU exactly
      1/2 is NO match -- the one difference from matchers that test ``>=``.
    * An object is a label that owns at least one pixel.  A label without pixels (a dead or duplicate seed of ``split``) is no
      object: never a false positive or a false negative.
    * A pixel whose label exceeds its side's capacity is background on that side; the largest labels are still reported in
      ``counts_pred`` / ``counts_truth`` and ``overflowed()`` flags the image.

    ``max_regions``: an int or a ``(pred, truth)`` pair fixes the capacities: a fixed number of launches, no synchronisation, the
    call can be captured into a graph.  None finds the largest labels on the device, reads them back once (the one synchronisation)
    and uses exactly those capacities (1 where there is no label).  ``pred_counts`` / ``truth_counts``: int32 [N], the labels in use
    per image where the caller has them (``SplitResult.counts``); None = found on the device.  Everything the device writes is
    integer and independent of launch order.  Memory: 4 N cap_pred (bit_length(cap_truth) + 1) bytes of workspace besides the
    tables -- never a cap_pred x cap_truth table."""
    caps = _match_capacities(max_regions)
    pair = _LabelPair("match_labels", pred, truth, pred_counts, truth_counts)

    def run(cap_p, cap_t, want):
        tabs = [torch.empty((pair.N, c), dtype=torch.int32, device=pair.dev) for c in (cap_p, cap_t, cap_p, cap_p, cap_t)]
        workspace = _Workspace(lambda n: K.regions_match_workspace(n, cap_p, cap_t, pair.dev))
        for at, p, t, cp, ct in pair.calls(want):
            K.regions_match_labels(p, t, cap_p, cap_t, cp, ct, *(x[at] for x in tabs), want_counts=want, ws=workspace(len(p)))
        return MatchTable(*pair.counts, cap_p, cap_t, *tabs)

    if caps is not None:
        return run(*caps, pair.own)
    return run(*_largest_labels(lambda: run(1, 1, pair.own), *pair.sides), (False, False))


_OVERLAP_HOST = ("area_pred", "area_truth", "iou_partner", "iou_inter", "inter_partner_truth", "inter_truth", "inter_partner_pred",
                 "inter_pred", "n_pairs")


@dataclasses.dataclass
class OverlapTable:
    """``overlap_labels`` of N image pairs as device tensors, all int32 but the keys.  ``counts_pred`` / ``counts_truth`` [N], the
    capacities and ``area_pred`` [N, cap_pred] / ``area_truth`` [N, cap_truth] as in ``MatchTable``.  ``n_pairs`` [N]: the (pred,
    truth) pairs that share a pixel; ``dropped`` [N]: the runs of pixels whose pair found no room (0 unless ``max_pairs`` was too
    small).  Row g - 1 of ``iou_partner`` / ``iou_inter`` [N, cap_truth]: the pred label of largest IoU with truth label g (0 =
    none) and the pixels shared with it; of ``inter_partner_truth`` / ``inter_truth``: the pred label of largest intersection and
    that intersection.  Row p - 1 of ``inter_partner_pred`` / ``inter_pred`` [N, cap_pred]: the same for pred label p over the
    truth labels.  ``slot_keys`` int64 [N, slots] and ``slot_counts`` [N, slots]: the raw pair table, key = (pred << 32) | truth,
    0 = empty, in no particular order -- ``pairs()`` reads it."""
    counts_pred: torch.Tensor
    counts_truth: torch.Tensor
    cap_pred: int
    cap_truth: int
    area_pred: torch.Tensor
    area_truth: torch.Tensor
    n_pairs: torch.Tensor
    dropped: torch.Tensor
    iou_partner: torch.Tensor
    iou_inter: torch.Tensor
    inter_partner_truth: torch.Tensor
    inter_truth: torch.Tensor
    inter_partner_pred: torch.Tensor
    inter_pred: torch.Tensor
    slot_keys: torch.Tensor
    slot_counts: torch.Tensor
    _host: typing.Optional[tuple] = dataclasses.field(default=None, repr=False, compare=False)

    def overflowed(self):
        """device bool [N]: a side of the image has labels above its capacity (they were taken for background), or pairs of it
        found no room in the table (they are missing from the pair list and from the partners)"""
        return (self.counts_pred > self.cap_pred) | (self.counts_truth > self.cap_truth) | (self.dropped > 0)

    def pairs(self):
        """The sparse contingency table on the host: int64 arrays ``(image, pred, truth, inter)``, one entry per pair that shares a
        pixel, sorted by (image, pred, truth).  One copy from the device (it synchronises)."""
        return _read_pairs(self.slot_keys, self.slot_counts)

    def score(self):
        """AJI and object-level Dice per image -> ``score.OverlapScore`` (``score.overlap_score`` has the formulas).  It
        synchronises: the integer tables are copied to the host once and kept."""
        from . import score as S
        return S.overlap_score(*_host_tables(self, _OVERLAP_HOST))


def _check_max_pairs(max_pairs):
    if max_pairs is not None and (isinstance(max_pairs, bool) or int(max_pairs) != max_pairs or not 1 <= max_pairs <= 1 << 29):
        raise ValueError(f"max_pairs must be an integer in [1, 2^29] or None, got {max_pairs!r}")


def overlap_labels(pred, truth, max_regions=None, max_pairs=None, pred_counts=None, truth_counts=None):
    """Every overlapping pair of objects of two label images, and each object's best partner -> ``OverlapTable``: what the scores
    that look below IoU 1/2 need (``OverlapTable.score``: AJI and object-level Dice; ``OverlapTable.pairs``: the sparse contingency
    table, for any other).

    ``pred``, ``truth``, ``max_regions``, ``pred_counts`` / ``truth_counts`` and the treatment of labels (0 and below, and labels
    above their side's capacity, are background) are those of ``match_labels``.  Per image, with Ap / At the areas and I(p, g) the
    pixels that carry both labels:

    * the best-IoU partner of truth label g is the pred label p with I > 0 that maximises ``I / (Ap + At - I)``, fractions compared
      by cross-multiplication in 64-bit integers, ties to the lower p;
    * the best-intersection partner of a label of either side is the label of the other side of largest I, ties to the lower.

    The pairs are collected in a per-image hash table of ``slots`` = the smallest power of two >= 2 ``max_pairs`` entries.
    ``max_pairs=int`` (with ``max_regions`` given) fixes it: four launches, no synchronisation, the call can be captured into a
    graph; pairs that find no room are counted in ``dropped`` and ``overflowed()`` flags the image.  ``max_pairs=None`` starts from
    4 (cap_pred + cap_truth) (at most H W), reads ``dropped.max()`` back and doubles while it is non-zero -- it ends because an image has at most
    H W pairs -- so the table returned has lost no pair.  Everything the device writes is integer and independent of launch and
    arrival order, except the position of a pair in the raw table.  Memory besides the tables: 12 N slots + 8 N (2 cap_truth +
    cap_pred) bytes of workspace, whose first 12 N slots bytes the result keeps -- never a cap_pred x cap_truth table."""
    caps = _match_capacities(max_regions)
    _check_max_pairs(max_pairs)
    pair = _LabelPair("overlap_labels", pred, truth, pred_counts, truth_counts)
    N, dev = pair.N, pair.dev

    def run(cap_p, cap_t, pairs, want):
        tabs = {k: torch.empty((N, (cap_p, cap_t)[side]), dtype=torch.int32, device=dev) for k, side in K._OVERLAP_TABLES}
        tabs.update(n_pairs=torch.empty((N,), dtype=torch.int32, device=dev), dropped=torch.empty((N,), dtype=torch.int32, device=dev))
        # (a workspace per call: the result views its pair table)
        calls = [K.regions_overlap_labels(p, t, cap_p, cap_t, pairs, cp, ct, **{k: x[at] for k, x in tabs.items()}, want_counts=want)
                 for at, p, t, cp, ct in pair.calls(want)]
        return OverlapTable(*pair.counts, cap_p, cap_t, **tabs, **_gather_slots(calls, ("slot_keys", "slot_counts")))

    want = pair.own
    if caps is None:
        caps, want = _largest_labels(lambda: run(1, 1, 1, pair.own), *pair.sides), (False, False)
    if max_pairs is not None:
        return run(caps[0], caps[1], int(max_pairs), want)
    most = pair.pred.shape[1] * pair.pred.shape[2]                       # an image has no more pairs than pixels
    return _grow_pairs(lambda pairs: run(caps[0], caps[1], pairs, want), 4 * (caps[0] + caps[1]), most)


@dataclasses.dataclass
class AdjacencyTable:
    """``adjacency_labels`` of N label images as device tensors, all int32 but the keys.  ``counts`` [N]: the largest label of every
    image, also above ``capacity``; ``connectivity``: 1 or 2, as asked for.  ``n_pairs`` [N]: the listed pairs; ``dropped`` [N]: the
    runs of sides or corners whose pair found no room (0 unless ``max_pairs`` was too small).  Row a - 1 of the [N, capacity] tables
    belongs to label a: ``n_neighbors``, ``contact``, ``background``, ``outside``, ``partner``, ``partner_sides``
    (``adjacency_labels`` has the rules).  ``slot_keys`` int64 [N, slots], ``slot_sides`` and ``slot_corners`` [N, slots]: the raw
    pair table, key = (a << 32) | b with a < b, 0 = empty, in no particular order -- ``pairs()`` and ``edge_index()`` read it."""
    counts: torch.Tensor
    capacity: int
    connectivity: int
    n_pairs: torch.Tensor
    dropped: torch.Tensor
    n_neighbors: torch.Tensor
    contact: torch.Tensor
    background: torch.Tensor
    outside: torch.Tensor
    partner: torch.Tensor
    partner_sides: torch.Tensor
    slot_keys: torch.Tensor
    slot_sides: torch.Tensor
    slot_corners: torch.Tensor

    def overflowed(self):
        """device bool [N]: the image has labels above the capacity (they were taken for background), or pairs of it found no room
        in the table (they are missing from the pair list, and n_neighbors / contact / partner are incomplete)"""
        return (self.counts > self.capacity) | (self.dropped > 0)

    def boundary(self):
        """int32 [N, capacity] on the device: ``contact + background + outside``, the crack length of every label
        (``ContourTable``'s ``cracks_all``)"""
        return self.contact + self.background + self.outside

    def touching_fraction(self):
        """float64 [N, capacity] on the device: ``contact / boundary()``, the share of a cell's outline that it has in common with
        other cells (CellProfiler's PercentTouching as a fraction); NaN where the boundary is 0 (a label without pixels)."""
        b = self.boundary().to(torch.float64)
        return torch.where(b > 0, self.contact.to(torch.float64) / b.clamp(min=1), torch.full_like(b, float("nan")))

    def pairs(self):
        """The listed pairs on the host: int64 arrays ``(image, a, b, sides, corners)`` with a < b, sorted by (image, a, b).  One
        copy from the device (it synchronises)."""
        return _read_pairs(self.slot_keys, self.slot_sides, self.slot_corners)

    def edge_index(self):
        """The cell graph in COO form, on the device: ``(edge_index, image, sides, corners)``, int64 [2, E] = the 0-based rows
        (a - 1, b - 1) of every listed pair, and int64 [E] each, in the order of ``pairs()``.  Made with torch ops whose output size
        depends on the data: it may synchronise and cannot be captured into a graph."""
        keys = self.slot_keys.reshape(-1)
        at = torch.nonzero(keys).reshape(-1)
        keys, image = keys[at], at // self.slot_keys.shape[1]
        order = torch.sort(keys, stable=True).indices
        order = order[torch.sort(image[order], stable=True).indices]
        keys, at = keys[order], at[order]
        edges = torch.stack([(keys >> 32) - 1, (keys & 0xFFFFFFFF) - 1])
        return (edges, image[order], self.slot_sides.reshape(-1)[at].to(torch.int64), self.slot_corners.reshape(-1)[at].to(torch.int64))

    def per_image(self):
        """A host list of N dicts of numpy arrays: the six label tables and ``boundary`` trimmed to min(count, capacity) rows, and
        ``pairs`` = int64 [n_pairs, 4] rows (a, b, sides, corners) sorted by (a, b).  It synchronises."""
        cols = {k: getattr(self, k) for k in ("n_neighbors", "contact", "background", "outside", "partner", "partner_sides")}
        cols["boundary"] = self.boundary()
        cols = {k: v.cpu().numpy() for k, v in cols.items()}
        counts = self.counts.cpu().numpy()
        image, *rest = self.pairs()
        listed = np.stack(rest, axis=1) if len(image) else np.zeros((0, 4), np.int64)
        out = []
        for n, c in enumerate(counts):
            d = {k: v[n, :min(int(c), self.capacity)] for k, v in cols.items()}
            d["pairs"] = listed[image == n]
            out.append(d)
        return out


def adjacency_labels(labels, connectivity=1, distance=None, radius_sq=None, max_regions=None, max_pairs=None, counts=None):
    """Which cells of a label image touch which, and what every cell's outline faces -> ``AdjacencyTable``: neighbour counts and
    the share of the outline in contact with other cells (CellProfiler's MeasureObjectNeighbors: NumberOfNeighbors,
    PercentTouching), and the list of touching pairs, i.e. the cell graph.

    ``labels``: int32 [H, W] or [N, H, W] (numpy or torch), independent images, e.g. ``split(...).labels``.  All rules are exact
    integers, per image:

    * A pixel's id is its label when ``1 <= label <= capacity``, else 0: a label above the capacity is background here, as in
      ``overlap_labels``; the largest label is still reported in ``counts`` and ``overflowed()`` flags the image.
    * Every unordered pair of 4-adjacent pixels of the image is one *interior side*; a pixel side that lies on the image edge is an
      *exterior side* of that pixel.
    * Per pair of labels a < b, both positive: ``sides(a, b)`` is the number of interior sides whose two ids are {a, b}.
      ``corners(a, b)`` is counted with ``connectivity=2`` only (0 otherwise): the number of unordered diagonal pixel pairs
      {(r, c), (r + 1, c + 1)} and {(r, c + 1), (r + 1, c)} whose ids are {a, b}, whether or not the two labels also share a side.
      A pair is *listed* iff ``sides > 0`` (connectivity 1) or ``sides + corners > 0`` (connectivity 2).
    * Per label a (row a - 1 of the int32 [N, capacity] tables): ``n_neighbors`` = the listed pairs that contain a; ``contact`` = the
      sum of ``sides`` over them; ``background`` = the interior sides with ids {a, 0}; ``outside`` = the exterior sides of a's pixels;
      ``partner`` / ``partner_sides`` = the listed neighbour of largest ``sides``, ties going to the lower label, and that count (a
      neighbour met at corners only has 0 sides); ``partner`` is 0 without a neighbour.  A label without pixels has an all-zero row.
    * ``contact + background + outside = 4 area - 2 (interior sides with both ids a)``: ``boundary()``, which is ``cracks_all`` of
      ``contour_labels`` for the same label.

    By hand::

        1 1 2      sides   (1,2)=1 (1,3)=2 (2,3)=2          background  [1, 0, 1]    n_neighbors [2, 2, 2]
        1 3 2      corners (1,2)=1 (1,3)=2 (2,3)=2 (conn 2) outside     [4, 3, 3]    partner     [3, 3, 1]
        0 3 3                                               contact     [3, 3, 4]    (label 3: a tie at 2 sides, the lower label)

    ``distance=`` / ``radius_sq=`` (one of them, as ``morph.expand_labels`` takes them): the label image goes through
    ``morph.expand_labels`` first, so that two cells whose gap the expansion closes touch -- CellProfiler's neighbours within a
    distance.  ``background``, ``outside`` and the identity then refer to the EXPANDED image, not to the cells as given.

    The pairs are collected as ``overlap_labels`` collects them, in a per-image hash table of ``slots`` = the smallest power of two
    >= 2 ``max_pairs`` entries.  With ``max_regions`` and ``max_pairs`` both integers the call is four launches that depend on shape
    and capacities alone (after those of the expansion, which are fixed by the shape too): nothing synchronises and the call can be
    captured into a graph; pairs that find no room are counted in ``dropped``.  ``max_pairs=None`` starts from min(4 capacity,
    4 H W), reads ``dropped.max()`` back and doubles while it is non-zero (an image has fewer than 4 H W pairs), so the table returned
    has lost no pair.  ``max_regions=None`` finds the largest label first and reads it back (the one synchronisation); ``counts``:
    int32 [N], the labels in use per image where the caller has them (``SplitResult.counts``).  Everything the device writes is
    integer and independent of launch and arrival order, except the position of a pair in the raw table.  Memory besides the
    tables: 16 N slots + 8 N capacity bytes of workspace, whose first 16 N slots bytes the result keeps."""
    conn = _check_connectivity(connectivity)
    _check_max_regions(max_regions)
    _check_max_pairs(max_pairs)
    r2 = None
    if distance is not None or radius_sq is not None:
        from . import morph as M
        r2 = M._r2("adjacency_labels", distance, radius_sq, name="distance")
    img = _LabelImage("adjacency_labels", labels).with_counts(counts)
    if r2 is not None:
        img.labels = M.expand_labels(img.labels, radius_sq=r2)
    t, counts = img.place()
    N, H, W = t.shape
    dev = t.device

    def run(cap, pairs, want):
        tabs = {k: torch.empty((N, cap), dtype=torch.int32, device=dev) for k in K._ADJACENCY_TABLES}
        tabs.update(n_pairs=torch.empty((N,), dtype=torch.int32, device=dev), dropped=torch.empty((N,), dtype=torch.int32, device=dev))
        # (a workspace per call: the result views its pair table)
        calls = [K.regions_adjacency_labels(t[a:b], cap, pairs, conn, counts[a:b] if want else None,
                                            **{k: x[a:b] for k, x in tabs.items()}, want_counts=want) for a, b in img.chunks]
        return AdjacencyTable(counts, cap, conn, **tabs, **_gather_slots(calls, ("slot_keys", "slot_sides", "slot_corners")))

    if max_regions is not None:
        cap, want = int(max_regions), img.own
    else:
        (cap,), want = _largest_labels(lambda: run(1, 1, True), img), False      # (the pass that finds the largest labels)
    if max_pairs is not None:
        return run(cap, int(max_pairs), want)
    most = min(4 * H * W, 1 << 29)                                       # an image has fewer pairs than sides and diagonals
    return _grow_pairs(lambda pairs: run(cap, pairs, want), 4 * cap, most)


def adjacency(m, connectivity=1, distance=None, radius_sq=None, max_regions=None, max_pairs=None):
    """``adjacency_labels`` for a boolean mask: ``label(m, connectivity)`` first, then the above with the same ``connectivity``.
    The components of a mask never touch each other, so this is of use with ``distance=`` / ``radius_sq=``: components closer than
    twice that distance become neighbours."""
    conn = _check_connectivity(connectivity)
    _check_max_regions(max_regions)
    _check_max_pairs(max_pairs)
    if distance is not None or radius_sq is not None:
        from . import morph as M
        M._r2("adjacency", distance, radius_sq, name="distance")
    return adjacency_labels(label(m, conn), conn, distance, radius_sq, max_regions, max_pairs)


_HAUSDORFF_HOST = ("area_pred", "area_truth", "d2_truth", "d2_pred")


@dataclasses.dataclass
class HausdorffTable:
    """``hausdorff_labels`` of N image pairs as device int32 tensors.  ``counts_pred`` / ``counts_truth`` [N], the capacities and
    ``area_pred`` [N, cap_pred] / ``area_truth`` [N, cap_truth] are those of the ``OverlapTable`` it was made from, ``dropped`` [N]
    too.  Row g - 1 of ``partner_truth`` / ``d2_truth`` [N, cap_truth]: the pred label that truth label g is held against and the
    squared Hausdorff distance H2 between the two; row p - 1 of ``partner_pred`` / ``d2_pred`` [N, cap_pred]: the same for pred label
    p over the truth labels.  ``partner = 0`` and ``d2 = -1`` where the row is no object or the other side has none."""
    counts_pred: torch.Tensor
    counts_truth: torch.Tensor
    cap_pred: int
    cap_truth: int
    area_pred: torch.Tensor
    area_truth: torch.Tensor
    dropped: torch.Tensor
    partner_truth: torch.Tensor
    d2_truth: torch.Tensor
    partner_pred: torch.Tensor
    d2_pred: torch.Tensor
    _host: typing.Optional[tuple] = dataclasses.field(default=None, repr=False, compare=False)

    def overflowed(self):
        """device bool [N]: as ``OverlapTable.overflowed`` -- a side of the image has labels above its capacity (they were taken
        for background), or pairs of it found no room in the overlap table (an object may then have missed its partner)"""
        return (self.counts_pred > self.cap_pred) | (self.counts_truth > self.cap_truth) | (self.dropped > 0)

    def score(self):
        """Object-level Hausdorff distance per image -> ``score.HausdorffScore`` (``score.hausdorff_score`` has the formulas).  It
        synchronises: the integer tables are copied to the host once and kept."""
        from . import score as S
        return S.hausdorff_score(*_host_tables(self, _HAUSDORFF_HOST))


def _check_hausdorff_shape(shape):
    """squared distances are int32: (H - 1)^2 + (W - 1)^2 has to fit"""
    H, W = int(shape[-2]), int(shape[-1])
    if (H - 1) ** 2 + (W - 1) ** 2 > (1 << 31) - 1:
        raise ValueError(f"hausdorff_labels: squared distances in a {H}x{W} image do not fit int32: need (H - 1)^2 + (W - 1)^2 < 2^31")


def hausdorff_labels(pred, truth, overlap=None, max_regions=None, max_pairs=None, pred_counts=None, truth_counts=None):
    """The squared Hausdorff distance of every object of two label images to its partner on the other side -> ``HausdorffTable``:
    what the object-level Hausdorff distance of the GlaS challenge needs (``HausdorffTable.score``).

    ``pred``, ``truth``, ``max_regions``, ``max_pairs``, ``pred_counts`` / ``truth_counts``, the objects (labels that own a pixel)
    and the background (0 and below, and labels above their side's capacity) are those of ``overlap_labels``.  ``overlap``: the
    ``OverlapTable`` of the same pair where the caller has it (``max_regions``, if given as well, has to agree with it); None runs
    ``overlap_labels`` with the arguments given here.  Per image, for pixel sets A and B:

    * ``d2(A -> B)`` = the maximum over ALL pixels a of A -- not its boundary: the farthest pixel may lie inside -- of the minimum
      over the pixels b of B of ``dr^2 + dc^2``, and ``H2(A, B) = max(d2(A -> B), d2(B -> A))``, exact integers.
    * The partner of an object is its best-intersection partner of ``overlap_labels`` (``inter_partner_truth`` /
      ``inter_partner_pred``, ties to the lower label) where it has one.  An object that overlaps nothing takes the object of the
      other side of smallest H2, ties to the lower label (the rule of the GlaS evaluation); 0 when the other side has no object.

    Needs ``(H - 1)^2 + (W - 1)^2 < 2^31`` (``ValueError`` before any launch).  With ``max_regions`` and ``max_pairs`` (or an
    ``OverlapTable``) given, six launches whose grids depend on the shape and the capacities alone follow the overlap's, nothing
    synchronises and the call can be captured into a graph; everything written is integer and independent of launch and arrival
    order.  Cost: one workgroup per (object, partner) computes both directions, each about ``|bounding box of A| runs(B)``
    distance evaluations, runs(B) = the horizontal runs of B's pixels, staged in LDS a fixed number at a time
    (``kernels.regions_hausdorff_stage_runs()``; an object with more is handled in chunks); an object that overlaps nothing costs
    one bounding-box test per object of the other side and one such job per object that the boxes do not rule out (at worst every
    one of them).  Measured once, on synthetic blobs: DESIGN.md.  Memory besides the tables: 32 bytes per label of either side --
    never a cap_pred x cap_truth table."""
    caps = _match_capacities(max_regions)
    _check_max_pairs(max_pairs)
    if overlap is not None:
        if not isinstance(overlap, OverlapTable):
            raise TypeError(f"hausdorff_labels: overlap must be an OverlapTable or None, got {type(overlap).__name__}")
        if caps is not None and caps != (overlap.cap_pred, overlap.cap_truth):
            raise ValueError(f"hausdorff_labels: max_regions {caps} against an OverlapTable of capacities "
                             f"{(overlap.cap_pred, overlap.cap_truth)}")
    for x in (pred, truth):
        if len(getattr(x, "shape", ())) in (2, 3):
            _check_hausdorff_shape(x.shape)                              # before anything is copied anywhere
    pair = _LabelPair("hausdorff_labels", pred, truth, pred_counts, truth_counts)
    N, dev = pair.N, pair.dev
    if overlap is None:
        overlap = overlap_labels(pair.pred, pair.truth, max_regions=max_regions, max_pairs=max_pairs,
                                 pred_counts=None if pair.own[0] else pair.counts[0], truth_counts=None if pair.own[1] else pair.counts[1])
    elif overlap.area_pred.shape[0] != N or overlap.area_pred.device != dev:
        raise ValueError(f"hausdorff_labels: an OverlapTable of {overlap.area_pred.shape[0]} images on {overlap.area_pred.device} for "
                         f"{N} images on {dev}")
    cap_p, cap_t = overlap.cap_pred, overlap.cap_truth
    tabs = {k: torch.empty((N, cap), dtype=torch.int32, device=dev)
            for k, cap in (("partner_truth", cap_t), ("d2_truth", cap_t), ("partner_pred", cap_p), ("d2_pred", cap_p))}
    workspace = _Workspace(lambda n: K.regions_hausdorff_workspace(n, cap_p, cap_t, dev))
    for at, p, t, _, _ in pair.calls((False, False)):
        K.regions_hausdorff_labels(p, t, cap_p, cap_t, overlap.inter_partner_truth[at], overlap.inter_partner_pred[at],
                                   **{k: x[at] for k, x in tabs.items()}, ws=workspace(len(p)))
    return HausdorffTable(overlap.counts_pred, overlap.counts_truth, cap_p, cap_t, overlap.area_pred, overlap.area_truth, overlap.dropped,
                          **tabs)


_SQRT2 = 2.0 ** 0.5
_SHAPE_COLUMNS = ("central_moments", "axis_lengths", "eccentricity", "orientation", "perimeter", "equivalent_diameter", "extent",
                  "circularity")


@dataclasses.dataclass
class ShapeTable:
    """``shape_labels`` of N label images as device tensors.  ``table``: the ``RegionTable`` of the same images (row k = label
    k + 1); ``moments`` int64 [N, cap, 3] = (Sxx, Syy, Sxy) about the corner (r0, c0) of the row's bounding box; ``tallies`` int32
    [N, cap, 4] = (edge pixels, straight, diagonal, mixed); ``edges`` bool of the label image's shape, the inner boundary of every
    object.  The rules are in ``shape_labels``' docstring.  Every method but ``per_image`` runs on the device in float64, is
    computed from the integer tables only and gives NaN in unused rows, as ``RegionTable.centroid`` does."""
    table: RegionTable
    moments: torch.Tensor
    tallies: torch.Tensor
    edges: torch.Tensor

    def _area(self):
        return self.table.area.to(torch.float64)

    def central_moments(self):
        """float64 [N, cap, 3] = (mu20, mu02, mu11) = (Sxx / A - (Sx / A)^2, Syy / A - (Sy / A)^2, Sxy / A - Sx Sy / A^2) with x
        along the rows and y along the columns, Sx = sum_rc[0] - A r0 and Sy = sum_rc[1] - A c0 formed in int64."""
        t = self.table
        a64 = t.area.to(torch.int64).unsqueeze(-1)
        s = (t.sum_rc - a64 * t.bbox[..., :2].to(torch.int64)).to(torch.float64)
        a = self._area()
        mx, my = s[..., 0] / a, s[..., 1] / a
        m = self.moments.to(torch.float64)
        return torch.stack([m[..., 0] / a - mx * mx, m[..., 1] / a - my * my, m[..., 2] / a - mx * my], dim=-1)

    def _eigen(self):
        """(lambda1, lambda2 clamped at 0) of the matrix of central moments"""
        mu = self.central_moments()
        mean, half = (mu[..., 0] + mu[..., 1]) / 2, (mu[..., 0] - mu[..., 1]) / 2
        root = torch.sqrt(half * half + mu[..., 2] * mu[..., 2])
        return mean + root, (mean - root).clamp(min=0)               # (clamp keeps NaN)

    def axis_lengths(self):
        """float64 [N, cap, 2] = (4 sqrt(lambda1), 4 sqrt(lambda2)): the axes of the ellipse with the object's second moments,
        lambda = (mu20 + mu02) / 2 +- sqrt(((mu20 - mu02) / 2)^2 + mu11^2), lambda2 clamped at 0."""
        l1, l2 = self._eigen()
        return torch.stack([4 * torch.sqrt(l1), 4 * torch.sqrt(l2)], dim=-1)

    def eccentricity(self):
        """float64 [N, cap] = sqrt(1 - lambda2 / lambda1), 0 where lambda1 == 0 (a single pixel)."""
        l1, l2 = self._eigen()
        return torch.where(l1 == 0, torch.zeros_like(l1), torch.sqrt(1 - l2 / l1))

    def orientation(self):
        """float64 [N, cap] = 0.5 atan2(2 mu11, mu20 - mu02): the angle of the major axis against the row axis, in (-pi/2, pi/2],
        0 for an isotropic object.  scikit-image's special case for mu20 == mu02 (+-pi/4 by the sign of mu11 in its own axis
        convention) is NOT reproduced, and no parity with its sign convention is claimed."""
        mu = self.central_moments()
        return 0.5 * torch.atan2(2 * mu[..., 2], mu[..., 0] - mu[..., 1])

    def perimeter(self):
        """float64 [N, cap] = straight + sqrt(2) diagonal + (1 + sqrt(2)) / 2 mixed: the 4-neighbourhood estimator that
        scikit-image documents; 0 for objects of one or two pixels."""
        t = self.tallies.to(torch.float64)
        p = t[..., 1] + _SQRT2 * t[..., 2] + (1 + _SQRT2) / 2 * t[..., 3]
        return torch.where(self.table.area > 0, p, torch.full_like(p, float("nan")))

    def equivalent_diameter(self):
        """float64 [N, cap] = sqrt(4 A / pi): the diameter of the disc of the object's area."""
        a = self._area()
        return torch.where(a > 0, torch.sqrt(4 * a / np.pi), torch.full_like(a, float("nan")))

    def extent(self):
        """float64 [N, cap] = A / ((r1 - r0) (c1 - c0)): the filled fraction of the bounding box."""
        b = self.table.bbox.to(torch.int64)
        return self._area() / ((b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])).to(torch.float64)

    def circularity(self):
        """float64 [N, cap] = 4 pi A / perimeter^2, inf where the perimeter is 0."""
        p = self.perimeter()
        return 4 * np.pi * self._area() / (p * p)

    def per_image(self):
        """``RegionTable.per_image`` with the columns ``moments``, ``tallies`` and one per method above added, trimmed alike.  The
        one method that synchronises."""
        out = self.table.per_image()
        cols = {"moments": self.moments, "tallies": self.tallies, **{k: getattr(self, k)() for k in _SHAPE_COLUMNS}}
        for k, v in cols.items():
            v = v.cpu().numpy()
            for n, d in enumerate(out):
                d[k] = v[n, :len(d["area"])]
        return out


def _check_shape_size(what, shape):
    """the second moments are int64: Sxx <= area (H - 1)^2 < 2^61 needs H, W <= 32768"""
    if len(shape) in (2, 3) and max(int(shape[-2]), int(shape[-1])) > K.REGIONS_SHAPE_MAX_SIDE:
        raise ValueError(f"{what}: a {shape[-2]}x{shape[-1]} image: H, W <= {K.REGIONS_SHAPE_MAX_SIDE} keep the second moments in int64")


def _labels_and_table(what, labels, table, max_regions, counts, masks_go_to, check_size=None):
    """The arguments that ``shape_labels``, ``hull_labels`` and ``contour_labels`` share -> (the placed ``_LabelImage``, the
    ``RegionTable`` of those images).  Every argument error is raised before anything is copied; a table of None runs
    ``measure_labels`` with ``max_regions`` and ``counts``."""
    _check_max_regions(max_regions)
    if table is not None and not isinstance(table, RegionTable):
        raise TypeError(f"{what}: table must be a RegionTable or None, got {type(table).__name__}")
    img = _LabelImage(what, labels, masks_go_to, check_size)
    N = img.N
    if table is not None:
        if max_regions is not None and int(max_regions) != table.capacity:
            raise ValueError(f"{what}: max_regions {max_regions} against a RegionTable of capacity {table.capacity}")
        if tuple(table.bbox.shape) != (N, table.capacity, 4):
            raise ValueError(f"{what}: a RegionTable of {tuple(table.bbox.shape[:2])} (images, capacity) with capacity "
                             f"{table.capacity} for {N} images")
    if table is None:
        img.with_counts(counts, what="measure_labels")                   # (read by measure_labels below, and refused in its name)
    t, _ = img.place()
    if table is None:
        table = measure_labels(t, max_regions=max_regions, counts=counts)
    elif table.bbox.device != t.device:
        raise ValueError(f"{what}: a RegionTable on {table.bbox.device} for label images on {t.device}")
    return img, table


def boundaries(x, connectivity=1):
    """The inner boundary of every object -> device ``torch.bool`` of the input's shape (the edge-pixel rule of ``shape_labels``).
    ``x``: an int32 label image ([H, W] or [N, H, W], 0 and below = background), or a boolean mask, which goes through
    ``label(x, connectivity)`` first: the components of that connectivity are the objects, so with connectivity 1 two diagonal
    foreground pixels may be different objects, each the other's "not this object".  Never synchronises."""
    t = _tensor(x)
    if torch.is_tensor(t) and t.dtype == torch.bool:
        t = label(t, connectivity)
    else:
        _check_connectivity(connectivity)
    img = _LabelImage("boundaries", t, masks_go_to="label first, which boundaries does for them")
    lab, _ = img.place()
    edges = torch.empty(lab.shape, dtype=torch.uint8, device=lab.device)
    for a, b in img.chunks:
        K.regions_edges_labels(lab[a:b], edges=edges[a:b])
    edges = edges.view(torch.bool)
    return edges[0] if img.two_d else edges


def shape_labels(labels, table=None, max_regions=None, counts=None):
    """Second moments and perimeter tallies of every label of a label image, and the map of its boundaries -> ``ShapeTable``: what
    elongation, axis lengths, orientation, perimeter and circularity are formed from, without a copy of the masks to the host.

    ``labels``: int32 [H, W] or [N, H, W] (numpy or torch) with H, W <= 32768 (``ValueError`` before anything is copied).  All rules
    are exact integers:

    * Objects.  A pixel's object id is ``max(label, 0)``: 0 and below are background.  The images of a batch are independent: the
      last row of one and the first row of the next are no neighbours.
    * Edge pixel.  A pixel whose id is positive and at least one of whose four neighbours has a different id; a neighbour outside
      the image has id 0.  Per object this is the object minus its erosion by the 4-neighbourhood with ``border_value=0``; another
      positive label counts as "not this object".  The capacity plays no part in this rule.
    * Second moments of label l, relative to the top-left corner (r0, c0) of its bounding box, x = r - r0, y = c - c0:
      ``Sxx = sum x^2``, ``Syy = sum y^2``, ``Sxy = sum x y``, int64.  (Relative to the box so that the float64 formulas of
      ``ShapeTable`` do not cancel on a slide-sized image; sum x and sum y follow exactly from ``sum_rc``, ``area`` and ``bbox``.)
    * Perimeter tallies.  For every edge pixel of object l, n4 = how many of its 4 neighbours are edge pixels of the same object
      l, nd = how many of its 4 diagonal neighbours are, code = ``1 + 2 n4 + 10 nd``.  Codes 5, 7, 15, 17, 25, 27 are *straight*,
      21 and 33 *diagonal*, 13 and 23 *mixed*, every other code is uncounted.  Four int32 tallies per object: edge pixels, straight,
      diagonal, mixed -- the weights of ``perimeter = straight + sqrt(2) diagonal + (1 + sqrt(2)) / 2 mixed``.  A filled 5 x 5 square
      has (16, 16, 0, 0).

    Rows of labels above the capacity are not written; a label without a pixel has an all-zero row.  The rules are restated in
    numpy by tests/shape_ref.py and pinned to ``scipy.ndimage`` constructions (``binary_erosion``; ``convolve`` with
    ``[[10, 2, 10], [2, 1, 2], [10, 2, 10]]`` and ``bincount``; ``sum_labels``; tests/golden/shape_vectors.npz).  Parity with
    ``skimage.measure.regionprops`` itself is NOT pinned: scikit-image is not a dependency of this project.

    ``table``: the ``RegionTable`` of the same label image where the caller has it (``measure_labels``; a table of another N,
    capacity or device raises ``ValueError``, and so does a ``max_regions`` that disagrees with it); None runs ``measure_labels``
    with ``max_regions`` and ``counts`` as given here.  With a table, or an int ``max_regions``, three launches whose grids depend
    on the shape and the capacity alone follow, nothing synchronises and the call can be captured into a graph; all accumulation is
    integer atomics, so the result does not depend on launch or arrival order."""
    img, table = _labels_and_table("shape_labels", labels, table, max_regions, counts, "shape", _check_shape_size)
    t, N, dev = img.labels, img.N, img.labels.device
    cap = table.capacity
    edges = torch.empty(t.shape, dtype=torch.uint8, device=dev)
    moments = torch.empty((N, cap, 3), dtype=torch.int64, device=dev)
    tallies = torch.empty((N, cap, 4), dtype=torch.int32, device=dev)
    bbox = table.bbox.contiguous()
    for a, b in img.chunks:
        K.regions_edges_labels(t[a:b], edges=edges[a:b])
        K.regions_shape_labels(t[a:b], edges[a:b], cap, bbox[a:b], moments=moments[a:b], tallies=tallies[a:b])
    edges = edges.view(torch.bool)
    return ShapeTable(table, moments, tallies, edges[0] if img.two_d else edges)


def shape(m, connectivity=1, max_regions=None, intensity=None):
    """``shape_labels`` for a boolean mask: ``label(m, connectivity)``, ``measure_labels`` of the labels (with ``intensity``, uint8
    of the mask's shape, or None) and ``shape_labels`` on that table -> ``ShapeTable``.  ``label`` numbers as
    ``scipy.ndimage.label``, so row k is the same component as row k of ``measure(m)`` and ``ShapeTable.table`` holds what
    ``measure`` gives.  ``max_regions`` as in ``measure_labels``: an int means no synchronisation."""
    _check_max_regions(max_regions)
    _check_shape_size("shape", tuple(getattr(m, "shape", ())))
    lab = label(m, connectivity)
    return shape_labels(lab, table=measure_labels(lab, intensity=intensity, max_regions=max_regions))


_HULL_COLUMNS = ("convex_area", "solidity", "feret_diameter_max", "feret_diameter_min", "n_vertices", "too_large")


@dataclasses.dataclass
class HullTable:
    """``hull_labels`` of N label images as device tensors.  ``table``: the ``RegionTable`` of the same images (row k = label
    k + 1); ``hull`` int32 [N, cap, 5] = (n_vertices, area2, feret_max2, width_cross, width_len2) of the convex hull of the label's
    pixel squares: all zero for a label without a pixel, all -1 for one whose bounding box is too large.  The rules are in
    ``hull_labels``' docstring.  Every method but ``per_image`` runs on the device, is computed from the integer tables only and,
    but for ``too_large``, gives float64 with NaN in unused and in too-large rows."""
    table: RegionTable
    hull: torch.Tensor

    def _measured(self, x):
        ok = (self.table.area > 0) & (self.hull[..., 0] >= 0)
        return torch.where(ok, x, torch.full_like(x, float("nan")))

    def too_large(self):
        """device bool [N, cap]: the label's bounding box has more than ``kernels.REGIONS_HULL_MAX_SIDE`` rows or columns, so the
        object is counted (its ``table`` row is complete) but its hull is not measured."""
        return self.hull[..., 0] < 0

    def n_vertices(self):
        """float64 [N, cap]: the strict vertices of the hull, at least 4."""
        return self._measured(self.hull[..., 0].to(torch.float64))

    def convex_area(self):
        """float64 [N, cap] = area2 / 2: the area of the hull of the pixel squares, >= the pixel count.  NOT scikit-image's
        ``area_convex``, which counts the pixels of a rasterised hull of the pixel centres' offsets."""
        return self._measured(self.hull[..., 1].to(torch.float64) / 2)

    def solidity(self):
        """float64 [N, cap] = area / convex_area, in (0, 1], exactly 1 for a filled rectangle."""
        return self.table.area.to(torch.float64) / self.convex_area()

    def feret_diameter_max(self):
        """float64 [N, cap] = sqrt(feret_max2): the largest distance between two points of the object's pixel squares (a single
        pixel: sqrt 2).  NOT scikit-image's ``feret_diameter_max``, which measures a marching-squares contour at level 0.5."""
        return self._measured(torch.sqrt(self.hull[..., 2].clamp(min=0).to(torch.float64)))

    def feret_diameter_min(self):
        """float64 [N, cap] = width_cross / sqrt(width_len2): the smallest distance between two parallel lines that hold the object
        between them (one of them runs along a hull edge)."""
        return self._measured(self.hull[..., 3].to(torch.float64) / torch.sqrt(self.hull[..., 4].clamp(min=0).to(torch.float64)))

    def per_image(self):
        """``RegionTable.per_image`` with the columns ``hull`` and one per method above added, trimmed alike.  The one method that
        synchronises."""
        out = self.table.per_image()
        cols = {"hull": self.hull, **{k: getattr(self, k)() for k in _HULL_COLUMNS}}
        for k, v in cols.items():
            v = v.cpu().numpy()
            for n, d in enumerate(out):
                d[k] = v[n, :len(d["area"])]
        return out


def hull_labels(labels, table=None, max_regions=None, counts=None):
    """The convex hull of every label of a label image, as integers -> ``HullTable``: what convex area, solidity (one cell or a
    clump?) and the largest and smallest Feret diameter are formed from, without a copy of the masks to the host.

    ``labels``: int32 [H, W] or [N, H, W] (numpy or torch).  Everything the device writes is an exact integer:

    * Objects.  A pixel's object id is ``max(label, 0)``: 0 and below are background.  The images of a batch are independent.  A
      label need not be connected: the hull is that of all its pixels.
    * Point set.  An object is the union of the closed unit squares of its pixels: pixel (r, c) contributes the lattice points
      (r, c), (r + 1, c), (r, c + 1), (r + 1, c + 1), and the hull is the convex hull of those points.  So every object, a single
      pixel included, has a hull of at least 4 vertices and positive area: there is no degenerate case.
    * Candidates.  Only the leftmost and the rightmost pixel of the object in each pixel row can contribute vertices; a row of the
      bounding box without a pixel of the label contributes nothing.  Hence at most ``2 (rows + 1)`` vertices, ``rows`` being the
      height of the bounding box.
    * Per label, int32 ``hull[N, cap, 5]``: ``n_vertices``, the strict vertices (no three consecutive ones collinear); ``area2``,
      twice the hull's area by the shoelace formula; ``feret_max2``, the largest squared distance between two vertices;
      ``width_cross`` and ``width_len2``, the minimum width as an exact fraction.
    * Minimum width.  For every hull edge e from a to b let ``len2(e) = |b - a|^2`` and ``cross(e)`` the maximum over the hull's
      vertices v of ``|(b - a) x (v - a)|``; the width across e is ``cross(e) / sqrt(len2(e))``.  Stored is the edge that minimises
      ``(cross^2 / len2, len2)``, the fractions compared by cross-multiplication in unsigned 64-bit integers; the second key makes
      the pair unique (equal width and equal len2 give equal cross).
    * Side limit.  A bounding box of more than ``kernels.REGIONS_HULL_MAX_SIDE`` = 1024 rows or columns is too large: all five
      entries are -1 and ``HullTable.too_large()`` flags the row; the object is counted, not measured, as rows above a capacity are
      elsewhere.  Within the limit cross <= 2^21, cross^2 <= 2^42 and len2 <= 2^21: every compared product is below 2^64 and every
      output fits int32.
    * A label without a pixel has an all-zero row; rows of labels above the capacity are not written.  No workspace.

    A filled 5 x 5 square has (4, 50, 50, 25, 25), a single pixel (4, 2, 2, 1, 1).  The rules are restated in Python integers by
    tests/hull_ref.py and pinned to ``scipy.spatial.ConvexHull`` over all corners of all pixels (tests/golden/hull_vectors.npz).
    Parity with ``skimage.measure.regionprops`` is NOT claimed and scikit-image is not a dependency: its ``area_convex`` counts the
    pixels of a rasterised hull (an integer, where ``convex_area`` here is the exact area of the polygon round the pixel squares),
    and its ``feret_diameter_max`` measures a marching-squares contour through the pixel edges' midpoints (shorter than the
    distance between pixel corners used here).

    ``table``, ``max_regions`` and ``counts`` as in ``shape_labels``.  With a table, or an int ``max_regions``, one launch whose
    grid depends on (N, capacity) alone follows, nothing synchronises and the call can be captured into a graph; there are no
    atomics, so the result does not depend on launch order."""
    img, table = _labels_and_table("hull_labels", labels, table, max_regions, counts, "hull")
    t, cap = img.labels, table.capacity
    hull = torch.empty((img.N, cap, 5), dtype=torch.int32, device=t.device)
    bbox = table.bbox.contiguous()
    for a, b in img.chunks:
        K.regions_hull_labels(t[a:b], cap, bbox[a:b], hull=hull[a:b])
    return HullTable(table, hull)


def hull(m, connectivity=1, max_regions=None, intensity=None):
    """``hull_labels`` for a boolean mask: ``label(m, connectivity)``, ``measure_labels`` of the labels (with ``intensity``, uint8
    of the mask's shape, or None) and ``hull_labels`` on that table -> ``HullTable``.  Row k is the same component as row k of
    ``measure(m)``.  ``max_regions`` as in ``measure_labels``: an int means no synchronisation."""
    _check_max_regions(max_regions)
    lab = label(m, connectivity)
    return hull_labels(lab, table=measure_labels(lab, intensity=intensity, max_regions=max_regions))


_CONTOUR_COLUMNS = ("n_vertices", "too_large", "truncated", "is_simple", "crack_perimeter", "enclosed_area", "hole_area")


@dataclasses.dataclass
class ContourTable:
    """``contour_labels`` of N label images as device tensors.  ``table``: the ``RegionTable`` of the same images (row k = label
    k + 1); ``contour`` int32 [N, cap, 4] = (n_vertices, n_cracks, area2, cracks_all) of the label's outer boundary ring: all zero
    for a label without a pixel in its box, all -1 for one whose bounding box is too large; ``vertices`` int32
    [N, cap, max_vertices, 2] = the ring's first ``min(n_vertices, max_vertices)`` lattice vertices as (row, col), (-1, -1) after
    them; ``connectivity`` as traced.  The rules are in ``contour_labels``' docstring.  Every method but ``per_image`` and
    ``geojson`` runs where the tensors are, is computed from the integer tables only and gives either bool or float64 with NaN in
    unused and in too-large rows."""
    table: RegionTable
    contour: torch.Tensor
    vertices: torch.Tensor
    connectivity: int = 1

    def _ok(self):
        return (self.table.area > 0) & (self.contour[..., 0] > 0)

    def _measured(self, x):
        return torch.where(self._ok(), x, torch.full_like(x, float("nan")))

    @property
    def max_vertices(self):
        return int(self.vertices.shape[2])

    def too_large(self):
        """bool [N, cap]: the label's bounding box has more than ``kernels.REGIONS_CONTOUR_MAX_SIDE`` rows or columns, so the object
        is counted (its ``table`` row is complete) but not traced."""
        return self.contour[..., 0] < 0

    def truncated(self):
        """bool [N, cap]: the ring has more vertices than ``vertices`` has slots; ``n_vertices`` is still the true count."""
        return self.contour[..., 0] > self.max_vertices

    def is_simple(self):
        """bool [N, cap]: ``n_cracks == cracks_all`` in a traced row, i.e. every boundary crack of the label lies on the traced
        ring: the label is one piece (of the connectivity traced) without a hole, and the ring is all of its boundary."""
        return self._ok() & (self.contour[..., 1] == self.contour[..., 3])

    def n_vertices(self):
        """float64 [N, cap]: the vertices of the ring, even and at least 4, also where the ring is truncated."""
        return self._measured(self.contour[..., 0].to(torch.float64))

    def crack_perimeter(self):
        """float64 [N, cap] = n_cracks: the length of the ring along the pixel sides (the city-block perimeter of the outline)."""
        return self._measured(self.contour[..., 1].to(torch.float64))

    def enclosed_area(self):
        """float64 [N, cap] = area2 / 2: the area inside the ring, holes included; for a one-piece label >= its pixel count."""
        return self._measured(self.contour[..., 2].to(torch.float64) / 2)

    def hole_area(self):
        """float64 [N, cap] = area2 / 2 - area: for a one-piece label the pixels the ring encloses that are not the label's (its
        holes and whatever lies in them); negative where further pieces of the label lie outside the ring."""
        return self.enclosed_area() - self.table.area.to(torch.float64)

    def per_image(self):
        """``RegionTable.per_image`` with the columns ``contour``, one per method above and ``polygon`` added, trimmed alike;
        ``polygon`` is a list of int32 [n, 2] arrays (row, col), n = min(n_vertices, max_vertices), 0 for a row that is not
        traced.  Synchronises."""
        out = self.table.per_image()
        cols = {"contour": self.contour, **{k: getattr(self, k)() for k in _CONTOUR_COLUMNS}}
        cols = {k: v.cpu().numpy() for k, v in cols.items()}
        verts = self.vertices.cpu().numpy()
        for n, d in enumerate(out):
            rows = len(d["area"])
            for k, v in cols.items():
                d[k] = v[n, :rows]
            kept = np.clip(cols["contour"][n, :rows, 0], 0, self.max_vertices)
            d["polygon"] = [verts[n, k, :kept[k]].copy() for k in range(rows)]
        return out

    def geojson(self, image=0, origin=(0, 0), scale=1.0, properties=None):
        """The rings of one image as a GeoJSON ``FeatureCollection`` (a host ``dict``, ready for ``json.dump``; QuPath, shapely
        and geopandas read it): one ``Polygon`` feature per traced row whose ring is complete -- unused, too-large and truncated
        rows are left out.  A lattice vertex (row, col) becomes ``[origin[0] + scale * col, origin[1] + scale * row]`` (x, y), so
        ``origin`` is the (x, y) of the image's top-left corner in the target frame and ``scale`` its pixel size there; the ring
        is closed (the first point is repeated last) and, y pointing down, runs clockwise on screen.  ``properties`` of a
        feature: ``row`` (k; the label is k + 1), ``area`` (the pixel count), and one entry per item of ``properties``, a dict
        name -> a sequence with one value per row of this image.  Synchronises."""
        n = int(image)
        if not 0 <= n < self.contour.shape[0]:
            raise IndexError(f"geojson: image {image} of {self.contour.shape[0]}")
        extra = {k: (v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in (properties or {}).items()}
        rows = self.contour.shape[1]
        for k, v in extra.items():
            if v.ndim < 1 or len(v) < rows:
                raise ValueError(f"geojson: properties[{k!r}] needs one value per row ({rows}), got shape {v.shape}")
        contour, verts, area = self.contour[n].cpu().numpy(), self.vertices[n].cpu().numpy(), self.table.area[n].cpu().numpy()
        ox, oy, scale = float(origin[0]), float(origin[1]), float(scale)
        features = []
        for k in range(rows):
            nv = int(contour[k, 0])
            if area[k] <= 0 or nv <= 0 or nv > self.max_vertices:
                continue
            ring = [[ox + scale * int(c), oy + scale * int(r)] for r, c in verts[k, :nv].tolist()]
            props = {"row": k, "area": int(area[k]), **{name: v[k].tolist() for name, v in extra.items()}}
            features.append({"type": "Feature", "properties": props,
                             "geometry": {"type": "Polygon", "coordinates": [ring + [ring[0]]]}})
        return {"type": "FeatureCollection", "features": features}


def _check_max_vertices(max_vertices):
    if max_vertices is not None and (isinstance(max_vertices, bool) or int(max_vertices) != max_vertices or max_vertices < 0):
        raise ValueError(f"max_vertices must be a non-negative integer or None, got {max_vertices!r}")


def contour_labels(labels, table=None, max_regions=None, counts=None, connectivity=1, max_vertices=None):
    """The outer boundary of every label of a label image as an ordered polygon of lattice vertices -> ``ContourTable``: what a
    GeoJSON or QuPath export, shapely, or a comparison with polygon annotations needs, without a copy of the label image to the
    host.

    ``labels``: int32 [H, W] or [N, H, W] (numpy or torch).  Everything the device writes is an exact integer:

    * Objects.  A pixel's object id is ``max(label, 0)``: 0 and below are background.  The images of a batch are independent.
      Pixel (r, c) is the closed unit square with the lattice corners (r, c) and (r + 1, c + 1), as in ``hull_labels``.  For
      label l the object is the pixels with id l inside the label's box from the ``RegionTable``, the box cut to the image first;
      a pixel outside the box is "not the object" whatever it holds, and so is every other positive label.
    * Crack.  A unit side of a pixel of the object whose neighbour across that side is not in the object.
    * Start.  (pr, pc) is the first pixel of the object in row-major order.  The ring starts at lattice vertex (pr, pc), heading
      east along that pixel's top side, the object on the right hand: with rows pointing down that is clockwise on screen, and
      the shoelace sum ``sum(c_i r_{i+1} - c_{i+1} r_i)`` over the ring, twice its area, comes out positive.
    * Step.  Move one lattice unit, one crack, along the heading.  At the vertex (r, c) reached look at the pixel ahead on the
      right, R, and the one ahead on the left, L: heading E, R = (r, c) and L = (r - 1, c); S, R = (r, c - 1) and L = (r, c);
      W, R = (r - 1, c - 1) and L = (r, c - 1); N, R = (r - 1, c) and L = (r - 1, c - 1).  R not in the object: turn right --
      but with ``connectivity=2`` and L in the object turn left, across to the diagonal pixel.  R and L both in: turn left.  R
      in and L out: straight on.
    * Stop on arriving at (pr, pc) with the new heading east.  The successor rule permutes the cracks of a finite bitmap, so the
      walk returns to its first crack; the kernel's loop is bounded by ``2 rows cols + rows + cols`` steps, the cracks of the box,
      all the same.
    * Vertices.  A lattice vertex is emitted where the heading changes; the start vertex is such a corner and comes first.  So the
      ring is strict (no three consecutive vertices collinear), its edges alternate horizontal and vertical, ``n_vertices`` is
      even and at least 4, and a lattice point may occur twice in a ring, at a pinch point.
    * What is traced.  Only the ring through the start crack: the outer boundary of the component that holds the label's first
      pixel, 4-connected at connectivity 1 and 8-connected at 2.  Holes and further pieces of a disconnected label are not
      traced; ``cracks_all``, the number of all cracks of the label, tells: it equals ``n_cracks`` exactly when there are none.
    * Per label, int32 ``contour[N, cap, 4]`` = ``n_vertices`` (the true count, also above ``max_vertices``), ``n_cracks`` (the
      ring's length), ``area2`` (twice the area the ring encloses), ``cracks_all``; and int32 ``vertices[N, cap, max_vertices, 2]``
      = the first ``min(n_vertices, max_vertices)`` vertices as absolute (row, col), every slot after them (-1, -1).
    * Side limit.  A bounding box of more than ``kernels.REGIONS_CONTOUR_MAX_SIDE`` = 512 rows or columns is too large: the four
      entries are -1, there is no vertex and ``ContourTable.too_large()`` flags the row; the object is counted, not traced.
    * A label without a pixel in its box has an all-zero row and no vertex; rows of labels above the capacity are not written.

    A single pixel at (0, 0) has the ring (0, 0), (0, 1), (1, 1), (1, 0) and the row (4, 4, 2, 4); a filled 5 x 5 square (4, 20,
    50, 20); a 3 x 3 square without its centre (4, 12, 18, 16).  The rule is restated in plain loops by tests/contour_ref.py and
    pinned to ``scipy.ndimage.binary_fill_holes`` of the first component with the complementary structure
    (tests/golden/contour_vectors.npz).  Parity with ``cv2.findContours`` (which joins pixel centres) or
    ``skimage.measure.find_contours`` (marching squares at half-pixel positions) is NOT claimed: neither is a dependency.

    ``table``, ``max_regions`` and ``counts`` as in ``shape_labels``; ``connectivity`` 1 or 2 as above.  ``max_vertices=int`` fixes
    the vertex slots per label (0: count only): with a table, or an int ``max_regions``, one launch whose grid depends on (N,
    capacity) alone follows, nothing synchronises and the call can be captured into a graph.  ``max_vertices=None`` makes a
    counting-only launch first, reads the largest ``n_vertices`` back (the one synchronisation) and runs with ``max(4, that)``, so
    that no ring is truncated.  There are no atomics: the result does not depend on launch order."""
    conn = _check_connectivity(connectivity)
    _check_max_vertices(max_vertices)
    img, table = _labels_and_table("contour_labels", labels, table, max_regions, counts, "contours")
    t, N, cap, chunks = img.labels, img.N, table.capacity, img.chunks
    bbox = table.bbox.contiguous()
    contour = torch.empty((N, cap, 4), dtype=torch.int32, device=t.device)
    if max_vertices is None:
        for a, b in chunks:
            K.regions_contour_labels(t[a:b], cap, bbox[a:b], conn, 0, contour=contour[a:b])
        maxv = max(4, int(contour[..., 0].max()))                        # the one synchronisation
    else:
        maxv = int(max_vertices)
    vertices = torch.empty((N, cap, maxv, 2), dtype=torch.int32, device=t.device)
    for a, b in chunks:
        K.regions_contour_labels(t[a:b], cap, bbox[a:b], conn, maxv, contour=contour[a:b], vertices=vertices[a:b] if maxv else None)
    return ContourTable(table, contour, vertices, conn)


def contours(m, connectivity=1, max_regions=None, max_vertices=None):
    """``contour_labels`` for a boolean mask: ``label(m, connectivity)``, ``measure_labels`` of the labels and ``contour_labels`` on
    that table with the same connectivity -> ``ContourTable``.  Row k is the same component as row k of ``measure(m)``; every
    component is one piece, so ``is_simple()`` says whether it has a hole.  ``max_regions`` as in ``measure_labels`` and
    ``max_vertices`` as in ``contour_labels``: ints mean no synchronisation."""
    _check_max_regions(max_regions)
    _check_max_vertices(max_vertices)
    lab = label(m, connectivity)
    return contour_labels(lab, table=measure_labels(lab, max_regions=max_regions), connectivity=connectivity, max_vertices=max_vertices)


TEXTURE_LEVELS = K.TEXTURE_LEVELS
_TEXTURE_COLUMNS = ("contrast", "dissimilarity", "homogeneity", "asm", "energy", "mean", "variance", "correlation",
                    "difference_entropy", "sum_entropy", "sum_average")


def _check_texture(levels, distance):
    if isinstance(levels, bool) or not isinstance(levels, (int, np.integer)) or levels not in TEXTURE_LEVELS:
        raise ValueError(f"levels must be one of {TEXTURE_LEVELS}, got {levels!r}")
    if isinstance(distance, bool) or not isinstance(distance, (int, np.integer)) or not 1 <= distance <= K.TEXTURE_MAX_DISTANCE:
        raise ValueError(f"distance must be an integer in [1, {K.TEXTURE_MAX_DISTANCE}], got {distance!r}")
    return int(levels), int(distance)


def _check_texture_size(what, shape):
    """the pair counts are int32: a direction has fewer than H W <= 2^30 pairs"""
    if len(shape) in (2, 3) and int(shape[-2]) * int(shape[-1]) > K.TEXTURE_MAX_PIXELS:
        raise ValueError(f"{what}: a {shape[-2]}x{shape[-1]} image: H W <= 2^30 keeps the pair counts in int32")


def _entropy(counts, total, dims):
    """-sum q log2 q over ``dims`` of q = counts / total, 0 log 0 = 0"""
    q = counts.to(torch.float64) / total
    return -torch.where(q > 0, q * torch.log2(q), torch.zeros_like(q)).sum(dim=dims)


@dataclasses.dataclass(eq=False)
class TextureTable:
    """``texture_labels`` of N label images as device tensors.  ``table``: the ``RegionTable`` of the same images (row k = label
    k + 1).  Per (image, row, direction), the directions being 0, 45, 90 and 135 degrees at ``distance``, of the symmetric grey-level
    co-occurrence matrix S of the pixel pairs inside the label at ``levels`` = L grey levels: ``pairs`` int32 [N, cap, 4]; ``diff``
    and ``marg`` int32 [N, cap, 4, L]; ``sum`` int32 [N, cap, 4, 2L - 1]; ``sq`` and ``cross`` int64 [N, cap, 4]; ``matrix`` int32
    [N, cap, 4, L, L] = S, or None.  ``Mq`` int32 numpy [N, 3] and ``options`` are what ``stain.texture_labels`` made it with, None
    for a plane.  The rules are in ``texture_labels``' docstring.  With T = 2 pairs, M1 = sum i marg[i] and M2 = sum i^2 marg[i],
    every method but ``per_image`` runs on the device in float64, is computed from the integer tables only and returns [N, cap, 4]
    with NaN where ``pairs == 0``; ``average=True`` returns [N, cap]: the mean over the directions that are not NaN, NaN where none
    is."""
    table: RegionTable
    pairs: torch.Tensor
    diff: torch.Tensor
    sum: torch.Tensor
    marg: torch.Tensor
    sq: torch.Tensor
    cross: torch.Tensor
    matrix: typing.Optional[torch.Tensor]
    levels: int
    distance: int
    Mq: typing.Optional[np.ndarray] = None
    options: object = None

    def _total(self):
        """T = 2 pairs in float64, NaN where there is no pair"""
        t = 2.0 * self.pairs.to(torch.float64)
        return torch.where(self.pairs > 0, t, torch.full_like(t, float("nan")))

    def _out(self, x, average):
        x = torch.where(self.pairs > 0, x, torch.full_like(x, float("nan")))
        if not average:
            return x
        ok = ~torch.isnan(x)
        return torch.where(ok, x, torch.zeros_like(x)).sum(dim=-1) / ok.sum(dim=-1).to(torch.float64)

    def _weighted(self, hist, weight):
        """sum_k weight(k) hist[k] in float64"""
        k = torch.arange(hist.shape[-1], dtype=torch.float64, device=hist.device)
        return (hist.to(torch.float64) * weight(k)).sum(dim=-1)

    def _moments(self):
        """M1 = sum i marg[i] and M2 = sum i^2 marg[i], int64"""
        i = torch.arange(self.levels, dtype=torch.int64, device=self.marg.device)
        m = self.marg.to(torch.int64)
        return (m * i).sum(dim=-1), (m * i * i).sum(dim=-1)

    def _central(self, raw):
        """T raw - M1^2 in float64 (raw: int64 M2 or cross) and T: an exact int64 product where pairs < 2^20 (T < 2^21, raw and
        M1 <= 31^2 T: every product below 2^62), float64 beyond"""
        M1, _ = self._moments()
        T = 2 * self.pairs.to(torch.int64)
        exact = (T * raw - M1 * M1).to(torch.float64)
        Tf, M1f = T.to(torch.float64), M1.to(torch.float64)
        return torch.where(self.pairs < (1 << 20), exact, Tf * raw.to(torch.float64) - M1f * M1f)

    def contrast(self, average=False):
        """sum k^2 diff[k] / T"""
        return self._out(self._weighted(self.diff, lambda k: k * k) / self._total(), average)

    def dissimilarity(self, average=False):
        """sum k diff[k] / T"""
        return self._out(self._weighted(self.diff, lambda k: k) / self._total(), average)

    def homogeneity(self, average=False):
        """sum diff[k] / (1 + k^2) / T: the inverse difference moment"""
        return self._out(self._weighted(self.diff, lambda k: 1.0 / (1.0 + k * k)) / self._total(), average)

    def asm(self, average=False):
        """sq / T^2: the angular second moment"""
        T = self._total()
        return self._out(self.sq.to(torch.float64) / (T * T), average)

    def energy(self, average=False):
        """sqrt(asm)"""
        T = self._total()
        return self._out(torch.sqrt(self.sq.to(torch.float64) / (T * T)), average)

    def mean(self, average=False):
        """M1 / T: the mean grey level of the pixels that pair"""
        return self._out(self._moments()[0].to(torch.float64) / self._total(), average)

    def variance(self, average=False):
        """(T M2 - M1^2) / T^2"""
        T = self._total()
        return self._out(self._central(self._moments()[1]) / (T * T), average)

    def correlation(self, average=False):
        """(T cross - M1^2) / (T M2 - M1^2), NaN where the denominator is 0 (one grey level only)"""
        num, den = self._central(self.cross), self._central(self._moments()[1])
        return self._out(torch.where(den != 0, num / den, torch.full_like(den, float("nan"))), average)

    def difference_entropy(self, average=False):
        """-sum q log2 q over q = diff / T"""
        return self._out(_entropy(self.diff, self._total().unsqueeze(-1), -1), average)

    def sum_entropy(self, average=False):
        """-sum q log2 q over q = sum / T"""
        return self._out(_entropy(self.sum, self._total().unsqueeze(-1), -1), average)

    def sum_average(self, average=False):
        """sum k sum[k] / T"""
        return self._out(self._weighted(self.sum, lambda k: k) / self._total(), average)

    def entropy(self, average=False):
        """-sum p log2 p over p = matrix / T; the table must have been made with ``want_matrix=True``"""
        if self.matrix is None:
            raise ValueError("entropy: the table was made without the matrix (want_matrix=False)")
        return self._out(_entropy(self.matrix, self._total().unsqueeze(-1).unsqueeze(-1), (-2, -1)), average)

    def overflowed(self):
        """device bool [N]: the image has labels above the table's rows"""
        return self.table.overflowed()

    def per_image(self):
        """``RegionTable.per_image`` with the integer tables that the table has and one column per method above (``entropy`` with
        the matrix) added, trimmed alike.  The one method that synchronises."""
        out = self.table.per_image()
        cols = {k: getattr(self, k) for k in ("pairs", "diff", "sum", "marg", "sq", "cross")}
        cols.update({k: getattr(self, k)() for k in _TEXTURE_COLUMNS})
        if self.matrix is not None:
            cols.update(matrix=self.matrix, entropy=self.entropy())
        for k, v in cols.items():
            v = v.cpu().numpy()
            for n, d in enumerate(out):
                d[k] = v[n, :len(d["area"])]
        return out


def _texture(img, table, levels, distance, want_matrix, plane=None, images=None, od_q=None, mq=None, Mq=None, options=None):
    """the launches of ``texture_labels`` and ``stain.texture_labels`` on placed operands -> ``TextureTable``"""
    t, N, cap, dev, L = img.labels, img.N, table.capacity, img.labels.device, levels
    new = lambda dtype, *tail: torch.empty((N, cap, 4) + tail, dtype=dtype, device=dev)  # noqa: E731
    out = {"pairs": new(torch.int32), "diff": new(torch.int32, L), "sum": new(torch.int32, 2 * L - 1), "marg": new(torch.int32, L),
           "sq": new(torch.int64), "cross": new(torch.int64)}
    if want_matrix:
        out["matrix"] = new(torch.int32, L, L)
    bbox = table.bbox.contiguous()
    for a, b in img.chunks:
        K.texture_labels(t[a:b], cap, bbox[a:b], None if plane is None else plane[a:b], None if images is None else images[a:b], od_q,
                         None if mq is None else mq[a:b], L, distance, want_matrix, **{k: v[a:b] for k, v in out.items()})
    return TextureTable(table, out["pairs"], out["diff"], out["sum"], out["marg"], out["sq"], out["cross"], out.get("matrix"), L,
                        distance, Mq, options)


def texture_labels(labels, intensity, levels=16, distance=1, table=None, max_regions=None, counts=None, want_matrix=False):
    """How the grey values of ``intensity`` are arranged inside every label of a label image -> ``TextureTable``: the grey-level
    co-occurrence matrices that Haralick's texture features are formed from (QuPath's "Haralick features", CellProfiler's
    ``MeasureTexture``), without a copy of the image to the host.

    ``labels``: int32 [H, W] or [N, H, W] (numpy or torch) with H W <= 2^30; ``intensity``: uint8 of the same shape, for example
    a plane of ``stain.separate(dtype="u8")`` (``stain.texture_labels`` reads an RGB image instead).  Everything the device writes
    is an exact integer:

    * Level.  Every pixel has a level in 0 .. 255: the byte of ``intensity``.
    * Grey level.  ``g = (level * L) >> 8`` with L = ``levels`` in {8, 16, 32}: the bin rule of ``stain.quantify_labels``' ``hist``.
    * Offsets.  For ``distance`` d in 1 .. 8 the four directions k = 0 .. 3 are ``(dr, dc)`` = ``(0, d)``, ``(d, d)``, ``(d, 0)``,
      ``(d, -d)``: 0, 45, 90 and 135 degrees with the row axis downwards.
    * Pairs.  A pixel p = (r, c) with ``0 < labels[p] = l <= capacity`` forms a pair with q = (r + dr, c + dc) when q lies inside
      the image and ``labels[q] == l``; nothing else forms a pair.  The ordered count is ``C_k[g(p)][g(q)] += 1``.  A label need not
      be connected: two of its pieces exactly an offset apart do pair.  Pixels of another label, of the background (``<= 0``) or
      outside the image never pair.  The images of a batch are independent.
    * Symmetric matrix.  ``S_k = C_k + C_k^T``; its total is ``T_k = 2 pairs_k``.
    * Tables, per (image, row = label - 1, direction): ``pairs`` int32 [N, cap, 4], the number of pairs; ``diff`` int32
      [N, cap, 4, L], ``diff[k]`` = the sum of ``S_ij`` over ``abs(i - j) = k``; ``sum`` int32 [N, cap, 4, 2L - 1], ``sum[k]`` = the
      same over ``i + j = k``; ``marg`` int32 [N, cap, 4, L], ``marg[i]`` = the sum of ``S_ij`` over j; ``sq`` int64 [N, cap, 4] =
      the sum of ``S_ij^2``; ``cross`` int64 [N, cap, 4] = the sum of ``i j S_ij``; and only with ``want_matrix=True`` ``matrix``
      int32 [N, cap, 4, L, L] = S itself.
    * Empty rows.  A label without a pixel, or without a pair in a direction, has all zeros there (and NaN in every method of the
      table).  Rows of labels above the capacity are not written; they are counted in ``table.counts`` as elsewhere.
    * Bounds.  With H W <= 2^30, ``2 pairs < 2^31``: every int32 entry fits, ``sq < 2^62`` and ``cross < 2^41``.  ``N cap 4
      (2L - 1)`` and, with the matrix, ``N cap 4 L^2`` per kernel call stay below 2^31.

    Hand case: labels ``[[1,1,1,2],[1,1,2,2],[0,1,2,-3]]`` over the plane ``[[0,40,40,255],[100,40,255,200],[7,250,31,9]]`` with
    L = 8 and d = 1 have the grey levels ``[[0,1,1,7],[3,1,7,6],[0,7,0,0]]``.  Label 1 has in direction 0 three pairs, ``diff`` =
    (2, 2, 2, 0, ..), ``marg`` = (1, 4, 0, 1, 0, 0, 0, 0), ``sq`` = 8 and ``cross`` = 8, and in direction 1 two pairs, ``diff`` =
    (0, 2, 0, 0, 2, 0, ..), ``sq`` = 4 and ``cross`` = 42.  Label 2 has in direction 0 one pair, ``sq`` = 2 and ``cross`` = 84, in
    direction 1 none (all zero), and in direction 3 two pairs, ``marg`` = (1, 0, 0, 0, 0, 0, 1, 2), ``sq`` = 6 and ``cross`` = 98.

    The rules are restated in numpy by tests/texture_ref.py (tests/golden/texture_vectors.npz) and, on a full rectangle, held
    against an independent ``scipy.sparse`` construction.  Parity with ``skimage.feature.graycomatrix`` is claimed for d = 1 only,
    with ``symmetric=True`` and its angles 0, pi/4, pi/2 and 3 pi/4 matched to the offsets above: scikit-image rounds its diagonal
    offsets ``d cos``, ``d sin`` differently for d > 1, where the offsets here stay ``(d, d)``.  scikit-image is not a dependency
    of this project and was not run.

    ``table``, ``max_regions`` and ``counts`` as in ``hull_labels``.  With a table, or an int ``max_regions``, one launch whose grid
    depends on (N, capacity) alone follows, nothing synchronises and the call can be captured into a graph: one workgroup per label
    walks the label's bounding box and counts into tables in its own local memory, there are no global atomics and no workspace,
    so the result does not depend on launch or arrival order.  Argument errors are raised before the library is loaded."""
    what = "texture_labels"
    L, d = _check_texture(levels, distance)
    v = _as_intensity(intensity, _as_labels(labels, what).shape)
    img, table = _labels_and_table(what, labels, table, max_regions, counts, "label first", _check_texture_size)
    N, H, W = img.labels.shape
    return _texture(img, table, L, d, bool(want_matrix), plane=v.to(img.labels.device).contiguous().view(N, H, W))
