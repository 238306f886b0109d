"""Polygons to pixels on the device: label images and masks from vertex rings (csrc/polygons.hip).

The inverse of ``regions.contour_labels`` / ``ContourTable.geojson``: ground truth that comes as polygons (QuPath GeoJSON,
MoNuSeg-style rings) becomes a label image for ``regions.match_labels`` and ``inference.evaluate_instances``, and a region of
interest drawn by a pathologist becomes the mask of ``detect_slide(roi=...)``.  ``rasterize`` holds the rule."""
from dataclasses import dataclass

import numpy as np
import torch

from . import kernels as K

RULES = {"evenodd": K.CS_POLYGON_EVENODD, "nonzero": K.CS_POLYGON_NONZERO}
MODES = {"labels": torch.int32, "mask": torch.uint8}
# Rows of a shape that one workgroup paints; a taller host-side shape is cut into bands of this many rows so that a slide-sized
# outline spreads over the device.  Chosen from the sweep of tools/polygon_microbench.py (profiles/polygon_microbench.json, table
# in DESIGN.md, "Polygons to pixels"): 16 keeps small cells whole and gives a 16384-row outline 918 items.
BAND_ROWS = 16
_TABLES = ("vertices", "ring_start", "ring_count", "shape_rings", "image_shapes")


@dataclass
class PolygonSet:
    """Shapes of N images as int32 tensors, all on the host or all on one device.  ``vertices`` [V, 2] = (row, col) in units of
    ``1 / 2**sub`` pixel; ring r is the rows ``ring_start[r] .. ring_start[r] + ring_count[r]`` of it (both [R]; a count of 0
    draws nothing), so a packed table and the padded ``ContourTable.vertices`` are both served; shape s owns the rings
    ``shape_rings[s] .. shape_rings[s + 1]`` ([S + 1]) and image n the shapes ``image_shapes[n] .. image_shapes[n + 1]``
    ([N + 1]).  ``properties``: None or a host list with one entry per shape (``from_geojson`` keeps each feature's)."""
    vertices: torch.Tensor
    ring_start: torch.Tensor
    ring_count: torch.Tensor
    shape_rings: torch.Tensor
    image_shapes: torch.Tensor
    sub: int = 4
    properties: object = None

    @property
    def n_images(self):
        return int(self.image_shapes.numel()) - 1

    @property
    def n_shapes(self):
        return int(self.shape_rings.numel()) - 1

    def to(self, device):
        """the same set with every tensor on ``device``"""
        return PolygonSet(*(getattr(self, k).to(device) for k in _TABLES), sub=self.sub, properties=self.properties)


def _check_sub(sub, what):
    if isinstance(sub, bool) or not isinstance(sub, (int, np.integer)) or not 0 <= sub <= K.POLYGON_MAX_SUB:
        raise ValueError(f"{what}: sub must be an integer in [0, {K.POLYGON_MAX_SUB}], got {sub!r}")
    return int(sub)


def quantize(v, sub):
    """float or integer coordinates in pixels -> int64 in units of ``1 / 2**sub`` pixel: ``numpy.rint(v * 2**sub)`` in float64 (ties
    to even); integers are multiplied exactly."""
    v = np.asarray(v)
    if v.dtype.kind not in "iuf":
        raise TypeError(f"coordinates must be numbers, got dtype {v.dtype}")
    if v.dtype.kind == "f" and not np.isfinite(v).all():
        raise ValueError("coordinates must be finite")
    scaled = np.rint(v.astype(np.float64) * float(1 << sub))               # the range is checked before anything becomes an integer
    if scaled.size and np.abs(scaled).max() > K.POLYGON_MAX_COORD:
        raise ValueError(f"a quantised coordinate leaves [-2^28, 2^28] at sub={sub}")
    return v.astype(np.int64) << sub if v.dtype.kind in "iu" else scaled.astype(np.int64)


def _ring(r, sub, xy, what):
    if torch.is_tensor(r):
        r = r.detach().cpu().numpy()
    r = np.asarray(r)
    if r.size == 0:
        return np.zeros((0, 2), np.int64)
    if r.ndim != 2 or r.shape[1] < 2:
        raise ValueError(f"{what}: a ring is an [n, 2] array, got shape {r.shape}")
    try:
        q = quantize(r[:, :2], sub)
    except ValueError as e:
        raise ValueError(f"{what}: {e}") from None
    if xy:
        q = q[:, ::-1]
    if len(q) > 1 and (q[0] == q[-1]).all():                               # a repeated closing point
        q = q[:-1]
    return q


def _is_ring(shape):
    """a shape is one ring (points) or a list of rings: an array says so by its rank, a list by its first element that is not
    empty -- a point has rank 1, a ring rank 2; a list of nothing but empty elements is a list of empty rings"""
    if torch.is_tensor(shape) or isinstance(shape, np.ndarray):
        return shape.ndim == 2
    for x in shape:
        if torch.is_tensor(x) or np.size(x):
            return not torch.is_tensor(x) and np.ndim(x) == 1
    return False


def from_rings(per_image, sub=4, xy=False, properties=None):
    """``per_image``: a list over images of lists of shapes; a shape is a ring or a list of rings (the first the outline, the
    others holes or further parts -- the rule makes no difference between them); a ring is an [n, 2] array of (row, col), or of
    (x, y) = (col, row) with ``xy``.  Floats are quantised on the host as ``numpy.rint(v * 2**sub)`` in float64; integer arrays
    are multiplied by ``2**sub`` exactly, so with ``sub=0`` they pass through unchanged.  A repeated closing point is dropped.
    -> a host ``PolygonSet`` in the packed layout."""
    sub = _check_sub(sub, "from_rings")
    verts, counts, shape_rings, image_shapes = [], [], [0], [0]
    for n, shapes in enumerate(per_image):
        for s, shape in enumerate(shapes):
            rings = [shape] if _is_ring(shape) else list(shape)
            for r in rings:
                q = _ring(r, sub, xy, f"from_rings: image {n} shape {s}")
                verts.append(q)
                counts.append(len(q))
            shape_rings.append(len(counts))
        image_shapes.append(len(shape_rings) - 1)
    if not 1 <= len(image_shapes) - 1 <= 65535:
        raise ValueError(f"from_rings: a set holds 1 to 65535 images, got {len(image_shapes) - 1}")
    v = np.concatenate(verts, 0) if verts else np.zeros((0, 2), np.int64)
    if len(v) >= 1 << 31:
        raise ValueError("from_rings: a set holds fewer than 2^31 vertices")
    counts = np.asarray(counts, np.int64)
    start = np.concatenate([[0], np.cumsum(counts)[:-1]]) if len(counts) else np.zeros((0,), np.int64)
    if properties is not None and len(properties) != len(shape_rings) - 1:
        raise ValueError(f"from_rings: {len(properties)} properties for {len(shape_rings) - 1} shapes")
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.int64).astype(np.int32)))
    return PolygonSet(i32(v).reshape(-1, 2), i32(start), i32(counts), i32(shape_rings), i32(image_shapes), sub,
                      None if properties is None else list(properties))


def _geometries(obj, ignore_other, props=None):
    """(rings of one shape, properties) for every Polygon / MultiPolygon under ``obj``"""
    if isinstance(obj, (list, tuple)):
        for o in obj:
            yield from _geometries(o, ignore_other, props)
        return
    if not isinstance(obj, dict):
        raise TypeError(f"from_geojson: expected a GeoJSON object (a dict) or a list of them, got {type(obj).__name__}")
    kind = obj.get("type")
    if kind == "FeatureCollection":
        for f in obj.get("features", ()):
            yield from _geometries(f, ignore_other)
    elif kind == "Feature":
        g = obj.get("geometry")
        if g is None:
            if not ignore_other:
                raise ValueError("from_geojson: a Feature without a geometry (ignore_other=True skips it)")
            return
        yield from _geometries(g, ignore_other, obj.get("properties"))
    elif kind == "Polygon":
        yield list(obj.get("coordinates", ())), props
    elif kind == "MultiPolygon":
        yield [ring for part in obj.get("coordinates", ()) for ring in part], props
    elif not ignore_other:
        raise ValueError(f"from_geojson: geometry type {kind!r} is not read: Polygon and MultiPolygon are (ignore_other=True skips it)")


def from_geojson(obj, origin=(0, 0), scale=1.0, sub=4, ignore_other=False):
    """The shapes of ONE image from GeoJSON -> a host ``PolygonSet``.  ``obj``: a ``FeatureCollection``, a ``Feature``, a bare
    geometry, or a list of those.  ``Polygon`` and ``MultiPolygon`` are read, one shape each: the rings after a polygon's first
    (its holes) and the parts of a multi-polygon are further rings of the same shape.  Any other geometry type raises
    ``ValueError`` naming it, unless ``ignore_other`` is set.  The mapping is the inverse of ``ContourTable.geojson``:
    ``col = (x - origin[0]) / scale``, ``row = (y - origin[1]) / scale`` in float64, then quantised as in ``from_rings``.  Each
    feature's ``properties`` is kept per shape (None for a bare geometry)."""
    sub = _check_sub(sub, "from_geojson")
    ox, oy, scale = float(origin[0]), float(origin[1]), float(scale)
    if not scale > 0:
        raise ValueError(f"from_geojson: scale must be positive, got {scale!r}")
    shapes, props = [], []
    for rings, p in _geometries(obj, ignore_other):
        out = []
        for ring in rings:
            xy = np.asarray(ring, np.float64).reshape(len(ring), -1)[:, :2] if len(ring) else np.zeros((0, 2))
            out.append(np.stack([(xy[:, 1] - oy) / scale, (xy[:, 0] - ox) / scale], 1))
        shapes.append(out)
        props.append(p)
    return from_rings([shapes], sub=sub, properties=props)


def from_contours(ct):
    """Every traced ring of a ``regions.ContourTable`` on the device -> a device ``PolygonSet`` with ``sub=0`` and one ring per
    shape, reading ``ct.vertices`` where it lies.  ``ring_count`` is ``n_vertices`` where ``0 < n_vertices <= max_vertices``,
    else 0: unused, too-large and truncated rows draw nothing.  ``image_shapes = arange(N + 1) * cap``, so the ring of label
    k + 1 paints k + 1.  Torch indexing only, no synchronisation: ``from_contours`` + ``rasterize`` can be captured into a graph."""
    if getattr(ct, "vertices", None) is None or not torch.is_tensor(ct.vertices) or ct.vertices.dim() != 4:
        raise ValueError("from_contours: expected a ContourTable with vertices (contour_labels with max_vertices > 0)")
    if not ct.vertices.is_cuda:
        raise ValueError("from_contours: the ContourTable must live on the device (PolygonSet.to moves a host set)")
    N, cap, maxv, _ = (int(v) for v in ct.vertices.shape)
    if N * cap * maxv >= 1 << 31 or N * cap + 1 >= 1 << 31:
        raise ValueError(f"from_contours: {N} x {cap} rings of {maxv} slots pass 2^31 vertices")
    dev = ct.vertices.device
    nv = ct.contour[..., 0].reshape(-1)
    count = torch.where((nv > 0) & (nv <= maxv), nv, torch.zeros_like(nv))
    rings = torch.arange(N * cap + 1, dtype=torch.int32, device=dev)
    return PolygonSet(ct.vertices.reshape(-1, 2), rings[:-1] * maxv, count, rings,
                      torch.arange(N + 1, dtype=torch.int32, device=dev) * cap, 0)


def _check_set(pset):
    """dtypes and shapes of every set; offsets and coordinates of a host set -> True where the set lies on the host"""
    if not isinstance(pset, PolygonSet):
        raise TypeError(f"rasterize: expected a PolygonSet, got {type(pset).__name__}")
    sub = _check_sub(pset.sub, "rasterize")
    tabs = [getattr(pset, k) for k in _TABLES]
    for k, t in zip(_TABLES, tabs):
        if not torch.is_tensor(t) or t.dtype != torch.int32:
            raise TypeError(f"rasterize: {k} must be an int32 tensor, got {getattr(t, 'dtype', type(t).__name__)}")
    if len({t.device for t in tabs}) != 1:
        raise ValueError("rasterize: the tensors of a PolygonSet live all on the host or all on one device")
    v, start, count, srings, ishapes = tabs
    if v.dim() != 2 or v.shape[1] != 2 or start.dim() != 1 or count.shape != start.shape or srings.dim() != 1 or ishapes.dim() != 1 \
            or srings.numel() < 1 or ishapes.numel() < 2:
        raise ValueError("rasterize: vertices [V, 2], ring_start and ring_count [R], shape_rings [S + 1], image_shapes [N + 1], "
                         f"got {[tuple(t.shape) for t in tabs]}")
    if v.shape[0] >= 1 << 31:
        raise ValueError("rasterize: a set holds fewer than 2^31 vertices")
    host = not v.is_cuda
    if host:
        V, R, S = int(v.shape[0]), int(start.numel()), int(srings.numel()) - 1
        st, ct, sr, im = (t.numpy().astype(np.int64) for t in (start, count, srings, ishapes))
        if (ct < 0).any() or (st < 0).any() or (st + ct > V).any():
            raise ValueError("rasterize: a ring leaves the vertex table (ragged ring_start / ring_count)")
        if sr[0] != 0 or sr[-1] != R or (np.diff(sr) < 0).any():
            raise ValueError(f"rasterize: shape_rings must rise from 0 to the number of rings ({R})")
        if im[0] != 0 or im[-1] != S or (np.diff(im) < 0).any():
            raise ValueError(f"rasterize: image_shapes must rise from 0 to the number of shapes ({S})")
        if V and int(v.abs().max()) > K.POLYGON_MAX_COORD:
            raise ValueError(f"rasterize: a quantised coordinate leaves [-2^28, 2^28] at sub={sub}")
    return host


def plan(pset, image_hw, band_rows=None):
    """The item table of a host-side set -> int32 [I, 3] = (shape, first row, rows) on the host: every shape's rows, cut to the
    image -- the rows i whose centre line lies at or below the shape's smallest vertex row and above its largest -- in bands of at
    most ``band_rows`` rows, in shape order.  Each clipped row of each shape lies in exactly one item."""
    if _check_set(pset) is not True:
        raise ValueError("plan: the planner reads a host-side set")
    return _plan(pset, image_hw, band_rows)


def _plan(pset, image_hw, band_rows):
    H, W = (int(v) for v in image_hw)
    band = BAND_ROWS if band_rows is None else band_rows
    if isinstance(band, bool) or not isinstance(band, (int, np.integer)) or band < 1:
        raise ValueError(f"band_rows must be a positive integer, got {band_rows!r}")
    sub = int(pset.sub)
    v, start, count, srings = (getattr(pset, k).numpy().astype(np.int64) for k in _TABLES[:4])
    before = np.concatenate([[0], np.cumsum(count)])
    per_shape = before[srings[1:]] - before[srings[:-1]]                   # vertices of every shape
    total = int(count.sum())
    # the vertex rows of every ring in ring order, which is shape order
    first = np.cumsum(count) - count
    rows = v[np.repeat(start - first, count) + np.arange(total), 0] if total else np.zeros((0,), np.int64)
    some = np.nonzero(per_shape > 0)[0]
    voff = (np.cumsum(per_shape) - per_shape)[some]
    lo = np.minimum.reduceat(rows, voff) if len(some) else np.zeros((0,), np.int64)
    hi = np.maximum.reduceat(rows, voff) if len(some) else np.zeros((0,), np.int64)
    # centre line Y = (2 i + 1) S against y = 2 row: the first i with Y >= y is floor((2 row + S - 1) / (2 S))
    first_row = lambda r: (2 * r + (1 << sub) - 1) >> (sub + 1)
    r0, r1 = np.clip(first_row(lo), 0, H), np.clip(first_row(hi), 0, H)
    live = r1 > r0
    some, r0, r1 = some[live], r0[live], r1[live]
    bands = -(-(r1 - r0) // band)
    shape = np.repeat(some, bands)
    k = np.arange(int(bands.sum())) - np.repeat(np.cumsum(bands) - bands, bands)
    at = np.repeat(r0, bands) + k * band
    n = np.minimum(band, np.repeat(r1, bands) - at)
    return np.stack([shape, at, n], 1).astype(np.int32).reshape(-1, 3)


def rasterize(pset, image_hw, mode="labels", rule="evenodd", values=None, out=None, clear=True, device=None, _band_rows=None):
    """The shapes of a ``PolygonSet`` as pixels -> int32 (``mode="labels"``) or uint8 (``mode="mask"``) [N, H, W] on the device.

    The rule is exact; no float decides a pixel.  Vertices are fixed-point: (row, col) integers in units of ``1/S`` pixel, with
    ``S = 2**sub`` and ``sub`` in 0..8; ``sub = 0`` is the lattice of ``contour_labels``.  Pixel (i, j) is the closed unit square
    with corners (i, j) and (i+1, j+1), as in ``hull_labels`` and ``contour_labels``.  Its centre decides.  In units of ``1/(2S)``
    the centre is ``Y = (2i+1)S``, ``X = (2j+1)S``; a vertex (R, C) is ``y = 2R``, ``x = 2C`` in the same units.

    For every edge a -> b of every ring of a shape, the closing edge last -> first included, let ``d = yb - ya`` and
    ``cross = (xb - xa)(Y - ya) - (X - xa) d``, in 64-bit integers.  The edge counts for the pixel when both of these hold:
    ``(ya <= Y) != (yb <= Y)``; and ``d > 0 and cross <= 0``, or ``d < 0 and cross >= 0``.  That is the ray from the centre
    towards smaller columns.  A counting edge weighs +1 if ``d > 0``, else -1.  The winding number of the pixel is the sum over
    all rings of the shape.  ``rule="evenodd"``, the default, takes the pixel when the winding number is odd; ``rule="nonzero"``
    takes it when the winding number is not 0.

    What follows: a centre that lies exactly on an edge or a vertex belongs to the side towards larger columns or larger rows
    (top- and left-inclusive, bottom- and right-exclusive), so two shapes that share an edge neither overlap nor leave a gap.
    Holes and the parts of a multi-polygon are further rings of the same shape.  Rings of fewer than 3 vertices, zero-area rings,
    repeated vertices and horizontal edges contribute nothing, by the rule itself.  Vertices may lie outside the image; only the
    pixels of the image are written.  For a ring traced by ``contour_labels``, at either connectivity, both rules give the ring's
    interior; for a label with ``is_simple()`` that is exactly the label's pixels.

    Overlaps: shape s of image n paints label ``s - image_shapes[n] + 1`` and the highest label wins (an integer maximum, so the
    result does not depend on the order of arrival); ``mode="mask"`` writes 1 where any shape covers the pixel.  ``values``: int32,
    one per shape of the set, written in place of the label (a gather after the kernel; labels only); the highest shape index
    still wins.  ``out``: a buffer to write, of the result's dtype and shape, contiguous, on the device; ``clear=False`` paints onto
    what it holds: labels by ``max`` (with ``values``: the larger of the value and what the pixel held, where a shape covers it),
    the mask by ``or``.

    A host-side set is checked (ragged offsets, coordinates within [-2^28, 2^28]), planned by ``plan`` -- every shape's clipped
    rows in bands of ``BAND_ROWS``, so a slide-sized outline spreads over the device; ``_band_rows`` overrides it for the tests --
    and uploaded to ``device``.  A device-side set (``from_contours``) goes as it is, one workgroup per shape, without a plan and
    without a synchronisation.  Limits: N <= 65535, H W < 2^31, ``max(H, W) << (sub + 1) < 2^30``.  Every argument error is raised
    before the library is loaded or the device is touched."""
    if rule not in RULES:
        raise ValueError(f"rasterize: rule must be one of {sorted(RULES)}, got {rule!r}")
    if mode not in MODES:
        raise ValueError(f"rasterize: mode must be one of {sorted(MODES)}, got {mode!r}")
    host = _check_set(pset)
    try:
        H, W = (int(v) for v in image_hw)
    except (TypeError, ValueError):
        raise TypeError(f"rasterize: image_hw must be a pair (H, W), got {image_hw!r}") from None
    N = pset.n_images
    K.polygons_check_size("rasterize", N, H, W, int(pset.sub))
    S = pset.n_shapes
    if values is not None:
        if mode != "labels":
            raise ValueError("rasterize: values replace labels: mode must be 'labels'")
        if torch.is_tensor(values):
            if values.dtype != torch.int32:
                raise TypeError(f"rasterize: values must be int32, got {values.dtype}")
        else:
            values = np.asarray(values)
            if values.dtype.kind not in "iu" or (values.size and (values.min() < -(1 << 31) or values.max() >= 1 << 31)):
                raise TypeError(f"rasterize: values must be int32, got {values.dtype}")
            values = torch.from_numpy(values.astype(np.int32))
        if values.dim() != 1 or values.numel() != S:
            raise ValueError(f"rasterize: values must hold one entry per shape ({S}), got shape {tuple(values.shape)}")
    if out is not None:
        if not torch.is_tensor(out) or out.dtype != MODES[mode] or tuple(out.shape) != (N, H, W):
            raise TypeError(f"rasterize: out must be {MODES[mode]} of shape {(N, H, W)}, got "
                            f"{getattr(out, 'dtype', type(out).__name__)} {tuple(getattr(out, 'shape', ()))}")
        if not out.is_cuda or not out.is_contiguous():
            raise ValueError("rasterize: out must be a contiguous device tensor")
        if device is not None and torch.device(device).type != "cuda":
            raise ValueError(f"rasterize: device must be a GPU, got {device!r}")
    items = None
    if host:
        items = _plan(pset, (H, W), _band_rows)
        device = out.device if out is not None else torch.device("cuda" if device is None else device)
        if device.type != "cuda":
            raise ValueError(f"rasterize: device must be a GPU, got {device!r}")
    else:
        if _band_rows is not None:
            raise ValueError("rasterize: a device-side set goes without a plan: _band_rows does not apply")
        device = pset.vertices.device
        if out is not None and out.device != device:
            raise ValueError("rasterize: out must live on the device of the set")

    # ---- the device from here on
    tabs = [getattr(pset, k).to(device).contiguous() for k in _TABLES]
    if items is not None:
        items = torch.from_numpy(items).to(device)
    if values is None:
        if out is None:
            out = torch.zeros((N, H, W), dtype=MODES[mode], device=device)
        elif clear:
            out.zero_()
        return K.polygons_rasterize(*tabs, out, int(pset.sub), RULES[rule], items)
    index = K.polygons_rasterize(*tabs, torch.zeros((N, H, W), dtype=torch.int32, device=device), int(pset.sub), RULES[rule], items)
    covered = index > 0
    shape = (index.long() - 1 + tabs[4][:-1].long()[:, None, None]).clamp_(0, max(S - 1, 0))
    painted = values.to(device)[shape] if S else torch.zeros_like(index)
    if out is None:
        return torch.where(covered, painted, torch.zeros_like(painted))
    if clear:
        out.copy_(torch.where(covered, painted, torch.zeros_like(painted)))
    else:
        out.copy_(torch.where(covered, torch.maximum(out, painted), out))
    return out


def roi_mask(roi, image_hw):
    """``detect_slide``'s ``roi``, checked on the host -> ``make``: ``make(device)`` gives the device uint8 [H, W] mask of 0 / 1.
    ``roi``: a ``PolygonSet`` of one image, a GeoJSON object (``from_geojson`` with its defaults), or a uint8 / bool [H, W] mask
    (numpy or torch; non-zero = inside).  A host-side set goes to ``rasterize`` as it is, so that it is planned: a slide-sized
    outline is cut into bands.  Only a set that already lives on the device goes without a plan."""
    H, W = image_hw
    if isinstance(roi, (dict, list, tuple)):
        roi = from_geojson(roi)
    if isinstance(roi, PolygonSet):
        _check_set(roi)
        if roi.n_images != 1:
            raise ValueError(f"detect_slide: roi must hold the shapes of one image, got {roi.n_images}")
        K.polygons_check_size("detect_slide: roi", 1, H, W, int(roi.sub))
        return lambda device: rasterize(roi, (H, W), mode="mask", device=None if roi.vertices.is_cuda else device)[0]
    m = torch.from_numpy(roi) if isinstance(roi, np.ndarray) else roi
    if not torch.is_tensor(m) or m.dtype not in (torch.uint8, torch.bool) or tuple(m.shape) != (H, W):
        raise TypeError(f"detect_slide: roi must be a PolygonSet, a GeoJSON object or a uint8 / bool mask shaped {(H, W)}, got "
                        f"{type(roi).__name__} {tuple(getattr(roi, 'shape', ()))}")
    return lambda device: (m.to(device) != 0).to(torch.uint8).contiguous()
