"""Plain-loop restatement of the per-label contour polygons (cellsegmentation_amd.regions.contour_labels / ContourTable), the
reference of tests/test_contour_gpu.py.  The rule, as the docstring of ``regions.contour_labels`` states it:

* a pixel's object id is max(label, 0); images of a batch are independent; pixel (r, c) is the closed unit square with the lattice
  corners (r, c) and (r + 1, c + 1); the object of label l is the pixels with id l inside the label's box (cut to the image), and
  everything else, other labels and pixels outside the box included, is "not the object";
* the ring starts at the lattice vertex (pr, pc) of the object's first pixel in row-major order, heading east along that pixel's
  top side, the object on the right hand;
* a step moves one crack along the heading; at the vertex (r, c) reached, R is the pixel ahead on the right and L the one ahead
  on the left (E: R = (r, c), L = (r - 1, c); S: R = (r, c - 1), L = (r, c); W: R = (r - 1, c - 1), L = (r, c - 1); N:
  R = (r - 1, c), L = (r - 1, c - 1)); R out: turn right, but with connectivity 2 and L in turn left; R and L in: turn left;
  R in, L out: straight on;
* the walk stops on arriving at (pr, pc) with the new heading east, and in any case after 2 rows cols + rows + cols steps;
* a vertex is emitted where the heading changes, the start vertex first;
* per label: n_vertices, n_cracks (the ring's length), area2 (the shoelace sum sum(c_i r_{i+1} - c_{i+1} r_i)), cracks_all (the
  (pixel of the object, side) pairs whose neighbour across the side is not in the object); a box of more than MAX_SIDE rows or
  columns: all -1; a label without a pixel in its box: all zero; vertex slots that are not used hold (-1, -1).

Pinned to scipy.ndimage.binary_fill_holes by tests/golden/contour_vectors.npz (tests/test_contour_host.py); scipy is not imported
here.  Row k of image n is label k + 1; rows of labels above the capacity do not exist.
"""
import numpy as np

import shape_ref as SR

MAX_SIDE = 512
COLUMNS = ("n_vertices", "crack_perimeter", "enclosed_area", "hole_area")
STEP = ((0, 1), (1, 0), (0, -1), (-1, 0))                                 # E, S, W, N
RIGHT = ((0, 0), (0, -1), (-1, -1), (-1, 0))                              # R of a heading, relative to the vertex; L of h is R of h - 1


def trace(obj, connectivity=1):
    """bool [rows, cols], the object inside its box -> (ring: list of (r, c) relative to the box, n_cracks, area2, hit_bound), or
    None where the box holds no pixel of the object"""
    rows, cols = obj.shape

    def inside(r, c):
        return 0 <= r < rows and 0 <= c < cols and bool(obj[r, c])

    start = next(((r, c) for r in range(rows) for c in range(cols) if obj[r, c]), None)
    if start is None:
        return None
    pr, pc = start
    r, c, h = pr, pc, 0
    ring, cracks, bound = [(pr, pc)], 0, 2 * rows * cols + rows + cols
    closed = False
    while cracks < bound:
        r, c = r + STEP[h][0], c + STEP[h][1]
        cracks += 1
        R = inside(r + RIGHT[h][0], c + RIGHT[h][1])
        L = inside(r + RIGHT[h - 1][0], c + RIGHT[h - 1][1])
        if not R:
            nh = (h + 3) % 4 if connectivity == 2 and L else (h + 1) % 4
        elif L:
            nh = (h + 3) % 4
        else:
            nh = h
        if (r, c) == (pr, pc) and nh == 0:
            closed = True
            break
        if nh != h:
            ring.append((r, c))
            h = nh
    n = len(ring)
    area2 = sum(ring[i][1] * ring[(i + 1) % n][0] - ring[(i + 1) % n][1] * ring[i][0] for i in range(n))
    return ring, cracks, area2, not closed


def cracks_all(obj):
    """bool [rows, cols] -> the number of (pixel of the object, side) pairs whose neighbour across the side is not in the object"""
    rows, cols = obj.shape
    total = 0
    for r in range(rows):
        for c in range(cols):
            if obj[r, c]:
                for dr, dc in STEP:
                    rr, cc = r + dr, c + dc
                    total += not (0 <= rr < rows and 0 <= cc < cols and obj[rr, cc])
    return total


def fill(ring, shape):
    """a ring of lattice vertices with axis-parallel edges -> bool [H, W]: the pixels whose centre has a non-zero winding number.
    The ray from the centre of pixel (i, j) towards smaller columns crosses the vertical edges at columns <= j that span row
    i + 1/2; one running down counts +1, one running up -1."""
    wind = np.zeros(shape, np.int64)
    n = len(ring)
    for k in range(n):
        (ra, ca), (rb, cb) = ring[k], ring[(k + 1) % n]
        if ca != cb:
            continue
        lo, hi, sign = (ra, rb, 1) if rb > ra else (rb, ra, -1)
        wind[lo:hi, ca:] += sign
    return wind != 0


def _one(lab, cap, bbox, connectivity):
    """one [H, W] label image and its boxes [cap, 4] -> (contour [cap, 4], the cap complete rings in absolute coordinates (None
    where none was traced), hit_bound bool [cap])"""
    H, W = lab.shape
    contour = np.zeros((cap, 4), np.int32)
    rings, hit = [None] * cap, np.zeros(cap, bool)
    for k in range(cap):
        r0, c0 = max(int(bbox[k, 0]), 0), max(int(bbox[k, 1]), 0)
        r1, c1 = min(int(bbox[k, 2]), H), min(int(bbox[k, 3]), W)
        if r1 - r0 <= 0 or c1 - c0 <= 0:
            continue
        if max(r1 - r0, c1 - c0) > MAX_SIDE:
            contour[k] = -1
            continue
        obj = lab[r0:r1, c0:c1] == k + 1
        got = trace(obj, connectivity)
        if got is None:
            continue
        ring, cracks, area2, hit[k] = got
        ring = [(r + r0, c + c0) for r, c in ring]
        contour[k] = (len(ring), cracks, area2, cracks_all(obj))
        rings[k] = ring
    return contour, rings, hit


def contour_labels(labels, max_regions=None, connectivity=1, max_vertices=None, bbox=None):
    """labels int [H, W] or [N, H, W] -> dict: counts, capacity, area, bbox, sum_rc as shape_ref.shape_labels gives them, contour
    int32 [N, cap, 4], vertices int32 [N, cap, max_vertices, 2] (max_vertices None: max(4, the largest n_vertices)), rings (per
    image a list of cap complete rings, None where none was traced), hit_bound bool [N, cap], connectivity.  ``bbox``: boxes to
    trace in, int [N, cap, 4], in place of the labels' own."""
    assert connectivity in (1, 2)
    labels = np.asarray(labels)
    ls = labels[None] if labels.ndim == 2 else labels
    t = SR.shape_labels(labels, max_regions)
    out = {k: t[k] for k in ("counts", "capacity", "area", "bbox", "sum_rc")}
    cap = out["capacity"]
    boxes = out["bbox"] if bbox is None else np.asarray(bbox)
    assert boxes.shape == (len(ls), cap, 4)
    per = [_one(x, cap, boxes[n], connectivity) for n, x in enumerate(ls)]
    top = max(4, max(int(p[0][:, 0].max()) for p in per)) if max_vertices is None else int(max_vertices)
    out["contour"] = np.stack([p[0] for p in per])
    out["vertices"] = np.full((len(ls), cap, top, 2), -1, np.int32)
    for n, p in enumerate(per):
        for k, ring in enumerate(p[1]):
            m = 0 if ring is None else min(len(ring), top)
            if m:
                out["vertices"][n, k, :m] = ring[:m]
    out["rings"] = [p[1] for p in per]
    out["hit_bound"] = np.stack([p[2] for p in per])
    out["connectivity"] = connectivity
    return out


def contours(m, connectivity=1, max_regions=None, max_vertices=None):
    """``contour_labels`` of the components of a boolean mask, numbered as scipy.ndimage.label (regions_ref.label)"""
    import regions_ref as R
    m = np.asarray(m)
    lab = np.stack([R.label(x, connectivity)[0] for x in m]) if m.ndim == 3 else R.label(m, connectivity)[0]
    return contour_labels(lab.astype(np.int32), max_regions, connectivity, max_vertices)


# ---- the columns of ContourTable, from the integer tables only -------------------------------------------------------------------
def too_large(t):
    return t["contour"][..., 0] < 0


def _ok(t):
    return (t["area"] > 0) & (t["contour"][..., 0] > 0)


def _measured(t, x):
    return np.where(_ok(t), x, np.nan)


def truncated(t):
    return t["contour"][..., 0] > t["vertices"].shape[2]


def is_simple(t):
    return _ok(t) & (t["contour"][..., 1] == t["contour"][..., 3])


def n_vertices(t):
    return _measured(t, t["contour"][..., 0].astype(np.float64))


def crack_perimeter(t):
    return _measured(t, t["contour"][..., 1].astype(np.float64))


def enclosed_area(t):
    return _measured(t, t["contour"][..., 2].astype(np.float64) / 2)


def hole_area(t):
    return enclosed_area(t) - t["area"].astype(np.float64)


def columns(t):
    """name -> float64 array, one per float method of ContourTable"""
    return {k: globals()[k](t) for k in COLUMNS}
