"""Pure-numpy restatement of the small-region clean-up (utils/image_processing.py:14-17 and the scikit-image / scipy functions it
calls), the reference of tests/test_regions_gpu.py and tools/regions_microbench.py.  Pinned to scipy.ndimage.label by
tests/golden/regions_vectors.npz (tests/test_regions_host.py); scipy is not imported here.

Labelling is run-based: the horizontal runs of True pixels are the nodes, runs of neighbouring rows that touch (connectivity 1:
share a column; connectivity 2: share a column or are diagonal neighbours) are united, the smaller run index becoming the parent.
Runs are found in row-major order, so the root of a component is the run that holds its lowest pixel, and numbering the roots in
index order is scipy's numbering.
"""
import numpy as np


def _runs(m):
    """(row, start, end) of every horizontal run of True pixels, row-major; end is exclusive."""
    H, W = m.shape
    p = np.zeros((H, W + 2), np.int8)
    p[:, 1:-1] = m
    d = np.diff(p, axis=1)
    rows, starts = np.nonzero(d == 1)
    ends = np.nonzero(d == -1)[1]
    return rows, starts, ends


def label(m, connectivity=1):
    """scipy.ndimage.label of a 2-D boolean array: (int32 labels, number of components)."""
    m = np.asarray(m)
    if m.dtype != np.bool_ or m.ndim != 2:
        raise TypeError("label expects a 2-D boolean array")
    if connectivity not in (1, 2):
        raise ValueError("connectivity must be 1 or 2")
    H, W = m.shape
    rows, starts, ends = _runs(m)
    n = len(rows)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    first = np.searchsorted(rows, np.arange(H + 1))        # runs of row r: first[r] .. first[r + 1]
    reach = connectivity - 1
    S, E = starts.tolist(), ends.tolist()
    for r in range(1, H):
        a, a_end = first[r - 1], first[r]
        b, b_end = first[r], first[r + 1]
        while a < a_end and b < b_end:
            if S[a] < E[b] + reach and S[b] < E[a] + reach:
                ra, rb = find(a), find(b)
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)
            if E[a] < E[b]:
                a += 1
            else:
                b += 1
    number = np.zeros(n, np.int64)
    count = 0
    for i in range(n):
        root = find(i)
        if root == i:
            count += 1
            number[i] = count
        else:
            number[i] = number[root]
    flat = np.zeros(H * W + 1, np.int64)
    lo = rows * W + starts
    hi = rows * W + ends
    np.add.at(flat, lo, number)
    np.add.at(flat, hi, -number)
    return np.cumsum(flat[:-1]).reshape(H, W).astype(np.int32), count


def component_areas(m, connectivity=1):
    """int32 map: under every pixel, the pixel count of the component of equal-valued pixels it lies in (foreground components
    under True pixels, background components under False pixels)."""
    m = np.asarray(m)
    out = np.zeros(m.shape, np.int32)
    for v in (m, ~m):
        lab, _ = label(v, connectivity)
        out[v] = np.bincount(lab.ravel())[lab[v]]
    return out


def remove_small_objects(m, min_size=64, connectivity=1):
    m = np.asarray(m)
    if min_size == 0:
        return m.copy()
    lab, _ = label(m, connectivity)
    small = np.bincount(lab.ravel()) < min_size
    small[0] = False
    out = m.copy()
    out[small[lab]] = False
    return out


def remove_small_holes(m, area_threshold=64, connectivity=1):
    return ~remove_small_objects(~np.asarray(m), area_threshold, connectivity)


def remove_small_regions(img_bin, min_object_size, hole_area_threshold, connectivity=1):
    """utils/image_processing.py:14-17 (the reference leaves connectivity at 1)."""
    return remove_small_holes(remove_small_objects(img_bin, min_object_size, connectivity), hole_area_threshold, connectivity)


def batched(fn, m, *args, **kw):
    """fn over [H, W] or every image of [N, H, W]; a function that returns (array, count) keeps the array."""
    m = np.asarray(m)
    one = lambda x: (lambda r: r[0] if isinstance(r, tuple) else r)(fn(x, *args, **kw))  # noqa: E731
    return one(m) if m.ndim == 2 else np.stack([one(x) for x in m])


def hsv_gate(images_u8, masks, v_max=170):
    """image_processing.py:117-120: mask & (V <= 170), V = the channel maximum (cv2's 8-bit HSV value)."""
    return np.logical_and(np.asarray(masks) != 0, np.asarray(images_u8).max(axis=-1) <= v_max)


def preprocess_masks(images_u8, masks, min_object_size=400, hole_area_threshold=120):
    """image_processing.py:114-124 over [H, W] or [N, H, W]."""
    return batched(remove_small_regions, hsv_gate(images_u8, masks), min_object_size, hole_area_threshold)


# ---- shapes shared by the golden vectors, the GPU tests and the microbenchmark ---------------------------------------------------
def blobs(n, H, W, seed, density=1 / 400.0, holes=True):
    """n boolean maps of overlapping discs (radius 2-14) with small discs punched out: objects and holes either side of the
    reference's thresholds (300 / 100 and 400 / 120)."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[:H, :W]
    out = np.zeros((n, H, W), bool)
    for i in range(n):
        k = max(1, int(H * W * density))
        for cy, cx, r in zip(rng.randint(0, H, k), rng.randint(0, W, k), rng.uniform(2, 14, k)):
            y0, y1, x0, x1 = max(0, int(cy - r)), min(H, int(cy + r) + 1), max(0, int(cx - r)), min(W, int(cx + r) + 1)
            out[i, y0:y1, x0:x1] |= (yy[y0:y1, x0:x1] - cy) ** 2 + (xx[y0:y1, x0:x1] - cx) ** 2 <= r * r
        if holes:
            for cy, cx, r in zip(rng.randint(0, H, k), rng.randint(0, W, k), rng.uniform(1, 7, k)):
                y0, y1, x0, x1 = max(0, int(cy - r)), min(H, int(cy + r) + 1), max(0, int(cx - r)), min(W, int(cx + r) + 1)
                out[i, y0:y1, x0:x1] &= (yy[y0:y1, x0:x1] - cy) ** 2 + (xx[y0:y1, x0:x1] - cx) ** 2 > r * r
    return out


def serpentine(H, W):
    """One 1-pixel-wide path: every even row is full, odd rows hold one pixel at alternating ends.  The foreground is ONE
    component of area ceil(H / 2) W + floor(H / 2); with W >= 2 the background is floor(H / 2) components of W - 1 pixels (each odd
    row's remainder), for connectivity 1 and 2 alike (the rows either side are full)."""
    m = np.zeros((H, W), bool)
    m[0::2] = True
    m[1::4, W - 1] = True
    m[3::4, 0] = True
    return m
