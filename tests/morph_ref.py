"""Host restatement (numpy) of cellsegmentation_amd.morph: the nearest-site transform, disk morphology and label expansion.

The rule: every pixel gets the nearest site (exact squared Euclidean distance), and among equally near sites the one with the
lowest row-major index.  ``nearest`` is the separable scheme the device runs -- per column the nearest site of the column, the one
above on a tie; per row the smallest key ``d2 * H * W + site`` over the columns -- and ``nearest_brute`` the definition, pixel by
pixel, for small maps.  The distances and the morphology are pinned to scipy by tests/golden/morph_vectors.npz."""
import numpy as np

NONE = np.int64(1) << 40          # vertical distance in a column without a site
KEY_MATRIX_MAX_W = 128            # wider rows are searched offset by offset instead of through a W x W matrix


def column_sites(sites):
    """sites bool [H, W] -> (g int64 [H, W] vertical distance to the nearest site of the column, NONE without one; row int64 [H, W]
    that site's row).  Of a site above and one below that are equally far, the one above."""
    H, W = sites.shape
    g = np.full((H, W), NONE, np.int64)
    row = np.full((H, W), -1, np.int64)
    last = np.full(W, -1, np.int64)
    for y in range(H):
        last = np.where(sites[y], y, last)
        ok = last >= 0
        g[y] = np.where(ok, y - last, NONE)
        row[y] = last
    nxt = np.full(W, -1, np.int64)
    for y in range(H - 1, -1, -1):
        nxt = np.where(sites[y], y, nxt)
        better = (nxt >= 0) & (nxt - y < g[y])           # strictly nearer only
        g[y] = np.where(better, nxt - y, g[y])
        row[y] = np.where(better, nxt, row[y])
    return g, row


def nearest(sites, limit=None):
    """sites bool [H, W] -> (d2 int32 [H, W], site int32 [H, W]); -1 / -1 everywhere without any site.  ``limit``: the caller only
    asks which pixels have d2 <= limit (and their sites); the search stops at dx^2 > limit, the answer is exact wherever d2 <= limit
    and some value above the limit elsewhere."""
    sites = np.asarray(sites, bool)
    H, W = sites.shape
    assert H * H + W * W < 2 ** 31
    if not sites.any():
        return np.full((H, W), -1, np.int32), np.full((H, W), -1, np.int32)
    g, row = column_sites(sites)
    big = np.int64(H) * W
    none_key = np.int64(2) ** 31 * big
    cols = np.arange(W, dtype=np.int64)
    g2 = np.where(g >= NONE, np.int64(2) ** 31, g * g)                        # no finite d2 reaches 2^31
    if limit is None and W <= KEY_MATRIX_MAX_W:
        dx2 = (cols[:, None] - cols[None, :]) ** 2                              # [x, x']
        best = np.empty((H, W), np.int64)
        for y in range(H):
            key = np.where(g[y] >= NONE, none_key, (dx2 + g2[y][None, :]) * big + (row[y] * W + cols)[None, :])
            best[y] = key.min(axis=1)
    else:
        # the same minimum, one offset at a time, until dx^2 exceeds every distance still standing (<=: a site at dx^2 == d2 ties)
        base = np.where(g >= NONE, none_key, g2 * big + row * W + cols[None, :])
        best = base.copy()
        for dx in range(1, W):
            if dx * dx > int(best.max() // big) or (limit is not None and dx * dx > limit):
                break
            shifted = base + np.int64(dx * dx) * big
            ok_l = g[:, :-dx] < NONE
            best[:, dx:] = np.minimum(best[:, dx:], np.where(ok_l, shifted[:, :-dx], none_key))
            ok_r = g[:, dx:] < NONE
            best[:, :-dx] = np.minimum(best[:, :-dx], np.where(ok_r, shifted[:, dx:], none_key))
    found = best < none_key                                                     # only a limited search leaves pixels without a site
    assert limit is not None or found.all()
    d2, site = np.where(found, best // big, 2 ** 31 - 1), np.where(found, best % big, -1)
    return d2.astype(np.int32), site.astype(np.int32)


def nearest_brute(sites):
    """the definition: for every pixel the smallest (d2, row-major index) over all sites (tiny maps)"""
    sites = np.asarray(sites, bool)
    H, W = sites.shape
    sy, sx = np.nonzero(sites)                          # row-major order
    d2 = np.full((H, W), -1, np.int32)
    site = np.full((H, W), -1, np.int32)
    if len(sy) == 0:
        return d2, site
    for y in range(H):
        for x in range(W):
            d = (sy - y) ** 2 + (sx - x) ** 2
            k = int(np.argmin(d))                       # the first minimum: the lowest index
            d2[y, x] = d[k]
            site[y, x] = sy[k] * W + sx[k]
    return d2, site


def _d2(sites, outside, limit):
    """int64 squared distance to the nearest site (exact up to ``limit``), the pixels beyond the edge counting as sites with
    ``outside``; NONE without any"""
    H, W = sites.shape
    d2 = nearest(sites, limit)[0].astype(np.int64)
    d2 = np.where(d2 < 0, NONE, d2)
    if outside:
        yy, xx = np.mgrid[0:H, 0:W].astype(np.int64)
        edge = np.minimum(np.minimum(yy + 1, H - yy), np.minimum(xx + 1, W - xx))
        d2 = np.minimum(d2, edge * edge)
    return d2


def binary_dilation(m, r2, border_value=0):
    m = np.asarray(m, bool)
    return _d2(m, border_value == 1, r2) <= r2


def binary_erosion(m, r2, border_value=0):
    m = np.asarray(m, bool)
    return m & (_d2(~m, border_value == 0, r2) > r2)


def binary_opening(m, r2, border_value=0):
    return binary_dilation(binary_erosion(m, r2, border_value), r2, border_value)


def binary_closing(m, r2, border_value=0):
    return binary_erosion(binary_dilation(m, r2, border_value), r2, border_value)


def expand_labels(labels, r2):
    """int32 [H, W]: a zero pixel whose nearest nonzero pixel lies within r2 takes its label"""
    labels = np.asarray(labels)
    assert labels.dtype == np.int32 and labels.ndim == 2
    d2, site = nearest(labels != 0, r2)
    if d2[0, 0] < 0:
        return labels.copy()
    near = labels.ravel()[np.maximum(site, 0)]                                  # (site -1: beyond the limit, not used)
    return np.where(labels != 0, labels, np.where(d2 <= r2, near, 0)).astype(np.int32)


def disk(r2):
    """the structuring element of the scipy comparison: dx^2 + dy^2 <= r2 on the (2 floor(sqrt(r2)) + 1)^2 grid"""
    k = int(np.floor(np.sqrt(r2)))
    while (k + 1) ** 2 <= r2:
        k += 1
    while k * k > r2:
        k -= 1
    yy, xx = np.mgrid[-k:k + 1, -k:k + 1]
    return yy * yy + xx * xx <= r2
