"""Brute-force numpy statement of the seeded split (cellsegmentation_amd.regions.split) and of the tables of a label image
(regions.measure_labels), the reference of tests/test_split_gpu.py and tools/regions_microbench.py --split.  Components come from
``scipy.ndimage.label``; inside a component every pixel is compared with every live seed of that component, in a plain loop.  The
tables come from ``scipy.ndimage`` sum / maximum / center_of_mass / mean / find_objects with ``labels=`` and ``index=``.

The rules (regions.split's docstring): the first S' = limit-clipped points of an image are its seeds; a seed is live when it lies
inside the image on a foreground pixel; a foreground pixel of a component with live seeds gets 1 + the k that minimises (d2, k)
over THAT component's live seeds; the components without one get S' + 1 + j in scipy's order; counts = S' + their number.
"""
import numpy as np
from scipy import ndimage as ndi

STRUCTURE = {1: ndi.generate_binary_structure(2, 1), 2: ndi.generate_binary_structure(2, 2)}


def n_seeds(n_points, limit):
    """Python's ``len(range(n_points)[:limit])``"""
    return n_points if limit is None else len(range(int(n_points))[:int(limit)])


def split_one(m, seeds, connectivity=1):
    """m bool [H, W]; seeds int [S', 2] (row, col), already cut to the limit -> (labels int32 [H, W], count, live bool [S'])"""
    m = np.asarray(m, bool)
    seeds = np.asarray(seeds, np.int64).reshape(-1, 2)
    H, W = m.shape
    comp, n_comp = ndi.label(m, structure=STRUCTURE[connectivity])
    home = np.zeros(len(seeds), np.int64)                  # the component under every live seed, 0 for a dead one
    for k, (r, c) in enumerate(seeds):
        if 0 <= r < H and 0 <= c < W and m[r, c]:
            home[k] = comp[r, c]
    out = np.zeros((H, W), np.int32)
    seedless = 0
    for j, box in enumerate(ndi.find_objects(comp), start=1):
        rr, cc = np.nonzero(comp[box] == j)
        rr, cc = rr + box[0].start, cc + box[1].start
        ks = np.nonzero(home == j)[0]
        if len(ks) == 0:
            seedless += 1
            out[rr, cc] = len(seeds) + seedless
            continue
        best_d = np.full(len(rr), np.iinfo(np.int64).max)
        best_k = np.zeros(len(rr), np.int64)
        for k in ks:                                        # rising k: a strict < keeps the lower index on a tie
            d = (rr - seeds[k, 0]) ** 2 + (cc - seeds[k, 1]) ** 2
            better = d < best_d
            best_d[better], best_k[better] = d[better], k
        out[rr, cc] = best_k + 1
    return out, len(seeds) + seedless, home > 0


def split(m, points, offsets=None, limits=None, connectivity=1):
    """m bool [H, W] or [N, H, W]; points int [P, 2] with offsets [N + 1] (None: one image owns them all; P may exceed
    offsets[-1]); limits None, one count or [N] -> dict: labels int32 of m's shape, counts int32 [N], n_seeds int32 [N], live bool [P]"""
    m = np.asarray(m, bool)
    ms = m[None] if m.ndim == 2 else m
    points = np.asarray(points, np.int64).reshape(-1, 2)
    off = np.asarray([0, len(points)] if offsets is None else offsets, np.int64)
    assert len(off) == len(ms) + 1
    lim = [None] * len(ms) if limits is None else np.broadcast_to(np.asarray(limits), (len(ms),))
    labels, counts, seeds_n = np.zeros(ms.shape, np.int32), np.zeros(len(ms), np.int32), np.zeros(len(ms), np.int32)
    live = np.zeros(len(points), bool)
    for n, x in enumerate(ms):
        s = n_seeds(off[n + 1] - off[n], lim[n])
        labels[n], counts[n], live[off[n]:off[n] + s] = split_one(x, points[off[n]:off[n] + s], connectivity)
        seeds_n[n] = s
    return {"labels": labels[0] if m.ndim == 2 else labels, "counts": counts, "n_seeds": seeds_n, "live": live}


def tables(labels, intensity=None, capacity=None, counts=None):
    """labels int [H, W] or [N, H, W] -> the dict layout of tests/props_ref.py (counts, capacity, area, bbox, sum_rc and, with
    intensity, intensity_sum / intensity_max) plus float64 ``centroid`` and ``intensity_mean`` straight from scipy (NaN where the
    label owns no pixel).  counts None: the largest label per image.  capacity None: the largest count (at least 1)."""
    labels = np.asarray(labels)
    ls = labels[None] if labels.ndim == 2 else labels
    vs = None if intensity is None else np.asarray(intensity).reshape(ls.shape)
    counts = np.asarray([max(int(x.max()), 0) for x in ls], np.int32) if counts is None else np.asarray(counts, np.int32)
    cap = max(1, int(counts.max())) if capacity is None else int(capacity)
    N, (H, W) = len(ls), ls.shape[1:]
    index = np.arange(1, cap + 1)
    rows, cols = np.mgrid[:H, :W]
    out = {"counts": counts, "capacity": cap, "area": np.zeros((N, cap), np.int32), "bbox": np.zeros((N, cap, 4), np.int32),
           "sum_rc": np.zeros((N, cap, 2), np.int64), "centroid": np.full((N, cap, 2), np.nan)}
    if vs is not None:
        out.update(intensity_sum=np.zeros((N, cap), np.int64), intensity_max=np.zeros((N, cap), np.int32),
                   intensity_mean=np.full((N, cap), np.nan))
    for n, lab in enumerate(ls):
        lab = np.where(lab > 0, lab, 0)
        out["area"][n] = np.rint(ndi.sum(np.ones((H, W), np.int64), lab, index))
        out["sum_rc"][n, :, 0] = np.rint(ndi.sum(rows, lab, index))
        out["sum_rc"][n, :, 1] = np.rint(ndi.sum(cols, lab, index))
        for k, sl in enumerate(ndi.find_objects(lab, max_label=cap)):
            if sl is not None:
                out["bbox"][n, k] = (sl[0].start, sl[1].start, sl[0].stop, sl[1].stop)
        used = out["area"][n] > 0
        if used.any():
            out["centroid"][n, used] = np.asarray(ndi.center_of_mass(np.ones((H, W)), lab, index[used])).reshape(-1, 2)
        if vs is not None:
            out["intensity_sum"][n] = np.rint(ndi.sum(vs[n].astype(np.int64), lab, index))
            out["intensity_max"][n] = np.where(used, ndi.maximum(vs[n].astype(np.int64), lab, index), 0)
            if used.any():
                out["intensity_mean"][n, used] = ndi.mean(vs[n].astype(np.float64), lab, index[used])
    return out


# ---- shapes shared by the golden vectors and the GPU tests ----------------------------------------------------------------------
def discs(H, W, centres, radius):
    yy, xx = np.mgrid[:H, :W]
    m = np.zeros((H, W), bool)
    for cy, cx in centres:
        m |= (yy - cy) ** 2 + (xx - cx) ** 2 <= radius * radius
    return m


def two_discs(H=37, W=130):
    """two overlapping discs with their centres on one row, 16 columns apart: column 68 is equidistant from both"""
    centres = [(18, 60), (18, 76)]
    return discs(H, W, centres, 12), np.asarray(centres, np.int64)


def foreign_seed(H=37, W=130):
    """Blob A (columns < 40) with its seed at its right edge, blob B (columns 42 .. 99) with its seed at its far end: the left part
    of B is nearer to A's seed than to its own.  -> (mask, points: A's seed first)"""
    m = np.zeros((H, W), bool)
    m[5:30, 10:40] = True
    m[8:28, 42:100] = True
    return m, np.asarray([[15, 39], [15, 97]], np.int64)


def random_seeds(masks, per_image, seed):
    """per_image random points per image, about two in three on the foreground -> (points [P, 2], offsets [N + 1])"""
    rng = np.random.RandomState(seed)
    pts, off = [], [0]
    for m in masks:
        fg = np.argwhere(m)
        for _ in range(per_image):
            if len(fg) and rng.rand() < 0.67:
                pts.append(fg[rng.randint(len(fg))])
            else:
                pts.append([rng.randint(m.shape[0]), rng.randint(m.shape[1])])
        off.append(len(pts))
    return np.asarray(pts, np.int64).reshape(-1, 2), np.asarray(off, np.int64)
