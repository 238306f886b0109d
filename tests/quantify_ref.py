"""A numpy restatement of cellsegmentation_amd.stain.quantify_labels (csrc/regions.hip, quantify_kernel): the quantised stain
matrix, the integer stain level of a pixel, the per-(label, compartment) tables, ``StainTable.classify`` and the positivity score.
int64 numpy and plain loops only; nothing of the library is imported."""
import math

import numpy as np

OD_UNIT = 4096
BINS = (0, 16, 32, 64, 128, 256)
H_VEC = np.asarray((0.650, 0.704, 0.286)) / np.linalg.norm((0.650, 0.704, 0.286))
DAB_VEC = np.asarray((0.268, 0.570, 0.776)) / np.linalg.norm((0.268, 0.570, 0.776))
HDAB = np.stack([H_VEC, DAB_VEC], axis=1)                                  # [3, 2]: Ruifrok's vectors as columns


def od_table(Io=240):
    v = np.arange(256, dtype=np.float64)
    return np.maximum(0.0, np.rint(OD_UNIT * np.log(Io / (v + 1.0)))).astype(np.int64)


def stain_matrix(S, residual=False):
    S = np.asarray(S, np.float64)
    if residual:
        c = np.cross(S[:, 0], S[:, 1])
        S = np.concatenate([S, (c / np.linalg.norm(c))[:, None]], axis=1)
    return S


def quantised_matrix(S=HDAB, residual=False, conc_max=8.0):
    """int64 [K, 3]: rint(2^24 255 pinv(S) / (4096 conc_max)); ValueError beyond int32"""
    M = np.rint(np.linalg.pinv(stain_matrix(S, residual)) * (float(1 << 24) * 255.0) / (float(OD_UNIT) * float(conc_max)))
    if not np.isfinite(M).all() or np.abs(M).max() > 2 ** 31 - 1:
        raise ValueError("the quantised matrix leaves int32")
    return M.astype(np.int64)


def levels(image_u8, Mq, Io=240):
    """uint8 [..., 3], Mq int [K, 3] -> int64 [..., K]: clamp((Mq od_q + 2^23) >> 24, 0, 255), the shift arithmetic"""
    q = od_table(Io)[np.asarray(image_u8)]                                 # int64 [..., 3]
    acc = q @ np.asarray(Mq, np.int64).T + (1 << 23)
    return np.clip(acc >> 24, 0, 255)


def positive_levels(pixel_threshold, conc_max=8.0):
    return [min(max(int(math.ceil(255.0 * float(t) / float(conc_max))), 0), 256) for t in pixel_threshold]


def quantify(images, labels, Mq, capacity, expanded=None, pos_levels=None, bins=0, Io=240):
    """images uint8 [N, H, W, 3], labels (and expanded or None) int [N, H, W], Mq int [N, K, 3] -> dict of int64 arrays: counts [N]
    (the largest label that owns a pixel), n [N, cap, C], sum, sumsq, max, pos [N, cap, C, K], hist [N, cap, C, K, bins] (with
    bins).  A plain loop over the pixels."""
    images, labels, Mq = np.asarray(images), np.asarray(labels).astype(np.int64), np.asarray(Mq, np.int64)
    N, H, W = labels.shape
    Kn, C, cap = Mq.shape[1], 1 if expanded is None else 2, int(capacity)
    L = [256] * Kn if pos_levels is None else list(pos_levels)
    out = {"counts": np.zeros(N, np.int64), "n": np.zeros((N, cap, C), np.int64)}
    for k in ("sum", "sumsq", "max", "pos"):
        out[k] = np.zeros((N, cap, C, Kn), np.int64)
    if bins:
        out["hist"] = np.zeros((N, cap, C, Kn, bins), np.int64)
    for n in range(N):
        lv = levels(images[n], Mq[n], Io)
        for r in range(H):
            for c in range(W):
                lab, comp = int(labels[n, r, c]), 0
                if lab <= 0:
                    if expanded is None or int(expanded[n][r][c]) <= 0:
                        continue
                    lab, comp = int(expanded[n][r][c]), 1
                out["counts"][n] = max(out["counts"][n], lab)
                if lab > cap:
                    continue
                out["n"][n, lab - 1, comp] += 1
                for s in range(Kn):
                    v = int(lv[r, c, s])
                    out["sum"][n, lab - 1, comp, s] += v
                    out["sumsq"][n, lab - 1, comp, s] += v * v
                    out["max"][n, lab - 1, comp, s] = max(out["max"][n, lab - 1, comp, s], v)
                    out["pos"][n, lab - 1, comp, s] += v >= L[s]
                    if bins:
                        out["hist"][n, lab - 1, comp, s, (v * bins) >> 8] += 1
    return out


def quantify_fast(images, labels, Mq, capacity, expanded=None, pos_levels=None, bins=0, Io=240):
    """``quantify`` by bincounts, for the larger cases (tests/test_quantify_host.py holds the two against each other)"""
    images, labels, Mq = np.asarray(images), np.asarray(labels).astype(np.int64), np.asarray(Mq, np.int64)
    N, H, W = labels.shape
    Kn, C, cap = Mq.shape[1], 1 if expanded is None else 2, int(capacity)
    L = [256] * Kn if pos_levels is None else list(pos_levels)
    out = {"counts": np.zeros(N, np.int64), "n": np.zeros((N, cap, C), np.int64)}
    for k in ("sum", "sumsq", "max", "pos"):
        out[k] = np.zeros((N, cap, C, Kn), np.int64)
    if bins:
        out["hist"] = np.zeros((N, cap, C, Kn, bins), np.int64)
    for n in range(N):
        own = np.maximum(labels[n], 0)
        comp = np.zeros_like(own)
        if expanded is not None:
            ring = (own == 0) & (np.asarray(expanded[n]) > 0)
            own = np.where(ring, np.asarray(expanded[n]).astype(np.int64), own)
            comp = ring.astype(np.int64)
        out["counts"][n] = own.max()
        keep = (own > 0) & (own <= cap)
        slot = ((own - 1) * C + comp)[keep]
        lv = levels(images[n], Mq[n], Io)[keep]                            # [m, K]
        out["n"][n] = np.bincount(slot, minlength=cap * C).reshape(cap, C)
        for s in range(Kn):
            v = lv[:, s]
            out["sum"][n, ..., s] = _sums(slot, v, cap * C).reshape(cap, C)
            out["sumsq"][n, ..., s] = _sums(slot, v * v, cap * C).reshape(cap, C)
            out["pos"][n, ..., s] = _sums(slot, (v >= L[s]).astype(np.int64), cap * C).reshape(cap, C)
            mx = np.zeros(cap * C, np.int64)
            np.maximum.at(mx, slot, v)
            out["max"][n, ..., s] = mx.reshape(cap, C)
            if bins:
                out["hist"][n, ..., s, :] = np.bincount(slot * bins + ((v * bins) >> 8), minlength=cap * C * bins).reshape(cap, C, bins)
    return out


def _sums(slot, v, size):
    """exact integer sums per slot (np.bincount's weights are float64: the sums here stay below 2^53, and are added as integers)"""
    acc = np.zeros(size, np.int64)
    np.add.at(acc, slot, v.astype(np.int64))
    return acc


# ---- the float64 methods of StainTable on the integer tables -------------------------------------------------------------------------
def mean(t):
    with np.errstate(divide="ignore", invalid="ignore"):
        return t["sum"].astype(np.float64) / t["n"].astype(np.float64)[..., None]


def std(t):
    n = t["n"][..., None]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.sqrt((n * t["sumsq"] - t["sum"] * t["sum"]).astype(np.float64)) / n.astype(np.float64)


def positive_fraction(t):
    with np.errstate(divide="ignore", invalid="ignore"):
        return t["pos"].astype(np.float64) / t["n"].astype(np.float64)[..., None]


def order_bin(hist, k):
    """the bin of a histogram that holds order statistic k (0-based) of what it counted"""
    return int(np.searchsorted(np.cumsum(np.asarray(hist, np.int64)), k, side="right"))


def quantile(t, q):
    """the centre in levels of the bin that holds order statistic ceil(q (n - 1)): (bin + 1/2) 256 / bins - 1/2; NaN where n == 0"""
    h = t["hist"]
    bins = h.shape[-1]
    out = np.full(h.shape[:-1], np.nan)
    for idx in np.ndindex(*h.shape[:-1]):
        n = int(t["n"][idx[:-1]])
        if n:
            out[idx] = (order_bin(h[idx], int(math.ceil(q * (n - 1)))) + 0.5) * (256.0 / bins) - 0.5
    return out


# ---- classes and the score ----------------------------------------------------------------------------------------------------------
def class_thresholds(thresholds, conc_max=8.0):
    return [int(np.rint(256.0 * 255.0 * float(t) / float(conc_max))) for t in thresholds]


def classify(t, thresholds, stain=1, compartment=0, conc_max=8.0):
    """int64 [N, cap]: the number of thresholds T with 256 sum >= T n (Python integers), -1 where n == 0"""
    T = class_thresholds(thresholds, conc_max)
    n, s = t["n"][:, :, compartment], t["sum"][:, :, compartment, stain]
    out = np.full(n.shape, -1, np.int64)
    for idx in np.ndindex(*n.shape):
        if int(n[idx]):
            out[idx] = sum(256 * int(s[idx]) >= Tk * int(n[idx]) for Tk in T)
    return out


def positivity(class_counts):
    """[N, <= 4] cells per class -> (n_cells [N], labelling index [N], H-score [N]); NaN without cells"""
    c = np.atleast_2d(np.asarray(class_counts, np.int64))
    n = c.sum(axis=1)
    li, hs = np.full(len(c), np.nan), np.full(len(c), np.nan)
    for i in range(len(c)):
        if n[i]:
            li[i] = 100.0 * float(n[i] - c[i, 0]) / float(n[i])
            hs[i] = 100.0 * float(sum(k * int(c[i, k]) for k in range(c.shape[1]))) / float(n[i])
    return n, li, hs


def score(t, thresholds, stain=1, compartment=0, conc_max=8.0):
    cls = classify(t, thresholds, stain, compartment, conc_max)
    return positivity(np.stack([(cls == k).sum(axis=1) for k in range(4)], axis=1))


# ---- fixtures -------------------------------------------------------------------------------------------------------------------------
def blocks(h, w, seed, n_labels=5, gaps=True):
    """int32 [h, w]: rectangles of labels 1 .. n_labels painted in order (later ones overwrite), some pixels <= 0"""
    rng = np.random.RandomState(seed)
    lab = np.zeros((h, w), np.int32)
    for l in range(1, n_labels + 1):
        r0, c0 = rng.randint(0, h), rng.randint(0, w)
        lab[r0:r0 + rng.randint(1, max(2, h)), c0:c0 + rng.randint(1, max(2, w // 2 + 1))] = l
    if gaps:
        lab[rng.rand(h, w) < 0.05] = -3
    return lab


def grow(lab, steps=2):
    """a stand-in for an expanded label image: every label grown ``steps`` times into zero pixels to its right and below (positive
    labels keep their pixels)"""
    out = lab.copy()
    for _ in range(steps):
        for axis in (1, 0):
            moved = np.roll(out, 1, axis=axis)
            moved[(slice(None), 0) if axis else (0, slice(None))] = 0
            out = np.where((out == 0) & (moved > 0), moved, out)
    return out
