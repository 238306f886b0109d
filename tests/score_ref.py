"""numpy restatement of the scoring of detected points against annotated ones (test_seg.py:120-141 get_prf1 with
metrics/metrics.py:56-66), the contract cellsegmentation_amd.score / csrc/score.hip are held to.  Beyond the reference it returns
which annotation every detection took and applies a per-image limit (Python's ``[:c]``) to the detections.

Per image, detections in order: the unflagged annotation of smallest squared distance (lowest index among equals) is flagged and
counted when ``d2 <= radius2``; squared distances are Python / int64 integers, no float decides.  tests/test_score_host.py pins
this file to tests/golden/score_vectors.npz, which the reference's own functions produced."""
import numpy as np

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


def _pts(x):
    x = np.asarray(x)
    return np.zeros((0, 2), np.int64) if x.size == 0 else x.astype(np.int64).reshape(-1, 2)


def score(hat, gt, limit=None, radius2=256):
    """-> (tp, fp, fn, match int32 [len(hat)]); match: annotation index, -1 false positive, -2 beyond the limit"""
    hat, gt = _pts(hat), _pts(gt)
    match = np.full(len(hat), -2, np.int32)
    kept = len(hat[:limit]) if limit is not None else len(hat)
    flag = np.zeros(len(gt), bool)
    tp = 0
    for i in range(kept):
        match[i] = -1
        r, c = int(hat[i, 0]), int(hat[i, 1])
        if not (I32_MIN <= r <= I32_MAX and I32_MIN <= c <= I32_MAX) or not len(gt):
            continue                                                      # a coordinate outside int32 matches nothing
        # |differences| are capped at 2^30 so that the int64 sum cannot overflow; a capped one is far beyond any radius2 < 2^31
        d2 = np.minimum(np.abs(gt[:, 0] - r), 1 << 30) ** 2 + np.minimum(np.abs(gt[:, 1] - c), 1 << 30) ** 2
        free = np.flatnonzero(~flag)
        if not len(free):
            continue
        j = int(free[np.argmin(d2[free])])                                # argmin: the first (lowest index) of equal minima
        if d2[j] <= radius2:
            flag[j] = True
            match[i] = j
            tp += 1
    return tp, kept - tp, int((~flag).sum()), match


def prf(tp, fp, fn):
    """metrics/metrics.py:60-64 in Python arithmetic -> float64 triple"""
    tp, fp, fn = int(tp), int(fp), int(fn)
    p = 1 if tp + fp == 0 else tp / (tp + fp)
    r = 1 if tp + fn == 0 else tp / (tp + fn)
    f1 = 0 if p + r == 0 else (2 * p * r) / (p + r)
    return np.asarray([p, r, f1], np.float64)


def score_batch(hat, hat_off, gt, gt_off, limits=None, radius2=256):
    """ragged batches -> (counts int64 [N, 3], prf float64 [N, 3], match int32 [hat_off[-1]])"""
    hat, gt = _pts(hat), _pts(gt)
    N = len(hat_off) - 1
    counts, ratios, match = np.zeros((N, 3), np.int64), np.zeros((N, 3), np.float64), []
    for n in range(N):
        lim = None if limits is None else int(limits if np.ndim(limits) == 0 else limits[n])
        tp, fp, fn, m = score(hat[hat_off[n]:hat_off[n + 1]], gt[gt_off[n]:gt_off[n + 1]], lim, radius2)
        counts[n] = (tp, fp, fn)
        ratios[n] = prf(tp, fp, fn)
        match.append(m)
    return counts, ratios, (np.concatenate(match) if match else np.zeros(0, np.int32))


def ragged(arrays):
    """[k_i, 2] arrays -> (concatenated int64 [sum k, 2], offsets int64 [N + 1])"""
    arrays = [_pts(a) for a in arrays]
    off = np.zeros(len(arrays) + 1, np.int64)
    np.cumsum([len(a) for a in arrays], out=off[1:])
    return (np.concatenate(arrays) if arrays else np.zeros((0, 2), np.int64)), off


def random_points(rng, n, field):
    """n integer points on a field x field square"""
    return rng.randint(0, field, size=(n, 2)).astype(np.int64)


def field_for(n_hat, n_gt, radius2=256):
    """a field edge on which about half of n_hat random detections find one of n_gt random annotations of their own: the
    expected number of annotations within the radius of a point is about 0.7"""
    return max(8, int(np.sqrt(max(n_gt, n_hat, 1) * np.pi * radius2 / 0.7)))
