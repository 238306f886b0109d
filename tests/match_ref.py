"""The numpy statement of ``regions.match_labels`` and ``MatchTable.score``: per image a dense contingency table of the two label
images, every pair tried for ``2 I > U`` in Python integers' int64, and the score formulas in plain float64.  Independent of the
device's voting trick; only for small label counts (the table is (cap_pred + 1) x (cap_truth + 1)).

Inputs: int32 label images [H, W] or [N, H, W], values <= 0 = background.  A label above its side's capacity is background on that
side; the counts still report the true largest labels.
"""
import numpy as np

import score_ref

TABLES = ("counts_pred", "counts_truth", "area_pred", "area_truth", "match", "inter", "match_truth")
SCORES = ("n_pred", "n_truth", "tp", "fp", "fn", "precision", "recall", "f1", "sq", "pq")


def match(pred, truth, cap_pred=None, cap_truth=None):
    """-> dict: counts_pred, counts_truth int32 [N] (the largest labels), cap_pred, cap_truth (None: the largest count of the batch,
    at least 1), area_pred int32 [N, cap_pred], area_truth int32 [N, cap_truth], match, inter int32 [N, cap_pred], match_truth
    int32 [N, cap_truth]"""
    pred, truth = np.asarray(pred), np.asarray(truth)
    assert pred.shape == truth.shape and pred.ndim in (2, 3)
    if pred.ndim == 2:
        pred, truth = pred[None], truth[None]
    pred, truth = np.maximum(pred.astype(np.int64), 0), np.maximum(truth.astype(np.int64), 0)
    N = len(pred)
    counts_p, counts_t = pred.reshape(N, -1).max(axis=1), truth.reshape(N, -1).max(axis=1)
    cp = max(1, int(counts_p.max())) if cap_pred is None else int(cap_pred)
    ct = max(1, int(counts_t.max())) if cap_truth is None else int(cap_truth)
    out = {"counts_pred": counts_p.astype(np.int32), "counts_truth": counts_t.astype(np.int32), "cap_pred": cp, "cap_truth": ct,
           "area_pred": np.zeros((N, cp), np.int32), "area_truth": np.zeros((N, ct), np.int32), "match": np.zeros((N, cp), np.int32),
           "inter": np.zeros((N, cp), np.int32), "match_truth": np.zeros((N, ct), np.int32)}
    for n in range(N):
        p, g = np.where(pred[n] > cp, 0, pred[n]), np.where(truth[n] > ct, 0, truth[n])
        tab = np.zeros((cp + 1, ct + 1), np.int64)
        np.add.at(tab, (p.ravel(), g.ravel()), 1)
        area_p, area_t = tab.sum(axis=1)[1:], tab.sum(axis=0)[1:]
        inter = tab[1:, 1:]
        hit = 2 * inter > area_p[:, None] + area_t[None, :] - inter       # every pair
        assert hit.sum(axis=0).max(initial=0) <= 1 and hit.sum(axis=1).max(initial=0) <= 1
        out["area_pred"][n], out["area_truth"][n] = area_p, area_t
        for i, j in zip(*np.nonzero(hit)):
            out["match"][n, i], out["inter"][n, i], out["match_truth"][n, j] = j + 1, inter[i, j], i + 1
    return out


def iou(t):
    """float64 [N, cap_pred]: inter / union where matched, 0 elsewhere"""
    q = np.zeros(t["match"].shape, np.float64)
    for n, i in zip(*np.nonzero(t["match"])):
        I = int(t["inter"][n, i])
        U = int(t["area_pred"][n, i]) + int(t["area_truth"][n, t["match"][n, i] - 1]) - I
        q[n, i] = np.float64(I) / np.float64(U)
    return q


def score(t, iou_threshold=0.5):
    """-> dict of per-image arrays: n_pred, n_truth, tp, fp, fn int64; precision, recall, f1, sq, pq float64"""
    q = iou(t)
    N = len(q)
    out = {k: np.zeros((N,), np.int64 if k in SCORES[:5] else np.float64) for k in SCORES}
    for n in range(N):
        rows = [q[n, i] for i in range(q.shape[1]) if t["match"][n, i] > 0 and q[n, i] >= iou_threshold]   # ascending pred label
        tp = len(rows)
        n_pred, n_truth = int((t["area_pred"][n] > 0).sum()), int((t["area_truth"][n] > 0).sum())
        p, r, f1 = score_ref.prf(tp, n_pred - tp, n_truth - tp)
        sq = np.sum(np.asarray(rows, np.float64)) / tp if tp else 0.0
        for k, v in zip(SCORES, (n_pred, n_truth, tp, n_pred - tp, n_truth - tp, p, r, f1, sq, sq * f1)):
            out[k][n] = v
    return out


def runs(*pairs):
    """(label, pixel count), ... -> a one-row int32 label image"""
    return np.concatenate([np.full(k, v, np.int32) for v, k in pairs])[None]


def hand_cases():
    """name -> (pred, truth, cap_pred or None, cap_truth or None): one-row images, worked by hand"""
    return {
        "half_twice": (runs((1, 4)), runs((1, 2), (2, 2)), None, None),
        "two_thirds": (runs((1, 2), (0, 1)), runs((1, 3)), None, None),
        "false_candidate": (runs((1, 10)), runs((3, 4), (1, 3), (2, 3)), None, None),
        "out_of_range_candidate": (runs((1, 10)), runs((5, 4), (6, 4), (3, 2)), None, 6),
        "background_majority": (runs((1, 10)), runs((1, 4), (0, 6)), None, None),
        "identical_with_empty": (runs((1, 3), (0, 2), (3, 4)), runs((1, 3), (0, 2), (3, 4)), None, None),
    }


def blocks(H=64, W=64):
    """every 2 x 2 block its own label, 1 .. H W / 4"""
    r, c = np.mgrid[:H, :W]
    return ((r // 2) * (W // 2) + c // 2 + 1).astype(np.int32)


def noisy_pair(masks, seed, label):
    """bool [N, H, W] -> (pred, truth) int32: ``label`` of the masks, and of the masks rolled by up to +-2 pixels and XOR-ed with
    2 % noise.  label: bool [H, W] -> int labels [H, W]."""
    rng = np.random.RandomState(seed)
    pred, truth = [], []
    for m in masks:
        moved = np.roll(m, (rng.randint(-2, 3), rng.randint(-2, 3)), axis=(0, 1)) ^ (rng.rand(*m.shape) < 0.02)
        pred.append(label(m))
        truth.append(label(moved))
    return np.stack(pred).astype(np.int32), np.stack(truth).astype(np.int32)
