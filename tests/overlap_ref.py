"""The numpy statement of ``regions.overlap_labels`` and ``OverlapTable.score``: per image the dense contingency table of the two
label images, every rule applied to it in Python integers, and AJI / object-level Dice in plain float64.  It shares nothing with the
device's hash table or with ``score.overlap_score``; only for small label counts (the table is (cap_pred + 1) x (cap_truth + 1)).

Inputs: int32 label images [H, W] or [N, H, W], values <= 0 = background.  A label above its side's capacity is background on that
side; the counts still report the true largest labels.

Per image, Ap / At the areas, I(p, g) the shared pixels:
  best-IoU partner of truth g          the p with I > 0 maximising I / (Ap + At - I); equal fractions go to the lower p
  best-intersection partner of g / p   the label of the other side with the largest I > 0; equal I goes to the lower label
  AJI                                  over truth objects (At > 0) in ascending label: with a best-IoU partner j, C += I(j, g),
                                       U += Ap[j] + At[g] - I and j is used; without, U += At[g]; then U += Ap of every unused pred
                                       object; C / U, 1.0 when U == 0
  object-level Dice                    1/2 (sum_g At[g] / sum At * D(g, S*(g)) + sum_p Ap[p] / sum Ap * D(G*(p), p)), D = 2 I /
                                       (Ap + At) and 0 without a partner, S* / G* the best-intersection partners; a side without
                                       objects adds 0; 1.0 when neither side has an object
"""
from fractions import Fraction

import numpy as np

from match_ref import runs

TABLES = ("counts_pred", "counts_truth", "area_pred", "area_truth", "n_pairs", "iou_partner", "iou_inter", "inter_partner_truth",
          "inter_truth", "inter_partner_pred", "inter_pred")
PAIRS = ("image", "pred", "truth", "inter")
SCORES = ("n_pred", "n_truth", "n_pairs", "aji_inter", "aji_union", "aji", "dice_obj")


def overlap(pred, truth, cap_pred=None, cap_truth=None):
    """-> dict: the TABLES (int32; counts and n_pairs [N], the others [N, cap_pred] or [N, cap_truth]), cap_pred, cap_truth (None:
    the largest count of the batch, at least 1) and pairs = (image, pred, truth, inter) int64, sorted"""
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
           "n_pairs": np.zeros((N,), np.int32)}
    for k in TABLES[2:]:
        if k != "n_pairs":
            out[k] = np.zeros((N, cp if k in ("area_pred", "inter_partner_pred", "inter_pred") else ct), np.int32)
    listed = []
    for n in range(N):
        p, g = np.where(pred[n] > cp, 0, pred[n]), np.where(truth[n] > ct, 0, truth[n])
        tab = np.zeros((cp + 1, ct + 1), np.int64)
        np.add.at(tab, (p.ravel(), g.ravel()), 1)
        area_p, area_t = [int(v) for v in tab.sum(axis=1)], [int(v) for v in tab.sum(axis=0)]
        out["area_pred"][n], out["area_truth"][n] = area_p[1:], area_t[1:]
        best_iou, most_t, most_p = {}, {}, {}                              # truth -> (fraction, pred); truth -> (I, pred); pred -> (I, truth)
        for i, j in zip(*(k + 1 for k in np.nonzero(tab[1:, 1:]))):        # row-major: ascending pred label, then truth label,
            i, j, I = int(i), int(j), int(tab[i, j])                       # so only a strictly better pair replaces a holder
            listed.append((n, i, j, I))
            out["n_pairs"][n] += 1
            q = Fraction(I, area_p[i] + area_t[j] - I)                     # exact
            if j not in best_iou or q > best_iou[j][0]:
                best_iou[j] = (q, i)
            if j not in most_t or I > most_t[j][0]:
                most_t[j] = (I, i)
            if i not in most_p or I > most_p[i][0]:
                most_p[i] = (I, j)
        for j, (_, i) in best_iou.items():
            out["iou_partner"][n, j - 1], out["iou_inter"][n, j - 1] = i, int(tab[i, j])
        for j, (I, i) in most_t.items():
            out["inter_partner_truth"][n, j - 1], out["inter_truth"][n, j - 1] = i, I
        for i, (I, j) in most_p.items():
            out["inter_partner_pred"][n, i - 1], out["inter_pred"][n, i - 1] = j, I
    out["pairs"] = tuple(np.asarray([row[k] for row in listed], np.int64) for k in range(4))
    return out


def score(t):
    """the tables of ``overlap`` -> dict of per-image arrays: n_pred, n_truth, n_pairs, aji_inter, aji_union int64; aji, dice_obj
    float64"""
    N = len(t["area_pred"])
    out = {k: np.zeros((N,), np.float64 if k in ("aji", "dice_obj") else np.int64) for k in SCORES}
    for n in range(N):
        ap, at = [int(v) for v in t["area_pred"][n]], [int(v) for v in t["area_truth"][n]]
        truth_objects = [g for g in range(len(at)) if at[g] > 0]
        pred_objects = [p for p in range(len(ap)) if ap[p] > 0]
        C, U, used = 0, 0, set()
        for g in truth_objects:
            j = int(t["iou_partner"][n, g])
            if j > 0:
                I = int(t["iou_inter"][n, g])
                C, U = C + I, U + ap[j - 1] + at[g] - I
                used.add(j - 1)
            else:
                U += at[g]
        for p in pred_objects:
            if p not in used:
                U += ap[p]
        dice_t = np.float64(0.0)
        for g in truth_objects:
            s = int(t["inter_partner_truth"][n, g])
            if s > 0:
                d = np.float64(2 * int(t["inter_truth"][n, g])) / np.float64(ap[s - 1] + at[g])
                dice_t = dice_t + np.float64(at[g]) / np.float64(sum(at)) * d
        dice_p = np.float64(0.0)
        for p in pred_objects:
            s = int(t["inter_partner_pred"][n, p])
            if s > 0:
                d = np.float64(2 * int(t["inter_pred"][n, p])) / np.float64(ap[p] + at[s - 1])
                dice_p = dice_p + np.float64(ap[p]) / np.float64(sum(ap)) * d
        out["n_pred"][n], out["n_truth"][n], out["n_pairs"][n] = len(pred_objects), len(truth_objects), int(t["n_pairs"][n])
        out["aji_inter"][n], out["aji_union"][n] = C, U
        out["aji"][n] = np.float64(C) / np.float64(U) if U else 1.0
        out["dice_obj"][n] = (dice_t + dice_p) / 2 if (truth_objects or pred_objects) else 1.0
    return out


def hand_cases():
    """name -> (pred, truth): one-row int32 images, worked by hand (tests/test_overlap_host.py has the answers)"""
    return {
        # truth 1 on columns 0-5; pred 1 on 0-1; pred 2 on 2-4 and 6-32 (30 px): IoU 2/6 against 3/33, intersection 2 against 3
        "iou_vs_inter": (runs((1, 2), (2, 3), (0, 1), (2, 27)), runs((1, 6), (0, 27))),
        "iou_tie": (runs((1, 2), (2, 2)), runs((1, 4))),                  # 2/4 twice: the lower pred label by both rules
        "shared_pred": (runs((1, 6)), runs((1, 3), (2, 3))),             # one pred serves two truths: a union for each
        "both_empty": (runs((0, 5)), runs((0, 5))),
        "pred_empty": (runs((0, 3)), runs((1, 3))),
        "truth_empty": (runs((2, 3)), runs((0, 3))),
        # six pairs in a chain: (1,1)=2 (1,2)=1 (2,2)=2 (2,3)=1 (3,3)=2 (3,4)=1, then truth 4 alone
        "six_pairs": (runs((1, 3), (2, 3), (3, 3), (0, 1)), runs((1, 2), (2, 3), (3, 3), (4, 2))),
        "five_labels": (runs((1, 2), (2, 2), (3, 2), (4, 2), (5, 2)), runs((1, 1), (2, 2), (3, 2), (4, 2), (5, 3))),
        "negative": (runs((1, 3), (-4, 2), (2, 2)), runs((-1, 2), (1, 3), (2, 2))),
        # equal intersections on the pred side: pred 1 shares 2 px with truth 1 and with truth 2 -> truth 1
        "inter_tie": (runs((1, 4), (0, 1)), runs((1, 2), (2, 3))),
    }


def stacked(cases=None):
    """the hand cases, each padded with background to the widest, as one batch -> (names, pred, truth int32 [N, 1, W])"""
    cases = hand_cases() if cases is None else cases
    W = max(p.shape[1] for p, _ in cases.values())
    pad = lambda x: np.pad(x, ((0, 0), (0, W - x.shape[1])))  # noqa: E731
    return list(cases), np.stack([pad(p) for p, _ in cases.values()]), np.stack([pad(t) for _, t in cases.values()])
