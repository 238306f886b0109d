"""Detected cell centres against annotated ones: the reference's ``get_prf1`` (test_seg.py:120-141) with ``euclid_dist`` and
``precision_recall`` (metrics/metrics.py:56-66), on the HIP path (csrc/score.hip), for a whole batch in one launch.

Per image, in the order of the detections: a detection takes the nearest annotation that no earlier detection has taken (the
lowest index among equally near ones, as the reference's strict ``<``) and keeps it when the distance is ``<= radius``; otherwise
it is a false positive, also when a nearer annotation is already taken.  ``tp`` = matches, ``fp`` = detections - tp, ``fn`` =
annotations left over.  Coordinates are integers, so the kernel compares squared distances in integers (``d2 <= floor(radius^2)``)
and no float decides anything; the ratios are formed on the host in float64 exactly as ``precision_recall`` forms them.

The result depends on the order of the detections.  ``detect.detect_points`` fixes that order (weight descending, then label
descending), and ``DetectResult.score`` scores the device-resident detections of a batch without copying them back.

``label_score`` is the object-level counterpart for label images: from the integer tables of ``regions.match_labels`` (areas,
partner at IoU > 1/2, intersection) it forms TP / FP / FN at an IoU threshold, the same precision / recall / F1, and segmentation
and panoptic quality -- a few thousand rows of host float64 arithmetic.  ``overlap_score`` does the same for the tables of
``regions.overlap_labels`` (best partner by IoU and by intersection, below IoU 1/2 too): AJI and object-level Dice.
"""
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import kernels as K
from ._args import _device
from ._points import _I32, PointSet, ragged  # noqa: F401  (ragged: the tools build their batches with score.ragged)


def precision_recall(tp, fp, fn, return_f1=False):
    """metrics/metrics.py:60-66 for scalars or integer arrays, in float64: ``p = 1 if tp + fp == 0 else tp / (tp + fp)``,
    ``r = 1 if tp + fn == 0 else tp / (tp + fn)`` and, with return_f1, ``f1 = 0 if p + r == 0 else 2 p r / (p + r)``."""
    a = [np.asarray(v) for v in (tp, fp, fn)]
    for v in a:
        if v.dtype.kind not in "iu":
            raise TypeError(f"precision_recall: counts must be integers, got {v.dtype}")
        if v.size and int(v.min()) < 0:
            raise ValueError("precision_recall: counts must be non-negative")
    tp, fp, fn = (v.astype(np.float64) for v in a)
    with np.errstate(divide="ignore", invalid="ignore"):
        p = np.where(tp + fp == 0, 1.0, tp / (tp + fp))
        r = np.where(tp + fn == 0, 1.0, tp / (tp + fn))
        if not return_f1:
            return p[()], r[()]
        f1 = np.where(p + r == 0, 0.0, (2 * p * r) / (p + r))
    return p[()], r[()], f1[()]


@dataclass
class ScoreResult:
    """Per image (arrays of length N): ``tp``, ``fp``, ``fn`` int64; ``precision``, ``recall``, ``f1`` float64.  ``match`` (int32,
    one entry per detection row, or None): the index of the annotation taken within the detection's own image, -1 for a false
    positive, -2 for a detection that was not scored (beyond its image's limit)."""
    tp: np.ndarray
    fp: np.ndarray
    fn: np.ndarray
    precision: np.ndarray
    recall: np.ndarray
    f1: np.ndarray
    match: object = None


def radius_squared(radius):
    """``floor(radius^2)`` of a non-negative number, below 2^31: integer d2 <= it exactly where sqrt(d2) <= radius."""
    if isinstance(radius, bool) or not isinstance(radius, (int, float, np.integer, np.floating)):
        raise TypeError(f"radius must be a number, got {radius!r}")
    r = float(radius)
    if not math.isfinite(r) or r < 0:
        raise ValueError(f"radius must be finite and non-negative, got {radius!r}")
    r2 = math.floor(r * r)
    if r2 >= 1 << 31:
        raise ValueError(f"radius^2 must stay below 2^31, got radius {radius!r}")
    return int(r2)


def _prepare(points, offsets, n_images, gt_xy):
    """annotations -> their PointSet with (row, col) rows, host rows as int32; no device work"""
    gt = PointSet(points, offsets, None, n_images, "points")
    if gt.on_device:
        gt.pts = gt.pts.flip(1) if gt_xy else gt.pts
        return gt
    g = gt.pts
    if g.size and (int(g.min()) < _I32[0] or int(g.max()) > _I32[1]):
        raise ValueError("points: an annotation coordinate does not fit int32")
    g = g.astype(np.int32)
    gt.pts = np.ascontiguousarray(g[:, ::-1] if gt_xy else g)
    return gt


def _run(hat, n_hat_rows, gt, radius2, return_match, force_block=False):
    """uploaded detections + prepared annotations -> ScoreResult (one copy of the counts to the host, one of match if asked for)"""
    gt.upload(hat.pts_dev.device, torch.int32)
    counts, match = K.score_points(hat.pts_dev, hat.off_dev, gt.pts_dev, gt.off_dev, hat.lim_dev, radius2, want_match=return_match,
                                   force_block=force_block)
    c = counts.cpu().numpy().astype(np.int64)
    if c.min(initial=0) < 0:
        raise ValueError("score_points: the offsets do not describe the point arrays")
    p, r, f1 = precision_recall(c[:, 0], c[:, 1], c[:, 2], return_f1=True)
    m = match[:n_hat_rows].cpu().numpy() if return_match else None
    return ScoreResult(c[:, 0].copy(), c[:, 1].copy(), c[:, 2].copy(), p, r, f1, m)


def score_points(points_hat, points, hat_offsets=None, offsets=None, limits=None, radius=16, gt_xy=False, return_match=False,
                 _force_block=False):
    """Score detections ``points_hat`` against annotations ``points`` -> ScoreResult.

    One pair of ``[n, 2]`` integer arrays, or ragged batches: image n owns ``points_hat[hat_offsets[n]:hat_offsets[n + 1]]`` and
    ``points[offsets[n]:offsets[n + 1]]``.  numpy or torch, on the host or the device.  Both sides use the same coordinate
    convention, unless ``gt_xy``: then the annotations are (x, y) as ``PointTestset`` reads them while the detections are
    (row, col).  ``limits``: None, one count or one per image, applied to every image's detections as Python's slice ``[:c]``
    (what ``DetectResult.per_image`` does with a regression count); detections beyond it are not scored.  ``radius``: a
    non-negative number, the reference's CELL_RADIUS_PXS = 16.  ``_force_block`` (tests) takes the 256-thread path at any size."""
    radius2 = radius_squared(radius)
    hat = PointSet(points_hat, hat_offsets, limits, None, "points_hat")
    gt = _prepare(points, offsets, hat.n_images, gt_xy)
    hat.upload(_device(points_hat, points, hat_offsets, offsets))
    return _run(hat, hat.rows, gt, radius2, return_match, _force_block)


def get_prf1(points_hat, points):
    """test_seg.py:120-141 with its signature and return: ``(p, r, f1, tp, fp, fn)`` of one image, radius 16, both point lists in
    the same coordinate convention; ``np.asarray([])`` is an empty list."""
    res = score_points(points_hat, points)
    return float(res.precision[0]), float(res.recall[0]), float(res.f1[0]), int(res.tp[0]), int(res.fp[0]), int(res.fn[0])


@dataclass
class PositivityScore:
    """Per image (arrays of length N): ``class_counts`` int64 [N, 4], the cells of class 0 (negative), 1+, 2+ and 3+; ``n_cells``
    int64; ``labelling_index`` float64, the positive cells (class >= 1) per cell in percent; ``h_score`` float64 =
    ``100 sum_k k f_k`` with ``f_k`` the fraction of cells in class k, from 0 to 300.  Both are NaN for an image without cells."""
    class_counts: np.ndarray
    n_cells: np.ndarray
    labelling_index: np.ndarray
    h_score: np.ndarray


def positivity_score(class_counts):
    """The cells per intensity class ([m] or [N, m] non-negative integers, 2 <= m <= 4: class 0 = negative, then 1+, 2+, 3+; for
    example the classes of ``stain.StainTable.classify`` counted per image) -> ``PositivityScore``, in numpy float64: the labelling
    index ``100 (n - n_0) / n`` and the H-score ``100 (n_1 + 2 n_2 + 3 n_3) / n``, NaN where ``n = 0``."""
    c = np.asarray(class_counts)
    if c.dtype.kind not in "iu" or c.ndim not in (1, 2) or not 2 <= c.shape[-1] <= 4 or (c.size and int(c.min()) < 0):
        raise ValueError("positivity_score: expected non-negative integer cell counts shaped [m] or [N, m] with 2 <= m <= 4 classes")
    c = np.atleast_2d(c).astype(np.int64)
    c = np.concatenate([c, np.zeros((c.shape[0], 4 - c.shape[1]), np.int64)], axis=1)
    n = c.sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        li = 100.0 * (n - c[:, 0]).astype(np.float64) / n.astype(np.float64)
        hs = 100.0 * (c[:, 1] + 2 * c[:, 2] + 3 * c[:, 3]).astype(np.float64) / n.astype(np.float64)
    return PositivityScore(c, n, li, hs)


@dataclass
class LabelScore:
    """Per image (arrays of length N): ``n_pred``, ``n_truth`` (objects: labels that own a pixel, within the capacity), ``tp``,
    ``fp``, ``fn`` int64; ``precision``, ``recall``, ``f1``, ``sq``, ``pq`` float64."""
    n_pred: np.ndarray
    n_truth: np.ndarray
    tp: np.ndarray
    fp: np.ndarray
    fn: np.ndarray
    precision: np.ndarray
    recall: np.ndarray
    f1: np.ndarray
    sq: np.ndarray
    pq: np.ndarray


def check_iou_threshold(iou_threshold):
    """a float in [0.5, 1] -> float; anything else raises ValueError (below 1/2 a label may have several partners)"""
    t = iou_threshold
    if isinstance(t, bool) or not isinstance(t, (int, float, np.integer, np.floating)) or not 0.5 <= float(t) <= 1.0:
        raise ValueError(f"iou_threshold must be a number in [0.5, 1], got {iou_threshold!r}")
    return float(t)


def label_score(area_pred, area_truth, match, inter, iou_threshold=0.5):
    """The integer tables of ``regions.match_labels`` on the host ([N, cap_pred], [N, cap_truth], [N, cap_pred], [N, cap_pred]) ->
    ``LabelScore``, in numpy float64.  Per image: row p is a TP iff it is matched and ``inter / union >= iou_threshold`` (union =
    area_pred + area_truth[match] - inter, a float64 quotient of the two integers); ``fp = n_pred - tp``, ``fn = n_truth - tp``;
    precision, recall and F1 are ``precision_recall``'s, conventions for empty sides included; ``sq`` = the sum of the TP rows'
    IoU in ascending pred label / tp, 0.0 without a TP; ``pq = sq * f1`` -- F1 is panoptic quality's recognition quality."""
    thr = check_iou_threshold(iou_threshold)
    ap, at, m, it = (np.asarray(x).astype(np.int64) for x in (area_pred, area_truth, match, inter))
    if ap.ndim != 2 or at.ndim != 2 or m.shape != ap.shape or it.shape != ap.shape or at.shape[0] != ap.shape[0]:
        raise ValueError("label_score: expected area_pred, match, inter [N, cap_pred] and area_truth [N, cap_truth]")
    if m.size and (int(m.min()) < 0 or int(m.max()) > at.shape[1]):
        raise ValueError("label_score: match holds a label outside area_truth")
    matched = m > 0
    union = ap + np.take_along_axis(at, np.where(matched, m - 1, 0), axis=1) - it if at.shape[1] else ap
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = np.where(matched, it / union, 0.0)
    hit = matched & (iou >= thr)
    n_pred, n_truth, tp = (ap > 0).sum(axis=1), (at > 0).sum(axis=1), hit.sum(axis=1)
    fp, fn = n_pred - tp, n_truth - tp
    p, r, f1 = (np.atleast_1d(v) for v in precision_recall(tp, fp, fn, True))
    sq = np.asarray([np.sum(iou[n][hit[n]]) / tp[n] if tp[n] else 0.0 for n in range(len(tp))], np.float64)
    return LabelScore(n_pred.astype(np.int64), n_truth.astype(np.int64), tp.astype(np.int64), fp.astype(np.int64), fn.astype(np.int64),
                      p.astype(np.float64), r.astype(np.float64), f1.astype(np.float64), sq, sq * f1)


@dataclass
class OverlapScore:
    """Per image (arrays of length N): ``n_pred``, ``n_truth`` (objects: labels that own a pixel, within the capacity), ``n_pairs``
    (the (pred, truth) pairs that share a pixel), ``aji_inter``, ``aji_union`` int64; ``aji``, ``dice_obj`` float64."""
    n_pred: np.ndarray
    n_truth: np.ndarray
    n_pairs: np.ndarray
    aji_inter: np.ndarray
    aji_union: np.ndarray
    aji: np.ndarray
    dice_obj: np.ndarray


def overlap_score(area_pred, area_truth, iou_partner, iou_inter, inter_partner_truth, inter_truth, inter_partner_pred, inter_pred,
                  n_pairs):
    """The integer tables of ``regions.overlap_labels`` on the host (``area_pred``, ``inter_partner_pred``, ``inter_pred`` [N,
    cap_pred]; the others [N, cap_truth]; ``n_pairs`` [N]) -> ``OverlapScore``, in numpy float64.  An object is a label whose
    area is positive.  Per image, with Ap / At the areas:

    * AJI (aggregated Jaccard index).  Every truth object g with a best-IoU partner j = ``iou_partner`` adds ``I = iou_inter`` to C
      and ``Ap[j] + At[g] - I`` to U and marks j used; one without a partner adds ``At[g]`` to U.  A pred object may serve several
      truth objects and adds a union for each.  Every pred object never used adds ``Ap`` to U.  ``aji = C / U``, one float64
      quotient of the two integers ``aji_inter`` / ``aji_union``; 1.0 when U = 0 (no object on either side, the convention of
      ``precision_recall`` for empty sides).
    * Object-level Dice.  ``dice_obj = (T + P) / 2`` with ``T = sum_g (At[g] / sum At) * 2 I / (Ap[s] + At[g])`` over the truth
      objects in ascending label, s = ``inter_partner_truth`` and I = ``inter_truth`` (the term is 0 without a partner), and P the
      same sum over the pred objects with ``inter_partner_pred`` / ``inter_pred``.  A side without objects contributes 0; 1.0 when
      both sides have none.

    Partners by IoU for AJI and by intersection for Dice, ties to the lower label: the rules of ``regions.overlap_labels``."""
    ap, at, jp, ji, sp, si, gp, gi = (np.asarray(x).astype(np.int64) for x in (
        area_pred, area_truth, iou_partner, iou_inter, inter_partner_truth, inter_truth, inter_partner_pred, inter_pred))
    npairs = np.asarray(n_pairs).astype(np.int64)
    if ap.ndim != 2 or at.ndim != 2 or at.shape[0] != ap.shape[0] or any(x.shape != at.shape for x in (jp, ji, sp, si)) or any(
            x.shape != ap.shape for x in (gp, gi)) or npairs.shape != ap.shape[:1]:
        raise ValueError("overlap_score: expected area_pred, inter_partner_pred, inter_pred [N, cap_pred], area_truth, iou_partner, "
                         "iou_inter, inter_partner_truth, inter_truth [N, cap_truth] and n_pairs [N]")
    for part, cap in ((jp, ap.shape[1]), (sp, ap.shape[1]), (gp, at.shape[1])):
        if part.size and (int(part.min()) < 0 or int(part.max()) > cap):
            raise ValueError("overlap_score: a partner table holds a label outside the other side's areas")
    N = ap.shape[0]
    out = OverlapScore(*(np.zeros((N,), np.int64) for _ in range(5)), *(np.zeros((N,), np.float64) for _ in range(2)))
    for n in range(N):
        used = np.zeros((ap.shape[1] + 1,), bool)
        C = U = 0
        for g in np.nonzero(at[n])[0]:
            j = int(jp[n, g])
            if j:
                C += int(ji[n, g])
                U += int(ap[n, j - 1]) + int(at[n, g]) - int(ji[n, g])
                used[j] = True
            else:
                U += int(at[n, g])
        U += int(ap[n][(ap[n] > 0) & ~used[1:]].sum())
        sides = []
        for own, other, partner, inter in ((at[n], ap[n], sp[n], si[n]), (ap[n], at[n], gp[n], gi[n])):
            total, acc = np.float64(own.sum()), np.float64(0.0)
            for k in np.nonzero(own)[0]:
                if partner[k]:
                    acc += (np.float64(own[k]) / total) * (np.float64(2 * inter[k]) / np.float64(other[partner[k] - 1] + own[k]))
            sides.append(acc)
        n_truth, n_pred = int((at[n] > 0).sum()), int((ap[n] > 0).sum())
        out.n_pred[n], out.n_truth[n], out.n_pairs[n], out.aji_inter[n], out.aji_union[n] = n_pred, n_truth, npairs[n], C, U
        out.aji[n] = np.float64(C) / np.float64(U) if U else 1.0
        out.dice_obj[n] = 0.5 * (sides[0] + sides[1]) if n_pred or n_truth else 1.0
    return out


@dataclass
class HausdorffScore:
    """Per image (arrays of length N): ``n_pred``, ``n_truth`` (objects: labels that own a pixel, within the capacity) int64;
    ``term_truth``, ``term_pred``, ``hausdorff_obj`` float64, in pixels."""
    n_pred: np.ndarray
    n_truth: np.ndarray
    term_truth: np.ndarray
    term_pred: np.ndarray
    hausdorff_obj: np.ndarray


def hausdorff_score(area_pred, area_truth, d2_truth, d2_pred):
    """The integer tables of ``regions.hausdorff_labels`` on the host (``area_pred``, ``d2_pred`` [N, cap_pred]; ``area_truth``,
    ``d2_truth`` [N, cap_truth]) -> ``HausdorffScore``, in numpy float64.  An object is a label whose area is positive; ``d2`` is
    the squared Hausdorff distance of the object to its partner.  Per image, with Ap / At the areas:

    * ``term_truth = sum_g (At[g] / sum At) * sqrt(d2_truth[g])`` over the truth objects in ascending label, ``term_pred`` the same
      sum over the pred objects, and ``hausdorff_obj = (term_truth + term_pred) / 2``: the object-level Hausdorff distance of the
      GlaS challenge, where lower is better.
    * No object on either side: all three are 0.0.  Exactly one side without objects: the objects of the other have no partner, the
      score is undefined and ``hausdorff_obj`` and that side's term are ``inf`` (the empty side's term is 0.0) -- a value that cannot
      be taken for a good one."""
    ap, at, dt, dp = (np.asarray(x).astype(np.int64) for x in (area_pred, area_truth, d2_truth, d2_pred))
    if ap.ndim != 2 or at.ndim != 2 or at.shape[0] != ap.shape[0] or dt.shape != at.shape or dp.shape != ap.shape:
        raise ValueError("hausdorff_score: expected area_pred, d2_pred [N, cap_pred] and area_truth, d2_truth [N, cap_truth]")
    N = ap.shape[0]
    out = HausdorffScore(*(np.zeros((N,), np.int64) for _ in range(2)), *(np.zeros((N,), np.float64) for _ in range(3)))
    for n in range(N):
        terms = []
        for own, d2 in ((at[n], dt[n]), (ap[n], dp[n])):
            total, acc = np.float64(own.sum()), np.float64(0.0)
            for k in np.nonzero(own)[0]:
                acc += (np.float64(own[k]) / total) * (np.sqrt(np.float64(d2[k])) if d2[k] >= 0 else np.inf)
            terms.append(acc)
        out.n_truth[n], out.n_pred[n] = int((at[n] > 0).sum()), int((ap[n] > 0).sum())
        out.term_truth[n], out.term_pred[n] = terms
        out.hausdorff_obj[n] = 0.5 * (terms[0] + terms[1])
    return out
