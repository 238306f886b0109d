"""The numpy statement of ``regions.hausdorff_labels`` and ``HausdorffTable.score``: per pair of objects the dense table of
squared pixel distances in int64, a loop over every candidate for an object that overlaps nothing, and the score in plain float64.
It shares nothing with the device's staged runs or with ``score.hausdorff_score``; the partners of overlapping objects come from
tests/overlap_ref.py.  Only for small objects (the distance table of a pair is |A| x |B|).

Inputs: int32 label images [H, W] or [N, H, W], values <= 0 = background.  A label above its side's capacity is background on that
side.  An object is a label that owns a pixel.  Per image:

  d2(A -> B)   the maximum over ALL pixels a of A of the minimum over the pixels b of B of dr^2 + dc^2
  H2(A, B)     max(d2(A -> B), d2(B -> A))
  partner      the best-intersection partner of ``overlap_ref`` where the object has one; otherwise the object of the other side
               of smallest H2, equal H2 going to the lower label; 0 when the other side has no object
  d2           H2(object, partner); -1 where the row is no object or has no partner
  score        1/2 (sum_g At[g] / sum At * sqrt(d2_truth[g]) + sum_p Ap[p] / sum Ap * sqrt(d2_pred[p])) over the objects in
               ascending label; 0.0 when neither side has an object, inf when exactly one side has none
"""
import numpy as np

import overlap_ref as O
from match_ref import runs

TABLES = ("partner_truth", "d2_truth", "partner_pred", "d2_pred")
CARRIED = ("counts_pred", "counts_truth", "area_pred", "area_truth")
SCORES = ("n_pred", "n_truth", "term_truth", "term_pred", "hausdorff_obj")


def directed(a, b):
    """a, b: int64 [k, 2] pixel coordinates, neither empty -> d2(a -> b) as a Python int"""
    worst = 0
    for at in range(0, len(a), 512):                                   # (a block of the table at a time)
        d = ((a[at:at + 512, None, :] - b[None, :, :]) ** 2).sum(axis=2)
        worst = max(worst, int(d.min(axis=1).max()))
    return worst


def h2(a, b):
    return max(directed(a, b), directed(b, a))


def hausdorff(pred, truth, cap_pred=None, cap_truth=None):
    """-> dict: the TABLES (int32 [N, cap_truth] / [N, cap_pred]), the CARRIED tables of ``overlap_ref.overlap``, cap_pred,
    cap_truth, and ``overlap`` = that reference's whole result"""
    ov = O.overlap(pred, truth, cap_pred, cap_truth)
    cp, ct = ov["cap_pred"], ov["cap_truth"]
    pred, truth = np.asarray(pred), np.asarray(truth)
    if pred.ndim == 2:
        pred, truth = pred[None], truth[None]
    N = len(pred)
    out = {k: ov[k] for k in CARRIED}
    out.update(cap_pred=cp, cap_truth=ct, overlap=ov)
    out.update(partner_truth=np.zeros((N, ct), np.int32), d2_truth=np.full((N, ct), -1, np.int32),
               partner_pred=np.zeros((N, cp), np.int32), d2_pred=np.full((N, cp), -1, np.int32))
    for n in range(N):
        p = np.where((pred[n] > cp) | (pred[n] < 0), 0, pred[n])
        g = np.where((truth[n] > ct) | (truth[n] < 0), 0, truth[n])
        px_p = {int(k): np.argwhere(p == k).astype(np.int64) for k in np.unique(p) if k > 0}
        px_t = {int(k): np.argwhere(g == k).astype(np.int64) for k in np.unique(g) if k > 0}
        for own, other, given, partner, d2 in ((px_t, px_p, ov["inter_partner_truth"][n], out["partner_truth"][n], out["d2_truth"][n]),
                                               (px_p, px_t, ov["inter_partner_pred"][n], out["partner_pred"][n], out["d2_pred"][n])):
            for k in sorted(own):
                if given[k - 1] > 0:
                    partner[k - 1], d2[k - 1] = given[k - 1], h2(own[k], other[int(given[k - 1])])
                    continue
                best = None
                for c in sorted(other):                                   # ascending: only a strictly smaller H2 replaces the holder
                    d = h2(own[k], other[c])
                    if best is None or d < best[0]:
                        best = (d, c)
                if best is not None:
                    d2[k - 1], partner[k - 1] = best
    return out


def score(t):
    """the tables of ``hausdorff`` -> dict of per-image arrays: n_pred, n_truth int64; term_truth, term_pred, hausdorff_obj
    float64"""
    N = len(t["area_pred"])
    out = {k: np.zeros((N,), np.int64 if k in ("n_pred", "n_truth") else np.float64) for k in SCORES}
    for n in range(N):
        terms = []
        for area, d2 in ((t["area_truth"][n], t["d2_truth"][n]), (t["area_pred"][n], t["d2_pred"][n])):
            area = [int(v) for v in area]
            acc = np.float64(0.0)
            for k in range(len(area)):
                if area[k] > 0:
                    acc = acc + np.float64(area[k]) / np.float64(sum(area)) * (np.sqrt(np.float64(int(d2[k]))) if d2[k] >= 0 else np.inf)
            terms.append(acc)
        n_truth, n_pred = int((t["area_truth"][n] > 0).sum()), int((t["area_pred"][n] > 0).sum())
        out["n_pred"][n], out["n_truth"][n] = n_pred, n_truth
        if n_pred and n_truth:
            out["term_truth"][n], out["term_pred"][n] = terms
            out["hausdorff_obj"][n] = (terms[0] + terms[1]) / 2
        elif n_pred or n_truth:
            out["term_truth"][n], out["term_pred"][n] = (np.inf if n_truth else 0.0), (np.inf if n_pred else 0.0)
            out["hausdorff_obj"][n] = np.inf
    return out


def square_in_frame():
    """A = the filled 5 x 5 square at rows and columns 2..6 of a 9 x 9 image, B = the image's one-pixel frame: d2(A -> B) = 16 at
    A's centre only (A's boundary pixels reach 4), d2(B -> A) = 8 at the corners"""
    a, b = np.zeros((9, 9), np.int32), np.ones((9, 9), np.int32)
    a[2:7, 2:7] = 1
    b[1:8, 1:8] = 0
    return a, b


def hand_cases():
    """name -> (pred, truth): small int32 images worked by hand (tests/test_hausdorff_host.py has the answers)"""
    sq, frame = square_in_frame()
    return {
        "apart": (runs((1, 3), (0, 6)), runs((0, 5), (1, 1), (0, 3))),        # pred on columns 0..2, truth on column 5: 25 both ways
        "identical": (runs((0, 1), (2, 4), (0, 1)), runs((0, 1), (2, 4), (0, 1))),
        "square_in_frame": (sq, frame),
        "frame_in_square": (frame, sq),
        "both_empty": (runs((0, 5)), runs((0, 5))),
        "pred_empty": (runs((0, 5)), runs((0, 1), (1, 3), (0, 1))),
        "truth_empty": (runs((2, 3), (0, 2)), runs((-1, 5))),
        # truth 1 on columns 0..8 meets pred 1 on 2 px (columns 3..4, H2 = 16) and pred 2 on 3 px (6..8, H2 = 36): partner 2,
        # the larger intersection, not the smaller distance
        "larger_intersection": (runs((0, 3), (1, 2), (0, 1), (2, 3), (0, 1)), runs((1, 9), (0, 1))),
        # truth 1 (columns 4..5) overlaps nothing; pred 1 (0..1) and pred 3 (8..9) mirror each other at H2 = 16 (label 2 owns
        # nothing and is no candidate), pred 4 (12) is farther: the lower label
        "mirror_tie": (runs((1, 2), (0, 6), (3, 2), (0, 2), (4, 1)), runs((0, 4), (1, 2), (0, 7))),
        # truth 1 (column 0) overlaps nothing: pred 2 (column 3) is nearer than pred 1 (columns 6..7)
        "nearest_candidate": (runs((0, 3), (2, 1), (0, 2), (1, 2)), runs((1, 1), (0, 7))),
    }


def stacked(cases=None):
    """the hand cases, each padded with background to the largest, as one batch -> (names, pred, truth int32 [N, H, W])"""
    cases = hand_cases() if cases is None else cases
    H, W = max(p.shape[0] for p, _ in cases.values()), max(p.shape[1] for p, _ in cases.values())
    pad = lambda x: np.pad(x, ((0, H - x.shape[0]), (0, W - x.shape[1])))  # noqa: E731
    return list(cases), np.stack([pad(p) for p, _ in cases.values()]), np.stack([pad(t) for _, t in cases.values()])


def comb(teeth_rows, W):
    """int32 [teeth_rows + 1, W]: row 0 full, below it every other column: teeth_rows ceil(W / 2) + 1 horizontal runs"""
    m = np.zeros((teeth_rows + 1, W), np.int32)
    m[0] = 1
    m[1:, ::2] = 1
    return m
