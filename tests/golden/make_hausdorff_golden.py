"""Writes tests/golden/hausdorff_vectors.npz: small pairs of label images with the tables of ``regions.hausdorff_labels`` and the
score of ``HausdorffTable.score``, by a route that shares nothing with tests/hausdorff_ref.py: the directed distance d2(A -> B) is
``scipy.ndimage.distance_transform_edt`` of the complement of B sampled on A, squared and rounded (a Euclidean distance between
pixels is the root of an integer, so rounding its square recovers the integer), intersections come from ``numpy.unique`` of the
label pairs, and the score is summed with ``math.fsum``.  The host test holds the reference to these bytes; the GPU test holds the
kernels to them.

    python tests/golden/make_hausdorff_golden.py
"""
import math
import os
import sys

import numpy as np
import scipy.ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import hausdorff_ref as HR  # noqa: E402  (the inputs only: hand cases and the comb)
import match_ref as M  # noqa: E402
import regions_ref as R  # noqa: E402

TABLES = ("area_pred", "area_truth", "partner_truth", "d2_truth", "partner_pred", "d2_pred")
SCORES = ("term_truth", "term_pred", "hausdorff_obj")


def cases():
    """name -> (pred, truth int32 [N, H, W])"""
    _, pred, truth = HR.stacked()
    yield "hand", (pred, truth)
    masks = R.blobs(2, 40, 70, seed=3, density=1 / 200.0)
    pred, truth = M.noisy_pair(masks, 4, lambda m: R.label(m)[0])
    truth[0][truth[0] == 2] = 0                                          # objects of pred that overlap nothing
    pred[1][pred[1] == 1] = 0                                            # and of truth
    yield "blobs", (pred, truth)


def h2(a, b):
    """bool [H, W] masks, neither empty -> the squared Hausdorff distance"""
    to_b, to_a = scipy.ndimage.distance_transform_edt(~b), scipy.ndimage.distance_transform_edt(~a)
    return max(int(np.rint(to_b[a].max() ** 2)), int(np.rint(to_a[b].max() ** 2)))


def tables(pred, truth):
    N = len(pred)
    cp, ct = max(1, int(pred.max())), max(1, int(truth.max()))
    out = {"area_pred": np.zeros((N, cp), np.int32), "area_truth": np.zeros((N, ct), np.int32),
           "partner_truth": np.zeros((N, ct), np.int32), "d2_truth": np.full((N, ct), -1, np.int32),
           "partner_pred": np.zeros((N, cp), np.int32), "d2_pred": np.full((N, cp), -1, np.int32)}
    for n in range(N):
        sides = {"pred": np.maximum(pred[n], 0), "truth": np.maximum(truth[n], 0)}
        for own, other in (("truth", "pred"), ("pred", "truth")):
            labels, areas = np.unique(sides[own][sides[own] > 0], return_counts=True)
            candidates = np.unique(sides[other][sides[other] > 0])
            for k, area in zip(labels, areas):
                out[f"area_{own}"][n, k - 1] = area
                mask = sides[own] == k
                met, inter = np.unique(sides[other][mask & (sides[other] > 0)], return_counts=True)
                if len(met):
                    partner = int(met[np.argmax(inter)])                 # argmax: the first of equals = the lower label
                    d2 = h2(mask, sides[other] == partner)
                elif len(candidates):
                    dist = [h2(mask, sides[other] == c) for c in candidates]
                    partner, d2 = int(candidates[int(np.argmin(dist))]), min(dist)
                else:
                    continue
                out[f"partner_{own}"][n, k - 1], out[f"d2_{own}"][n, k - 1] = partner, d2
    return out


def scores(t):
    N = len(t["area_pred"])
    out = {k: np.zeros((N,), np.float64) for k in SCORES}
    for n in range(N):
        terms = {}
        for side in ("truth", "pred"):
            area, d2 = t[f"area_{side}"][n].astype(np.int64), t[f"d2_{side}"][n]
            terms[side] = math.fsum(float(a) / float(area.sum()) * (math.sqrt(int(d)) if d >= 0 else math.inf)
                                    for a, d in zip(area, d2) if a > 0)
        out["term_truth"][n], out["term_pred"][n] = terms["truth"], terms["pred"]
        out["hausdorff_obj"][n] = (terms["truth"] + terms["pred"]) / 2
    return out


def main():
    out = {}
    for name, (pred, truth) in cases():
        t = tables(pred, truth)
        out[f"{name}.pred"], out[f"{name}.truth"] = pred, truth
        for key in TABLES:
            out[f"{name}.{key}"] = t[key]
        for key, col in scores(t).items():
            out[f"{name}.score.{key}"] = col
    path = os.path.join(HERE, "hausdorff_vectors.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
