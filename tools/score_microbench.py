"""Point-scoring timing: one cs_score_points launch on --images images of --cells annotations and as many detections each
(about half of them match), device-event timed after warm-up, next to the numpy restatement (tests/score_ref.py) on the host for
the same inputs.  Only the launch is timed: the points are on the device beforehand and nothing is copied back inside the timed
region.  Checks that the GPU counts equal the restatement's.

    python tools/score_microbench.py --images 1024 --cells 32 --path wave
    python tools/score_microbench.py --images 1 --cells 4096 --path block [--reps 20] [--json PATH]

--labels times ``regions.match_labels`` (object matching of two label images at IoU > 1/2) with a fixed ``max_regions`` on the blob
batches of tools/regions_microbench.py (128 x 299^2, and one 4096^2): pred = ``split`` at one seed per component, truth = the same
masks shifted by a few pixels and relabelled.  Device events around the whole call, the median of 7 after a warm-up, next to two
``measure_labels`` calls (one per label image: the same walk done twice) on the same inputs.  Two images of the batch are checked
against tests/match_ref.py, the whole-slide image against a sparse pair count.

    python tools/score_microbench.py --labels [--json PATH]

--labels --overlap also times ``regions.overlap_labels`` (every overlapping pair and each label's best partner: the tables behind
AJI and object-level Dice) on the same label pairs with the same ``max_regions`` and ``max_pairs = 4 max_regions``, timed the same
way right after ``match_labels``; the pair list of two images is checked against a sparse pair count on the host.

    python tools/score_microbench.py --labels --overlap [--json PATH]

--labels --overlap --hausdorff also times ``regions.hausdorff_labels`` (the squared Hausdorff distance of every object to its
partner: the table behind the object-level Hausdorff distance) on the same label pairs WITH that overlap table given, so the time is
the six launches of its own, next to ``overlap_labels_ms`` from the same run.  It reports the jobs at most (one per object with a
partner, one per candidate for every other object: the bounding boxes spare most of the latter), the objects without a partner and
the largest number of horizontal runs of one object
(``kernels.regions_hausdorff_stage_runs()`` of them are staged at a time).  Up to 200 objects of the first image are checked
against ``scipy.ndimage.distance_transform_edt`` on the box that holds the object and its partner.

    python tools/score_microbench.py --labels --overlap --hausdorff [--json PATH]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import score_ref as R  # noqa: E402
from cellsegmentation_amd import kernels as K  # noqa: E402


def time_dev(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), ts


def sparse_match(pred, truth, cap):
    """one image pair -> (match, inter) int64 [cap] from the distinct (pred, truth) pairs: for label counts a dense table cannot hold"""
    p, g = (np.where((x < 0) | (x > cap), 0, x).astype(np.int64).ravel() for x in (pred, truth))
    ap, at = np.bincount(p, minlength=cap + 1), np.bincount(g, minlength=cap + 1)
    keys, inter = np.unique(p * (cap + 1) + g, return_counts=True)
    kp, kg = keys // (cap + 1), keys % (cap + 1)
    hit = (kp > 0) & (kg > 0) & (2 * inter > ap[kp] + at[kg] - inter)
    match, shared = np.zeros(cap + 1, np.int64), np.zeros(cap + 1, np.int64)
    match[kp[hit]], shared[kp[hit]] = kg[hit], inter[hit]
    return match[1:], shared[1:]


def sparse_pairs(pred, truth, cap):
    """one image pair -> (pred, truth, inter) int64 of the distinct pairs of positive labels within cap, sorted"""
    p, g = (np.where((x < 0) | (x > cap), 0, x).astype(np.int64).ravel() for x in (pred, truth))
    both = (p > 0) & (g > 0)
    keys, inter = np.unique(p[both] * (cap + 1) + g[both], return_counts=True)
    return keys // (cap + 1), keys % (cap + 1), inter.astype(np.int64)


def most_runs(labels):
    """int label images [N, H, W] -> the largest number of horizontal runs that one label of one image has"""
    most = 0
    for lab in labels:
        starts = (lab > 0) & (lab != np.pad(lab, ((0, 0), (1, 0)))[:, :-1])
        if starts.any():
            most = max(most, int(np.bincount(lab[starts]).max()))
    return most


def edt_h2(pred, truth, p, g):
    """one image pair -> the squared Hausdorff distance of pred label p and truth label g, by distance transforms on the box that
    holds both"""
    import scipy.ndimage
    rows, cols = np.nonzero((pred == p) | (truth == g))
    box = (slice(rows.min(), rows.max() + 1), slice(cols.min(), cols.max() + 1))
    a, b = pred[box] == p, truth[box] == g
    to_b, to_a = scipy.ndimage.distance_transform_edt(~b), scipy.ndimage.distance_transform_edt(~a)
    return max(int(np.rint(to_b[a].max() ** 2)), int(np.rint(to_a[b].max() ** 2)))


def hausdorff_part(G, pred, truth, hp, ht, o, cap, pairs):
    """the --hausdorff columns of one label pair and whether the checked objects agree with the host"""
    ms, ts = time_dev(lambda: G.hausdorff_labels(pred, truth, overlap=o), 7)
    h = G.hausdorff_labels(pred, truth, overlap=o)
    own = G.hausdorff_labels(pred, truth, max_regions=cap, max_pairs=pairs)
    ok = all(torch.equal(getattr(h, k), getattr(own, k)) for k in ("partner_truth", "d2_truth", "partner_pred", "d2_pred"))
    tabs = {k: getattr(h, k).cpu().numpy() for k in ("area_pred", "area_truth", "partner_truth", "d2_truth", "partner_pred", "d2_pred")}
    given = {"truth": o.inter_partner_truth.cpu().numpy(), "pred": o.inter_partner_pred.cpu().numpy()}
    jobs = lone = 0
    for side, other in (("truth", "pred"), ("pred", "truth")):
        obj = tabs[f"area_{side}"] > 0
        alone = obj & (given[side] == 0)
        lone += int(alone.sum())
        jobs += int((obj & ~alone).sum()) + int((alone.sum(axis=1) * (tabs[f"area_{other}"] > 0).sum(axis=1)).sum())
        ok &= bool(np.array_equal(tabs[f"partner_{side}"][~alone], given[side][~alone]))
        ok &= bool(((tabs[f"d2_{side}"] >= 0) == (tabs[f"partner_{side}"] > 0)).all())
    for g in np.nonzero(tabs["partner_truth"][0])[0][:100]:
        ok &= edt_h2(hp[0], ht[0], tabs["partner_truth"][0, g], g + 1) == tabs["d2_truth"][0, g]
    for p in np.nonzero(tabs["partner_pred"][0])[0][:100]:
        ok &= edt_h2(hp[0], ht[0], p + 1, tabs["partner_pred"][0, p]) == tabs["d2_pred"][0, p]
    sc = h.score().hausdorff_obj
    fin = np.isfinite(sc)
    return {"hausdorff_labels_ms": ms, "hausdorff_labels_ms_all": ts, "hausdorff_jobs": jobs, "objects_without_partner": lone,
            "most_runs": max(most_runs(hp), most_runs(ht)), "stage_runs": K.regions_hausdorff_stage_runs(),
            "hausdorff_obj_mean": float(sc[fin].mean()) if fin.any() else 0.0, "hausdorff_undefined": int((~fin).sum())}, bool(ok)


def labels_main(args):
    import match_ref as M
    import regions_microbench as RM
    from cellsegmentation_amd import regions as G
    dev = torch.device("cuda:0")
    res = {}
    for name, masks in RM.mask_sets():
        cap = RM.MAX_REGIONS[name]
        d = torch.from_numpy(masks).to(dev)
        pts, off = RM.seeds_in_components(G.label(d).cpu().numpy(), 1, seed=1)
        pred = G.split(d, torch.from_numpy(pts).to(dev), torch.from_numpy(off).to(dev)).labels
        truth = G.label(torch.from_numpy(np.roll(masks, (3, 2), axis=(1, 2))).to(dev))
        match_ms, ts = time_dev(lambda: G.match_labels(pred, truth, max_regions=cap), 7)
        twice_ms, _ = time_dev(lambda: (G.measure_labels(pred, max_regions=cap), G.measure_labels(truth, max_regions=cap)), 7)
        t = G.match_labels(pred, truth, max_regions=cap)
        ok = True
        hp, ht = pred.cpu().numpy(), truth.cpu().numpy()
        for i in range(min(2, len(masks))):
            got = {k: getattr(t, k)[i].cpu().numpy() for k in ("area_pred", "area_truth", "match", "inter", "match_truth")}
            if cap <= 1024:
                ref = M.match(hp[i], ht[i], cap, cap)
                ok &= all(np.array_equal(got[k], ref[k][0]) for k in got)
            else:
                match, shared = sparse_match(hp[i], ht[i], cap)
                ok &= bool(np.array_equal(got["match"], match) and np.array_equal(got["inter"], shared))
        extra = {}
        if args.overlap:
            pairs = 4 * cap
            over_ms, over_ts = time_dev(lambda: G.overlap_labels(pred, truth, max_regions=cap, max_pairs=pairs), 7)
            o = G.overlap_labels(pred, truth, max_regions=cap, max_pairs=pairs)
            image, op, og, oi = o.pairs()
            for i in range(min(2, len(masks))):
                want = sparse_pairs(hp[i], ht[i], cap)
                ok &= all(np.array_equal(a[image == i], b) for a, b in zip((op, og, oi), want))
            ok &= bool(torch.equal(o.area_pred, t.area_pred) and torch.equal(o.area_truth, t.area_truth))
            os_ = o.score()
            extra = {"overlap_labels_ms": over_ms, "overlap_labels_ms_all": over_ts, "max_pairs": pairs, "pairs": int(len(image)),
                     "dropped": int(o.dropped.sum()), "aji_mean": float(os_.aji.mean()), "dice_obj_mean": float(os_.dice_obj.mean())}
            if args.hausdorff:
                more, same = hausdorff_part(G, pred, truth, hp, ht, o, cap, pairs)
                extra.update(more)
                ok &= same
        s = t.score()
        res[name] = {"match_labels_ms": match_ms, "match_labels_ms_all": ts, "two_measure_labels_ms": twice_ms, "max_regions": cap,
                     "objects_pred": int(s.n_pred.sum()), "objects_truth": int(s.n_truth.sum()), "matched": int(s.tp.sum()),
                     "pq_mean": float(s.pq.mean()), "overflowed": int(t.overflowed().sum()), **extra, "equal_to_host": bool(ok)}
        print(json.dumps({name: res[name]}), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    if not all(v["equal_to_host"] for v in res.values()):
        sys.exit(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--labels", action="store_true", help="time regions.match_labels next to two measure_labels calls instead")
    ap.add_argument("--overlap", action="store_true", help="with --labels: also time regions.overlap_labels on the same label pairs")
    ap.add_argument("--hausdorff", action="store_true", help="with --labels --overlap: also time regions.hausdorff_labels on that table")
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--cells", type=int, default=32, help="annotations and detections per image")
    ap.add_argument("--path", choices=("wave", "block"), default="wave", help="block: the 256-thread path at any size")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None, help="also write the result to this file")
    args = ap.parse_args()
    if args.overlap and not args.labels:
        ap.error("--overlap goes with --labels")
    if args.hausdorff and not args.overlap:
        ap.error("--hausdorff goes with --labels --overlap")
    if args.labels:
        return labels_main(args)
    if args.path == "wave" and args.cells > 64:
        ap.error("the wave path serves at most 64 annotations per image")
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(0)
    field = R.field_for(args.cells, args.cells)
    hat, hoff = R.ragged([R.random_points(rng, args.cells, field) for _ in range(args.images)])
    gt, goff = R.ragged([R.random_points(rng, args.cells, field) for _ in range(args.images)])
    d = [torch.from_numpy(a).to(dev) for a in (hat, hoff, gt.astype(np.int32), goff)]
    ws = K.score_workspace(args.images, len(gt), dev)
    ms, ts = time_dev(lambda: K.score_points(*d, force_block=args.path == "block", ws=ws), args.reps)
    counts = K.score_points(*d, force_block=args.path == "block", ws=ws)[0].cpu().numpy()
    t0 = time.perf_counter()
    want = R.score_batch(hat, hoff, gt, goff)[0]
    host_ms = (time.perf_counter() - t0) * 1e3
    res = {"images": args.images, "cells": args.cells, "path": args.path, "device_ms": ms, "device_ms_all": ts, "host_ms": host_ms,
           "matched": int(counts[:, 0].sum()), "detections": int(len(hat)), "equal_to_host": bool(np.array_equal(counts, want))}
    print(json.dumps(res), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    if not res["equal_to_host"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
