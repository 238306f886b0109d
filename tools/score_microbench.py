"""Point-scoring timing: one cs_score_points launch on --images images of --cells annotations and as many detections each
(about half of them match), device-event timed after warm-up, next to the numpy restatement (tests/score_ref.py) on the host for
the same inputs.  Only the launch is timed: the points are on the device beforehand and nothing is copied back inside the timed
region.  Checks that the GPU counts equal the restatement's.

    python tools/score_microbench.py --images 1024 --cells 32 --path wave
    python tools/score_microbench.py --images 1 --cells 4096 --path block [--reps 20] [--json PATH]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--cells", type=int, default=32, help="annotations and detections per image")
    ap.add_argument("--path", choices=("wave", "block"), default="wave", help="block: the 256-thread path at any size")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None, help="also write the result to this file")
    args = ap.parse_args()
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
