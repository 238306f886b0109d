"""Cell localisation timing: 128 probability maps of 299^2 (quantise + blur + mean shift + clustering, one batch) and one stitched
4096^2 mask, device-event timed after warm-up, next to the numpy restatement (tests/detect_ref.py) on the host for the same work.
Checks that the GPU outputs equal the restatement.

    python tools/detect_microbench.py [--reps 5] [--host-maps 128] [--json PATH]
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

import detect_ref as R  # noqa: E402
from cellsegmentation_amd import detect as D  # noqa: E402


def blob_probs(n, H, W, density, seed):
    """float32 maps with Gaussian blobs of radius 3-6 px (roughly cell-sized)."""
    rng = np.random.RandomState(seed)
    out = np.zeros((n, H, W), np.float32)
    k = 13
    yy, xx = np.mgrid[-k:k + 1, -k:k + 1]
    for i in range(n):
        m = np.zeros((H + 2 * k, W + 2 * k), np.float32)
        for cy, cx in zip(rng.randint(0, H, int(H * W * density)), rng.randint(0, W, int(H * W * density))):
            r = rng.uniform(3, 6)
            blob = np.exp(-(yy ** 2 + xx ** 2) / (2 * r * r)).astype(np.float32)
            np.maximum(m[cy:cy + 2 * k + 1, cx:cx + 2 * k + 1], blob, out=m[cy:cy + 2 * k + 1, cx:cx + 2 * k + 1])
        out[i] = m[k:k + H, k:k + W]
    return out


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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-maps", type=int, default=128, help="maps of the batch also run (and checked) on the host")
    ap.add_argument("--json", default=None, help="also write the results to this file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {}
    # ---- 128 maps of 299^2
    probs = blob_probs(128, 299, 299, 1 / 1500, seed=1)
    pd = torch.from_numpy(probs).to(dev)

    def gpu_batch():
        return D._detect(pd, None, 0.2, 16, 10, 11, (15, 15), 3., 0., 100, False)
    ms, ts = time_dev(gpu_batch, args.reps)
    out = gpu_batch()
    t0 = time.perf_counter()
    ok = True
    for i in range(args.host_maps):
        want = R.detect(R.quantize(probs[i]), None, eps=11)[0]
        ok &= bool(np.array_equal(out.points[out.offsets[i]:out.offsets[i + 1]], want))
    host_ms = (time.perf_counter() - t0) * 1e3
    res["batch128_299"] = {"device_ms": ms, "device_ms_all": ts, "host_ms": host_ms, "host_maps": args.host_maps,
                           "cells": int(out.offsets[-1]), "windows_kept": int(out.n_kept.sum()), "equal_to_host": ok}
    print(json.dumps({"batch128_299": res["batch128_299"]}), flush=True)
    # ---- one stitched 4096^2 mask: 299^2 patches overlapping by 16 px, border-aligned last row / column
    H = W = 4096
    step = 299 - 16
    origins = list(range(0, H - 299 + 1, step))
    if origins[-1] != H - 299:
        origins.append(H - 299)
    grid = [(r, c) for r in origins for c in origins]
    patches = blob_probs(len(grid), 299, 299, 1 / 1500, seed=2)
    pq = D.quantize(torch.from_numpy(patches).to(dev))
    whole = D.stitch_patches(pq, grid, (H, W))

    def gpu_whole():
        return D._detect(whole[None], None, 0.2, 16, 10, 11, (15, 15), 3., 0., 100, False)
    ms, ts = time_dev(gpu_whole, args.reps)
    out = gpu_whole()
    t0 = time.perf_counter()
    mask = R.stitch(R.quantize(patches), grid, (H, W))
    want = R.detect(mask, None, eps=11)[0]
    host_ms = (time.perf_counter() - t0) * 1e3
    ok = bool(np.array_equal(whole.cpu().numpy(), mask)) and bool(np.array_equal(out.points, want))
    res["stitched_4096"] = {"device_ms": ms, "device_ms_all": ts, "host_ms": host_ms, "patches": len(grid), "cells": int(out.offsets[-1]),
                            "windows_kept": int(out.n_kept.sum()), "equal_to_host": ok}
    print(json.dumps({"stitched_4096": res["stitched_4096"]}), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    if not all(v["equal_to_host"] for v in res.values()):
        sys.exit(1)


if __name__ == "__main__":
    main()
