"""Small-region clean-up timing: remove_small_regions(., 300, 100) of 128 thresholded maps of 299^2 (one batch) and of one 4096^2
whole-image mask, device-event timed after warm-up, next to the numpy restatement (tests/regions_ref.py) on the host for the
same work.  Checks that the GPU outputs equal the restatement.

    python tools/regions_microbench.py [--reps 5] [--host-maps 128] [--json PATH]
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

import regions_ref as R  # noqa: E402
from cellsegmentation_amd import regions as G  # noqa: E402

MIN_OBJECT, MAX_HOLE = 300, 100


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


def case(name, masks, reps, host_maps, dev):
    d = torch.from_numpy(masks).to(dev)
    out = torch.empty_like(d)
    ms, ts = time_dev(lambda: G.remove_small_regions(d, MIN_OBJECT, MAX_HOLE, out=out), reps)
    got = out.cpu().numpy()
    t0 = time.perf_counter()
    ok = True
    for i in range(host_maps):
        ok &= bool(np.array_equal(got[i], R.remove_small_regions(masks[i], MIN_OBJECT, MAX_HOLE)))
    host_ms = (time.perf_counter() - t0) * 1e3
    res = {"device_ms": ms, "device_ms_all": ts, "host_ms": host_ms, "host_maps": host_maps, "pixels_changed": int((got != masks).sum()),
           "equal_to_host": ok}
    print(json.dumps({name: res}), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-maps", type=int, default=128, help="maps of the batch also run (and checked) on the host")
    ap.add_argument("--json", default=None, help="also write the results to this file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"batch128_299": case("batch128_299", R.blobs(128, 299, 299, seed=1), args.reps, min(args.host_maps, 128), dev)}
    # one whole-image mask: 299^2 blob patches tiled into 4096^2 (objects and holes cross the patch seams)
    patches = R.blobs(14 * 14, 299, 299, seed=2)
    whole = patches.reshape(14, 14, 299, 299).transpose(0, 2, 1, 3).reshape(14 * 299, 14 * 299)[:4096, :4096]
    res["whole_4096"] = case("whole_4096", np.ascontiguousarray(whole)[None], args.reps, 1, dev)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    if not all(v["equal_to_host"] for v in res.values()):
        sys.exit(1)


if __name__ == "__main__":
    main()
