"""Augmented input staging timing (csrc/augment.hip): stage_tiles at the tile-classifier workload (225 tiles of 32x32 per 299^2
image, 64 images) and stage_images at 299^2 with B = 8 and B = 64, device-event timed after warm-up.  Each shape runs plain, flips
only, jitter without contrast (one launch) and full jitter (memset + mean reduction + apply), next to tiles.gather_tiles -- the
kernel this one generalises -- on the same inputs in the same run, the variants alternating within every repetition.  Timed is the
raw call on device-resident operands (kernels.stage_augmented), as a training loop with a prepared epoch issues it; the public
stage_tiles / stage_images add the host-side validation and the upload of the per-tile arrays, reported once per shape as host_ms.

Bytes moved per call: 3 bytes read per output pixel (once more for the reduction of full jitter) and 8 elements written per pixel.
No threshold is fixed: the yardstick is gather_tiles in the same run.  gather_tiles cuts square tiles only, so the whole-image
shapes (299^2 is square) use it with size 299.

    python tools/augment_microbench.py [--reps 20] [--dtype bf16] [--json PATH]
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

from cellsegmentation_amd import augment as A  # noqa: E402
from cellsegmentation_amd import kernels as K  # noqa: E402
from cellsegmentation_amd import synth, tiles  # noqa: E402


def time_alternating(fns, reps):
    """{name: fn} -> {name: (median ms, all ms)}: warm every variant up, then time them in turn within each repetition"""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(4):                                            # four calls per window: the small shapes take microseconds
                fn()
            b.record()
            torch.cuda.synchronize()
            ts[k].append(a.elapsed_time(b) / 4)
    return {k: (float(np.median(v)), v) for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--dtype", choices=["bf16", "fp32"], default="bf16")
    ap.add_argument("--json", default=None, help="also write the results to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("augment_microbench needs a GPU: there is nothing to time without one")
    dev = torch.device("cuda:0")
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    esize = 2 if dtype == torch.bfloat16 else 4
    images = torch.from_numpy(synth.ihc_tiles(64, 299, 3)).to(dev)
    res = {}
    ti_all, rc_all = tiles.tile_index(64, (299, 299), 20, 32)
    shapes = [("tiles_64x225x32", 64, ti_all, rc_all, 32),
              ("images_8x299", 8, np.arange(8, dtype=np.int32), np.zeros((8, 2), np.int32), 299),
              ("images_64x299", 64, np.arange(64, dtype=np.int32), np.zeros((64, 2), np.int32), 299)]
    for name, n_img, ti, rc, size in shapes:
        T = len(ti)
        g = torch.Generator().manual_seed(1)
        full = A.draw_color_jitter(T, generator=g)
        no_contrast = A.draw_color_jitter(T, contrast=0, generator=g)
        flips = (np.arange(T) % 4).astype(np.int8)

        def up(a, dt):
            return torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dt)
        d_ti, d_rc, d_fl = up(ti, torch.int32), up(rc, torch.int32), up(flips, torch.int8)
        d_full = (up(full[0], torch.int8), up(full[1], torch.float32))
        d_noc = (up(no_contrast[0], torch.int8), up(no_contrast[1], torch.float32))
        out = torch.empty((T, size, size, 8), dtype=dtype, device=dev)
        ws = K.stage_augmented_workspace(T, dev)

        def stage(fl, jt, contrast):
            return lambda: K.stage_augmented(images, d_ti, d_rc, size, size, fl, jt[0], jt[1], contrast, dtype, out=out, ws=ws)
        fns = {"gather_tiles": lambda: tiles.gather_tiles(images, d_ti, d_rc, size, dtype),
               "plain": stage(None, (None, None), False), "flips": stage(d_fl, (None, None), False),
               "jitter_no_contrast": stage(d_fl, d_noc, False), "jitter_full": stage(d_fl, d_full, True)}
        # the outputs agree before anything is timed
        ok = bool(torch.equal(fns["plain"]().clone(), fns["gather_tiles"]()))
        t0 = time.perf_counter()
        pub = A.stage_tiles(images, ti, rc, size, flips, full, dtype)
        torch.cuda.synchronize()
        host_ms = (time.perf_counter() - t0) * 1e3
        ok &= bool(torch.equal(pub, fns["jitter_full"]()))
        timed = time_alternating(fns, args.reps)
        pixels = T * size * size
        row = {"tiles": T, "tile": size, "dtype": args.dtype, "equal": ok, "public_call_host_ms": host_ms}
        base = timed["gather_tiles"][0]
        for k, (ms, all_ms) in timed.items():
            moved = pixels * (3 * (2 if k == "jitter_full" else 1) + 8 * esize)
            row[k] = {"us": ms * 1e3, "us_min": min(all_ms) * 1e3, "us_max": max(all_ms) * 1e3, "bytes": moved,
                      "TB_per_s": moved / (ms * 1e-3) / 1e12, "ratio_to_gather_tiles": ms / base}
        res[name] = row
        print(json.dumps({name: row}), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    if not all(v["equal"] for v in res.values()):
        sys.exit(1)


if __name__ == "__main__":
    main()
