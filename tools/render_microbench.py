"""Times the two launches of cellsegmentation_amd.render (csrc/render.hip) on an MI355X: device events around each launch, outputs
preallocated, `inner` launches back to back between two events, median of 9 such repetitions after a warm-up, with their spread
(max - min) beside it.

    python tools/render_microbench.py [--sizes 4096 16384] [--json profiles/render_microbench.json]

Per size a synthetic slide of ``size`` x ``size`` RGB noise, made on the device, and

    copy            a device-to-device copy of the image, the yardstick: 6 bytes per pixel
    mask            compose with the mask fill: 3 + 1 read, 3 written = 7 bytes per pixel
    heat_u8         compose with the uint8 heat fill through the colour table in LDS: 7 bytes per pixel
    heat_f32        compose with float32 probabilities and a threshold: 3 + 4 read, 3 written = 10 bytes per pixel
    outlines        compose with the outline of an int32 label image of 48 x 48 cells, 40 x 40 of each labelled: 3 + 4 read once from
                    memory (the rows above and below come from the cache), 3 written = 10 bytes per pixel
    mask_outlines   the mask fill and the outlines in one launch: 11 bytes per pixel
    outlines_sparse the outlines of a label image that keeps one cell in 16 (a slide is mostly background): 10 bytes per pixel
    points_<n>      draw_points of n = 10^3 and 10^5 filled r = 4 dots at uniform random places

``<pass>_over_copy`` is the time of the pass over that of the copy in the same run, ``<pass>_GBps`` the bytes above per second.  A 4096^2
image and its outputs (50 MB each) stay in the 256 MiB Infinity Cache between launches; at 16384^2 (805 MB) nothing does."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cellsegmentation_amd import kernels as K  # noqa: E402
from cellsegmentation_amd import render  # noqa: E402

BYTES = {"copy": 6, "mask": 7, "heat_u8": 7, "heat_f32": 10, "outlines": 10, "mask_outlines": 11, "outlines_sparse": 10}


def time_dev(fn, reps=9, inner=20):
    """-> (median ms, max - min ms) per call, each repetition timing `inner` calls back to back between two events"""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / inner)
    return float(np.median(ts)), float(max(ts) - min(ts))


def bench(size, dev, inner):
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randint(0, 256, (1, size, size, 3), generator=g, device=dev, dtype=torch.uint8)
    heat = torch.randint(0, 256, (1, size, size), generator=g, device=dev, dtype=torch.uint8)
    mask = (heat > 127).to(torch.uint8)
    probs = heat.to(torch.float32) / 255
    r = torch.arange(size, device=dev)
    cell = (r // 48)[:, None] * ((size + 47) // 48) + (r // 48)[None, :] + 1
    inside = ((r % 48) < 40)[:, None] & ((r % 48) < 40)[None, :]
    labels = torch.where(inside, cell, torch.zeros_like(cell)).to(torch.int32)[None].contiguous()
    sparse = torch.where(cell[None] % 16 == 1, labels, torch.zeros_like(labels)).contiguous()
    del cell, inside
    table = torch.from_numpy(render.jet()).to(dev)
    out = torch.empty_like(x)
    row = {"size": [size, size]}
    passes = {
        "copy": lambda: out.copy_(x),
        "mask": lambda: K.render_compose(x, K.CS_RENDER_FILL_MASK, mask, out=out),
        "heat_u8": lambda: K.render_compose(x, K.CS_RENDER_FILL_HEAT_U8, heat, colormap=table, out=out),
        "heat_f32": lambda: K.render_compose(x, K.CS_RENDER_FILL_HEAT_F32, probs, 0.5, colormap=table, out=out),
        "outlines": lambda: K.render_compose(x, labels=labels, out=out),
        "mask_outlines": lambda: K.render_compose(x, K.CS_RENDER_FILL_MASK, mask, labels=labels, out=out),
        "outlines_sparse": lambda: K.render_compose(x, labels=sparse, out=out),
    }
    px = size * size
    for name, fn in passes.items():
        row[f"{name}_ms"], row[f"{name}_spread_ms"] = time_dev(fn, inner=inner)
        row[f"{name}_GBps"] = BYTES[name] * px / row[f"{name}_ms"] / 1e6
    for name in passes:
        if name != "copy":
            row[f"{name}_over_copy"] = row[f"{name}_ms"] / row["copy_ms"]
    off1 = lambda n: torch.tensor([0, n], dtype=torch.int64, device=dev)  # noqa: E731
    for n in (1000, 100000):
        pts = torch.randint(0, size, (n, 2), generator=g, device=dev, dtype=torch.int64)
        off = off1(n)
        row[f"points_{n}_ms"], row[f"points_{n}_spread_ms"] = time_dev(lambda: K.render_points(out, pts, off, radius=4), inner=inner)
        row[f"points_{n}_over_copy"] = row[f"points_{n}_ms"] / row["copy_ms"]
        row[f"points_{n}_Mpoints_per_s"] = n / row[f"points_{n}_ms"] / 1e3
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 16384])
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for size in args.sizes:
        rows.append(bench(size, dev, inner=20 if size <= 8192 else 5))
        print(json.dumps(rows[-1]), flush=True)
    out = {"device": torch.cuda.get_device_name(0), "rows": rows}
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
