"""Times cellsegmentation_amd.polygons.rasterize (csrc/polygons.hip) on an MI355X: device events around 20 launches back to back,
outputs preallocated, median of 9 such repetitions after a warm-up, with their spread (max - min) beside it (``time_dev`` of
tools/tissue_microbench.py).  Calls that plan on the host and upload are timed by the wall clock around the synchronised call,
median of 5 after a warm-up.  Before anything is timed the device is held to the plain-loop restatement tests/polygon_ref.py on a
small case; a mismatch ends the run.

    python tools/polygon_microbench.py [--cases a b c] [--json PATH]

    a   every ring of ``regions.contour_labels`` of a synthetic 4096^2 label image (discs on a grid of ``pitch`` pixels: about
        10^4, 4 10^4 and 10^5 cells) through ``from_contours`` + ``rasterize``, next to ``contour_labels`` itself (table given,
        ``max_vertices=256``) and next to a memset plus a device-to-device copy of the label image -- what writing the labels costs
        at least.  ``equal`` says that the round trip gave the label image back.
    b   one 5 000-vertex outline with a 16384^2 box in mask mode, next to the memset of that mask; ``band_rows`` is swept -- the
        item table is made once per value, the clear and the launch are timed, 5 back to back, median of 5 -- and the whole
        call (plan, upload, clear, launch) is timed by the wall clock at the default.
    c   10^5 host-side cell polygons of 24 vertices as a packed table on 4096^2: the launch alone at several ``band_rows`` and
        at the default, the planner alone, and the whole call.

Both sides of every ratio are timed in the same process on the same device.  The memset and copy figures are recorded as
yardsticks of what writing the image costs at least; no ratio is formed with them here."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from cellsegmentation_amd import kernels as K  # noqa: E402
from cellsegmentation_amd import polygons as P  # noqa: E402
from cellsegmentation_amd import regions as G  # noqa: E402
from stain_microbench import time_wall  # noqa: E402
from tissue_microbench import time_dev  # noqa: E402

BANDS = (4, 8, 16, 32, 64, 128, 256, 1024, 16384)
CELL_BANDS = (4, 8, 16, 64)


def check_small(dev):
    import polygon_ref as PR
    rng = np.random.default_rng(0)
    shapes = [[np.rint(rng.uniform(-5, 75, (int(rng.integers(3, 12)), 2)) * 16).astype(np.int64)] for _ in range(8)]
    ps = P.from_rings([shapes], sub=0)
    ps.sub = 4
    for rule in P.RULES:
        for mode in P.MODES:
            got = P.rasterize(ps, (70, 70), mode=mode, rule=rule, device=dev, _band_rows=16).cpu().numpy()
            want = PR.rasterize([[[r.tolist() for r in s] for s in shapes]], (70, 70), 4, rule, mode)
            if got.tobytes() != want.tobytes():
                raise SystemExit(f"polygon_microbench: the device differs from the restatement ({rule}, {mode})")


def disc_labels(size, pitch, dev):
    """int32 [1, size, size]: a disc of radius 0.3 .. 0.45 pitch in every cell of a pitch x pitch grid, numbered row-major"""
    g = torch.Generator(device=dev).manual_seed(pitch)
    cells = -(-size // pitch)
    i = torch.arange(size, device=dev)
    ci = i // pitch
    off = (i % pitch).float() - (pitch - 1) / 2
    rad = (0.3 + 0.15 * torch.rand((cells, cells), generator=g, device=dev)) * pitch
    d2 = off[:, None] ** 2 + off[None, :] ** 2
    inside = d2 < rad[ci][:, ci] ** 2
    lab = (ci[:, None] * cells + ci[None, :] + 1).to(torch.int32)
    return torch.where(inside, lab, torch.zeros_like(lab))[None].contiguous(), cells * cells


def case_a(dev, rows):
    for pitch in (40, 20, 13):
        lab, cells = disc_labels(4096, pitch, dev)
        table = G.measure_labels(lab, max_regions=cells)
        ct = G.contour_labels(lab, table=table, max_vertices=256)
        out = torch.empty_like(lab)
        dst = torch.empty_like(lab)
        row = {"case": "a", "size": [4096, 4096], "cells": cells, "pitch": pitch,
               "truncated": int(ct.truncated().sum()), "equal": bool(torch.equal(P.rasterize(P.from_contours(ct), (4096, 4096)), lab))}
        timed = {"contour_labels": lambda: G.contour_labels(lab, table=table, max_vertices=256),
                 "from_contours_rasterize": lambda: P.rasterize(P.from_contours(ct), (4096, 4096), out=out),
                 "memset_copy": lambda: (out.zero_(), dst.copy_(lab)), "memset": lambda: out.zero_()}
        for key, fn in timed.items():
            row[f"{key}_ms"], row[f"{key}_spread_ms"] = time_dev(fn)
        row["rasterize_over_contour_labels"] = row["from_contours_rasterize_ms"] / row["contour_labels_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)


def launch_only(ps, hw, mode, band, dev):
    """-> (fn, n_items, out): fn clears the preallocated output ``out`` and launches with the item table of ``band``"""
    tabs = [getattr(ps, k).to(dev).contiguous() for k in P._TABLES]
    items = torch.from_numpy(P.plan(ps, hw, band)).to(dev)
    out = torch.empty((ps.n_images,) + tuple(hw), dtype=P.MODES[mode], device=dev)
    return (lambda: K.polygons_rasterize(*tabs, out.zero_(), ps.sub, K.CS_POLYGON_EVENODD, items)), len(items), out


def case_b(dev, rows):
    size, n = 16384, 5000
    rng = np.random.default_rng(1)
    ang = np.arange(n) * (2 * math.pi / n)
    rad = 7000 + 600 * np.sin(7 * ang) + rng.uniform(-40, 40, n)
    ring = np.stack([size / 2 + rad * np.sin(ang), size / 2 + rad * np.cos(ang)], 1)
    ps = P.from_rings([[ring]], sub=4)
    mask = torch.empty((1, size, size), dtype=torch.uint8, device=dev)
    row = {"case": "b", "size": [size, size], "vertices": n}
    row["memset_ms"], row["memset_spread_ms"] = time_dev(lambda: mask.zero_())
    del mask
    sweep = []
    for band in BANDS:
        fn, items, out = launch_only(ps, (size, size), "mask", band, dev)
        ms, spread = time_dev(fn, reps=5, inner=5)
        sweep.append({"band_rows": band, "items": items, "clear_launch_ms": ms, "spread_ms": spread, "covered": int(out.sum())})
        del fn, out
        torch.cuda.empty_cache()
    row["sweep"] = sweep
    row["default_band_rows"] = P.BAND_ROWS
    out = torch.empty((1, size, size), dtype=torch.uint8, device=dev)
    row["whole_call_ms"], row["whole_call_spread_ms"] = time_wall(lambda: P.rasterize(ps, (size, size), mode="mask", out=out))
    best = min(sweep, key=lambda s: s["clear_launch_ms"])
    row["best_band_rows"] = best["band_rows"]
    rows.append(row)
    print(json.dumps(row), flush=True)


def case_c(dev, rows):
    size, cells, n = 4096, 100000, 24
    rng = np.random.default_rng(2)
    centre = rng.uniform(0, size, (cells, 1, 2))
    ang = np.arange(n) * (2 * math.pi / n)
    rad = rng.uniform(4, 9, (cells, 1)) * (1 + 0.15 * rng.standard_normal((cells, n)))
    rings = centre + rad[..., None] * np.stack([np.sin(ang), np.cos(ang)], 1)[None]
    ps = P.from_rings([[r for r in rings]], sub=4)
    row = {"case": "c", "size": [size, size], "cells": cells, "vertices_per_cell": n, "sweep": []}
    for band in CELL_BANDS:
        fn, items, out = launch_only(ps, (size, size), "labels", band, dev)
        ms, spread = time_dev(fn)
        row["sweep"].append({"band_rows": band, "items": items, "clear_launch_ms": ms, "spread_ms": spread})
        del fn, out
    fn, items, out = launch_only(ps, (size, size), "labels", None, dev)
    row["items"] = items
    row["clear_launch_ms"], row["clear_launch_spread_ms"] = time_dev(fn)
    row["memset_ms"], row["memset_spread_ms"] = time_dev(lambda: out.zero_())
    row["labelled_pixels"] = int((fn() > 0).sum())
    row["whole_call_ms"], row["whole_call_spread_ms"] = time_wall(lambda: P.rasterize(ps, (size, size), out=out))
    row["plan_ms"], row["plan_spread_ms"] = time_wall(lambda: P.plan(ps, (size, size)))
    rows.append(row)
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["a", "b", "c"], choices=["a", "b", "c"])
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    check_small(dev)
    rows = []
    for c in args.cases:
        {"a": case_a, "b": case_b, "c": case_c}[c](dev, rows)
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "checked_against": "tests/polygon_ref.py", "rows": rows}, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
