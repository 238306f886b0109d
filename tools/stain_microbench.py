"""Times the five launches of cellsegmentation_amd.stain (csrc/stain.hip) on an MI355X, and ``estimate`` and ``normalize`` end to
end: device events around each launch, outputs preallocated, 20 launches back to back between two events, median of 9 such
repetitions after a warm-up, with their spread (max - min) beside it.  ``estimate`` and ``normalize`` hold copies to the host, so
they are timed by the wall clock around the synchronised call, median of 5 after a warm-up.

    python tools/stain_microbench.py [--size 4096 16384] [--json PATH]
    python tools/stain_microbench.py --quantify [--size 4096] [--json PATH]
    python tools/stain_microbench.py --texture [--size 4096] [--json PATH]

Synthetic slides of ``size`` x ``size`` RGB pixels, made on the device (those of tools/tissue_microbench.py):

    near_constant   glass: one colour plus 0..2 per channel; no pixel is kept, the histograms stay empty
    half_tissue     the upper half glass, the lower half stained noise, most of it kept
    noise           uniform noise in every channel: about half of the pixels is kept and the bins are hit widely

``n_kept`` of every row says how many pixels the estimation passes did work for.

The yardstick is a device-to-device copy of the same image, timed in the same process: it reads and writes 3 bytes per pixel.
``moments`` and the two histograms read 3, ``apply`` reads 3 and writes 3 as the copy does, ``separate`` writes 2 (uint8) or 8
(fp32) bytes per pixel for two stains.  A 4096^2 image (50 MB) stays in the 256 MiB Infinity Cache between launches, a 16384^2
image (805 MB) cannot.

``--quantify`` times the per-cell stain tables instead: ``stain.quantify_labels``' one launch pair (cs_stain_quantify_labels) on a
synthetic H-DAB slide of about 10^4 labelled cells (discs on a grid, a DAB amplitude per cell), next to the path it replaces on the
same inputs -- ``separate(dtype="u8")``, then per stain the contiguous copy of its channel and ``measure_labels(intensity=)`` -- and
next to the device-to-device copy of the image; timed the same way, in one process.

``--texture`` times the per-cell co-occurrence tables (cs_regions_texture_labels, one launch) on the same slide and labels: the
plane route over the slide's haematoxylin plane at 16 and 32 grey levels, with the matrix, and at distance 4, and the stain route
over the RGB slide, next to ``quantify_labels``, ``measure_labels`` and the copy on the same inputs; and the same launches over a
uniform plane / slide, where every pixel has one level and all adds of a wave meet in one counter: the gap between the two is what
that hot spot costs."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from cellsegmentation_amd import kernels as K  # noqa: E402
from cellsegmentation_amd import stain  # noqa: E402
from tissue_microbench import slides, time_dev  # noqa: E402


def time_wall(fn, reps=5):
    """-> (median ms, max - min ms) of a call that synchronises with the host itself"""
    fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts)), float(max(ts) - min(ts))


def bench(name, x, opts):
    dev = x.device
    _, H, W, _ = x.shape
    row = {"slide": name, "size": [H, W]}
    od, beta_q = torch.from_numpy(stain.od_table(opts.Io)).to(dev), opts.beta_q
    est = stain.estimate(x[0], options=opts)
    row["n_kept"], row["ok"] = est.n_kept, est.ok
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a[None], dtype=np.float32)).to(dev)  # noqa: E731
    V = f32(np.linalg.svd(est.vectors)[0][:, :2])                          # a plane that holds the vectors
    P, A = f32(np.linalg.pinv(est.vectors)), f32(stain.normalizer(est, stain.TARGET_HDAB))
    dst = torch.empty_like(x)
    timed = {"copy": lambda: dst.copy_(x)}
    mom = torch.zeros((1, 10), dtype=torch.int64, device=dev)
    timed["moments"] = lambda: K.stain_moments(x, od, beta_q, out=mom)
    ah = torch.zeros((1, opts.angle_bins), dtype=torch.int64, device=dev)
    timed["angle_hist"] = lambda: K.stain_angle_hist(x, od, beta_q, V, opts.angle_bins, out=ah)
    ch = torch.zeros((1, 2, opts.conc_bins), dtype=torch.int64, device=dev)
    timed["conc_hist"] = lambda: K.stain_conc_hist(x, od, beta_q, P, opts.conc_bins, opts.conc_max, out=ch)
    timed["apply"] = lambda: K.stain_apply(x, od, A, opts.Io, out=dst)
    for key, fn in timed.items():
        row[f"{key}_ms"], row[f"{key}_spread_ms"] = time_dev(fn)
    del dst
    for key, as_u8, dtype in (("separate_u8", True, torch.uint8), ("separate_f32", False, torch.float32)):
        out = torch.empty((1, H, W, 2), dtype=dtype, device=dev)
        row[f"{key}_ms"], row[f"{key}_spread_ms"] = time_dev(lambda: K.stain_separate(x, od, P, as_u8, opts.conc_max, out=out))
        del out
    for key in ("moments", "angle_hist", "conc_hist", "apply", "separate_u8", "separate_f32"):
        row[f"{key}_over_copy"] = row[f"{key}_ms"] / row["copy_ms"]
    px = H * W
    row["copy_GBps"] = 6 * px / row["copy_ms"] / 1e6
    row["moments_GBps"] = 3 * px / row["moments_ms"] / 1e6
    row["apply_GBps"] = 6 * px / row["apply_ms"] / 1e6
    row["estimate_ms"], row["estimate_spread_ms"] = time_wall(lambda: stain.estimate(x[0], options=opts))
    out = torch.empty_like(x)
    row["normalize_ms"], row["normalize_spread_ms"] = time_wall(lambda: stain.normalize(x[0], options=opts, out=out))
    return row


def hdab_cells(size, dev, pitch=40, radius=12, seed=0):
    """-> (uint8 [1, size, size, 3] slide, int32 [1, size, size] labels, cells): discs of haematoxylin on a grid of ``pitch``
    pixels, label k + 1 = disc k, a DAB amplitude per cell in [0, 1.5] over the disc and a little beyond it, noise on top"""
    g = torch.Generator(device=dev).manual_seed(seed)
    per = size // pitch
    yy = torch.arange(size, device=dev)
    cell, off = torch.clamp(yy // pitch, max=per - 1), yy - (torch.clamp(yy // pitch, max=per - 1) * pitch + pitch // 2)
    d2 = off[:, None] ** 2 + off[None, :] ** 2
    index = cell[:, None] * per + cell[None, :]
    labels = torch.where(d2 <= radius * radius, index + 1, torch.zeros_like(index)).to(torch.int32)
    amp = torch.rand((per * per,), generator=g, device=dev) * 1.5
    S = torch.from_numpy(np.asarray(stain.HDAB, np.float32)).to(dev)       # [3, 2]
    x = torch.empty((size, size, 3), dtype=torch.uint8, device=dev)
    for r0 in range(0, size, 512):                                        # in bands: the float image of a 16384^2 slide is 3 GB
        rows = slice(r0, min(r0 + 512, size))
        c = torch.rand((rows.stop - r0, size, 2), generator=g, device=dev) * 0.05
        c[..., 0] += 1.2 * (d2[rows] <= radius * radius)
        c[..., 1] += amp[index[rows]] * (d2[rows] <= (radius + 4) ** 2)
        rgb = 240.0 * torch.exp(-(c @ S.T)) + 1.5 * torch.randn((rows.stop - r0, size, 3), generator=g, device=dev)
        x[rows] = rgb.round().clamp(0, 255).to(torch.uint8)
    return x[None].contiguous(), labels[None].contiguous(), per * per


def bench_quantify(size, opts, dev):
    from cellsegmentation_amd import morph
    x, lab, cells = hdab_cells(size, dev)
    _, H, W, _ = x.shape
    row = {"slide": "hdab_cells", "size": [H, W], "cells": cells, "labelled_fraction": float((lab > 0).float().mean())}
    od = torch.from_numpy(stain.od_table(opts.Io)).to(dev)
    Mq = torch.from_numpy(stain.quantised_matrix(stain.HDAB, False, opts.conc_max)[None]).to(dev)
    P = torch.from_numpy(np.ascontiguousarray(np.linalg.pinv(stain.HDAB)[None], dtype=np.float32)).to(dev)
    levels = stain.positive_levels((0.2, 0.2), 2, opts.conc_max)
    ring = morph.expand_labels(lab, 4)
    dst = torch.empty_like(x)
    timed = {"copy": lambda: dst.copy_(x)}
    for key, kw in (("quantify", {}), ("quantify_pos", {"pos_levels": levels}), ("quantify_ring", {"expanded": ring}),
                    ("quantify_hist256", {"bins": 256}), ("quantify_ring_pos_hist64", {"expanded": ring, "pos_levels": levels, "bins": 64})):
        t = K.stain_quantify_labels(x, lab, od, Mq, cells, **kw)
        timed[key] = lambda kw=kw, t=t: K.stain_quantify_labels(x, lab, od, Mq, cells, **kw, **t)
    conc = torch.empty((1, H, W, 2), dtype=torch.uint8, device=dev)
    chan = [torch.empty((1, H, W), dtype=torch.uint8, device=dev) for _ in range(2)]
    m = dict(zip(("counts", "area", "bbox", "sums", "isum", "imax"), K.regions_measure_labels(lab, cells, chan[0])))
    timed["separate_u8"] = lambda: K.stain_separate(x, od, P, True, opts.conc_max, out=conc)
    timed["channel_copy"] = lambda: chan[0].copy_(conc[..., 0])
    timed["measure_labels"] = lambda: K.regions_measure_labels(lab, cells, chan[0], **m)

    def two_pass():
        K.stain_separate(x, od, P, True, opts.conc_max, out=conc)
        for k in range(2):
            chan[k].copy_(conc[..., k])
            K.regions_measure_labels(lab, cells, chan[k], **m)

    timed["two_pass"] = two_pass
    for key, fn in timed.items():
        row[f"{key}_ms"], row[f"{key}_spread_ms"] = time_dev(fn)
    for key in timed:
        if key != "copy":
            row[f"{key}_over_copy"] = row[f"{key}_ms"] / row["copy_ms"]
    row["two_pass_over_quantify"] = row["two_pass_ms"] / row["quantify_ms"]
    # the fused table against the path it replaces, on the values both have: the sums agree to one level per pixel
    t = K.stain_quantify_labels(x, lab, od, Mq, cells)
    two_pass()
    row["max_abs_mean_difference_levels"] = float(((t["sum"][0, :, 0, 1] - m["isum"][0]).abs().double() / m["area"][0].clamp(min=1)).max())
    return row


def bench_texture(size, opts, dev):
    x, lab, cells = hdab_cells(size, dev)
    _, H, W, _ = x.shape
    row = {"slide": "hdab_cells", "size": [H, W], "cells": cells, "labelled_fraction": float((lab > 0).float().mean())}
    od = torch.from_numpy(stain.od_table(opts.Io)).to(dev)
    Mq = torch.from_numpy(stain.quantised_matrix(stain.HDAB, False, opts.conc_max)[None]).to(dev)
    P = torch.from_numpy(np.ascontiguousarray(np.linalg.pinv(stain.HDAB)[None], dtype=np.float32)).to(dev)
    m = dict(zip(("counts", "area", "bbox", "sums", "isum", "imax"), K.regions_measure_labels(lab, cells)))
    bbox, mq0 = m["bbox"], Mq[:, 0].contiguous()
    plane = K.stain_separate(x, od, P, True, opts.conc_max)[..., 0].contiguous()        # the haematoxylin plane of the noisy slide
    flat_plane, flat_x = torch.full_like(plane, 100), torch.full_like(x, 120)           # every level equal: all adds of a wave meet
    dst = torch.empty_like(x)
    q = K.stain_quantify_labels(x, lab, od, Mq, cells)
    timed = {"copy": lambda: dst.copy_(x), "quantify": lambda: K.stain_quantify_labels(x, lab, od, Mq, cells, **q),
             "measure_labels": lambda: K.regions_measure_labels(lab, cells, **{k: v for k, v in m.items() if v is not None})}
    cases = (("plane_L16", dict(plane=plane, levels=16)), ("plane_L32", dict(plane=plane, levels=32)),
             ("plane_L16_matrix", dict(plane=plane, levels=16, want_matrix=True)),
             ("stain_L16", dict(images_u8=x, od_q=od, Mq=mq0, levels=16)),
             ("plane_L16_d4", dict(plane=plane, levels=16, distance=4)),
             ("uniform_plane_L16", dict(plane=flat_plane, levels=16)), ("uniform_plane_L32", dict(plane=flat_plane, levels=32)),
             ("uniform_stain_L16", dict(images_u8=flat_x, od_q=od, Mq=mq0, levels=16)))
    for key, kw in cases:
        t = K.texture_labels(lab, cells, bbox, **kw)
        row[f"{key}_pairs"] = int(t["pairs"].sum())
        kw = {k: v for k, v in kw.items() if k != "want_matrix"}
        timed[f"texture_{key}"] = lambda kw=kw, t=t: K.texture_labels(lab, cells, bbox, **kw, **t)
    for key, fn in timed.items():
        row[f"{key}_ms"], row[f"{key}_spread_ms"] = time_dev(fn)
    for key in timed:
        if key != "copy":
            row[f"{key}_over_copy"] = row[f"{key}_ms"] / row["copy_ms"]
    for key in ("plane_L16", "plane_L32", "stain_L16"):
        row[f"uniform_over_noise_{key}"] = row[f"texture_uniform_{key}_ms"] / row[f"texture_{key}_ms"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs="+", default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--quantify", action="store_true")
    ap.add_argument("--texture", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    opts = stain.StainOptions()
    rows = []
    if args.quantify or args.texture:
        for size in args.size or [4096]:
            rows.append((bench_texture if args.texture else bench_quantify)(size, opts, dev))
            print(json.dumps(rows[-1]), flush=True)
            torch.cuda.empty_cache()
        args.size = []
    elif args.size is None:
        args.size = [4096, 16384]
    for size in args.size:
        imgs = slides(size, dev)
        for name in list(imgs):
            rows.append(bench(name, imgs.pop(name), opts))
            print(json.dumps(rows[-1]), flush=True)
            torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
