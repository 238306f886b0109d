"""Times the four launches of cellsegmentation_amd.tissue (csrc/tissue.hip) on an MI355X: device events around each launch, outputs
preallocated, 20 launches back to back between two events, median of 9 such repetitions after a warm-up, with their spread (max -
min) beside it.  The default 8192^2 image is 201 MB and can stay in the 256 MiB Infinity Cache between launches that only read it;
``--size 16384`` (805 MB) cannot.

    python tools/tissue_microbench.py [--size 8192] [--patch 299] [--slide] [--json PATH]

Synthetic slides of ``size`` x ``size`` RGB pixels, made on the device:

    near_constant   glass: one colour plus 0..2 per channel, so nearly every pixel falls into three bins of the histogram
    half_tissue     the upper half glass, the lower half stained noise
    noise           uniform noise in every channel: the histogram's bins are hit evenly

The yardstick of the two pixel passes is a device-to-device copy of the same image, timed in the same process: it reads and writes
3 bytes per pixel, the histogram reads 3 and the mask reads 3 and writes 1.  ``near_constant_vs_noise`` compares the histogram of the
glass with that of the noise: were the glass slower by more than the run-to-run spread, the histogram would be contending on one
bin.  Coverage and selection run on the patch grid of ``tiles.sample_patches`` for ``patch``.

``--slide``: ``inference.detect_slide`` on the half_tissue slide with a synthetic ResNet-18, with and without ``tissue=True``,
wall-clock around the call (synchronised), and the number of patches each ran."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cellsegmentation_amd import kernels as K  # noqa: E402
from cellsegmentation_amd import tiles, tissue  # noqa: E402


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


def slides(size, dev):
    """name -> uint8 [1, size, size, 3] on the device"""
    g = torch.Generator(device=dev).manual_seed(0)
    glass = torch.tensor([236, 228, 231], dtype=torch.uint8, device=dev)
    near = glass + torch.randint(0, 3, (1, size, size, 3), generator=g, device=dev, dtype=torch.uint8)
    noise = torch.randint(0, 256, (1, size, size, 3), generator=g, device=dev, dtype=torch.uint8)
    half = near.clone()
    lo = torch.tensor([150, 60, 120], dtype=torch.uint8, device=dev)
    span = torch.tensor([80, 100, 80], dtype=torch.float32, device=dev)
    stain = (torch.rand((size - size // 2, size, 3), generator=g, device=dev) * span).to(torch.uint8) + lo
    half[0, size // 2:] = stain
    return {"near_constant": near.contiguous(), "half_tissue": half.contiguous(), "noise": noise.contiguous()}


def bench_launches(name, x, patch):
    dev = x.device
    _, H, W, _ = x.shape
    px = H * W
    row = {"slide": name, "size": [H, W]}
    dst = torch.empty_like(x)
    row["copy_ms"], row["copy_spread_ms"] = time_dev(lambda: dst.copy_(x))
    for ch, code in tissue.CHANNELS.items():
        hist = torch.zeros((1, 256), dtype=torch.int64, device=dev)
        row[f"histogram_{ch}_ms"], row[f"histogram_{ch}_spread_ms"] = time_dev(lambda: K.tissue_histogram(x, code, hist=hist))
        thr = torch.tensor(tissue.otsu(K.tissue_histogram(x, code)), dtype=torch.int32, device=dev)
        out = torch.empty((1, H, W), dtype=torch.uint8, device=dev)
        row[f"mask_{ch}_ms"], row[f"mask_{ch}_spread_ms"] = time_dev(lambda: K.tissue_mask(x, thr, code, out=out))
        row[f"threshold_{ch}"] = int(thr[0])
    m = K.tissue_mask(x, thr.new_tensor(tissue.otsu(K.tissue_histogram(x, 0))), 0)
    rc = torch.from_numpy(np.asarray(tiles.sample_patches((H, W), patch), np.int32)).to(dev)
    ti = torch.zeros((len(rc),), dtype=torch.int32, device=dev)
    row["patches"] = len(rc)
    row["coverage_ms"], row["coverage_spread_ms"] = time_dev(lambda: K.tissue_coverage(m, ti, rc, patch, patch))
    cover = K.tissue_coverage(m, ti, rc, patch, patch)
    need = tissue.TissueOptions().pixels(patch, patch)
    row["select_ms"], row["select_spread_ms"] = time_dev(lambda: K.tissue_select(cover, need))
    row["selected"] = int(K.tissue_select(cover, need)[1])
    # against the copy: bytes moved per pixel are 6 (copy), 3 (histogram), 4 (mask)
    row["copy_GBps"] = 6 * px / row["copy_ms"] / 1e6
    row["histogram_chroma_GBps"] = 3 * px / row["histogram_chroma_ms"] / 1e6
    row["mask_chroma_GBps"] = 4 * px / row["mask_chroma_ms"] / 1e6
    row["histogram_over_copy"] = row["histogram_chroma_ms"] / row["copy_ms"]
    row["mask_over_copy"] = row["mask_chroma_ms"] / row["copy_ms"]
    return row


def bench_slide(x, patch, batch):
    from cellsegmentation_amd import inference, synth
    from cellsegmentation_amd.model import resnet as RN
    dev = x.device
    m = RN.MILresnet18()
    sd = m.state_dict()
    synth.fill_state_dict(sd)
    m.load_state_dict(sd)
    m = m.to(dev)
    out = {"patch": patch, "batch_size": batch}
    for key, arg in (("all_patches", None), ("tissue", True)):
        ts = []
        for _ in range(6):                                                  # the first run warms up
            torch.cuda.synchronize()
            t = time.perf_counter()
            res = inference.detect_slide(x[0], m, dev, batch_size=batch, patch_size=patch, tissue=arg)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t) * 1e3)
        out[f"{key}_ms"], out[f"{key}_spread_ms"] = float(np.median(ts[1:])), float(max(ts[1:]) - min(ts[1:]))
        out[f"{key}_patches_run"] = res.tissue.n_selected if res.tissue is not None else len(tiles.sample_patches(x.shape[1:3], patch))
        out[f"{key}_cell_count"] = res.cell_count
    out["speedup"] = out["all_patches_ms"] / out["tissue_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--patch", type=int, default=299)
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--slide", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    imgs = slides(args.size, dev)
    rows = []
    for name, x in imgs.items():
        rows.append(bench_launches(name, x, args.patch))
        print(json.dumps(rows[-1]), flush=True)
    by = {r["slide"]: r for r in rows}
    near, noise = by["near_constant"], by["noise"]
    spread = max(near["histogram_chroma_spread_ms"], noise["histogram_chroma_spread_ms"])
    verdict = {"near_constant_ms": near["histogram_chroma_ms"], "noise_ms": noise["histogram_chroma_ms"], "spread_ms": spread,
               "near_constant_not_slower": near["histogram_chroma_ms"] <= noise["histogram_chroma_ms"] + spread}
    out = {"device": torch.cuda.get_device_name(0), "rows": rows, "near_constant_vs_noise": verdict}
    print(json.dumps({"near_constant_vs_noise": verdict}), flush=True)
    if args.slide:
        out["slide"] = bench_slide(imgs["half_tissue"], args.patch, args.batch_size)
        print(json.dumps({"slide": out["slide"]}), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    return 0 if verdict["near_constant_not_slower"] else 1


if __name__ == "__main__":
    sys.exit(main())
