"""Cell localisation timing: 128 probability maps of 299^2 (quantise + smoothing + mean shift + clustering, one batch) and one
stitched 4096^2 mask, device-event timed after warm-up, next to the numpy restatement (tests/detect_ref.py, tests/edt_ref.py) on the
host for the same work.  Checks that the GPU outputs equal the restatement.  --method picks the smoothing: the Gaussian blur, the
exact distance transform, or both on the same maps in one run (the blur is then the yardstick of the distance form); the distance
form is also timed on its worst case, a 4096^2 map that is all foreground but one pixel (smoothing kernels alone).

The 4096^2 grid is also stitched from segment logits: detect.stitch_logits batch by batch next to softmax_channel_fwd + quantize +
stitch_patches on the same logits, with the peak device memory either takes (--stitch-only runs nothing else), and blended
(detect.StitchBlend, batches of 16, with and without the four flip views of test-time augmentation) next to the streamed stitch and
to the two forward passes that detect_slide runs per batch.

    python tools/detect_microbench.py [--method both] [--reps 5] [--host-maps 128] [--stitch-only] [--json PATH]
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
import edt_ref as E  # noqa: E402
from cellsegmentation_amd import detect as D  # noqa: E402
from cellsegmentation_amd import kernels as K  # noqa: E402


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


def host_detect(method, mask):
    return R.detect(mask, None, eps=11)[0] if method == "gaussianblur" else E.detect(mask, None, eps=11)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--method", choices=["gaussianblur", "distancetransform", "both"], default="gaussianblur")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-maps", type=int, default=128, help="maps of the batch also run (and checked) on the host")
    ap.add_argument("--stitch-only", action="store_true", help="only the streamed / resident stitch of segment logits")
    ap.add_argument("--json", default=None, help="also write the results to this file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {}
    methods = ["gaussianblur", "distancetransform"] if args.method == "both" else [args.method]
    if args.stitch_only:
        methods = []
    # ---- 128 maps of 299^2
    if methods:
        probs = blob_probs(128, 299, 299, 1 / 1500, seed=1)
        pd = torch.from_numpy(probs).to(dev)
    taps = D.gaussian_taps(15, 3.)

    for method in methods:
        opts = D.DetectOptions(eps=11, method=method)

        def gpu_batch():
            return D._detect(pd, None, opts)

        def gpu_smooth():
            return K.detect_blur(pd, taps, taps) if method == "gaussianblur" else K.detect_edt_smooth(pd, 10)
        ms, ts = time_dev(gpu_batch, args.reps)
        sm_ms, _ = time_dev(gpu_smooth, args.reps)
        out = gpu_batch()
        t0 = time.perf_counter()
        ok = True
        for i in range(args.host_maps):
            want = host_detect(method, R.quantize(probs[i]))
            ok &= bool(np.array_equal(out.points[out.offsets[i]:out.offsets[i + 1]], want))
        host_ms = (time.perf_counter() - t0) * 1e3
        key = "batch128_299" if method == "gaussianblur" else "batch128_299_dt"
        res[key] = {"method": method, "device_ms": ms, "device_ms_all": ts, "smoothing_ms": sm_ms, "host_ms": host_ms,
                    "host_maps": args.host_maps, "cells": int(out.offsets[-1]), "windows_kept": int(out.n_kept.sum()), "equal_to_host": ok}
        print(json.dumps({key: res[key]}), flush=True)
    # ---- one stitched 4096^2 mask: 299^2 patches overlapping by 16 px, border-aligned last row / column
    H = W = 4096
    step = 299 - 16
    origins = list(range(0, H - 299 + 1, step))
    if origins[-1] != H - 299:
        origins.append(H - 299)
    grid = [(r, c) for r in origins for c in origins]
    if methods:
        patches = blob_probs(len(grid), 299, 299, 1 / 1500, seed=2)
        pq = D.quantize(torch.from_numpy(patches).to(dev))
        whole = D.stitch_patches(pq, grid, (H, W))
        mask = R.stitch(R.quantize(patches), grid, (H, W))
        stitched_ok = bool(np.array_equal(whole.cpu().numpy(), mask))
    for method in methods:
        opts = D.DetectOptions(eps=11, method=method)

        def gpu_whole():
            return D._detect(whole[None], None, opts)

        def gpu_smooth():
            return K.detect_blur(whole[None], taps, taps) if method == "gaussianblur" else K.detect_edt_smooth(whole[None], 10)
        ms, ts = time_dev(gpu_whole, args.reps)
        sm_ms, _ = time_dev(gpu_smooth, args.reps)
        out = gpu_whole()
        t0 = time.perf_counter()
        want = host_detect(method, mask)
        host_ms = (time.perf_counter() - t0) * 1e3
        ok = stitched_ok and bool(np.array_equal(out.points, want))
        key = "stitched_4096" if method == "gaussianblur" else "stitched_4096_dt"
        res[key] = {"method": method, "device_ms": ms, "device_ms_all": ts, "smoothing_ms": sm_ms, "host_ms": host_ms, "patches": len(grid),
                    "cells": int(out.offsets[-1]), "windows_kept": int(out.n_kept.sum()), "equal_to_host": ok}
        print(json.dumps({key: res[key]}), flush=True)
    # ---- the same 4096^2 grid from segment LOGITS: streamed stitch_logits (batches of 16, one launch each, the mask and the corner
    # table resident) next to the resident path softmax_channel_fwd + quantize + stitch_patches on the same logits (every patch and
    # the 4 H W byte owner map resident); peak = rise of torch.cuda.max_memory_allocated over what is allocated before the call
    logits = (4 * torch.randn((len(grid), 2, 299, 299), generator=torch.Generator().manual_seed(3))).to(dev)
    rc = torch.tensor(grid, dtype=torch.int32, device=dev)

    def streamed():
        m = torch.zeros((H, W), dtype=torch.uint8, device=dev)
        for i in range(0, len(grid), 16):
            K.stitch_logits(m, logits[i:i + 16], rc[i:i + 16], 1)
        return m

    def resident():
        return K.stitch_patches(K.detect_quantize(K.softmax_channel_fwd(logits, 1)), rc, H, W)

    def peak_rise(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        del out
        return int(torch.cuda.max_memory_allocated() - before)
    def one_launch():                                                       # the kernel alone: every patch in one call
        return K.stitch_logits(torch.zeros((H, W), dtype=torch.uint8, device=dev), logits, rc, 1)
    same = bool(torch.equal(streamed(), resident())) and bool(torch.equal(one_launch(), resident()))
    rounds = {name: time_dev(fn, args.reps) for name, fn in (("streamed", streamed), ("resident", resident))}   # time_dev warms up
    again = {name: time_dev(fn, args.reps) for name, fn in (("resident", resident), ("streamed", streamed))}   # alternated order
    res["stitch_logits_4096"] = {"patches": len(grid), "batch": 16, "launches_streamed": (len(grid) + 15) // 16,
                                 "streamed_ms": min(rounds["streamed"][0], again["streamed"][0]),
                                 "resident_ms": min(rounds["resident"][0], again["resident"][0]),
                                 "streamed_ms_all": rounds["streamed"][1] + again["streamed"][1],
                                 "resident_ms_all": rounds["resident"][1] + again["resident"][1],
                                 "one_launch_ms": time_dev(one_launch, args.reps)[0],
                                 "streamed_peak_bytes": peak_rise(streamed), "resident_peak_bytes": peak_rise(resident),
                                 "logit_bytes": logits.numel() * 4, "mask_bytes": H * W, "equal_to_resident": same}
    print(json.dumps({"stitch_logits_4096": res["stitch_logits_4096"]}), flush=True)
    # ---- the same grid and logits BLENDED (detect.StitchBlend: zeroed accumulators, one add per batch of 16, one finish), without
    # and with the four flip views of test-time augmentation (the views are the flipped logits, so the mask must not change)
    views = {0: logits, 1: logits.flip(-1).contiguous(), 2: logits.flip(-2).contiguous(), 3: logits.flip(-2, -1).contiguous()}
    codes = {c: torch.full((16,), c, dtype=torch.uint8, device=dev) for c in views}

    def blended(tta=(0,)):
        sb = D.StitchBlend((H, W), (299, 299), device=dev)
        for i in range(0, len(grid), 16):
            for c in tta:
                sb.add(views[c][i:i + 16], rc[i:i + 16], codes[c][:len(rc[i:i + 16])], 1)
        return sb.finish()

    def blended_tta():
        return blended((0, 1, 2, 3))
    plain, mask_b = streamed().cpu().numpy(), blended().cpu().numpy()
    cover = np.zeros((H, W), np.int32)
    for r, c in grid:
        cover[r:r + 299, c:c + 299] += 1
    same = bool(np.array_equal(mask_b[cover == 1], plain[cover == 1])) and bool(np.array_equal(blended_tta().cpu().numpy(), mask_b))
    rounds = {name: time_dev(fn, args.reps) for name, fn in (("streamed", streamed), ("blended", blended), ("tta", blended_tta))}
    again = {name: time_dev(fn, args.reps) for name, fn in (("tta", blended_tta), ("blended", blended), ("streamed", streamed))}
    sb = D.StitchBlend((H, W), (299, 299), device=dev).add(logits[:16], rc[:16])
    # the yardstick of the loop: what detect_slide runs per batch of 16 next to one stitch call (ResNet-18, its default compute
    # dtype: gather_tiles, the segment forward, the image forward for the count)
    from cellsegmentation_amd import synth, tiles
    from cellsegmentation_amd.model import resnet as RN
    model = RN.MILresnet18()
    sd = model.state_dict()
    synth.fill_state_dict(sd)
    model.load_state_dict(sd)
    model = model.to(dev).eval()
    slide = torch.randint(0, 256, (1, H, W, 3), dtype=torch.uint8, device=dev, generator=torch.Generator(dev).manual_seed(4))
    ti = torch.zeros((16,), dtype=torch.int32, device=dev)

    def forwards():
        with torch.no_grad():
            x = tiles.gather_tiles(slide, ti, rc[:16], 299, model.compute_dtype)
            model.setmode("segment")
            out = model(x).float().contiguous()
            model.setmode("image")
            return out, model(x)[1]
    forward_ms = time_dev(forwards, args.reps)[0]
    del model, slide
    px =len(grid) * 299 * 299                                             # patch pixels of one view
    res["stitch_blend_4096"] = {"patches": len(grid), "batch": 16, "adds": (len(grid) + 15) // 16, "adds_tta": 4 * ((len(grid) + 15) // 16),
                                "streamed_ms": min(rounds["streamed"][0], again["streamed"][0]),
                                "blended_ms": min(rounds["blended"][0], again["blended"][0]),
                                "blended_tta_ms": min(rounds["tta"][0], again["tta"][0]),
                                "blended_ms_all": rounds["blended"][1] + again["blended"][1],
                                "blended_tta_ms_all": rounds["tta"][1] + again["tta"][1],
                                "finish_ms": time_dev(sb.finish, args.reps)[0],
                                "forwards_ms_per_batch": forward_ms, "batches": (len(grid) + 15) // 16,
                                "blended_peak_bytes": peak_rise(blended), "blended_tta_peak_bytes": peak_rise(blended_tta),
                                "streamed_peak_bytes": peak_rise(streamed),
                                "accumulator_bytes": 12 * H * W,
                                # zeroing; per patch pixel 12 accumulator bytes read, 12 written and 8 logit bytes; finish 12 + 1
                                "bytes_moved_blended": 12 * H * W + px * (24 + 8) + 13 * H * W,
                                "bytes_moved_tta": 12 * H * W + 4 * px * (24 + 8) + 13 * H * W,
                                "bytes_moved_streamed": H * W + px * (1 + 8),
                                "single_cover_fraction": float((cover == 1).mean()),
                                "equal_to_resident": same}
    print(json.dumps({"stitch_blend_4096": res["stitch_blend_4096"]}), flush=True)
    del logits, views
    if "distancetransform" in methods:
        # ---- the distance form's worst case: every pixel's row search runs to the one background pixel's column
        worst = torch.full((1, H, W), 255, dtype=torch.uint8, device=dev)
        worst[0, H // 2, W // 2] = 0
        ms, ts = time_dev(lambda: K.detect_edt_smooth(worst, 10), args.reps)
        yy, xx = np.mgrid[0:H, 0:W]
        d2 = (yy - H // 2) ** 2 + (xx - W // 2) ** 2
        ok = bool(np.array_equal(K.detect_edt_sq(worst, 10)[0].cpu().numpy(), d2))
        ok &= bool(np.array_equal(K.detect_edt_smooth(worst, 10)[0].cpu().numpy(), E.normalise(d2)))
        res["worst_4096_dt"] = {"method": "distancetransform", "smoothing_ms": ms, "smoothing_ms_all": ts, "equal_to_host": ok}
        print(json.dumps({"worst_4096_dt": res["worst_4096_dt"]}), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    if not all(v.get("equal_to_host", True) and v.get("equal_to_resident", True) for v in res.values()):
        sys.exit(1)


if __name__ == "__main__":
    main()
