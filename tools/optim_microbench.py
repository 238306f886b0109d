"""Optimizer update timing on the ResNet-50 tile step's parameter set: cellsegmentation_amd.optim.SGD and Adam (one launch), their
capturable forms (SGD: lr and momentum read from device memory; Adam: step counts and lr on the device, one more tiny launch) and
torch.optim.SGD / Adam (foreach), as the reference's drivers construct them (train_tile.py:280-303: SGD with momentum 0.9 and weight
decay 1e-4; train_tile.py:282: Adam with weight decay 1e-4).  Shapes from the model (tile mode, encoder unfrozen: the tensors that
receive a gradient in that step), random values, static gradients; device-event time per step() after a warm-up (median over --reps;
alone on an idle queue, and queued behind other device work so that the host's enqueue time is hidden) and the achieved bandwidth
from the latter, at 20 B per parameter for SGD (read p, g, buf; write p, buf) and 28 B for Adam (read p, g, m, v; write p, m, v).
One process, one GPU.

    python tools/optim_microbench.py [--reps 50] [--warmup 10]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cellsegmentation_amd import optim as O  # noqa: E402
from cellsegmentation_amd.model import resnet as R  # noqa: E402


def tile_step_shapes():
    m = R.MILresnet50()
    m.setmode("tile")
    m.set_encoder_grads(True)
    # (upconv5-8 stay trainable in every mode but receive no gradient in a tile step: the optimizer skips them)
    return [tuple(p.shape) for n, p in m.named_parameters() if p.requires_grad and not n.startswith("upconv")]


def time_steps(opt, warmup, reps, blocker):
    """(step_ms, device_ms).  step_ms: device events around ONE step() on an idle queue -- what a loop sees, the host's enqueue work
    included when it is the longer part.  device_ms: `reps` steps enqueued while the device is busy with `blocker()` (a long matrix
    product), events around them on the stream: the kernels run back to back, so the host's share is hidden and the quotient is
    the device time of one update."""
    for _ in range(warmup):
        opt.step()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        opt.step()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    dv = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        blocker()
        a.record()
        for _ in range(reps):
            opt.step()
        b.record()
        torch.cuda.synchronize()
        dv.append(a.elapsed_time(b) / reps)
    return float(np.median(ts)), float(np.median(dv))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    shapes = tile_step_shapes()
    n_params = sum(int(np.prod(s)) for s in shapes)
    gen = torch.Generator().manual_seed(1)
    grads = [torch.randn(s, generator=gen).to(dev) for s in shapes]
    big = torch.randn(8192, 8192, device=dev)
    blocker = lambda: [torch.mm(big, big) for _ in range(8)]          # tens of ms of device work: `reps` step() calls enqueue behind it
    res = {"tensors": len(shapes), "parameters": n_params, "reps": args.reps, "warmup": args.warmup}
    sgd, adam = dict(lr=5e-4, momentum=0.9, weight_decay=1e-4), dict(lr=5e-4, weight_decay=1e-4)
    # name -> (constructor, bytes moved per parameter and step)
    makers = {"hip_sgd": (lambda ps: O.SGD(ps, **sgd), 20),
              "hip_sgd_capturable": (lambda ps: O.SGD(ps, capturable=True, **sgd), 20),
              "torch_sgd": (lambda ps: torch.optim.SGD(ps, **sgd), 20),
              "hip_adam": (lambda ps: O.Adam(ps, **adam), 28),
              "hip_adam_capturable": (lambda ps: O.Adam(ps, capturable=True, **adam), 28),
              "torch_adam": (lambda ps: torch.optim.Adam(ps, **adam), 28)}
    for name, (make, nbytes) in makers.items():
        ps = [(0.05 * torch.randn(s, generator=gen)).to(dev).requires_grad_() for s in shapes]
        for p, g in zip(ps, grads):
            p.grad = g
        step_ms, device_ms = time_steps(make(ps), args.warmup, args.reps, blocker)
        res[name] = {"step_ms": step_ms, "device_ms": device_ms, "bytes_per_step": nbytes * n_params,
                     "gb_per_s": nbytes * n_params / (device_ms * 1e-3) / 1e9}
        del ps
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
