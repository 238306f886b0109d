"""Sliding-window tiling on the device: the host computes the tile grid exactly like the reference's
``get_tiles`` (dataset/dataset.py:718-742, including the border-aligned last row/column); the pixels are gathered, scaled
(ToTensor) and normalised (ImageNet mean/std, dataset/dataset.py:78-83) by one HIP kernel straight into the NHWC compute
layout, so overlapping tiles never cross PCIe more than once."""
import ctypes

import numpy as np
import torch

from . import _lib
from . import kernels as K
from .synth import IMAGENET_MEAN, IMAGENET_STD


def _axis_origins(length, interval, size):
    o = list(range(0, length - size + 1, interval))
    if not o:
        raise ValueError("tile larger than the image")
    if o[-1] + size != length:
        o.append(length - size)
    return o


def get_tiles(shape_hw, interval, size):
    """[(row, col)] upper-left corners, same order as the reference's get_tiles(image, interval, size)."""
    h, w = shape_hw
    return [(x, y) for x in _axis_origins(h, interval, size) for y in _axis_origins(w, interval, size)]


def _pair(v, what):
    try:
        a, b = (v, v) if np.ndim(v) == 0 else v
        a, b = int(a), int(b)
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be an integer or a pair of integers, got {v!r}") from None
    if a <= 0 or b <= 0:
        raise ValueError(f"{what} must be positive, got {v!r}")
    return a, b


def sample_patches(size_hw, patch_size=(299, 299), interval=None):
    """[(x, y)] patch corners of a whole slide or ROI, in the order of the reference's ``MaskTestset.sample_patches``
    (dataset/dataset.py:577-612; both of its modes walk the same grid): x outer, y inner, the last origin of an axis aligned to
    the border.  ``size_hw[k]`` pairs with ``patch_size[k]`` and ``interval[k]``; interval=None is ``patch_size - 16``
    (dataset/dataset.py:540,548).  A patch larger than the image raises ``ValueError`` (the reference dies with ``IndexError``)."""
    ph, pw = _pair(patch_size, "patch_size")
    ih, iw = (ph - 16, pw - 16) if interval is None else _pair(interval, "interval")
    if ih <= 0 or iw <= 0:
        raise ValueError(f"interval must be positive, got {(ih, iw)} for patch_size {(ph, pw)}")
    h, w = int(size_hw[0]), int(size_hw[1])
    return [(x, y) for x in _axis_origins(h, ih, ph) for y in _axis_origins(w, iw, pw)]


def tile_index(n_images, shape_hw, interval, size):
    """tileIDX (image id per tile) and the (row, col) grid for n_images equally sized images (dataset/dataset.py:118-140)."""
    grid = np.asarray(get_tiles(shape_hw, interval, size), dtype=np.int32)
    tile_img = np.repeat(np.arange(n_images, dtype=np.int32), len(grid))
    tile_rc = np.tile(grid, (n_images, 1))
    return tile_img, tile_rc


def gather_tiles(images_u8, tile_img, tile_rc, size, dtype=torch.bfloat16, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """images_u8: uint8 [n, H, W, 3] on the GPU; tile_img int32 [T]; tile_rc int32 [T, 2] -> NHWC [T, size, size, 8] dtype."""
    if images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or images_u8.shape[-1] != 3:
        raise TypeError("gather_tiles expects uint8 images shaped [n, H, W, 3]")
    n, H, W, _ = images_u8.shape
    dev = images_u8.device
    ti = torch.as_tensor(tile_img, dtype=torch.int32, device=dev).contiguous()
    rc = torch.as_tensor(tile_rc, dtype=torch.int32, device=dev).contiguous()
    T = ti.numel()
    out = torch.empty((T, size, size, 8), dtype=dtype, device=dev)
    m = (ctypes.c_float * 3)(*[float(v) for v in mean])
    s = (ctypes.c_float * 3)(*[float(v) for v in std])
    _lib.check(_lib.load().cs_tile_gather(K._p(images_u8), n, H, W, K._p(ti), K._p(rc), T, size, m, s, K._code(dtype), K._p(out), K._stream()),
               "tile_gather")
    return out
