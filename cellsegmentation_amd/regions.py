"""Small-region clean-up of segmentation masks: the reference's ``remove_small_regions`` (utils/image_processing.py:14-17), i.e.
``skimage.morphology.remove_small_objects`` followed by ``remove_small_holes``, on the HIP path (csrc/regions.hip).

Semantics, restated from scikit-image (which labels with ``scipy.ndimage.label``):

* ``connectivity`` 1 is the 4-neighbourhood (the default, and the only one the reference uses), 2 the 8-neighbourhood; the
  background is labelled with the same connectivity as the foreground.
* ``remove_small_objects`` clears every ``True`` component with fewer than ``min_size`` pixels (strict); ``min_size=0`` copies.
* ``remove_small_holes`` is ``~remove_small_objects(~m, area_threshold)``: every ``False`` component below the threshold becomes
  ``True``, the ones that touch the image border included.
* ``remove_small_regions`` removes objects first and takes the holes of the result.
* ``label`` numbers components by their lowest row-major pixel index, as ``scipy.ndimage.label``.

All of it is integer work: bit-exact and independent of launch order.  The labelling is pinned to ``scipy.ndimage.label``
(tests/golden/regions_vectors.npz); parity with scikit-image itself is NOT pinned (it is not a dependency of this project): its
two wrappers are restated.  Only boolean input is taken: scikit-image treats an integer array as a label image, which is a
different operation, and that raises ``TypeError`` here.

Every function takes ``[H, W]`` or ``[N, H, W]`` (numpy or torch; N independent images) and returns a device tensor of the same
shape.  A call enqueues a number of launches fixed by the shape and never synchronises, so it can be captured into a graph.

``measure`` turns the same labelling into one table row per foreground component (``RegionTable``: count, area, bounding box,
centroid, intensity sum / mean / maximum), pinned to ``scipy.ndimage`` (sum, mean, maximum, center_of_mass, find_objects;
tests/golden/props_vectors.npz).  With a fixed ``max_regions`` it keeps the contract above; with ``max_regions=None`` it reads the
largest component count back once to size the tables.
"""
import dataclasses
import typing

import numpy as np
import torch

from . import kernels as K

_MAX_PIXELS = (1 << 31) - 1           # per kernel call; larger batches are cut into chunks of whole images
_MAX_IMAGES = 65535


def _device():
    return torch.device("cuda", torch.cuda.current_device())


def _check_connectivity(connectivity):
    if connectivity not in (1, 2):
        raise ValueError(f"connectivity must be 1 (4-neighbourhood) or 2 (8-neighbourhood), got {connectivity!r}")
    return int(connectivity)


def _check_size(value, name):
    if isinstance(value, bool) or int(value) != value or value < 0:
        raise ValueError(f"{name} must be a non-negative integer, got {value!r}")
    return min(int(value), _MAX_PIXELS)           # no component has more pixels than a call


def _as_masks(m, what):
    """boolean numpy / torch [H,W] or [N,H,W] -> (uint8 device view [N,H,W], was_2d); argument errors before any device work."""
    t = torch.from_numpy(np.ascontiguousarray(m)) if isinstance(m, np.ndarray) else m
    if not torch.is_tensor(t):
        raise TypeError(f"{what}: expected a numpy array or a torch tensor")
    if t.dtype != torch.bool:
        raise TypeError(f"{what}: expected a boolean mask, got {t.dtype} (an integer array is a label image in scikit-image: not supported)")
    if t.dim() not in (2, 3):
        raise ValueError(f"{what}: expected [H, W] or [N, H, W], got shape {tuple(t.shape)}")
    if t.numel() == 0:
        raise ValueError(f"{what}: empty mask of shape {tuple(t.shape)}")
    if t.shape[-1] * t.shape[-2] > _MAX_PIXELS:
        raise ValueError(f"{what}: one image of {t.shape[-2]}x{t.shape[-1]} has 2^31 pixels or more")
    two_d = t.dim() == 2
    if two_d:
        t = t.unsqueeze(0)
    if not t.is_cuda:
        t = t.to(_device())
    return t.contiguous().view(torch.uint8), two_d


def _chunks(t):
    """whole images per kernel call"""
    N, H, W = t.shape
    per = max(1, min(_MAX_IMAGES, _MAX_PIXELS // (H * W)))
    return [(i, min(i + per, N)) for i in range(0, N, per)]


def _run(t, fn, out):
    """fn(chunk, out_chunk, workspace) over the chunks of t [N,H,W]; out: a tensor of t's shape"""
    ws, ws_n = None, 0
    for a, b in _chunks(t):
        if ws_n != b - a:
            ws, ws_n = K.regions_workspace(b - a, t.shape[1], t.shape[2], t.device), b - a
        fn(t[a:b], out[a:b], ws)
    return out


def _int32_like(t):
    return torch.empty(t.shape, dtype=torch.int32, device=t.device)


def label(m, connectivity=1):
    """``scipy.ndimage.label`` of every image: int32 device tensor, 0 = background, components numbered from 1 by their lowest
    row-major pixel index."""
    conn = _check_connectivity(connectivity)
    t, two_d = _as_masks(m, "label")
    out = _run(t, lambda x, o, ws: K.regions_label(x, conn, out=o, ws=ws), _int32_like(t))
    return out[0] if two_d else out


def component_areas(m, connectivity=1):
    """int32 device tensor: under every pixel, the pixel count of the connected component of equal-valued pixels it lies in
    (foreground components under ``True`` pixels, background components under ``False`` pixels)."""
    conn = _check_connectivity(connectivity)
    t, two_d = _as_masks(m, "component_areas")
    out = _run(t, lambda x, o, ws: K.regions_areas(x, conn, out=o, ws=ws), _int32_like(t))
    return out[0] if two_d else out


def _filtered(t, two_d, fn):
    out = _run(t, fn, torch.empty_like(t)).view(torch.bool)
    return out[0] if two_d else out


def remove_small_objects(m, min_size=64, connectivity=1):
    """``skimage.morphology.remove_small_objects`` of a boolean mask -> device ``torch.bool``."""
    size, conn = _check_size(min_size, "min_size"), _check_connectivity(connectivity)
    t, two_d = _as_masks(m, "remove_small_objects")
    return _filtered(t, two_d, lambda x, o, ws: K.regions_filter(x, 1, size, conn, out=o, ws=ws))


def remove_small_holes(m, area_threshold=64, connectivity=1):
    """``skimage.morphology.remove_small_holes`` of a boolean mask -> device ``torch.bool``."""
    size, conn = _check_size(area_threshold, "area_threshold"), _check_connectivity(connectivity)
    t, two_d = _as_masks(m, "remove_small_holes")
    return _filtered(t, two_d, lambda x, o, ws: K.regions_filter(x, 0, size, conn, out=o, ws=ws))


def remove_small_regions(img_bin, min_object_size, hole_area_threshold, connectivity=1, out=None):
    """utils/image_processing.py:14-17 -> device ``torch.bool``.  ``out``: a device ``torch.bool`` tensor of the input's shape to
    write into (it may be ``img_bin`` itself: in place); with it and a device input nothing is allocated but the workspace."""
    mo, ho = _check_size(min_object_size, "min_object_size"), _check_size(hole_area_threshold, "hole_area_threshold")
    conn = _check_connectivity(connectivity)
    if out is not None and not (torch.is_tensor(out) and out.is_cuda and out.dtype == torch.bool and out.is_contiguous()
                                and tuple(out.shape) == tuple(getattr(img_bin, "shape", ()))):
        raise ValueError("remove_small_regions: out must be a contiguous device torch.bool tensor of the input's shape")
    t, two_d = _as_masks(img_bin, "remove_small_regions")
    if out is None:
        return _filtered(t, two_d, lambda x, o, ws: K.regions_remove_small(x, mo, ho, conn, out=o, ws=ws))
    o8 = out.view(torch.uint8)
    _run(t, lambda x, o, ws: K.regions_remove_small(x, mo, ho, conn, out=o, ws=ws), o8.unsqueeze(0) if two_d else o8)
    return out


def threshold(probs, thr):
    """``probs > thr`` as numpy evaluates it for a float32 array and a Python float (``thr`` rounded to float32 first) -> device
    ``torch.bool``, same shape."""
    t = torch.from_numpy(np.ascontiguousarray(probs)) if isinstance(probs, np.ndarray) else probs
    if not torch.is_tensor(t) or t.dtype != torch.float32:
        raise TypeError(f"threshold expects float32 probabilities, got {getattr(t, 'dtype', type(t))}")
    if not t.is_cuda:
        t = t.to(_device())
    return K.regions_threshold(t.contiguous(), float(thr)).view(torch.bool)


@dataclasses.dataclass
class RegionTable:
    """Per-component measurements of N masks as device tensors; row k of image n is scipy label k + 1 and rows from
    min(count, capacity) on are zero.  ``counts`` int32 [N] is the true component count, also above the capacity; ``area`` int32
    [N, cap]; ``bbox`` int32 [N, cap, 4] = (r0, c0, r1, c1), half-open (the ``find_objects`` slices); ``sum_rc`` int64 [N, cap, 2];
    ``intensity_sum`` int64 [N, cap] and ``intensity_max`` int32 [N, cap], or None without an intensity image."""
    counts: torch.Tensor
    capacity: int
    area: torch.Tensor
    bbox: torch.Tensor
    sum_rc: torch.Tensor
    intensity_sum: typing.Optional[torch.Tensor] = None
    intensity_max: typing.Optional[torch.Tensor] = None

    def centroid(self):
        """float64 [N, cap, 2] = ``scipy.ndimage.center_of_mass`` (sum_rc / area), NaN in unused rows; on the device."""
        return self.sum_rc.to(torch.float64) / self.area.to(torch.float64).unsqueeze(-1)

    def mean_intensity(self):
        """float64 [N, cap] = ``scipy.ndimage.mean`` of the intensity (intensity_sum / area), NaN in unused rows; on the device."""
        if self.intensity_sum is None:
            raise ValueError("mean_intensity: the table was measured without an intensity image")
        return self.intensity_sum.to(torch.float64) / self.area.to(torch.float64)

    def overflowed(self):
        """device bool [N]: the image has more components than the table has rows"""
        return self.counts > self.capacity

    def per_image(self):
        """A host list of N dicts of numpy arrays trimmed to min(count, capacity) rows: ``area``, ``bbox``, ``centroid`` and, with
        an intensity image, ``intensity_sum``, ``intensity_mean``, ``intensity_max``.  The one method that synchronises."""
        cols = {"area": self.area, "bbox": self.bbox, "centroid": self.centroid()}
        if self.intensity_sum is not None:
            cols.update(intensity_sum=self.intensity_sum, intensity_mean=self.mean_intensity(), intensity_max=self.intensity_max)
        cols = {k: v.cpu().numpy() for k, v in cols.items()}
        counts = self.counts.cpu().numpy()
        return [{k: v[n, :min(int(c), self.capacity)] for k, v in cols.items()} for n, c in enumerate(counts)]


def _as_intensity(v, shape):
    """uint8 numpy / torch of the mask's shape -> the tensor (not yet on the device); argument errors only"""
    t = torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v
    if not torch.is_tensor(t):
        raise TypeError("measure: intensity must be a numpy array or a torch tensor")
    if t.dtype != torch.uint8:
        raise TypeError(f"measure: intensity must be uint8, got {t.dtype}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"measure: intensity of shape {tuple(t.shape)} for a mask of shape {tuple(shape)}")
    return t


def measure(m, intensity=None, connectivity=1, max_regions=None):
    """One row per connected foreground component of every image -> ``RegionTable``.  ``intensity``: uint8 of the mask's shape, or
    None.  ``max_regions=int`` fixes the rows per image (capped at H W; components numbered above it are counted, not measured):
    nothing synchronises and the call can be captured into a graph.  ``max_regions=None`` numbers first, reads the largest count
    back (the one synchronisation) and measures with exactly that capacity (1 when there is no component)."""
    conn = _check_connectivity(connectivity)
    if max_regions is not None and (isinstance(max_regions, bool) or int(max_regions) != max_regions or max_regions < 1):
        raise ValueError(f"max_regions must be a positive integer or None, got {max_regions!r}")
    v = None if intensity is None else _as_intensity(intensity, getattr(m, "shape", ()))
    t, two_d = _as_masks(m, "measure")
    N, H, W = t.shape
    if v is not None:
        v = v.to(t.device).contiguous().view(N, H, W)
    chunks = _chunks(t)
    counts = torch.empty((N,), dtype=torch.int32, device=t.device)
    ws, ws_n, numbered = None, 0, False

    def workspace(n):
        nonlocal ws, ws_n
        if ws_n != n:
            ws, ws_n = K.regions_workspace(n, H, W, t.device), n
        return ws

    if max_regions is None:
        for a, b in chunks:
            K.regions_number(t[a:b], conn, counts=counts[a:b], ws=workspace(b - a))
        cap = max(1, int(counts.max()))                                  # the one synchronisation
        numbered = len(chunks) == 1                                      # one call: its workspace still holds the numbering
    else:
        cap = min(int(max_regions), H * W)
    dev = t.device
    area = torch.empty((N, cap), dtype=torch.int32, device=dev)
    bbox = torch.empty((N, cap, 4), dtype=torch.int32, device=dev)
    sums = torch.empty((N, cap, 2), dtype=torch.int64, device=dev)
    isum = None if v is None else torch.empty((N, cap), dtype=torch.int64, device=dev)
    imax = None if v is None else torch.empty((N, cap), dtype=torch.int32, device=dev)
    for a, b in chunks:
        K.regions_measure(t[a:b], cap, None if v is None else v[a:b], conn, numbered, counts[a:b], area[a:b], bbox[a:b], sums[a:b],
                          None if v is None else isum[a:b], None if v is None else imax[a:b], ws=workspace(b - a))
    return RegionTable(counts, cap, area, bbox, sums, isum, imax)
