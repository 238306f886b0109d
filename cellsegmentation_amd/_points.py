"""The ragged point set that ``score``, ``spatial``, ``regions.split``, ``render.draw_points`` and ``DetectResult`` share: integer
``points`` [P, 2], ``offsets`` [N + 1] (image n owns ``points[offsets[n]:offsets[n + 1]]``) and ``limits`` (None, one count or one per
image: Python's ``[:c]`` of every image's points), numpy or torch, on the host or the device -> three device tensors, the operand of
csrc/cs_points.h.  Argument errors come before any device work."""
import numpy as np
import torch

_I32 = (-(1 << 31), (1 << 31) - 1)
_INT_DTYPES = (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64)


def points(x, what):
    """-> ([n, 2] integer numpy array or torch tensor, is_torch); an empty 1-D array (``np.asarray([])``) is no points."""
    if not torch.is_tensor(x):
        x = np.asarray(x)
        if x.size == 0 and x.ndim <= 2:
            return np.zeros((0, 2), np.int64), False
    if x.ndim != 2 or x.shape[1] != 2:
        raise ValueError(f"{what}: expected points shaped [n, 2], got shape {tuple(x.shape)}")
    if torch.is_tensor(x):
        if x.dtype not in _INT_DTYPES:
            raise TypeError(f"{what}: expected integer coordinates, got {x.dtype}")
        return x, True
    if x.dtype.kind not in "iu":
        raise TypeError(f"{what}: expected integer coordinates, got {x.dtype}")
    if x.dtype == np.uint64 and x.size and int(x.max()) > np.iinfo(np.int64).max:
        raise ValueError(f"{what}: a coordinate does not fit int64")
    return x, False


def offsets(off, n_points, n_images, what):
    """offsets (None = one image; numpy / sequence / torch, host or device) -> (host int64 array or None, device tensor or None)"""
    if off is None:
        return np.asarray([0, n_points], np.int64), None
    if torch.is_tensor(off):
        if off.dtype not in _INT_DTYPES or off.dim() != 1:
            raise TypeError(f"{what}: expected a 1-D integer tensor")
        if off.is_cuda:
            if n_images is not None and off.numel() != n_images + 1:
                raise ValueError(f"{what}: expected {n_images + 1} offsets, got {off.numel()}")
            return None, off.to(torch.int64)
        off = off.numpy()
    off = np.asarray(off)
    if off.ndim != 1 or off.dtype.kind not in "iu" or len(off) < 2:
        raise ValueError(f"{what}: expected a 1-D integer sequence of N + 1 offsets")
    off = off.astype(np.int64)
    if off[0] != 0 or off[-1] != n_points or np.any(np.diff(off) < 0):
        raise ValueError(f"{what}: offsets must rise from 0 to the number of points ({n_points})")
    if n_images is not None and len(off) != n_images + 1:
        raise ValueError(f"{what}: expected {n_images + 1} offsets, got {len(off)}")
    return off, None


def ragged(per_image):
    """a sequence of N per-image point arrays ([k, 2], or empty) -> (points [sum k, 2], offsets int64 [N + 1]), on the host"""
    arrs = []
    for i, a in enumerate(per_image):
        a, is_torch = points(a, f"points of image {i}")
        arrs.append(a.cpu().numpy() if is_torch else a)
    off = np.zeros(len(arrs) + 1, np.int64)
    if arrs:
        np.cumsum([len(a) for a in arrs], out=off[1:])
    pts = np.concatenate([a.astype(np.int64) for a in arrs]) if arrs else np.zeros((0, 2), np.int64)
    return pts, off


def limits(limits, n_images):
    """None, one count or one per image -> host int32 [N] (or a device tensor as given) with Python's [:c] meaning kept"""
    if limits is None:
        return None
    if torch.is_tensor(limits) and limits.is_cuda:
        if limits.dtype not in _INT_DTYPES or limits.dim() != 1 or limits.numel() != n_images:
            raise ValueError(f"limits: expected {n_images} integers")
        return limits
    lim = np.asarray(limits.numpy() if torch.is_tensor(limits) else limits)
    if lim.dtype.kind not in "iu":
        raise TypeError(f"limits: expected integers, got {lim.dtype}")
    if lim.ndim == 0:
        lim = np.full(n_images, int(lim))
    if lim.shape != (n_images,):
        raise ValueError(f"limits: expected one count or {n_images} counts, got shape {lim.shape}")
    return np.clip(lim.astype(np.int64), *_I32).astype(np.int32)          # clipping keeps the slice's meaning: n_hat < 2^31


class PointSet:
    """One checked point set: ``pts`` [P, 2], ``off`` [N + 1] and ``lim`` [N] | None, each a host numpy array or a device tensor as
    given (``on_device``: the points are; ``off`` is None where the offsets are a device tensor, ``off_dev``); ``n_images``, ``rows``.
    Nothing here touches the device until ``upload``.

    ``points_``: one ``[k, 2]`` array of a single image, the concatenated points of ``offsets_`` (host or device offsets), or --
    ``per_image`` -- a sequence of one array per image.  ``n_images``: the N the set must have, None = whatever the offsets say.
    ``max_images``: the images of one call (``regions.split`` serves a larger batch in chunks)."""

    def __init__(self, points_, offsets_=None, limits_=None, n_images=None, what="points", per_image=False, max_images=65535):
        if per_image:
            if n_images is not None and len(points_) != n_images:
                raise ValueError(f"{what}: {n_images} images but {len(points_)} point arrays")
            self.pts, self.off, self.on_device, self.off_dev = *ragged(points_), False, None
        else:
            self.pts, is_torch = points(points_, what)
            self.on_device = is_torch and self.pts.is_cuda
            if is_torch and not self.on_device:
                self.pts = self.pts.numpy()
            if offsets_ is None and n_images not in (None, 1):
                raise ValueError(f"{what}: {n_images} images: pass one point array per image, or offsets")
            self.off, self.off_dev = offsets(offsets_, self.pts.shape[0], n_images, f"{what} offsets")
        self.n_images = (len(self.off) if self.off is not None else self.off_dev.numel()) - 1
        if self.n_images < 1 or self.n_images > max_images:
            raise ValueError(f"{what}: a call takes 1 to {max_images} images, got {self.n_images}")
        self.lim = limits(limits_, self.n_images)
        if not self.on_device:
            self.pts = self.pts.astype(np.int64, copy=False)               # uint64 too: points() has checked that it fits
        self.rows = int(self.pts.shape[0])
        if self.rows >= 1 << 31:
            raise ValueError(f"{what}: a call takes fewer than 2^31 points")

    def upload(self, dev, dtype=torch.int64):
        """-> self, with ``pts_dev`` (of ``dtype``), ``off_dev`` int64 and ``lim_dev`` int32 | None contiguous on ``dev``"""
        def up(x, dt):
            x = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
            return x.to(device=dev, dtype=dt).contiguous()

        self.pts_dev = up(self.pts, dtype)
        self.off_dev = up(self.off_dev if self.off is None else self.off, torch.int64)
        self.lim_dev = None if self.lim is None else up(self.lim, torch.int32)
        return self
