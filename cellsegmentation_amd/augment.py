"""Training augmentation on the staged input path (csrc/augment.hip): the reference's flips and colour jitter applied while the
uint8 images resident in HBM are cropped, scaled (ToTensor) and normalised into the NHWC-8 operand the models accept as "already
staged" -- ``tiles.gather_tiles`` with two more steps, and the same bits where neither is asked for.

* Flips: ``LystoDataset(augment=True)`` adds every training image three more times with ``transformIDX`` 1, 2, 3 (horizontal,
  vertical, both), applied between ToTensor and Normalize; in modes 1-3 to the cropped tile (dataset/dataset.py:70-97, 118-120,
  209-211).  A flip code here is that ``transformIDX``.
* Colour jitter: ``Maskset(augment=True)`` applies ``ColorJitter(brightness=0.1, contrast=0.3, saturation=0.4, hue=0.05)`` between
  ToTensor and Normalize (dataset/dataset.py:483-495).  A jitter record is what ``ColorJitter.get_params`` of torchvision 0.11.2
  returns: the order of the four ops and their factors.  The arithmetic is torchvision's for float images, restated in
  include/cellseg_hip.h and tests/augment_ref.py; torchvision is not a dependency, so parity with torchvision itself is not pinned.

Per tile: crop -> /255 -> colour ops on the un-flipped crop -> flip -> (v - mean) / std.  The contrast op blends with the mean grey
of the whole tile (which a flip does not change); the kernels sum it order-independently, so two calls give the same bits.

Every argument is checked on the host before any device work.  ``TileTrainBatches`` and ``MaskTrainBatches`` stand where a
reference-style training script has ``DataLoader(dataset)`` when the data set already lives on the device.
"""
import math

import numpy as np
import torch

from . import kernels as K
from .synth import IMAGENET_MEAN, IMAGENET_STD

FLIP_NONE, FLIP_H, FLIP_V, FLIP_HV = 0, 1, 2, 3
OP_BRIGHTNESS, OP_CONTRAST, OP_SATURATION, OP_HUE = 0, 1, 2, 3
_MAX = (1 << 31) - 1


def draw_color_jitter(n, brightness=0.1, contrast=0.3, saturation=0.4, hue=0.05, generator=None):
    """n jitter records -> (order int8 [n, 4], factors float32 [n, 4]): slot k of a record holds the k-th op applied (0 brightness,
    1 contrast, 2 saturation, 3 hue) and its factor.  The defaults are Maskset's.

    Per record the draws are made the way ``ColorJitter.get_params`` of torchvision 0.11.2 makes them: ``torch.randperm(4)``, then
    one ``torch.empty(1).uniform_(lo, hi)`` each for brightness, contrast and saturation from ``[max(0, 1 - x), 1 + x]`` and for hue
    from ``[-x, x]``, in that order.  A parameter given as 0 or None disables its op: its slot gets code -1 (factor 0) and no number
    is drawn for it.  Draw-for-draw equality with torchvision under the same seed is the intent; it is not a guarantee, since no
    test here can compare against torchvision."""
    n = int(n)
    if n < 0:
        raise ValueError(f"draw_color_jitter: n must be non-negative, got {n}")
    ranges = []
    for name, x, centre, bound in (("brightness", brightness, 1.0, None), ("contrast", contrast, 1.0, None),
                                   ("saturation", saturation, 1.0, None), ("hue", hue, 0.0, 0.5)):
        if x is None or x == 0:
            ranges.append(None)
            continue
        if isinstance(x, bool) or not isinstance(x, (int, float)) or not math.isfinite(x) or x < 0:
            raise ValueError(f"draw_color_jitter: {name} must be a non-negative number, got {x!r}")
        if bound is not None and x > bound:
            raise ValueError(f"draw_color_jitter: {name} must be at most {bound}, got {x!r}")
        ranges.append((max(0.0, centre - x), centre + x) if centre else (-float(x), float(x)))
    order = np.full((n, 4), -1, np.int8)
    factors = np.zeros((n, 4), np.float32)
    for i in range(n):
        perm = torch.randperm(4, generator=generator).tolist()
        drawn = [None if r is None else float(torch.empty(1).uniform_(r[0], r[1], generator=generator)) for r in ranges]
        for k, op in enumerate(perm):
            if drawn[op] is not None:
                order[i, k] = op
                factors[i, k] = drawn[op]
    return order, factors


def _host(x, what):
    """sequence / numpy / torch (host or device) -> numpy on the host"""
    if torch.is_tensor(x):
        return x.detach().cpu().numpy()
    try:
        return np.asarray(x)
    except Exception as e:                                                 # ragged input
        raise TypeError(f"{what}: expected an array") from e


def _as_images(images_u8, what):
    if not torch.is_tensor(images_u8):
        raise TypeError(f"{what}: expected a torch tensor of uint8 images")
    if images_u8.dtype != torch.uint8:
        raise TypeError(f"{what}: expected uint8 images, got {images_u8.dtype}")
    if images_u8.dim() != 4 or images_u8.shape[-1] != 3:
        raise ValueError(f"{what}: expected images shaped [n, H, W, 3], got shape {tuple(images_u8.shape)}")
    if images_u8.numel() == 0:
        raise ValueError(f"{what}: empty images of shape {tuple(images_u8.shape)}")
    if images_u8.shape[0] > _MAX or images_u8.shape[1] * images_u8.shape[2] > _MAX:
        raise ValueError(f"{what}: 2^31 images, or pixels in one image, or more")
    return images_u8


def _as_ints(x, what, shape):
    a = _host(x, what)
    if a.dtype.kind not in "iu":
        raise TypeError(f"{what}: expected integers, got {a.dtype}")
    if a.shape != shape:
        raise ValueError(f"{what}: expected shape {list(shape)}, got {list(a.shape)}")
    return a.astype(np.int64)


def _as_flips(flips, T):
    if flips is None:
        return None
    a = _as_ints(flips, "flips", (T,))
    if a.size and (a.min() < 0 or a.max() > 3):
        raise ValueError("flips: a flip code is 0 (none), 1 (horizontal), 2 (vertical) or 3 (both)")
    return a.astype(np.int8)


def _as_jitter(jitter, T):
    """(order, factors) with T rows -> (int8 [T, 4], float32 [T, 4], some record holds a contrast op), or (None, None, False)"""
    if jitter is None:
        return None, None, False
    if not isinstance(jitter, (tuple, list)) or len(jitter) != 2:
        raise TypeError("jitter: expected the pair (order, factors)")
    order = _host(jitter[0], "jitter order")
    factors = _host(jitter[1], "jitter factors")
    if order.dtype.kind not in "iu":
        raise TypeError(f"jitter order: expected integers, got {order.dtype}")
    if factors.dtype.kind != "f":
        raise TypeError(f"jitter factors: expected floats, got {factors.dtype}")
    if order.shape != (T, 4) or factors.shape != (T, 4):
        raise ValueError(f"jitter: expected order and factors shaped [{T}, 4], got {list(order.shape)} and {list(factors.shape)}")
    order = order.astype(np.int64)
    if order.size and (order.min() < -1 or order.max() > 3):
        raise ValueError("jitter order: an op code is 0 brightness, 1 contrast, 2 saturation, 3 hue or -1 (unused slot)")
    for op in range(4):
        if ((order == op).sum(axis=1) > 1).any():
            raise ValueError(f"jitter order: op code {op} is repeated within a record")
    f32 = factors.astype(np.float32)
    if not np.isfinite(f32).all():
        raise ValueError("jitter factors: a factor is not finite")
    if ((order >= 0) & (order <= 2) & (f32 < 0)).any():
        raise ValueError("jitter factors: a brightness, contrast or saturation factor is negative")
    if ((order == 3) & (np.abs(f32) > 0.5)).any():
        raise ValueError("jitter factors: a hue factor lies outside [-0.5, 0.5]")
    return order.astype(np.int8), f32, bool((order == OP_CONTRAST).any())


def _stage(images_u8, tile_img, tile_rc, th, tw, flips, jitter, dtype, mean, std, what):
    images_u8 = _as_images(images_u8, what)
    n, H, W, _ = images_u8.shape
    th, tw = int(th), int(tw)
    if th < 1 or tw < 1 or th > H or tw > W:
        raise ValueError(f"{what}: a {th}x{tw} tile does not fit {H}x{W} images")
    K._code(dtype)
    ti = _host(tile_img, "tile_img")
    if ti.ndim != 1:
        raise ValueError(f"tile_img: expected shape [T], got {list(ti.shape)}")
    T = len(ti)
    if T < 1 or T > _MAX:
        raise ValueError(f"{what}: a call takes 0 < T < 2^31 tiles, got {T}")
    ti = _as_ints(ti, "tile_img", (T,))
    rc = _as_ints(tile_rc, "tile_rc", (T, 2))
    if ti.min() < 0 or ti.max() >= n:
        raise ValueError(f"tile_img: an image index lies outside 0..{n - 1}")
    if rc.min() < 0 or (rc[:, 0] + th > H).any() or (rc[:, 1] + tw > W).any():
        raise ValueError(f"tile_rc: a {th}x{tw} tile leaves its {H}x{W} image")
    fl = _as_flips(flips, T)
    order, factors, has_contrast = _as_jitter(jitter, T)
    if len(mean) != 3 or len(std) != 3:
        raise ValueError(f"{what}: mean and std have three entries")
    if not images_u8.is_cuda:
        raise RuntimeError("cellsegmentation_amd kernels need GPU tensors: the HIP path has no CPU fallback")
    dev = images_u8.device

    def up(a, dt):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dt)

    return K.stage_augmented(images_u8.contiguous(), up(ti, torch.int32), up(rc, torch.int32), th, tw, up(fl, torch.int8),
                             up(order, torch.int8), up(factors, torch.float32), has_contrast, dtype, mean, std)


def stage_tiles(images_u8, tile_img, tile_rc, size, flips=None, jitter=None, dtype=torch.bfloat16, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """``tiles.gather_tiles`` with augmentation: images_u8 uint8 [n, H, W, 3] on the GPU, tile_img [T] (image per tile), tile_rc
    [T, 2] (upper-left row, col) -> NHWC [T, size, size, 8] dtype.  flips: T flip codes (FLIP_NONE / FLIP_H / FLIP_V / FLIP_HV, the
    reference's transformIDX), applied to the cropped tile.  jitter: the pair (order, factors) of ``draw_color_jitter`` with T rows,
    applied per tile (a contrast op takes the mean of the tile).  Neither: the bits of ``gather_tiles``."""
    return _stage(images_u8, tile_img, tile_rc, size, size, flips, jitter, dtype, mean, std, "stage_tiles")


def stage_images(images_u8, flips=None, jitter=None, idx=None, dtype=torch.bfloat16, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """Whole images as one tile each: images_u8 uint8 [n, H, W, 3] on the GPU -> NHWC [B, H, W, 8] dtype.  idx selects and orders the
    images (default: all, in order); flips and jitter have one entry per OUTPUT image."""
    images_u8 = _as_images(images_u8, "stage_images")
    n, H, W, _ = images_u8.shape
    if idx is None:
        idx = np.arange(n)
    else:
        idx = _host(idx, "idx")
        if idx.ndim != 1:
            raise ValueError(f"idx: expected shape [B], got {list(idx.shape)}")
    return _stage(images_u8, idx, np.zeros((len(idx), 2), np.int64), H, W, flips, jitter, dtype, mean, std, "stage_images")


def _batches(n, batch_size):
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError(f"batch_size must be positive, got {batch_size}")
    return batch_size, (n + batch_size - 1) // batch_size


class TileTrainBatches:
    """Stands where ``DataLoader(LystoDataset in mode 3, batch_size)`` stands: yields ``(tiles [b, size, size, 8], labels int64 [b])``
    in the order of ``train_data``, the last batch short.

    train_data: the rows of ``make_train_data`` -- ``stage.make_train_data``'s int array ``[(tileIDX, x, y, label)]`` or the
    reference's ``(tileIDX, (x, y), label)`` tuples; (x, y) is the tile's (row, col).  transform_idx: one flip code per IMAGE (the
    reference's ``transformIDX``), or None.  The flip of a tile is ``transform_idx[tileIDX]``, the code of the image the tile was cut
    from.  The reference's mode 3 reads ``self.transformIDX[self.tileIDX[idx]]`` with ``idx`` the position in the shuffled
    ``train_data``, i.e. the code of some other tile's image: a bug of the reference's that is not reproduced here."""

    def __init__(self, images_u8, train_data, transform_idx, tile_size, batch_size, dtype=torch.bfloat16):
        self.images = _as_images(images_u8, "TileTrainBatches")
        rows = train_data
        if not (isinstance(rows, np.ndarray) and rows.ndim == 2) and not torch.is_tensor(rows):
            rows = [(int(t), int(g[0]), int(g[1]), int(lab)) for t, g, lab in rows]
        rows = _host(rows, "train_data")
        if rows.ndim != 2 or rows.shape[1] != 4 or rows.dtype.kind not in "iu":
            raise ValueError("train_data: expected integer rows (tileIDX, x, y, label)")
        rows = rows.astype(np.int64)
        n = self.images.shape[0]
        if len(rows) and (rows[:, 0].min() < 0 or rows[:, 0].max() >= n):
            raise ValueError(f"train_data: a tileIDX lies outside 0..{n - 1}")
        self.tile_img, self.tile_rc, labels = rows[:, 0], rows[:, 1:3], rows[:, 3]
        self.flips = None
        if transform_idx is not None:
            self.flips = _as_flips(transform_idx, n)[self.tile_img]
        self.tile_size = int(tile_size)
        self.batch_size, self._len = _batches(len(rows), batch_size)
        K._code(dtype)
        self.dtype = dtype
        self.labels = torch.from_numpy(labels).to(self.images.device)

    def __len__(self):
        return self._len

    def __iter__(self):
        for b in range(self._len):
            s = slice(b * self.batch_size, (b + 1) * self.batch_size)
            yield (stage_tiles(self.images, self.tile_img[s], self.tile_rc[s], self.tile_size, None if self.flips is None else self.flips[s],
                               None, self.dtype), self.labels[s])


class MaskTrainBatches:
    """Stands where ``DataLoader(Maskset(..., augment), batch_size, shuffle)`` stands: yields ``(images [b, H, W, 8], masks [b, ...],
    labels [b, ...])``, the last batch short.  masks and labels (tensors with one leading entry per image, on any device) pass through
    untouched, indexed like the images.  augment: every image gets a fresh ``draw_color_jitter`` record each epoch (each
    ``__iter__``), drawn from ``generator`` in the order the images are yielded; shuffle: a fresh ``torch.randperm`` from the same
    generator each epoch, drawn before the records."""

    def __init__(self, images_u8, masks, labels, batch_size, augment=False, shuffle=False, generator=None, dtype=torch.bfloat16):
        self.images = _as_images(images_u8, "MaskTrainBatches")
        n = self.images.shape[0]
        for what, t in (("masks", masks), ("labels", labels)):
            if not torch.is_tensor(t):
                raise TypeError(f"{what}: expected a torch tensor")
            if t.dim() < 1 or t.shape[0] != n:
                raise ValueError(f"{what}: expected one entry per image ({n}), got shape {tuple(t.shape)}")
        self.masks, self.labels = masks, labels
        self.batch_size, self._len = _batches(n, batch_size)
        self.augment, self.shuffle, self.generator = bool(augment), bool(shuffle), generator
        K._code(dtype)
        self.dtype = dtype

    def __len__(self):
        return self._len

    def __iter__(self):
        n = self.images.shape[0]
        order = torch.randperm(n, generator=self.generator) if self.shuffle else torch.arange(n)
        for b in range(self._len):
            idx = order[b * self.batch_size:(b + 1) * self.batch_size]
            jitter = draw_color_jitter(len(idx), generator=self.generator) if self.augment else None
            yield (stage_images(self.images, None, jitter, idx, self.dtype), self.masks[idx.to(self.masks.device)],
                   self.labels[idx.to(self.labels.device)])
