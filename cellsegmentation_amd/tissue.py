"""Tissue detection for whole-slide streaming on the HIP path (csrc/tissue.hip): which patches of a slide hold tissue at all, so that
``inference.detect_slide(..., tissue=...)`` spends its two forwards per patch on those only.  The reference runs every patch.

Images are uint8 RGB, ``[H, W, 3]`` or ``[N, H, W, 3]``, numpy or torch, on the host or the device; one image in gives one result
out (``[256]``, ``[H, W]``), a batch a batch.  A pixel's feature is an integer in [0, 255], selected by ``channel``:

* ``"chroma"`` (the default): ``max(r, g, b) - min(r, g, b)``.  White glass, grey shadow and black pen marks all score low, stained
  tissue scores high.
* ``"darkness"``: ``255 - ((77 r + 150 g + 29 b + 128) >> 8)``, the inverted integer luma.

Tissue is ``feature > threshold``; the threshold is given or Otsu's, computed exactly (``otsu``) from the 256-bin histogram of the
image.  A patch is kept when its window holds at least ``min_pixels`` tissue pixels.  Everything is integer arithmetic: the
histogram, the mask, the per-patch counts and the selection are the same bits whatever the launch geometry, and the kept patches
keep the order of ``tiles.sample_patches`` (``stitch_logits`` lets later patches overwrite earlier ones).

Argument errors are raised before the library is loaded or the device is touched.
"""
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import kernels as K
from ._args import _device, _tensor
from .tiles import _pair, sample_patches

CHANNELS = {"chroma": K.CS_TISSUE_CHROMA, "darkness": K.CS_TISSUE_DARKNESS}
MAX_IMAGES = 65535


def _channel(channel):
    if not isinstance(channel, str) or channel not in CHANNELS:
        raise ValueError(f"channel must be one of {sorted(CHANNELS)}, got {channel!r}")
    return CHANNELS[channel]


def _rgb(images_u8, what):
    """numpy / torch uint8 [H, W, 3] or [N, H, W, 3] -> (the [N, H, W, 3] tensor where it lives, one image given)"""
    t = _tensor(images_u8)
    if not torch.is_tensor(t):
        raise TypeError(f"{what}: expected a numpy array or a torch tensor")
    if t.dtype != torch.uint8:
        raise TypeError(f"{what}: expected uint8 RGB images, got {t.dtype}")
    if t.dim() not in (3, 4) or t.shape[-1] != 3:
        raise ValueError(f"{what}: expected [H, W, 3] or [N, H, W, 3], got shape {tuple(t.shape)}")
    one = t.dim() == 3
    if one:
        t = t.unsqueeze(0)
    N, H, W, _ = t.shape
    if t.numel() == 0:
        raise ValueError(f"{what}: empty images of shape {tuple(t.shape)}")
    if N > MAX_IMAGES or H * W >= 1 << 31:
        raise ValueError(f"{what}: a call takes up to {MAX_IMAGES} images of fewer than 2^31 pixels, got {(N, H, W)}")
    return t, one


def _check_threshold(v, what="threshold"):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not -1 <= v <= 255:
        raise ValueError(f"{what} must be an integer in [-1, 255] (tissue is feature > threshold), got {v!r}")
    return int(v)


def _thresholds(threshold, n, one):
    """None | int | one int per image -> a list of n ints, or None"""
    if threshold is None:
        return None
    if isinstance(threshold, (int, np.integer)) or np.ndim(threshold) == 0:
        return [_check_threshold(threshold)] * n
    thr = [_check_threshold(v) for v in (threshold.tolist() if hasattr(threshold, "tolist") else threshold)]
    if len(thr) != n:
        raise ValueError(f"threshold: {n} image{'s' if n != 1 else ''} but {len(thr)} thresholds")
    return thr


def histogram(images_u8, channel="chroma"):
    """The pixels of every image per value of its feature -> int64 ``[N, 256]`` on the device (``[256]`` for one image)."""
    code = _channel(channel)
    t, one = _rgb(images_u8, "histogram")
    h = K.tissue_histogram(t.to(_device(t)).contiguous(), code)
    return h[0] if one else h


def _otsu_one(h):
    Wt = sum(h)
    S = sum(v * c for v, c in enumerate(h))
    best_t, best_num, best_den = None, 0, 1
    w0 = S0 = 0
    for t in range(255):
        w0 += h[t]
        S0 += t * h[t]
        if w0 == 0 or Wt - w0 == 0:
            continue
        d = S0 * Wt - S * w0
        num, den = d * d, w0 * (Wt - w0)
        if best_t is None or num * best_den > best_num * den:              # strictly larger: the lowest t wins a tie
            best_t, best_num, best_den = t, num, den
    if best_t is None:
        return next((v for v, c in enumerate(h) if c), 0)
    return best_t


def otsu(hist):
    """Otsu's threshold of a 256-bin histogram, on the host in exact integer arithmetic -> a Python int (a list of ints for a
    batch ``[N, 256]``).  With ``w0(t) = sum_{v <= t} h[v]``, ``S0(t) = sum_{v <= t} v h[v]`` and the totals ``Wt``, ``S``, the result
    is the ``t`` in 0..254 with ``w0 > 0`` and ``Wt - w0 > 0`` that maximises ``(S0 Wt - S w0)^2 / (w0 (Wt - w0))`` -- the
    between-class variance times ``Wt^2``, class 0 being the values ``<= t``.  The fractions are compared by cross-multiplication
    in Python integers and the lowest ``t`` wins a tie.  A histogram with one occupied bin has no such ``t``: the result is that
    bin's value (0 for an empty histogram), so that nothing is tissue.  That case arises for synthetic inputs only -- a scanned
    slide is never one colour."""
    h = hist.detach().cpu().numpy() if torch.is_tensor(hist) else np.asarray(hist)
    if h.dtype.kind not in "iu" or h.ndim not in (1, 2) or h.shape[-1] != 256:
        raise ValueError(f"otsu: expected integer counts shaped [256] or [N, 256], got {h.dtype} {h.shape}")
    if h.size and int(h.min()) < 0:
        raise ValueError("otsu: negative counts")
    if h.ndim == 1:
        return _otsu_one([int(c) for c in h])
    return [_otsu_one([int(c) for c in row]) for row in h]


def _mask(dev_images, code, thr):
    """device images [N, H, W, 3], thr a list of N ints or None (Otsu: one small copy to the host) -> (uint8 [N, H, W], thr)"""
    if thr is None:
        thr = otsu(K.tissue_histogram(dev_images, code))
    return K.tissue_mask(dev_images, torch.tensor(thr, dtype=torch.int32).to(dev_images.device), code), thr


def mask(images_u8, threshold=None, channel="chroma"):
    """``feature > threshold`` as uint8 0 / 1 -> ``[N, H, W]`` on the device (``[H, W]`` for one image).  ``threshold=None``: Otsu's,
    per image -- one histogram launch, one 2 KB copy per image to the host, one mask launch; else an integer in [-1, 255] or one
    per image."""
    code = _channel(channel)
    t, one = _rgb(images_u8, "mask")
    thr = _thresholds(threshold, int(t.shape[0]), one)
    m, _ = _mask(t.to(_device(t)).contiguous(), code, thr)
    return m[0] if one else m


def coverage(mask, tile_img, tile_rc, size):
    """The non-zero pixels of ``mask`` (uint8 or bool, ``[H, W]`` or ``[N, H, W]``) under every window -> int32 ``[T]`` on the
    device.  Window t is ``[r, r + ph) x [c, c + pw)`` of image ``tile_img[t]`` with ``(r, c) = tile_rc[t]`` -- the convention of
    ``tiles.gather_tiles``; ``size``: an integer or ``(ph, pw)``.  Host-side tables are checked: a window that leaves its image is a
    ``ValueError``.  Tables that are already device tensors are not read back; the kernel clamps such a window to the image."""
    ph, pw = _pair(size, "size")
    m = _tensor(mask)
    if not torch.is_tensor(m) or m.dtype not in (torch.uint8, torch.bool):
        raise TypeError("coverage: expected a uint8 or boolean mask (numpy or torch)")
    if m.dim() not in (2, 3) or m.numel() == 0:
        raise ValueError(f"coverage: expected a non-empty [H, W] or [N, H, W] mask, got shape {tuple(m.shape)}")
    if m.dim() == 2:
        m = m.unsqueeze(0)
    N, H, W = (int(v) for v in m.shape)
    if N > MAX_IMAGES or H * W >= 1 << 31:
        raise ValueError(f"coverage: a call takes up to {MAX_IMAGES} masks of fewer than 2^31 pixels, got {(N, H, W)}")
    ti, rc = _tensor(np.asarray(tile_img) if isinstance(tile_img, (list, tuple)) else tile_img), \
        _tensor(np.asarray(tile_rc) if isinstance(tile_rc, (list, tuple)) else tile_rc)
    for x, name in ((ti, "tile_img"), (rc, "tile_rc")):
        if not torch.is_tensor(x) or x.dtype not in (torch.int32, torch.int64):
            raise TypeError(f"coverage: {name} must hold integers (numpy or torch)")
    ti, rc = ti.reshape(-1), rc.reshape(-1, 2) if rc.numel() else rc.reshape(0, 2)
    if rc.shape[0] != ti.numel():
        raise ValueError(f"coverage: {ti.numel()} image indices but {rc.shape[0]} corners")
    if not ti.is_cuda and ti.numel() and (int(ti.min()) < 0 or int(ti.max()) >= N):
        raise ValueError(f"coverage: tile_img must index the {N} masks")
    if not rc.is_cuda and rc.numel() and (int(rc.min()) < 0 or int(rc[:, 0].max()) + ph > H or int(rc[:, 1].max()) + pw > W):
        raise ValueError(f"coverage: a {ph}x{pw} window leaves the {H}x{W} image")
    dev = _device(m, ti, rc)
    m = m.to(dev).contiguous()
    return K.tissue_coverage(m.view(torch.uint8) if m.dtype == torch.bool else m, ti.to(device=dev, dtype=torch.int32).contiguous(),
                             rc.to(device=dev, dtype=torch.int32).contiguous(), ph, pw)


@dataclass(frozen=True)
class TissueOptions:
    """How ``select_patches`` decides, checked once on the host.  ``channel`` and ``threshold`` (None: Otsu's) as in ``mask``.  A patch
    is kept when its window holds at least ``min_pixels`` tissue pixels; ``min_pixels=None`` means ``ceil(min_fraction * ph * pw)``,
    computed on the host.  ``opening_radius``, ``min_object_size`` and ``hole_area_threshold`` clean the tissue mask before the
    windows are counted, in that order: ``morph.binary_opening`` by the disk, then ``regions.remove_small_regions``; 0 reaches
    none of it."""
    channel: str = "chroma"
    threshold: object = None
    min_fraction: float = 0.01
    min_pixels: object = None
    min_object_size: int = 0
    hole_area_threshold: int = 0
    opening_radius: float = 0

    def __post_init__(self):
        from .regions import _check_size
        from .score import radius_squared
        _channel(self.channel)
        if self.threshold is not None:
            _check_threshold(self.threshold)
        f = self.min_fraction
        if isinstance(f, bool) or not isinstance(f, (int, float, np.integer, np.floating)) or not 0 <= f <= 1:
            raise ValueError(f"min_fraction must be a number in [0, 1], got {f!r}")
        p = self.min_pixels
        if p is not None and (isinstance(p, bool) or not isinstance(p, (int, np.integer)) or not 0 <= p < 1 << 31):
            raise ValueError(f"min_pixels must be None or a non-negative integer below 2^31, got {p!r}")
        _check_size(self.min_object_size, "min_object_size")
        _check_size(self.hole_area_threshold, "hole_area_threshold")
        try:
            radius_squared(self.opening_radius)
        except (TypeError, ValueError) as e:
            raise type(e)(f"opening_radius: {e}") from None

    def pixels(self, ph, pw):
        """the number of tissue pixels a ph x pw patch needs"""
        if self.min_pixels is not None:
            return int(self.min_pixels)
        return int(math.ceil(float(self.min_fraction) * (ph * pw)))


@dataclass
class TissueResult:
    """``select_patches`` of one slide: ``threshold`` the integer used; ``mask`` the cleaned tissue mask, device uint8 [H, W];
    ``corners`` int32 [T, 2], every (row, col) of ``tiles.sample_patches``; ``coverage`` device int32 [T], the tissue pixels under
    each; ``selected`` device int32 [n], the indices of the kept patches in rising order; ``n_selected`` = n; ``min_pixels`` the
    count a patch needed."""
    threshold: int
    mask: torch.Tensor
    corners: np.ndarray
    coverage: torch.Tensor
    selected: torch.Tensor
    n_selected: int
    min_pixels: int = 0

    @property
    def selected_corners(self):
        """int32 [n, 2] on the host: the corners of the kept patches, in the order of ``sample_patches``"""
        return self.corners[self.selected.cpu().numpy().astype(np.int64)]


def _check_options(options, what):
    if options is None or options is True:
        return TissueOptions()
    if not isinstance(options, TissueOptions):
        raise TypeError(f"{what}: expected a TissueOptions, True or None, got {type(options).__name__}")
    return options


def _select(dev_image, corners, tile_img, tile_rc, ph, pw, options, roi=None):
    """the device half of ``select_patches``: dev_image uint8 [1, H, W, 3]; corners int32 [T, 2] on the host, tile_img / tile_rc the
    same table on the device; ``roi``: None, or a device uint8 [H, W] mask of 0 / 1 that the cleaned tissue mask is ANDed with
    before the windows are counted (``detect_slide(roi=...)``)"""
    m, thr = _mask(dev_image, CHANNELS[options.channel], None if options.threshold is None else [int(options.threshold)])
    if options.opening_radius or options.min_object_size or options.hole_area_threshold:
        from . import morph as M
        from . import regions as Rg
        fg = m.view(torch.bool)
        if options.opening_radius:
            fg = M.binary_opening(fg, options.opening_radius, border_value=0)
        m = Rg.remove_small_regions(fg, options.min_object_size, options.hole_area_threshold, out=fg).view(torch.uint8)
    if roi is not None:
        m = m & roi[None]
    need = options.pixels(ph, pw)
    cover = K.tissue_coverage(m, tile_img, tile_rc, ph, pw)
    selected, n_selected = K.tissue_select(cover, need)
    n = int(n_selected.item())                                             # the second small synchronisation
    return TissueResult(int(thr[0]), m[0], corners, cover, selected[:n], n, need)


def select_patches(image_u8, patch_size=299, interval=None, options=None, device=None):
    """The patches of one slide or ROI that hold tissue -> ``TissueResult``.  image_u8: uint8 [H, W, 3], numpy or torch, moved to the
    device once; ``patch_size`` and ``interval`` as in ``tiles.sample_patches``, whose grid and order this keeps; ``options``: a
    ``TissueOptions`` (None: the defaults).  Four launches and two small synchronisations: the histogram (not with a given
    threshold) and the number of kept patches."""
    options = _check_options(options, "select_patches")
    ph, pw = _pair(patch_size, "patch_size")
    t, one = _rgb(image_u8, "select_patches")
    if not one:
        raise ValueError(f"select_patches: expected one image shaped [H, W, 3], got shape {tuple(t.shape)}")
    H, W = int(t.shape[1]), int(t.shape[2])
    corners = np.asarray(sample_patches((H, W), (ph, pw), interval), dtype=np.int32).reshape(-1, 2)
    if device is None:
        device = _device(t)
    rc = torch.from_numpy(corners).to(device)
    ti = torch.zeros((len(corners),), dtype=torch.int32, device=device)
    return _select(t.to(device).contiguous(), corners, ti, rc, ph, pw, options)
