"""Cell localisation from segmentation probability maps: the reference's ``meanshift_cluster`` (test_seg.py:319-365) and the
stitching of ``cell_detect`` (test_seg.py:182-316), on the HIP path (csrc/detect.hip).

Steps, each integer arithmetic or one correctly rounded fp64 operation, so the result is bit-exact and independent of launch order:

* quantise   ``u8 = trunc(255 p)`` in fp32 (``np.uint8(255 * mask)`` of a float32 map, test_seg.py:225).
* blur       ``method="gaussianblur"``: a separable integer Gaussian with BORDER_REFLECT_101.  Taps are ``rint(g_i 2^14)`` of the
             fp64-normalised Gaussian, the centre tap absorbing the remainder so they sum to 2^14; int32 row pass, int64 column
             pass, ``(s + 2^27) >> 28``.  This is within 1 LSB of a float64 Gaussian.  Agreement with cv2's own fixed-point 8-bit
             path is NOT pinned (cv2 is not a dependency of this project, and its tables for ``ksize <= 7`` with ``sigma <= 0``
             are not restated: those forms raise ``ValueError``).
* seeds      one ``window_size`` window per ``tiles.get_tiles`` corner whose blurred centre is above ``thr * 255`` (fp64).
* mean shift ``cv2.meanShift`` with ``TermCriteria(EPS, 0, 1e-5)``: cv2 rounds eps^2 to 0 and takes 100 iterations, so the loop
             never stops on convergence; stopping at a fixed point gives the same window.  ``max_iter`` defaults to 100.
* clusters   ``DBSCAN(eps, min_samples=1)``: connected components of ``dr^2 + dc^2 <= eps^2`` numbered by lowest point index;
             centroid ``rint(mean)``; weight = blurred value under the centroid.
* order      weight descending, then label descending (``np.argsort(w, kind="stable")[::-1]``).  The reference uses the default
             (unstable) argsort, so among equal weights its order is unspecified; here it is fixed.

``method="distancetransform"`` (test_seg.py:325-329) replaces the blur step of ``detect_points`` / ``inference.detect_cells``:

* threshold  foreground = ``u8 > thr_for_dt`` (default 10), background everything else.
* distance   ``D2`` = exact squared Euclidean distance to the nearest background pixel of the map (int32; 0 on background; ``-1``
             everywhere in a map without any background).  Maps with ``H^2 + W^2 >= 2^31`` raise ``ValueError``.  Pinned against
             ``scipy.ndimage.distance_transform_edt`` (tests/golden/edt_vectors.npz).
* normalise  ``M = max D2`` of the map itself (never of the batch); all zeros where ``M <= 0``; otherwise ``255 sqrt(D2 / M)`` rounded
             half to even, decided by the integer comparison ``4 255^2 D2 <> (2k + 1)^2 M``.  cv2 computes the distance in float32
             and normalises in floating point; agreement with cv2's own rounding is NOT pinned (cv2 is not a dependency).

Whole slides: ``stitch_patches`` builds the whole-image mask from patches that are all resident; ``stitch_logits`` builds the same
bytes batch by batch, straight from the segment logits (softmax channel, quantise and the overlap rule in one launch per batch, the
owner of a pixel decided from the batch's corners, no per-pixel state).  ``inference.detect_slide`` is the loop around it.
``StitchBlend`` / ``stitch_blend`` (not in the reference) average the overlaps instead: integer weighted sums of every covering
patch, flipped views included, in two whole-image accumulators (``detect_slide(blend=, tta=)``).

``meanshift_cluster`` itself still refuses ``"distancetransform"``; ``detect_points(mask, cell_counts=c,
method="distancetransform").per_image()[0]`` returns the pair it would.
"""
import math
from dataclasses import dataclass, field

import numpy as np
import torch

from . import kernels as K
from ._args import _device, _images, _tensor
from ._points import PointSet, ragged

_ONE = 1 << 14
_MAX_KSIZE = 31


def gaussian_taps(ksize, sigma):
    """int32 [ksize] taps summing to exactly 2^14 (host)."""
    k = int(ksize)
    if k != ksize or k < 1 or k % 2 == 0:
        raise ValueError(f"ksize must be a positive odd integer, got {ksize!r}")
    if k > _MAX_KSIZE:
        raise ValueError(f"ksize {k} > {_MAX_KSIZE} is not supported")
    sigma = float(sigma)
    if sigma <= 0:
        if k <= 7:
            raise ValueError("sigma <= 0 with ksize <= 7 selects cv2's fixed kernel tables, which are not supported")
        sigma = 0.3 * ((k - 1) * 0.5 - 1) + 0.8
    x = np.arange(k, dtype=np.float64) - (k - 1) / 2.0
    g = np.exp(-(x * x) / (2.0 * sigma * sigma))
    g = g / g.sum()
    t = np.rint(g * _ONE).astype(np.int64)
    t[k // 2] += _ONE - int(t.sum())
    return t.astype(np.int32)


def _blur_taps(ksize, sigmaX, sigmaY=0.0):
    try:
        kx, ky = (int(v) for v in ksize)
    except (TypeError, ValueError):
        raise ValueError(f"ksize must be a pair (kx, ky), got {ksize!r}") from None
    if kx == 0 or ky == 0:
        raise ValueError("ksize (0, 0) (size derived from sigma) is not supported: pass odd kernel sizes")
    sy = float(sigmaY) if sigmaY and float(sigmaY) > 0 else float(sigmaX)
    return gaussian_taps(kx, sigmaX), gaussian_taps(ky, sy)


def _ndim(x):
    return x.dim() if torch.is_tensor(x) else np.ndim(x)


def _as_u8_maps(masks, what):
    """uint8 numpy / torch [H,W] or [N,H,W] -> (device tensor [N,H,W], was_2d)."""
    t = _images(masks, what, torch.uint8, "a uint8 mask (quantise probabilities first), got {}", lift=True, to_device=True)
    return t.contiguous(), masks.ndim == 2


def quantize(probs):
    """fp32 probabilities (numpy or torch, any shape) -> uint8 ``trunc(255 p)`` on the device, same shape."""
    t = _tensor(probs)
    if t.dtype != torch.float32:
        raise TypeError(f"quantize expects float32 probabilities, got {t.dtype}")
    if not t.is_cuda:
        t = t.to(_device())
    return K.detect_quantize(t)


def gaussian_blur(mask_u8, ksize, sigmaX, sigmaY=0):
    """``cv2.GaussianBlur(mask, ksize, sigmaX, sigmaY)`` restated in integer arithmetic (module docstring).  mask_u8: uint8
    [H, W] or [N, H, W] (numpy or torch); returns a uint8 device tensor of the same shape."""
    tx, ty = _blur_taps(ksize, sigmaX, sigmaY)
    t, two_d = _as_u8_maps(mask_u8, "gaussian_blur")
    out = K.detect_blur(t, tx, ty)
    return out[0] if two_d else out


_METHODS = ("gaussianblur", "distancetransform")


def _check_method(method):
    if method not in _METHODS:
        raise ValueError("Smoothing method not found. ")


def _dt_threshold(thr_for_dt):
    """``u8 > thr`` for a real threshold is ``u8 > floor(thr)``; clamped to what an int32 holds (-1: all foreground)."""
    t = float(thr_for_dt)
    if not math.isfinite(t):
        raise ValueError(f"thr_for_dt must be finite, got {thr_for_dt!r}")
    return int(min(max(math.floor(t), -1), 255))


def _check_dt_shape(shape):
    H, W = (int(v) for v in shape[-2:])
    if H * H + W * W >= 1 << 31:
        raise ValueError(f"distance transform: H^2 + W^2 must stay below 2^31, got a {H}x{W} map")


def _dt_maps(mask_u8, what):
    if hasattr(mask_u8, "shape") and len(mask_u8.shape) >= 2:
        _check_dt_shape(mask_u8.shape)                                    # before the map is copied anywhere
    return _as_u8_maps(mask_u8, what)


def distance_transform_sq(mask_u8, thr_for_dt=10):
    """Exact squared Euclidean distance of every pixel with ``mask > thr_for_dt`` to the nearest pixel without (module docstring);
    ``-1`` everywhere in a map that has no such pixel.  mask_u8: uint8 [H, W] or [N, H, W] (numpy or torch); returns an int32
    device tensor of the same shape."""
    thr = _dt_threshold(thr_for_dt)
    t, two_d = _dt_maps(mask_u8, "distance_transform_sq")
    out = K.detect_edt_sq(t, thr)
    return out[0] if two_d else out


def distance_smooth(mask_u8, thr_for_dt=10):
    """The ``"distancetransform"`` smoothing (test_seg.py:325-329): threshold, exact distance transform, min-max normalisation of
    every map to 0..255, rounded half to even in integer arithmetic (module docstring).  Returns a uint8 device tensor of the
    same shape as mask_u8."""
    thr = _dt_threshold(thr_for_dt)
    t, two_d = _dt_maps(mask_u8, "distance_smooth")
    out = K.detect_edt_smooth(t, thr)
    return out[0] if two_d else out


def stitch_patches(patches, images_grid, image_hw):
    """Write patches uint8 [M, ph, pw] at upper-left corners images_grid [M, 2] (row, col) into a zeroed uint8 [H, W] mask; where
    patches overlap the one with the highest index wins, as the reference's write order (test_seg.py:255-257)."""
    p, _ = _as_u8_maps(patches, "stitch_patches")
    if _ndim(patches) != 3:
        raise ValueError("stitch_patches expects patches shaped [M, ph, pw]")
    M, ph, pw = p.shape
    H, W = (int(v) for v in image_hw)
    grid = np.asarray(images_grid.cpu() if torch.is_tensor(images_grid) else images_grid, dtype=np.int64).reshape(-1, 2)
    if len(grid) != M:
        raise ValueError(f"{M} patches but {len(grid)} corners")
    if M and (grid.min() < 0 or (grid[:, 0] + ph).max() > H or (grid[:, 1] + pw).max() > W):
        raise ValueError("a patch does not lie inside the image")
    corners = torch.from_numpy(grid.astype(np.int32)).to(p.device)
    return K.stitch_patches(p, corners, H, W)


def _check_stitch_logits(mask, logits, corners, ch):
    """Argument checks of stitch_logits, all on the host -> int64 numpy corners [B, 2].  The device check comes last, so that every
    other error is the same with host tensors."""
    if not torch.is_tensor(logits) or not torch.is_tensor(mask):
        raise TypeError("stitch_logits: expected torch tensors (the mask is written in place on the device)")
    if logits.dtype != torch.float32:
        raise TypeError(f"stitch_logits: expected float32 logits, got {logits.dtype}")
    if logits.dim() != 4:
        raise ValueError(f"stitch_logits expects logits shaped [B, C, ph, pw], got shape {tuple(logits.shape)}")
    if mask.dtype != torch.uint8:
        raise TypeError(f"stitch_logits: expected a uint8 mask, got {mask.dtype}")
    if mask.dim() != 2:
        raise ValueError(f"stitch_logits expects a mask shaped [H, W], got shape {tuple(mask.shape)}")
    B, C, ph, pw = logits.shape
    H, W = mask.shape
    if C < 2:
        raise ValueError(f"stitch_logits: the softmax needs at least two channels, got {C}")
    if int(ch) != ch or not 0 <= ch < C:
        raise ValueError(f"stitch_logits: channel {ch!r} is not one of the {C} channels")
    grid = np.asarray(corners.cpu() if torch.is_tensor(corners) else corners, dtype=np.int64).reshape(-1, 2)
    if len(grid) != B:
        raise ValueError(f"{B} patches but {len(grid)} corners")
    if B and (grid.min() < 0 or (grid[:, 0] + ph).max() > H or (grid[:, 1] + pw).max() > W):
        raise ValueError("a patch does not lie inside the image")
    if not mask.is_cuda or not mask.is_contiguous():
        raise ValueError("stitch_logits writes the mask in place: it must be a contiguous device tensor")
    if logits.device != mask.device:
        raise ValueError(f"stitch_logits: logits on {logits.device}, mask on {mask.device}")
    return grid


def stitch_logits(mask, logits, corners, ch=1):
    """Write ``quantize(softmax_channel_fwd(logits, ch))`` of a batch of segment logits fp32 [B, C, ph, pw] into the whole-image mask
    uint8 [H, W] (device) at upper-left corners [B, 2] (row, col), in place, in one launch -- ``cell_detect``'s
    ``whole_image_mask[...] = mask`` per patch (test_seg.py:255-257), a batch at a time.

    The mask is not cleared: pixels that no patch of the batch covers keep their value.  Inside the call a pixel covered by several
    patches is written once, by the one with the highest index (decided from the corners alone: no owner map, no atomics, the same
    bytes whatever order the workgroups run in); two patches may share a corner.  Across calls the stream orders the writes, so ALL
    CALLS FOR ONE MASK MUST BE ISSUED ON THE SAME STREAM.  Batch after batch in index order on a zeroed mask gives exactly
    ``stitch_patches(quantize(softmax_channel_fwd(all_logits, ch)), all_corners, (H, W))``, bit for bit, for any split into batches,
    with the mask and one batch resident instead of every patch and a 4 H W byte owner map.  Every workgroup walks the corners
    that follow its patch, so keep a batch at tens of patches (DESIGN.md has the figures).  Returns the mask."""
    grid = _check_stitch_logits(mask, logits, corners, ch)
    return K.stitch_logits(mask, logits.contiguous(), torch.from_numpy(grid.astype(np.int32)).to(mask.device), int(ch))


_MAX_TAP = 255
_WINDOWS = ("linear", "uniform")


def _check_ramp(ramp):
    if ramp is None:
        return _MAX_TAP
    if isinstance(ramp, bool) or not isinstance(ramp, (int, np.integer)) or not 1 <= ramp <= _MAX_TAP:
        raise ValueError(f"blend: ramp must be an integer in 1..{_MAX_TAP} (None: {_MAX_TAP}), got {ramp!r}")
    return int(ramp)


def blend_taps(n, window="linear", ramp=None):
    """The weights of one patch axis of ``n`` pixels for ``StitchBlend`` -> int32 numpy [n], every tap in 1..255.  ``"linear"``:
    ``min(i + 1, n - i, ramp)``, a ramp from 1 at either edge to ``ramp`` (None: 255) and flat between -- a patch's edge, where a
    zero-padded CNN is least reliable, counts least.  ``"uniform"``: all ones, the plain mean of the covering patches."""
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
        raise ValueError(f"blend_taps: n must be a positive integer, got {n!r}")
    if not isinstance(window, str) or window not in _WINDOWS:
        raise ValueError(f"blend_taps: window must be one of {_WINDOWS}, got {window!r}")
    ramp = _check_ramp(ramp)
    if window == "uniform":
        return np.ones((int(n),), np.int32)
    i = np.arange(int(n), dtype=np.int64)
    return np.minimum(np.minimum(i + 1, int(n) - i), ramp).astype(np.int32)


def _blend_windows(window, ramp, ph, pw):
    """``window`` / ``ramp`` of StitchBlend -> the (row taps [ph], column taps [pw]) int32 numpy pair"""
    if isinstance(window, str):
        return blend_taps(ph, window, ramp), blend_taps(pw, window, ramp)
    if ramp is not None:
        raise ValueError("blend: ramp goes with a named window, not with explicit taps")
    try:
        tr, tc = (np.asarray(t) for t in window)
    except (TypeError, ValueError):
        raise ValueError(f"blend: window must be one of {_WINDOWS} or a pair (row taps, column taps), got {window!r}") from None
    for t, n, axis in ((tr, ph, "row"), (tc, pw, "column")):
        if t.dtype.kind not in "iu" or t.shape != (n,):
            raise ValueError(f"blend: expected {n} integer {axis} taps, got {t.dtype} of shape {tuple(t.shape)}")
        if t.min() < 1 or t.max() > _MAX_TAP:
            raise ValueError(f"blend: every {axis} tap lies in 1..{_MAX_TAP}")
    return tr.astype(np.int32), tc.astype(np.int32)


class StitchBlend:
    """A whole-image mask in which overlapping patches are blended instead of overwritten, and to which flipped views of a patch
    (test-time augmentation) contribute like any other patch.  Integer arithmetic throughout (csrc/detect.hip):

    * level   ``q = uint32(256 * clamp(255 p, 0, 255))`` of the fp32 probability ``p = softmax_channel_fwd(logits, ch)``: 0..65280,
              ``q >> 8`` is the byte ``quantize`` makes of ``p``, a NaN gives 0.
    * weight  ``w = tr[i] * tc[j]`` for the pixel at row i, column j of its patch ON THE SLIDE; ``tr`` / ``tc`` are ``blend_taps`` of
              the patch sides (``window`` "linear" or "uniform", ``ramp``) or the explicit pair ``window=(row taps, column taps)``
              of integers in 1..255.
    * sums    per slide pixel ``num += w q`` (int64 [H, W]) and ``den += w`` (int32 [H, W]): 12 bytes per pixel, owned by this
              object and zeroed at the start.
    * finish  ``mask = num // (256 den)``, 0 where ``den == 0``.  A pixel that one patch covers holds exactly the byte
              ``stitch_logits`` writes; a patch added twice changes nothing.

    Being integer sums, the accumulators do not depend on how the patches are split into ``add`` calls or on their order.  ``add``
    is one launch without atomics; as with ``stitch_logits``, ALL CALLS FOR ONE ACCUMULATOR MUST BE ISSUED ON THE SAME STREAM."""

    def __init__(self, image_hw, patch_hw, window="linear", ramp=None, device=None):
        try:
            H, W = (int(v) for v in image_hw)
            ph, pw = (int(v) for v in patch_hw)
        except (TypeError, ValueError):
            raise ValueError(f"StitchBlend: image_hw and patch_hw are pairs of integers, got {image_hw!r} and {patch_hw!r}") from None
        if not (0 < ph <= H < 1 << 29 and 0 < pw <= W < 1 << 29):
            raise ValueError(f"StitchBlend: a {ph}x{pw} patch does not fit a {H}x{W} image (sides below 2^29)")
        tr, tc = _blend_windows(window, ramp, ph, pw)
        self.image_hw, self.patch_hw, self.taps = (H, W), (ph, pw), (tr, tc)
        self._wmax = int(tr.max()) * int(tc.max())
        self.n_added = 0                                                   # patches added since the last reset: the den bound
        device = _device() if device is None else torch.device(device)
        self.num = torch.zeros((H, W), dtype=torch.int64, device=device)
        self.den = torch.zeros((H, W), dtype=torch.int32, device=device)
        self._tr, self._tc = torch.from_numpy(tr).to(device), torch.from_numpy(tc).to(device)

    def _check_add(self, logits, corners, flips, ch):
        """Argument checks of add, all on the host -> (corners, flips) as device operands.  Corners and flips that are host data are
        checked by value and uploaded; device tensors are taken as they are, without a copy back (the kernel clips a patch that
        leaves the slide and reads the two low bits of a flip code).  The device check comes last, so that every other error is
        the same with host tensors."""
        if not torch.is_tensor(logits):
            raise TypeError("stitch_blend: expected the logits as a torch tensor")
        if logits.dtype != torch.float32:
            raise TypeError(f"stitch_blend: expected float32 logits, got {logits.dtype}")
        if logits.dim() != 4:
            raise ValueError(f"stitch_blend expects logits shaped [B, C, ph, pw], got shape {tuple(logits.shape)}")
        B, C, ph, pw = logits.shape
        (H, W), dev = self.image_hw, self.num.device
        if (ph, pw) != self.patch_hw:
            raise ValueError(f"stitch_blend: the taps are those of {self.patch_hw} patches, got {(ph, pw)}")
        if C < 2:
            raise ValueError(f"stitch_blend: the softmax needs at least two channels, got {C}")
        if int(ch) != ch or not 0 <= ch < C:
            raise ValueError(f"stitch_blend: channel {ch!r} is not one of the {C} channels")
        if torch.is_tensor(corners) and corners.is_cuda:
            if corners.dtype != torch.int32 or tuple(corners.shape) != (B, 2):
                raise ValueError(f"stitch_blend: device corners are int32 [{B}, 2], got {corners.dtype} {tuple(corners.shape)}")
            rc = corners.contiguous()
        else:
            grid = np.asarray(corners, dtype=np.int64).reshape(-1, 2)
            if len(grid) != B:
                raise ValueError(f"{B} patches but {len(grid)} corners")
            if B and (grid.min() < 0 or (grid[:, 0] + ph).max() > H or (grid[:, 1] + pw).max() > W):
                raise ValueError("a patch does not lie inside the image")
            rc = grid.astype(np.int32)
        if flips is None:
            fl = None
        elif torch.is_tensor(flips) and flips.is_cuda:
            if flips.dtype not in (torch.uint8, torch.int8) or tuple(flips.shape) != (B,):
                raise ValueError(f"stitch_blend: device flips are uint8 [{B}], got {flips.dtype} {tuple(flips.shape)}")
            fl = flips.contiguous().view(torch.uint8)
        else:
            fl = np.asarray(flips)
            if fl.dtype.kind not in "iu" or fl.shape != (B,):
                raise ValueError(f"stitch_blend: expected {B} integer flip codes, got {fl.dtype} of shape {tuple(fl.shape)}")
            if B and (fl.min() < 0 or fl.max() > 3):
                raise ValueError("stitch_blend: a flip code is 0 (none), 1 (horizontal), 2 (vertical) or 3 (both)")
            fl = fl.astype(np.uint8)
        if (self.n_added + B) * self._wmax >= 1 << 31:
            raise OverflowError(f"stitch_blend: {self.n_added} + {B} patches of weight up to {self._wmax} could overflow the int32 "
                                "weight sum; finish and reset, or use smaller taps")
        if not dev.type == "cuda":
            raise ValueError("stitch_blend adds in place on the device: the accumulators must be device tensors")
        if logits.device != dev:
            raise ValueError(f"stitch_blend: logits on {logits.device}, accumulators on {dev}")
        for t in (rc, fl):
            if torch.is_tensor(t) and t.device != dev:
                raise ValueError(f"stitch_blend: corners or flips on {t.device}, accumulators on {dev}")
        if isinstance(rc, np.ndarray):
            rc = torch.from_numpy(rc).to(dev)
        if isinstance(fl, np.ndarray):
            fl = torch.from_numpy(fl).to(dev)
        return rc, fl

    def add(self, logits, corners, flips=None, ch=1):
        """Add a batch of segment logits fp32 [B, C, ph, pw] at upper-left corners [B, 2] (row, col) in one launch -> self.
        ``flips``: B of ``augment``'s codes (0 none, 1 horizontal, 2 vertical, 3 both) saying that ``logits[b]`` are those of the
        flipped tile; logit pixel (i, j) then belongs to slide pixel ``(r + (ph-1-i if code & 2 else i), c + (pw-1-j if code & 1 else
        j))`` and is weighted by the taps of that position.  Corners, and (corner, flip) pairs, may repeat within a batch.  With
        corners and flips already int32 / uint8 device tensors nothing here synchronises with the host.  Raises OverflowError,
        before anything is enqueued, once ``patches added * max(tr) * max(tc)`` would reach 2^31 (the int32 weight sum)."""
        rc, fl = self._check_add(logits, corners, flips, ch)
        K.stitch_blend_add(self.num, self.den, logits.contiguous(), rc, self._tr, self._tc, fl, int(ch))
        self.n_added += int(logits.shape[0])
        return self

    def finish(self, out=None):
        """The blended uint8 [H, W] device mask of everything added so far (into ``out`` when given).  The accumulators are only
        read: ``finish`` may be called again, and more ``add`` calls may follow."""
        if out is not None and (not torch.is_tensor(out) or out.dtype != torch.uint8 or tuple(out.shape) != self.image_hw
                                or not out.is_contiguous() or out.device != self.num.device):
            raise ValueError(f"stitch_blend: out must be a contiguous uint8 {list(self.image_hw)} tensor on {self.num.device}")
        return K.stitch_blend_finish(self.num, self.den, out)

    def reset(self):
        """Zero the accumulators -> self."""
        self.num.zero_()
        self.den.zero_()
        self.n_added = 0
        return self


def stitch_blend(logits, corners, image_hw, flips=None, ch=1, window="linear", ramp=None):
    """``StitchBlend`` in one shot: the blended uint8 [H, W] device mask of one batch of logits fp32 [B, C, ph, pw] at ``corners``."""
    if not torch.is_tensor(logits) or logits.dim() != 4:
        raise ValueError("stitch_blend expects logits shaped [B, C, ph, pw] as a torch tensor")
    sb = StitchBlend(image_hw, logits.shape[-2:], window, ramp, logits.device)
    return sb.add(logits, corners, flips, ch).finish()


@dataclass
class DetectResult:
    """Cells of N maps: ``points[offsets[n]:offsets[n+1]]`` (int64 (row, col)) are map n's cluster centroids ordered by ``weights``
    (smoothed value under the centroid) descending, then label descending; ``n_kept[n]`` = seed windows kept."""
    points: np.ndarray
    weights: np.ndarray
    offsets: np.ndarray
    n_kept: np.ndarray
    cell_counts: object = None
    device_points: object = None      # the clustering kernel's own points / offsets, still on the device (filled by _detect):
    device_offsets: object = None     # score() reads these, so the detections are not uploaded again

    def per_image(self):
        """[(points[:count], points[count:])] per map, as ``meanshift_cluster`` returns; ``(points, [])`` without a count."""
        out = []
        for n in range(len(self.offsets) - 1):
            pts = self.points[self.offsets[n]:self.offsets[n + 1]]
            c = self.cell_counts
            if c is not None and not np.isscalar(c):
                c = c[n]
            out.append((pts, []) if c is None else (pts[:int(c)], pts[int(c):]))
        return out

    def score(self, points, offsets=None, gt_xy=False, radius=16, return_match=False):
        """Precision, recall and F1 of every map's kept detections -- ``per_image()[n][0]``, i.e. ``cell_counts`` applied as the
        limit -- against annotated points (score.score_points, test_seg.py:120-141) -> score.ScoreResult.  points: a sequence of one
        ``[k, 2]`` array per map, an ``[N, k, 2]`` array, one ``[k, 2]`` array for a single map, or a concatenated ``[G, 2]`` array
        with ``offsets`` [N + 1].  ``gt_xy``: the annotations are (x, y) while the detections are (row, col)."""
        from . import score as S
        N = len(self.offsets) - 1
        radius2 = S.radius_squared(radius)
        points, offsets = self._per_map(points, offsets)
        gt = S._prepare(points, offsets, N, gt_xy)
        pts, off = self._own_points()
        hat = PointSet(pts, off, self.cell_counts, N, "detections").upload(_device(pts))
        return S._run(hat, int(self.offsets[-1]), gt, radius2, return_match)

    def render(self, images_u8, **compose):
        """The maps' images annotated on the device -> uint8 of the images' shape: ``render.compose(images_u8, **compose)`` (mask=,
        heat=, outlines=, ... as there), then every map's kept detections -- ``per_image()[n][0]`` -- as red dots of radius 4 and
        its discarded ones as blue dots on top, straight from the device points and offsets: no host round trip."""
        from . import render as Rd
        return Rd.render_detections(self, images_u8, **compose)

    def _per_map(self, points, offsets):
        """a second point set in one of the forms ``score`` lists -> (points [G, 2], offsets [N + 1] or None for a single map)"""
        N = len(self.offsets) - 1
        if offsets is None:
            if isinstance(points, (list, tuple)):
                if len(points) != N:
                    raise ValueError(f"{N} maps but {len(points)} point arrays")
                points, offsets = ragged(points)
            elif _ndim(points) == 3:
                if points.shape[0] != N or points.shape[2] != 2:
                    raise ValueError(f"expected annotations shaped [{N}, k, 2], got {tuple(points.shape)}")
                offsets = np.arange(N + 1, dtype=np.int64) * int(points.shape[1])
                points = points.reshape(-1, 2)
            elif N != 1:
                raise ValueError(f"{N} maps: pass one point array per map, or offsets")
        return points, offsets

    def _own_points(self):
        """the detections where they are: the device buffers when ``_detect`` left them, else the host arrays"""
        if self.device_points is None:
            return np.asarray(self.points, np.int64).reshape(-1, 2), np.asarray(self.offsets, np.int64)
        return self.device_points, self.device_offsets

    def _neighbours(self, fn, image_hw, arg, other, other_offsets, other_xy, _bucket):
        pts, off = self._own_points()
        kw = {}
        if other is not None:
            kw["other"], kw["other_offsets"] = self._per_map(other, other_offsets)
            kw["other_xy"] = other_xy
        res = fn(pts, image_hw, arg, offsets=off, limits=self.cell_counts, _bucket=_bucket, **kw)
        rows = int(self.offsets[-1])                                       # the device buffer holds spare rows after the last map's
        for name in ("index", "d2", "counts", "labels", "core", "size", "n_core", "sums", "bbox"):
            if hasattr(res, name):
                setattr(res, name, getattr(res, name)[:rows])
        return res

    def nearest(self, image_hw, k=1, other=None, other_offsets=None, other_xy=False, _bucket=None):
        """The k nearest neighbours of every map's kept detections -- ``per_image()[n][0]``, i.e. ``cell_counts`` applied as the limit,
        as in ``score`` -- among themselves, or among a second point set ``other`` given in one of the forms ``score`` takes its
        annotations in (``other_xy`` as ``gt_xy`` there) -> spatial.NeighborTable, one row per row of ``points`` (spatial.nearest has
        the rules).  ``image_hw``: the (H, W) of the maps.  The device-resident points are read where they are."""
        from . import spatial as Sp
        return self._neighbours(Sp.nearest, image_hw, k, other, other_offsets, other_xy, _bucket)

    def count_within(self, image_hw, radii, other=None, other_offsets=None, other_xy=False, _bucket=None):
        """The number of kept detections (or of points of ``other``) within each of ``radii`` of every kept detection, and the
        per-map sums -> spatial.WithinCounts (spatial.count_within has the rules); the arguments are those of ``nearest``."""
        from . import spatial as Sp
        return self._neighbours(Sp.count_within, image_hw, radii, other, other_offsets, other_xy, _bucket)

    def cluster(self, image_hw, eps, min_samples=5, _bucket=None):
        """The DBSCAN clusters of every map's kept detections -- ``per_image()[n][0]``, as in ``nearest`` -- -> spatial.ClusterTable,
        one row per row of ``points`` (spatial.cluster has the rules); cluster c of map n is row ``offsets[n] + c`` of its tables.
        ``image_hw``: the (H, W) of the maps.  The device-resident points are read where they are."""
        from . import spatial as Sp

        def fn(pts, hw, eps, **kw):
            return Sp.cluster(pts, hw, eps, min_samples, **kw)
        return self._neighbours(fn, image_hw, eps, None, None, False, _bucket)

    def split(self, masks, connectivity=1, geodesic=False):
        """Split the cells of ``masks`` (bool [N, H, W], or [H, W] for one map: the segmentation the detections belong to) at every
        map's kept detections -- ``per_image()[n][0]``, i.e. ``cell_counts`` applied as the limit, as in ``score`` -- ->
        regions.SplitResult: label k + 1 of map n is its detection k (regions.split has the rules).  The device-resident points
        are read where they are.  ``geodesic``: ``regions.split_geodesic`` in its exact mode instead, whose cells are connected
        (a regions.GeodesicSplitResult)."""
        from . import regions as Rg
        pts, off = self._own_points()
        return (Rg.split_geodesic if geodesic else Rg.split)(masks, pts, off, limits=self.cell_counts, connectivity=connectivity)


@dataclass(frozen=True)
class DetectOptions:
    """The parameters of ``detect_points``, checked once on the host as far as they can be without an image; ``taps`` (the blur's
    two int32 tap arrays) or ``dt_thr`` (the distance method's integer threshold) keep what the checks computed."""
    thr: float = 0.2
    window_size: int = 16
    interval: int = 10
    eps: float = 15
    ksize: tuple = (15, 15)
    sigmaX: float = 3.
    sigmaY: float = 0.
    max_iter: int = 100
    method: str = "gaussianblur"
    thr_for_dt: float = 10
    taps: object = field(default=None, init=False, repr=False, compare=False)
    dt_thr: object = field(default=None, init=False, repr=False, compare=False)

    def __post_init__(self):
        _check_method(self.method)
        if self.method == "gaussianblur":
            object.__setattr__(self, "taps", _blur_taps(self.ksize, self.sigmaX, self.sigmaY))
        else:                                                             # ksize and sigma are not consulted
            object.__setattr__(self, "dt_thr", _dt_threshold(self.thr_for_dt))
        if self.eps < 0 or not math.isfinite(self.eps):
            raise ValueError("eps must be finite and non-negative")
        if int(self.max_iter) < 0:
            raise ValueError("max_iter must be non-negative")


def _detect(src, cell_counts, opts, force_global=False):
    """src: device [N,H,W] uint8 masks or fp32 probabilities (quantised inside the smoothing kernel); opts: DetectOptions."""
    blur = opts.method == "gaussianblur"
    if not blur:
        _check_dt_shape(src.shape)
    N, H, W = src.shape
    if K.detect_grid_size(H, W, opts.interval, opts.window_size) <= 0:
        raise ValueError(f"window_size {opts.window_size} does not fit a {H}x{W} map (or interval {opts.interval} is not positive)")
    blurred = K.detect_blur(src, *opts.taps) if blur else K.detect_edt_smooth(src, opts.dt_thr)
    pts, n_pts = K.detect_meanshift(blurred, int(opts.interval), int(opts.window_size), float(opts.thr) * 255.0, int(opts.max_iter))
    out_pts, out_w, out_off = K.detect_cluster(pts, n_pts, float(opts.eps), blurred, force_global=force_global)
    head = torch.cat([out_off, n_pts.to(torch.int64)]).cpu().numpy()        # the one synchronisation of the batch
    offsets, n_kept = head[:N + 1], head[N + 1:]
    total = int(offsets[-1])
    points = out_pts[:total].cpu().numpy()
    weights = out_w[:total].cpu().numpy().astype(np.int64)
    return DetectResult(points, weights, offsets, n_kept, cell_counts, out_pts, out_off)


def detect_points(masks_u8, cell_counts=None, thr=0.2, window_size=16, interval=10, eps=15, ksize=(15, 15), sigmaX=3., sigmaY=0.,
                  max_iter=100, _force_global=False, method="gaussianblur", thr_for_dt=10):
    """Smooth, seed, mean-shift and cluster a batch of uint8 maps [N, H, W] (or one [H, W]) -> DetectResult.  cell_counts: None,
    one count for every map, or one per map (applied by ``DetectResult.per_image``).  ``method="distancetransform"`` smooths by
    ``distance_smooth(., thr_for_dt)`` instead of the blur (ksize, sigmaX and sigmaY are then not consulted).  ``_force_global``
    (tests) takes the multi-launch clustering path at any size."""
    opts = DetectOptions(thr=thr, window_size=window_size, interval=interval, eps=eps, ksize=ksize, sigmaX=sigmaX, sigmaY=sigmaY,
                         max_iter=max_iter, method=method, thr_for_dt=thr_for_dt)                    # argument errors before any upload
    t, _ = _as_u8_maps(masks_u8, "detect_points") if method == "gaussianblur" else _dt_maps(masks_u8, "detect_points")
    return _detect(t, cell_counts, opts, _force_global)


_BLUR_KEYS = {"ksize", "sigmaX", "sigmaY", "borderType"}


def meanshift_cluster(mask, method, cell_count=None, thr_for_setting_points=0.2, window_size=16, interval=10, eps=15, **method_kwargs):
    """test_seg.py:319-365 with its signature and return shape: (points[:cell_count], points[cell_count:]) with a count,
    (points, []) without; points int64 [n, 2] (row, col).  mask: uint8 2-D numpy or torch."""
    if method == "distancetransform":
        raise NotImplementedError("meanshift_cluster: method 'distancetransform' is not implemented (use 'gaussianblur')")
    if method != "gaussianblur":
        raise ValueError("Smoothing method not found. ")
    unknown = set(method_kwargs) - _BLUR_KEYS
    if unknown:
        raise TypeError(f"meanshift_cluster: unexpected GaussianBlur arguments {sorted(unknown)}")
    if "ksize" not in method_kwargs or "sigmaX" not in method_kwargs:
        raise TypeError("meanshift_cluster: gaussianblur needs ksize and sigmaX (as cv2.GaussianBlur)")
    if method_kwargs.get("borderType", 4) != 4:
        raise ValueError("meanshift_cluster: only BORDER_DEFAULT (BORDER_REFLECT_101) is supported")
    if _ndim(mask) != 2:
        raise ValueError("meanshift_cluster expects a 2-D mask")
    res = detect_points(mask, cell_counts=cell_count, thr=thr_for_setting_points, window_size=window_size, interval=interval, eps=eps,
                        ksize=method_kwargs["ksize"], sigmaX=method_kwargs["sigmaX"], sigmaY=method_kwargs.get("sigmaY", 0))
    return res.per_image()[0]
