"""Stain separation (colour deconvolution) and Macenko stain normalisation on the HIP path (csrc/stain.hip).

Images are uint8 RGB, ``[H, W, 3]`` or ``[N, H, W, 3]``, numpy or torch, on the host or the device; one image in gives one result
out, a batch a batch (``estimate``: a list).  Everything works in optical density, fixed once on the host as a table of 256
integers (``od_table``): ``od_q[v] = max(0, rint(4096 ln(Io / (v + 1))))``, the float optical density being ``od_q / 4096``.  A pixel
is *kept* for estimation when none of its three ``od_q`` is below ``rint(4096 beta)`` and, with a ``mask`` (uint8 or bool ``[H, W]``
/ ``[N, H, W]``, for example ``tissue.mask``), the mask is non-zero there.

``estimate`` is Macenko's method with histograms in place of sorts: the integer moments of the kept pixels give the covariance of
their optical density (exactly, from Python integers), ``numpy.linalg.eigh`` its two leading eigenvectors ``V``, the device the
histogram of the angle of every kept pixel in that plane, the host the two robust extreme angles and from them the two stain
vectors; a second histogram, of the concentrations ``pinv(S) od``, gives the 99th percentile of each stain.  All host arithmetic is
float64 numpy on a few KB read back three times (the moments, the angle histogram, the concentration histogram); the slide
itself never leaves the device.  ``normalize`` re-expresses every pixel with a target's vectors and intensity range, ``separate``
writes the concentrations themselves -- as uint8 they are ready to be the ``intensity=`` of the per-cell tables.

Argument errors are raised before the library is loaded or the device is touched.
"""
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import kernels as K
from ._args import _device, _tensor
from .tissue import _rgb

OD_UNIT = 4096
MAX_ANGLE_BINS, MAX_CONC_BINS = 8192, 4096

#: Ruifrok and Johnston's haematoxylin and DAB optical-density vectors, unit length, as the columns of a [3, 2] matrix.
HDAB = np.stack([np.asarray(v, np.float64) / np.linalg.norm(v) for v in ((0.650, 0.704, 0.286), (0.268, 0.570, 0.776))], axis=1)
HDAB.setflags(write=False)


def _number(v, name, lo, hi, lo_open=False, hi_open=False):
    ok = not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating)) and math.isfinite(v)
    if not ok or v < lo or v > hi or (lo_open and v == lo) or (hi_open and v == hi):
        raise ValueError(f"{name} must be a number in {'(' if lo_open else '['}{lo}, {hi}{')' if hi_open else ']'}, got {v!r}")


def _count(v, name, hi):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= v <= hi:
        raise ValueError(f"{name} must be an integer in [1, {hi}], got {v!r}")


@dataclass(frozen=True)
class StainOptions:
    """How the stains of a slide are estimated, checked once on the host.  ``Io``: the transmitted light of clear glass, in (0, 256].
    ``beta``: the optical density every channel of a pixel must reach to be kept.  ``alpha``: the robust extremes of the angle are the
    ``alpha``-th and ``(100 - alpha)``-th percentiles, in [0, 50).  ``angle_bins`` (up to 8192) and ``conc_bins`` (up to 4096) are the
    resolutions of the two histograms, the second over ``[0, conc_max)``; ``conc_max`` is also the concentration that ``separate``
    maps to 255 in its uint8 form."""
    Io: float = 240
    beta: float = 0.15
    alpha: float = 1.0
    angle_bins: int = 1024
    conc_bins: int = 2048
    conc_max: float = 8.0

    def __post_init__(self):
        _number(self.Io, "Io", 0, 256, lo_open=True)
        _number(self.beta, "beta", 0, 5)
        _number(self.alpha, "alpha", 0, 50, hi_open=True)
        _count(self.angle_bins, "angle_bins", MAX_ANGLE_BINS)
        _count(self.conc_bins, "conc_bins", MAX_CONC_BINS)
        _number(self.conc_max, "conc_max", 0, 1e30, lo_open=True)

    @property
    def beta_q(self):
        return int(np.rint(OD_UNIT * float(self.beta)))


@dataclass(frozen=True, eq=False)                  # arrays inside: two estimates are equal when they are the same object
class StainEstimate:
    """The stains of one image: ``vectors`` float64 [3, 2], unit optical-density vectors as columns, haematoxylin (the larger red
    component) first; ``max_conc`` float64 [2], the 99th percentile of each concentration; ``n_kept`` the pixels it rests on;
    ``ok`` False where there was nothing to estimate from (fewer than 2 kept pixels, or all of them on one line) and the vectors
    are ``HDAB``."""
    vectors: np.ndarray
    max_conc: np.ndarray
    n_kept: int = 0
    ok: bool = True

    def __post_init__(self):
        v, c = np.array(self.vectors, np.float64), np.array(self.max_conc, np.float64)
        if v.shape != (3, 2) or c.shape != (2,) or not np.isfinite(v).all() or not np.isfinite(c).all() or (c <= 0).any():
            raise ValueError("StainEstimate: vectors must be finite [3, 2] and max_conc finite, positive [2]")
        object.__setattr__(self, "vectors", v)
        object.__setattr__(self, "max_conc", c)


#: A convention, not a calibration: Ruifrok's vectors with unit intensity range.  It pins the colours of the output so that slides
#: normalised to it are comparable with each other; a user normally passes the ``estimate`` of a slide they like instead.
TARGET_HDAB = StainEstimate(HDAB, np.ones(2))


def od_table(Io=240):
    """The quantised optical density of every byte value -> int32 [256]: ``max(0, rint(4096 ln(Io / (v + 1))))``, float64 on the host."""
    _number(Io, "Io", 0, 256, lo_open=True)
    v = np.arange(256, dtype=np.float64)
    return np.maximum(0.0, np.rint(OD_UNIT * np.log(float(Io) / (v + 1.0)))).astype(np.int32)


def _options(options, what):
    if options is None or options is True:
        return StainOptions()
    if not isinstance(options, StainOptions):
        raise TypeError(f"{what}: expected a StainOptions or None, got {type(options).__name__}")
    return options


def _mask(mask, shape, what):
    """None | uint8 / bool [H, W] or [N, H, W] -> None | the uint8 tensor shaped ``shape`` = (N, H, W), where it lives"""
    if mask is None:
        return None
    m = _tensor(mask)
    if not torch.is_tensor(m) or m.dtype not in (torch.uint8, torch.bool):
        raise TypeError(f"{what}: mask must be uint8 or boolean (numpy or torch)")
    if m.dim() == 2:
        m = m.unsqueeze(0)
    if tuple(m.shape) != tuple(shape):
        raise ValueError(f"{what}: mask of shape {tuple(m.shape)} for images of {tuple(shape)}")
    return m.view(torch.uint8) if m.dtype == torch.bool else m


def _per_image(x, n, kind, what):
    """one ``kind`` for all images, or a list of n"""
    if isinstance(x, kind):
        return [x] * n
    if isinstance(x, (list, tuple)) and len(x) == n and all(isinstance(e, kind) for e in x):
        return list(x)
    raise TypeError(f"{what}: expected a {kind.__name__} or a list of {n}")


def _upload(mats, dev):
    return torch.from_numpy(np.ascontiguousarray(np.stack(mats), dtype=np.float32)).to(dev)


def _od(options, dev):
    return torch.from_numpy(od_table(options.Io)).to(dev)


# ---- the host half of the estimate: float64 numpy on what the kernels counted ------------------------------------------------------
def plane_of_moments(m):
    """int64 [10] of ``cs_stain_moments`` -> float64 [3, 2], the two leading eigenvectors of the covariance of the kept pixels'
    optical density (the larger eigenvalue first, each flipped so that its components sum to >= 0); None with fewer than 2 kept
    pixels or a second eigenvalue <= 0.  The numerators ``n S_ij - S_i S_j`` are exact Python integers."""
    m = [int(v) for v in m]
    n, s = m[0], m[1:4]
    if n < 2:
        return None
    q = {(0, 0): m[4], (0, 1): m[5], (0, 2): m[6], (1, 1): m[7], (1, 2): m[8], (2, 2): m[9]}
    C = np.empty((3, 3), np.float64)
    for i in range(3):
        for j in range(3):
            C[i, j] = float(n * q[(min(i, j), max(i, j))] - s[i] * s[j]) / (float(n) * float(n - 1) * OD_UNIT * OD_UNIT)
    w, E = np.linalg.eigh(C)
    if not w[1] > 0:
        return None
    V = E[:, [2, 1]].copy()
    for k in range(2):
        if V[:, k].sum() < 0:
            V[:, k] = -V[:, k]
    return V


def order_bin(hist, k):
    """the bin of a histogram that holds order statistic k (0-based) of what it counted"""
    return int(np.searchsorted(np.cumsum(np.asarray(hist, np.int64)), k, side="right"))


def extreme_ranks(n, alpha):
    return int(math.floor(alpha / 100.0 * (n - 1))), int(math.ceil((100.0 - alpha) / 100.0 * (n - 1)))


def vectors_of_angles(V, phi_lo, phi_hi):
    """the two stain vectors ``V (cos phi, sin phi)`` as the columns of [3, 2], the one with the larger red component first"""
    a, b = V @ np.asarray([math.cos(phi_lo), math.sin(phi_lo)]), V @ np.asarray([math.cos(phi_hi), math.sin(phi_hi)])
    return np.stack([a, b] if a[0] >= b[0] else [b, a], axis=1)


def vectors_of_hist(V, hist, alpha):
    bins = len(hist)
    lo, hi = extreme_ranks(int(np.sum(hist)), alpha)
    phi = [-math.pi / 2 + (order_bin(hist, k) + 0.5) * math.pi / bins for k in (lo, hi)]
    return vectors_of_angles(V, phi[0], phi[1])


def max_conc_of_hist(hist, conc_max):
    """int64 [2, Bc] -> float64 [2]: the centre of the bin that holds order statistic ceil(0.99 (n - 1)) of each concentration"""
    bins = hist.shape[-1]
    return np.asarray([(order_bin(h, int(math.ceil(0.99 * (int(h.sum()) - 1)))) + 0.5) * conc_max / bins for h in hist], np.float64)


def normalizer(source, target):
    """float64 [3, 3] ``A`` with od_out = A od: the source's concentrations, rescaled to the target's range, in the target's vectors"""
    return target.vectors @ np.diag(target.max_conc / source.max_conc) @ np.linalg.pinv(source.vectors)


def stain_matrix(stains, residual=False):
    """HDAB-like [3, 2] or a StainEstimate -> float64 [3, K]; ``residual`` adds the unit vector along the cross product of the two"""
    S = np.array(stains.vectors if isinstance(stains, StainEstimate) else stains, np.float64)
    if S.shape != (3, 2) or not np.isfinite(S).all():
        raise ValueError(f"stains: expected a StainEstimate or a finite [3, 2] matrix of optical-density vectors, got shape {S.shape}")
    if residual:
        c = np.cross(S[:, 0], S[:, 1])
        if not np.linalg.norm(c) > 0:
            raise ValueError("stains: the two vectors are parallel, there is no residual direction")
        S = np.concatenate([S, (c / np.linalg.norm(c))[:, None]], axis=1)
    return S


def _fallback(n):
    return StainEstimate(HDAB, np.ones(2), n, False)


def _estimate(x, m, opts):
    """device images [N, H, W, 3], device mask [N, H, W] or None -> a list of N StainEstimate"""
    dev, N = x.device, int(x.shape[0])
    od, beta_q = _od(opts, dev), opts.beta_q
    moments = K.stain_moments(x, od, beta_q, m).cpu().numpy()              # the first small copy to the host
    planes = [plane_of_moments(row) for row in moments]
    n_kept = [int(row[0]) for row in moments]
    live = [k for k in range(N) if planes[k] is not None]
    if not live:
        return [_fallback(n) for n in n_kept]
    zero = np.zeros((3, 2))
    V = _upload([zero if p is None else p for p in planes], dev)
    angles = K.stain_angle_hist(x, od, beta_q, V, opts.angle_bins, m).cpu().numpy()          # the second
    S = {k: vectors_of_hist(planes[k], angles[k], float(opts.alpha)) for k in live}
    P = _upload([np.linalg.pinv(S[k]) if k in S else zero.T for k in range(N)], dev)
    conc = K.stain_conc_hist(x, od, beta_q, P, opts.conc_bins, opts.conc_max, m).cpu().numpy()   # the third
    return [StainEstimate(S[k], max_conc_of_hist(conc[k], float(opts.conc_max)), n_kept[k], True) if k in S else _fallback(n_kept[k])
            for k in range(N)]


def estimate(images, mask=None, options=None):
    """The stain vectors and intensity range of every image -> ``StainEstimate`` (a list of them for a batch).  Three launches and
    three small copies to the host (80 B, 8 KB and 32 KB per image with the default options)."""
    opts = _options(options, "estimate")
    t, one = _rgb(images, "estimate")
    m = _mask(mask, t.shape[:3], "estimate")
    dev = _device(t, m)
    est = _estimate(t.to(dev).contiguous(), None if m is None else m.to(dev).contiguous(), opts)
    return est[0] if one else est


def _apply(x, sources, target, opts, out=None):
    A = _upload([normalizer(s, target) for s in sources], x.device)
    return K.stain_apply(x, _od(opts, x.device), A, float(opts.Io), out=out)


def normalize(images, source=None, target=TARGET_HDAB, mask=None, options=None, out=None):
    """Every pixel re-expressed with the target's stain vectors and intensity range -> uint8 images of the same shape on the device:
    ``clamp(rint(Io exp(-(A od))), 0, 255)`` with ``A = target.vectors diag(target.max_conc / source.max_conc) pinv(source.vectors)``.
    ``source``: a ``StainEstimate`` (or one per image); None estimates each image, over ``mask`` where given.  ``target``: a
    ``StainEstimate``, by default the convention ``TARGET_HDAB``.  ``out``: a uint8 device tensor ``[N, H, W, 3]`` to write, not the
    images themselves."""
    opts = _options(options, "normalize")
    t, one = _rgb(images, "normalize")
    N = int(t.shape[0])
    if not isinstance(target, StainEstimate):
        raise TypeError(f"normalize: target must be a StainEstimate, got {type(target).__name__}")
    if source is not None:
        source = _per_image(source, N, StainEstimate, "normalize: source")
    m = _mask(mask, t.shape[:3], "normalize")
    dev = _device(t, m)
    x = t.to(dev).contiguous()
    if source is None:
        source = _estimate(x, None if m is None else m.to(dev).contiguous(), opts)
    y = _apply(x, source, target, opts, out)
    return y[0] if one and out is None else y


def separate(images, stains=HDAB, dtype="float", residual=False, options=None):
    """The stain concentrations ``pinv(S) od`` of every pixel -> ``[N, H, W, K]`` on the device (``[H, W, K]`` for one image), K = 2, or
    3 with ``residual`` (the third stain is the unit vector along the cross product of the two).  ``stains``: a [3, 2] matrix of
    optical-density vectors (``HDAB`` by default) or a ``StainEstimate``, the same for every image.  ``dtype="float"``: fp32
    concentrations; ``"u8"``: ``clamp(rint(255 c / options.conc_max), 0, 255)``, so that column 1 of an H-DAB separation is a
    uint8 DAB map for ``regions.measure_labels(..., intensity=)`` and ``inference.measure_slide_cells(..., intensity=)``."""
    opts = _options(options, "separate")
    if dtype not in ("float", "u8"):
        raise ValueError(f"dtype must be 'float' or 'u8', got {dtype!r}")
    t, one = _rgb(images, "separate")
    N = int(t.shape[0])
    P = [np.linalg.pinv(stain_matrix(stains, bool(residual)))] * N
    dev = _device(t)
    x = t.to(dev).contiguous()
    y = K.stain_separate(x, _od(opts, dev), _upload(P, dev), dtype == "u8", float(opts.conc_max))
    return y[0] if one else y


# ---- inference.detect_slide(..., stain=...) ------------------------------------------------------------------------------------------
def _check_slide_argument(stain, what):
    """True | StainOptions | (StainOptions or None, StainEstimate) -> (options, target)"""
    if isinstance(stain, tuple) and len(stain) == 2 and isinstance(stain[1], StainEstimate) and \
            (stain[0] is None or isinstance(stain[0], StainOptions)):
        return _options(stain[0], what), stain[1]
    if stain is True or isinstance(stain, StainOptions):
        return _options(stain, what), TARGET_HDAB
    raise TypeError(f"{what}: expected True, a StainOptions or an (options, target StainEstimate) pair, got {type(stain).__name__}")


def _normalize_slide(dev_image, dev_mask, options, target):
    """device image [1, H, W, 3], device mask [1, H, W] or None -> (the normalised copy, the slide's own StainEstimate)"""
    source = _estimate(dev_image, dev_mask, options)
    return _apply(dev_image, source, target, options), source[0]
