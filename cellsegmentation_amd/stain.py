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

``quantify_labels`` answers what the slide was stained for without a concentration image in between: one pass over the RGB image
and a label image (csrc/regions.hip) leaves, per cell and per compartment (the cell, and the ring an expansion adds around it),
exact integer tables of an integer stain level -- ``StainTable``, whose ``classify`` and ``score`` give the intensity classes, the
labelling index and the H-score.  ``texture_labels`` tabulates how that level is arranged inside every cell instead: the grey-level
co-occurrence tables of ``regions.texture_labels`` over one stain (``regions.TextureTable``, Haralick's features).

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


# ---- per-cell stain quantification: integer levels tabulated per (label, compartment) ------------------------------------------------
QUANTIFY_BINS = K.STAIN_QUANTIFY_BINS
LEVEL_SHIFT = 24


def quantised_matrix(stains, residual=False, conc_max=8.0):
    """``Mq`` int32 [K, 3] of one image: ``rint(2^24 255 pinv(S) / (4096 conc_max))`` in float64; ``ValueError`` where an entry
    leaves int32."""
    _number(conc_max, "conc_max", 0, 1e30, lo_open=True)
    M = np.rint(np.linalg.pinv(stain_matrix(stains, bool(residual))) * (float(1 << LEVEL_SHIFT) * 255.0) / (float(OD_UNIT) * float(conc_max)))
    if not np.isfinite(M).all() or np.abs(M).max() > 2 ** 31 - 1:
        raise ValueError(f"stains: the quantised matrix leaves int32 (largest entry {np.abs(M).max():.3g}): conc_max {conc_max} is too "
                         "small for these stain vectors")
    return M.astype(np.int32)


def positive_levels(pixel_threshold, n_stains, conc_max):
    """None | one concentration per stain -> None | the K levels ``clamp(ceil(255 t / conc_max), 0, 256)``"""
    if pixel_threshold is None:
        return None
    if isinstance(pixel_threshold, (str, bytes)) or not hasattr(pixel_threshold, "__len__") or len(pixel_threshold) != n_stains:
        raise ValueError(f"pixel_threshold must be None or {n_stains} concentrations, one per stain, got {pixel_threshold!r}")
    for t in pixel_threshold:
        _number(t, "pixel_threshold", -1e30, 1e30)
    return tuple(int(min(max(math.ceil(255.0 * float(t) / float(conc_max)), 0), 256)) for t in pixel_threshold)


def class_thresholds(thresholds, conc_max):
    """1 to 3 increasing concentrations -> the integers ``T = rint(256 255 t / conc_max)``, each in [0, 2^31)"""
    if isinstance(thresholds, (int, float, np.integer, np.floating)) and not isinstance(thresholds, bool):
        thresholds = (thresholds,)
    if isinstance(thresholds, (str, bytes)) or not hasattr(thresholds, "__len__") or not 1 <= len(thresholds) <= 3:
        raise ValueError(f"thresholds must be 1 to 3 increasing concentrations, got {thresholds!r}")
    for t in thresholds:
        _number(t, "thresholds", 0, 1e30)
    if any(b <= a for a, b in zip(thresholds, thresholds[1:])):
        raise ValueError(f"thresholds must increase, got {thresholds!r}")
    T = [int(np.rint(256.0 * 255.0 * float(t) / float(conc_max))) for t in thresholds]
    if T[-1] >= 1 << 31:
        raise ValueError(f"thresholds: {thresholds[-1]!r} is beyond 2^31 / 65280 of conc_max {conc_max}")
    return T


@dataclass(eq=False)
class StainTable:
    """``quantify_labels`` of N images as device tensors; row k belongs to label k + 1, compartment 0 is the label itself and
    compartment 1 (only with ``expanded``) the ring around it.  ``counts`` int32 [N]: the labels in use, also above the capacity;
    ``n`` int32 [N, cap, C] pixels; ``sum``, ``sumsq`` int64 and ``max``, ``pos`` int32 [N, cap, C, K] of the integer stain level
    (``pos`` None without a ``pixel_threshold``); ``hist`` int32 [N, cap, C, K, bins] or None.  ``Mq`` int32 numpy [N, K, 3],
    ``options`` and ``pos_levels`` are what it was made with.  The rules are in ``quantify_labels``' docstring.  Every method but
    ``per_image`` and ``score`` runs on the device in float64, is computed from the integer tables only and gives NaN where
    ``n == 0``."""
    counts: torch.Tensor
    capacity: int
    n: torch.Tensor
    sum: torch.Tensor
    sumsq: torch.Tensor
    max: torch.Tensor
    pos: object
    hist: object
    Mq: np.ndarray
    options: StainOptions
    pos_levels: object = None

    def _n(self):
        return self.n.to(torch.float64).unsqueeze(-1)

    def mean(self):
        """float64 [N, cap, C, K] = sum / n, in levels"""
        return self.sum.to(torch.float64) / self._n()

    def std(self):
        """float64 [N, cap, C, K] = sqrt(n sumsq - sum^2) / n, the population standard deviation in levels.  The numerator is an
        exact int64 where n < 2^23 (2^23 2^23 255^2 < 2^62); a larger region forms it in float64."""
        n64 = self.n.to(torch.int64).unsqueeze(-1)
        exact = (n64 * self.sumsq - self.sum * self.sum).to(torch.float64)
        s = self.sum.to(torch.float64)
        num = torch.where(n64 < (1 << 23), exact, (self._n() * self.sumsq.to(torch.float64) - s * s).clamp(min=0))
        return torch.sqrt(num) / self._n()

    def positive_fraction(self):
        """float64 [N, cap, C, K] = pos / n: the fraction of pixels at or above the stain's ``pixel_threshold``"""
        if self.pos is None:
            raise ValueError("positive_fraction: the table was made without a pixel_threshold")
        return self.pos.to(torch.float64) / self._n()

    def quantile(self, q):
        """float64 [N, cap, C, K]: the centre, in levels, of the histogram bin that holds order statistic ``ceil(q (n - 1))`` of the
        region's levels (``order_bin``): ``(bin + 1/2) 256 / bins - 1/2``, the level itself with 256 bins."""
        if self.hist is None:
            raise ValueError("quantile: the table was made without a histogram (bins=0)")
        _number(q, "q", 0, 1)
        bins = int(self.hist.shape[-1])
        k = torch.ceil(float(q) * (self._n() - 1)).to(torch.int64)
        b = (torch.cumsum(self.hist.to(torch.int64), dim=-1) <= k.unsqueeze(-1)).sum(dim=-1).to(torch.float64)
        centre = (b + 0.5) * (256.0 / bins) - 0.5
        return torch.where(self.n.unsqueeze(-1) > 0, centre, torch.full_like(centre, float("nan")))

    def concentration(self, levels):
        """levels (a tensor or a number) -> ``levels conc_max / 255``: the concentration a level stands for"""
        return levels * float(self.options.conc_max) / 255.0

    def overflowed(self):
        """device bool [N]: the image has labels above the table's rows"""
        return self.counts > self.capacity

    def classify(self, thresholds, stain=1, compartment=0):
        """int8 [N, cap] on the device: the number of ``thresholds`` (1 to 3 increasing concentrations) that the mean level of
        ``stain`` in ``compartment`` reaches, -1 where ``n == 0``.  Exact: threshold t is ``T = rint(256 255 t / conc_max)`` and
        reached iff ``256 sum >= T n`` in int64."""
        T = class_thresholds(thresholds, self.options.conc_max)
        s, c = self._pick(stain, compartment)
        n64, lhs = self.n[:, :, c].to(torch.int64), 256 * self.sum[:, :, c, s]
        cls = torch.zeros_like(n64)
        for t in T:
            cls += (lhs >= t * n64).to(torch.int64)
        return torch.where(n64 > 0, cls, torch.full_like(cls, -1)).to(torch.int8)

    def _pick(self, stain, compartment):
        Kn, C = int(self.sum.shape[3]), int(self.sum.shape[2])
        for v, hi, name in ((stain, Kn, "stain"), (compartment, C, "compartment")):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v < hi:
                raise ValueError(f"{name} must be an integer in [0, {hi}), got {v!r}")
        return int(stain), int(compartment)

    def score(self, thresholds, stain=1, compartment=0):
        """``score.positivity_score`` of the cells per class of ``classify`` -> ``PositivityScore``; one small copy to the host."""
        from .score import positivity_score
        cls = self.classify(thresholds, stain, compartment).to(torch.int64)
        per = torch.stack([(cls == k).sum(dim=1) for k in range(4)], dim=1)
        return positivity_score(per.cpu().numpy())

    def per_image(self):
        """A host list of N dicts of numpy arrays trimmed to min(count, capacity) rows: the integer tables that the table has, and
        ``mean`` and ``std``.  The one method that synchronises besides ``score``."""
        cols = {"n": self.n, "sum": self.sum, "sumsq": self.sumsq, "max": self.max, "mean": self.mean(), "std": self.std()}
        if self.pos is not None:
            cols["pos"] = self.pos
        if self.hist is not None:
            cols["hist"] = self.hist
        cols = {k: v.cpu().numpy() for k, v in cols.items()}
        counts = self.counts.cpu().numpy()
        return [{k: v[i, :min(int(c), self.capacity)] for k, v in cols.items()} for i, c in enumerate(counts)]


def quantify_labels(images, labels, stains=HDAB, residual=False, expanded=None, pixel_threshold=None, bins=0, table=None,
                    max_regions=None, counts=None, options=None):
    """How strongly every cell of a label image is stained -> ``StainTable``: one pass over the RGB image and the labels, no
    concentration image in between.

    ``images``: uint8 RGB [H, W, 3] or [N, H, W, 3]; ``labels`` (and ``expanded``, for example ``morph.expand_labels(labels, d)``, or
    None): int32 [H, W] or [N, H, W] of the same size.  ``stains``: a [3, 2] matrix of optical-density vectors or a ``StainEstimate``,
    or a list of N of them, one per image; ``residual`` adds the third stain as in ``separate``.  All rules are exact integers:

    * Quantised matrix.  With ``S`` the image's [3, K] stain matrix and ``P = pinv(S)``: ``Mq[s][j] = rint(2^24 255 P[s][j] /
      (4096 conc_max))``, float64 on the host, stored as int32 (``ValueError`` where an entry leaves int32).
    * Level.  Stain s of a pixel (R, G, B) has the level ``clamp((Mq[s][0] od_q[R] + Mq[s][1] od_q[G] + Mq[s][2] od_q[B] + 2^23) >>
      24, 0, 255)``, the sum in int64 and the shift arithmetic, ``od_q = od_table(options.Io)``: the uint8 concentration of
      ``separate(dtype="u8")`` to within one level, free of float rounding and of the order of evaluation.
    * Owner.  A pixel belongs to (row ``labels - 1``, compartment 0) where ``labels > 0``; else, with ``expanded``, to (row
      ``expanded - 1``, compartment 1) where ``expanded > 0``; else to nothing.  Compartment 0 is the cell as segmented (the
      nucleus), compartment 1 the ring that the expansion adds around it.
    * Tables.  Per (image, row, compartment): ``n`` pixels; per stain the ``sum``, the sum of squares ``sumsq`` and the ``max`` of
      the level, ``pos`` = the pixels with level >= ``L_s = clamp(ceil(255 t_s / conc_max), 0, 256)`` for ``pixel_threshold = (t_0,
      ..)``, one concentration per stain, and with ``bins`` (16, 32, 64, 128 or 256) ``hist`` = the pixels per ``bin = level bins
      >> 8``.  A row without a pixel is all zero.

    The rules are restated in numpy by tests/quantify_ref.py (tests/golden/quantify_vectors.npz).  ``table``: the ``RegionTable`` of
    the same labels where the caller has it: its capacity and counts are taken; otherwise ``max_regions`` and ``counts`` as in
    ``regions.measure_labels``: an int ``max_regions`` fixes the rows per image (larger labels are counted, not measured), two
    launches follow and nothing synchronises; None reads the largest label back first (the one synchronisation).  All accumulation
    is integer atomics: the result does not depend on launch or arrival order.  Argument errors are raised before the library is
    loaded."""
    from . import regions as Rg
    what = "quantify_labels"
    opts = _options(options, what)
    x, _ = _rgb(images, what)
    N, H, W, _ = x.shape
    Rg._check_max_regions(max_regions)
    if table is not None and not isinstance(table, Rg.RegionTable):
        raise TypeError(f"{what}: table must be a RegionTable or None, got {type(table).__name__}")
    if bins not in QUANTIFY_BINS or isinstance(bins, bool):
        raise ValueError(f"bins must be one of {QUANTIFY_BINS}, got {bins!r}")
    img = Rg._LabelImage(what, labels, masks_go_to="regions.label first")
    ring = None if expanded is None else Rg._LabelImage(what, expanded, masks_go_to="regions.label first")
    for name, side in (("labels", img), ("expanded", ring)):
        if side is not None and (side.N, tuple(side.labels.shape[-2:])) != (N, (H, W)):
            raise ValueError(f"{what}: {name} of shape {tuple(side.labels.shape)} for images of shape {tuple(x.shape)}")
    per = stains if isinstance(stains, (list, tuple)) else [stains] * N
    if len(per) != N:
        raise ValueError(f"{what}: {len(per)} stain matrices for {N} images")
    Mq = np.stack([quantised_matrix(s, residual, opts.conc_max) for s in per])
    levels = positive_levels(pixel_threshold, Mq.shape[1], opts.conc_max)
    if table is not None:
        if max_regions is not None and int(max_regions) != table.capacity:
            raise ValueError(f"{what}: max_regions {max_regions} against a RegionTable of capacity {table.capacity}")
        if tuple(table.counts.shape) != (N,):
            raise ValueError(f"{what}: a RegionTable of {tuple(table.counts.shape)[0]} images for {N} images")
        if counts is not None:
            raise ValueError(f"{what}: counts come with the table")
    else:
        img.with_counts(counts)
    dev = _device(x, img.labels)
    x = x.to(dev).contiguous()
    lab, counts = img.place(dev)
    ring = None if ring is None else ring.place(dev)[0]
    if table is not None:
        if table.counts.device != dev:
            raise ValueError(f"{what}: a RegionTable on {table.counts.device} for images on {dev}")
        counts = table.counts
    od, mq = _od(opts, dev), torch.from_numpy(Mq).to(dev)
    Kn, C = int(Mq.shape[1]), 1 if ring is None else 2

    def run(cap, want_counts):
        new = lambda dtype, *tail: torch.empty((N, cap, C) + tail, dtype=dtype, device=dev)  # noqa: E731
        t = {"n": new(torch.int32), "sum": new(torch.int64, Kn), "sumsq": new(torch.int64, Kn), "max": new(torch.int32, Kn),
             "pos": new(torch.int32, Kn)}
        if bins:
            t["hist"] = new(torch.int32, Kn, int(bins))
        for a, b in img.chunks:
            K.stain_quantify_labels(x[a:b], lab[a:b], od, mq[a:b], cap, None if ring is None else ring[a:b], levels, int(bins),
                                    counts[a:b] if want_counts else None, want_counts, **{k: v[a:b] for k, v in t.items()})
        return StainTable(counts, cap, t["n"], t["sum"], t["sumsq"], t["max"], t["pos"] if levels is not None else None, t.get("hist"),
                          Mq, opts, levels)

    if table is not None:
        return run(table.capacity, False)
    if max_regions is not None:
        return run(int(max_regions), img.own)
    return run(*Rg._largest_labels(lambda: run(1, True), img), False)   # (the pass that finds the largest labels; one synchronisation)


def texture_labels(images, labels, stains=HDAB, stain=0, residual=False, levels=16, distance=1, table=None, max_regions=None, counts=None,
                   want_matrix=False, options=None):
    """How one stain is arranged inside every cell of a label image -> ``regions.TextureTable``: ``regions.texture_labels`` over an
    RGB image, the level of a pixel being the integer level of stain ``stain`` by the rule of ``quantify_labels``, ``clamp((Mq[0]
    od_q[R] + Mq[1] od_q[G] + Mq[2] od_q[B] + 2^23) >> 24, 0, 255)`` with ``Mq`` = row ``stain`` of the image's
    ``quantised_matrix(stains, residual, options.conc_max)``; no concentration image lies in between.  ``stain=0`` is the first
    stain, haematoxylin under ``HDAB``: the default is chromatin texture.

    ``images``: uint8 RGB [H, W, 3] or [N, H, W, 3]; ``labels``: int32 [H, W] or [N, H, W] of the same size with H W <= 2^30;
    ``stains``: a [3, 2] matrix or a ``StainEstimate``, or a list of N of them; ``stain`` in [0, K), K = 3 with ``residual``.
    ``levels``, ``distance``, ``want_matrix`` and every rule of the tables as in ``regions.texture_labels``; ``table``,
    ``max_regions`` and ``counts`` as in ``regions.hull_labels``.  The table keeps ``Mq`` int32 [N, 3] and the options.  Every
    lane reads the three bytes of its own pixel: nothing is asked of the image's alignment.  Argument errors are raised before the
    library is loaded."""
    from . import regions as Rg
    what = "texture_labels"
    opts = _options(options, what)
    x, _ = _rgb(images, what)
    N, H, W, _ = x.shape
    L, d = Rg._check_texture(levels, distance)
    shape = tuple(Rg._as_labels(labels, what, "regions.label first").shape)
    if (1 if len(shape) == 2 else shape[0], shape[-2:]) != (N, (H, W)):
        raise ValueError(f"{what}: labels of shape {shape} for images of shape {tuple(x.shape)}")
    per = stains if isinstance(stains, (list, tuple)) else [stains] * N
    if len(per) != N:
        raise ValueError(f"{what}: {len(per)} stain matrices for {N} images")
    Mq = np.stack([quantised_matrix(s, residual, opts.conc_max) for s in per])
    if isinstance(stain, bool) or not isinstance(stain, (int, np.integer)) or not 0 <= stain < Mq.shape[1]:
        raise ValueError(f"stain must be an integer in [0, {Mq.shape[1]}), got {stain!r}")
    Mq = np.ascontiguousarray(Mq[:, int(stain)])
    img, table = Rg._labels_and_table(what, labels, table, max_regions, counts, "regions.label first", Rg._check_texture_size)
    dev = img.labels.device
    return Rg._texture(img, table, L, d, bool(want_matrix), images=x.to(dev).contiguous(), od_q=_od(opts, dev),
                       mq=torch.from_numpy(Mq).to(dev), Mq=Mq, options=opts)


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
