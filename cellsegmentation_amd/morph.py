"""Exact disk morphology of masks, the nearest-site transform and label expansion on the HIP path (csrc/morph.hip).

Everything here is one primitive, the exact squared Euclidean distance transform extended to carry the nearest site:

* A *site* is a pixel selected from the input: the ``True`` pixels of a mask (or the ``False`` ones), the nonzero pixels of a label
  image.  Every pixel is given **the nearest site, and among equally near sites the one with the lowest row-major index**;
  ``d2`` is the exact squared distance to it, ``site`` its flat index ``row * W + col`` within its image.  The tie rule is this
  project's own: ``scipy.ndimage.distance_transform_edt(return_indices=True)`` documents none.  The distances are pinned to scipy.
* An image without any site gives ``d2 = -1`` and ``site = -1`` everywhere (``detect.distance_transform_sq``'s convention).
* ``binary_dilation`` / ``binary_erosion`` / ``binary_opening`` / ``binary_closing`` are ``scipy.ndimage.binary_*`` with
  ``structure = (dx^2 + dy^2 <= r2)`` on the ``(2 floor(sqrt(r2)) + 1)^2`` grid, ``iterations=1`` and the same ``border_value``:
  dilation is ``D2_to_True <= r2``, erosion ``m & (D2_to_False > r2)``.  ``r2 = 0`` is the identity.  Pinned to scipy
  (tests/golden/morph_vectors.npz).
* ``expand_labels`` is ``skimage.segmentation.expand_labels`` with the tie rule above in place of whatever scipy's index transform
  does on ties; scikit-image is not a dependency, so only the pixels whose equally near label pixels all carry one label are pinned.

``radius`` / ``distance`` go through ``score.radius_squared``: ``r2 = floor(radius^2)``.  Every function also takes ``radius_sq=``
(an integer, instead of the radius) for radii such as sqrt(13) whose float square rounds down.

Inputs follow ``regions``: numpy or torch, ``[H, W]`` or ``[N, H, W]`` (N independent images), boolean masks (an integer array is
not a mask: ``TypeError``) or int32 label images; batches are cut into chunks of whole images.  An image needs
``H^2 + W^2 < 2^31``.  ``nearest_sites`` and ``expand_labels`` stage one row of packed words in LDS and raise ``ValueError`` for
rows wider than ``MAX_SITE_WIDTH`` = 40960 pixels; the four binary operations take every width.  Argument errors come before any
device work.  Results are device tensors of the input's shape.  It is all integer work: bit-exact and independent of launch order;
a call enqueues a number of launches fixed by the shape and never synchronises, so it can be captured into a graph.

Cost: morphology and label expansion search ``O(radius)`` offsets per pixel whatever the image holds.  Only ``nearest_sites``
searches as far as the nearest site lies.
"""
import numpy as np
import torch

from . import kernels as K
from ._args import _device, _images
from .regions import _as_labels, _chunks
from .score import radius_squared

MAX_SITE_WIDTH = 40960          # 4 bytes per pixel of a row in 160 KiB of LDS (cs_morph_max_site_width)


def _r2(what, radius, radius_sq, name="radius"):
    """``floor(radius^2)``, or ``radius_sq`` itself: exactly one of the two"""
    if (radius is None) == (radius_sq is None):
        raise ValueError(f"{what}: pass either {name} or radius_sq")
    if radius is not None:
        return radius_squared(radius)
    if isinstance(radius_sq, bool) or not isinstance(radius_sq, (int, np.integer)):
        raise TypeError(f"{what}: radius_sq must be an integer, got {radius_sq!r}")
    if not 0 <= radius_sq < 1 << 31:
        raise ValueError(f"{what}: radius_sq must be in [0, 2^31), got {radius_sq!r}")
    return int(radius_sq)


def _border(what, border_value):
    if isinstance(border_value, bool) or border_value not in (0, 1):
        raise ValueError(f"{what}: border_value must be 0 or 1, got {border_value!r}")
    return int(border_value)


def _on_device(t, what, sites):
    """the checked host or device tensor [H,W] / [N,H,W] -> (contiguous device [N,H,W], was_2d); shape limits first"""
    H, W = int(t.shape[-2]), int(t.shape[-1])
    if H * H + W * W >= 1 << 31:
        raise ValueError(f"{what}: an image needs H^2 + W^2 < 2^31, got {H}x{W}")
    if sites and W > MAX_SITE_WIDTH:
        raise ValueError(f"{what}: rows wider than {MAX_SITE_WIDTH} pixels are not supported, got {H}x{W}")
    two_d = t.dim() == 2
    if two_d:
        t = t.unsqueeze(0)
    if not t.is_cuda:
        t = t.to(_device())
    return t.contiguous(), two_d


def _masks(m, what, sites=False):
    t = _images(m, what, torch.bool, "a boolean mask, got {} (an integer array is a label image: see expand_labels)", noun="mask")
    t, two_d = _on_device(t, what, sites)
    return t.view(torch.uint8), two_d


def _run(t, fn, *outs):
    """fn(chunk, workspace, *out_chunks) over the chunks of t [N,H,W]"""
    ws, ws_n = None, 0
    for a, b in _chunks(t):
        if ws_n != b - a:
            ws, ws_n = K.morph_workspace(b - a, t.shape[1], t.shape[2], t.device), b - a
        fn(t[a:b], ws, *(o[a:b] for o in outs))


def nearest_sites(x, background=False):
    """``(d2, site)``, int32 device tensors of ``x``'s shape: for every pixel the exact squared Euclidean distance to the nearest
    site and that site's flat index ``row * W + col`` within its image -- among equally near sites the lowest index; both -1 in an
    image without a site.  ``x``: a boolean mask, whose ``True`` pixels are the sites (the ``False`` ones with ``background=True``),
    or an int32 label image, whose nonzero pixels are.  ``site`` indexes a flattened image: ``labels.flatten(-2).gather(-1,
    site.flatten(-2))`` is the label of the nearest site.  Rows up to ``MAX_SITE_WIDTH`` pixels.  Unlike the rest of this module
    the search is data-dependent, as far as the nearest site lies: sparse sites on a whole slide are its worst case."""
    if (x.dtype == torch.int32) if torch.is_tensor(x) else (isinstance(x, np.ndarray) and x.dtype == np.int32):
        if background:
            raise ValueError("nearest_sites: background=True takes a boolean mask")
        t, two_d = _on_device(_as_labels(x, "nearest_sites", masks_go_to="nearest_sites as they are"), "nearest_sites", True)
    else:
        t, two_d = _masks(x, "nearest_sites", sites=True)
    d2 = torch.empty(t.shape, dtype=torch.int32, device=t.device)
    site = torch.empty_like(d2)
    _run(t, lambda c, ws, d, s: K.morph_nearest(c, background, d2=d, site=s, ws=ws), d2, site)
    return (d2[0], site[0]) if two_d else (d2, site)


def _binary(what, m, radius, radius_sq, border_value, steps):
    """``steps``: 1 = erosion, 0 = dilation, in order"""
    r2, bv = _r2(what, radius, radius_sq), _border(what, border_value)
    t, two_d = _masks(m, what)
    for erode in steps:
        out = torch.empty_like(t)
        # the zero pixels are the sites of an erosion, the nonzero ones of a dilation: the outside is one where border_value says so
        _run(t, lambda c, ws, o: K.morph_binary(c, erode, r2, outside_is_site=bv != erode, out=o, ws=ws), out)
        t = out
    out = t.view(torch.bool)
    return out[0] if two_d else out


def binary_dilation(m, radius=None, border_value=0, radius_sq=None):
    """``scipy.ndimage.binary_dilation`` by the disk ``dx^2 + dy^2 <= r2`` -> device ``torch.bool``: ``D2_to_True <= r2``.  With
    ``border_value=1`` the pixels outside the image count as ``True``."""
    return _binary("binary_dilation", m, radius, radius_sq, border_value, (0,))


def binary_erosion(m, radius=None, border_value=0, radius_sq=None):
    """``scipy.ndimage.binary_erosion`` by the disk ``dx^2 + dy^2 <= r2`` -> device ``torch.bool``: ``m & (D2_to_False > r2)``.
    With ``border_value=0`` (the default, as in scipy) the pixels outside the image count as ``False``: the foreground is eaten from
    the image edge as well."""
    return _binary("binary_erosion", m, radius, radius_sq, border_value, (1,))


def binary_opening(m, radius=None, border_value=0, radius_sq=None):
    """``scipy.ndimage.binary_opening`` by the disk: the erosion, then the dilation of its result, both with ``border_value``."""
    return _binary("binary_opening", m, radius, radius_sq, border_value, (1, 0))


def binary_closing(m, radius=None, border_value=0, radius_sq=None):
    """``scipy.ndimage.binary_closing`` by the disk: the dilation, then the erosion of its result, both with ``border_value``.  As in
    scipy, the default ``border_value=0`` lets the erosion eat into foreground that touches the image edge, so the result need not
    contain the input there; ``border_value=1`` is the one to use for closing."""
    return _binary("binary_closing", m, radius, radius_sq, border_value, (0, 1))


def expand_labels(labels, distance=None, radius_sq=None):
    """``skimage.segmentation.expand_labels`` of an int32 label image -> int32 device tensor: every zero pixel whose nearest nonzero
    pixel lies within ``r2 = floor(distance^2)`` takes that pixel's label -- among equally near pixels the one with the lowest
    row-major index, where scikit-image inherits whatever scipy's index transform does on ties; nonzero pixels keep theirs.  No
    label appears or disappears, so the ``counts`` of the table that numbered the input stay valid for
    ``regions.measure_labels(expanded, counts=...)``.  Rows up to ``MAX_SITE_WIDTH`` pixels."""
    r2 = _r2("expand_labels", distance, radius_sq, name="distance")
    t, two_d = _on_device(_as_labels(labels, "expand_labels", masks_go_to="regions.label first"), "expand_labels", True)
    out = torch.empty_like(t)
    _run(t, lambda c, ws, o: K.morph_expand_labels(c, r2, out=o, ws=ws), out)
    return out[0] if two_d else out
