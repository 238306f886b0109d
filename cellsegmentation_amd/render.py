"""Annotated images on the HIP path (csrc/render.hip): the drawing that ends the reference's pipeline -- ``overlap_mask``,
``save_images_with_masks``, ``dotting`` and ``locate_cells`` of utils/image_processing.py -- done where the slide, its mask, its
labels and its points already are, so that nothing is copied to the host to be redrawn with OpenCV.

Images are uint8 RGB, ``[H, W, 3]`` or ``[N, H, W, 3]``, numpy or torch, on the host or the device; one image in gives one image
out, a batch a batch, always a device tensor.  Two kernels do the work:

``compose`` is one pass over the pixels, per pixel and channel value ``c`` in this order, all in integers:

* the fill, at most one of
  ``mask`` (uint8 or bool): ``c = (c + 255 * (mask != 0)) >> 1`` -- exactly what the reference's ``img * 0.5 + np.uint8(255 *
  img_bin) * 0.5`` gives when stored into a uint8 array; background pixels are halved too, as there;
  ``heat`` (uint8 ``h``, or float32 probabilities ``p`` with ``threshold``: ``h = p > threshold ? uint8(255 * p) : 0``, the
  reference's ``np.uint8(255 * masks[i] * classes)``): with ``k = colormap[255 - h if invert else h][channel]`` and ``s = c + k``,
  ``c = (s >> 1) + ((s & 1) & ((s >> 1) & 1))`` -- ``cv2.addWeighted(a, .5, b, .5, 0)``, the mean rounded half to even;
* the outline of ``outlines`` (an int32 label image, or a boolean mask that goes through ``regions.label`` first): exactly the
  pixels ``regions.boundaries`` marks get ``outline_color``, or ``palette[(id - 1) % len(palette)]``.  The rule is evaluated in the
  kernel from the labels; no edge map is stored.

``draw_points`` scatters dots or rings at points, in place on a device canvas, by this project's own raster rule: with ``d2 = dr^2 +
dc^2`` from the point, a filled mark (``thickness < 0``) is ``d2 <= r^2`` (1, 5, 13, 49 pixels for r = 0, 1, 2, 4) and a ring of
thickness ``t`` is ``(2r - t)^2 <= 4 d2 <= (2r + t)^2``.  OpenCV's midpoint circle is NOT reproduced: it cannot be compared here
and no pixel parity with ``cv2.circle`` is claimed.  Every write of a call carries one colour, so overlapping marks of a call do
not depend on any order; layers are separate calls in stream order and the later call wins.

The reference-named front ends below write no files: they return device tensors and PNG writing stays with the caller.  Painting
per-tile probabilities (the reference's ``heatmap()``, where the last overlapping tile wins) and text are not here.

Argument errors are raised before the library is loaded or the device is touched; nothing here synchronises with the host.
"""
import numpy as np
import torch

from . import kernels as K
from ._args import _device, _tensor
from ._points import PointSet
from .tissue import _rgb

MAX_RADIUS = K.RENDER_MAX_RADIUS
RED, BLUE = (255, 0, 0), (0, 0, 255)


def jet():
    """The default colour table of the heat fill -> numpy uint8 ``[256, 3]`` in RGB order: ``jet()[v] = clip(382 - abs(4 v - 255 k),
    0, 255)`` with k = 3, 2, 1 for R, G, B, integers only -- dark blue at 0 through cyan, green and yellow to dark red at 255.
    It is NOT ``cv2.COLORMAP_JET`` bit for bit (OpenCV's table cannot be compared here).  The reference blends OpenCV's BGR table
    into an RGB image, so its hot regions come out blue: ``colormap=jet()[:, ::-1]`` gives that look."""
    v = np.arange(256, dtype=np.int64)
    return np.stack([np.clip(382 - np.abs(4 * v - 255 * k), 0, 255) for k in (3, 2, 1)], axis=1).astype(np.uint8)


def _images_arg(images_u8, what):
    t, one = _rgb(images_u8, what)
    N, H, W, _ = t.shape
    if N * H * W >= 1 << 31:
        raise ValueError(f"{what}: a call takes images of fewer than 2^31 pixels in all, got {(N, H, W)}")
    return t, one


def _plane(x, what, name, dtypes, shape, one):
    """numpy / torch [N, H, W] (or [H, W] for one image) of one of ``dtypes`` -> the [N, H, W] tensor where it lives"""
    t = _tensor(x)
    if not torch.is_tensor(t):
        raise TypeError(f"{what}: {name} must be a numpy array or a torch tensor")
    if t.dtype not in dtypes:
        raise TypeError(f"{what}: {name} must be {' or '.join(str(d) for d in dtypes)}, got {t.dtype}")
    if one and t.dim() == 2:
        t = t.unsqueeze(0)
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what}: {name} must be shaped {tuple(shape[1:]) if one else tuple(shape)}, got {tuple(x.shape)}")
    return t


def _table(x, what, name, rows):
    """numpy / torch uint8 [rows, 3] (rows: a number or a (lo, hi) range) -> the host or device tensor"""
    t = _tensor(x)
    if not torch.is_tensor(t) or t.dtype != torch.uint8:
        raise TypeError(f"{what}: {name} must be a uint8 numpy array or torch tensor")
    lo, hi = rows if isinstance(rows, tuple) else (rows, rows)
    if t.dim() != 2 or t.shape[1] != 3 or not lo <= t.shape[0] <= hi:
        raise ValueError(f"{what}: {name} must be shaped [{lo if lo == hi else f'{lo}..{hi}'}, 3], got {tuple(t.shape)}")
    return t


def _u8(t, dev):
    t = t.to(dev).contiguous()
    return t.view(torch.uint8) if t.dtype == torch.bool else t


def compose(images_u8, mask=None, heat=None, threshold=None, colormap=None, invert=True, outlines=None, outline_color=(255, 255, 0),
            palette=None, connectivity=1, out=None):
    """Fill and outline images in one launch -> device uint8 of the images' shape (the rules are in the module's docstring).

    ``mask``: uint8 or bool ``[N, H, W]``; ``heat``: uint8, or float32 with ``threshold``; giving both is a ``ValueError``.
    ``colormap``: uint8 ``[256, 3]`` in the images' channel order, default ``jet()``; ``invert`` looks ``255 - h`` up, as the
    reference does.  ``outlines``: what ``regions.boundaries`` takes, ``connectivity`` for a boolean one; ``palette``: uint8 ``[P,
    3]``, ``1 <= P <= 256``, colours the outline by object id instead of ``outline_color``.  With no fill and no outlines the call is
    a plain copy.  ``out``: a contiguous device uint8 tensor of the images' shape; it may be the (device) images themselves,
    because every pixel is read once before it is written.  A call takes ``N <= 65535`` images of ``N H W < 2^31`` pixels."""
    from . import regions as Rg
    what = "compose"
    t, one = _images_arg(images_u8, what)
    shape = tuple(t.shape[:3])
    if mask is not None and heat is not None:
        raise ValueError("compose: at most one of mask and heat")
    fill, fmap = K.CS_RENDER_FILL_NONE, None
    if mask is not None:
        fill, fmap = K.CS_RENDER_FILL_MASK, _plane(mask, what, "mask", (torch.uint8, torch.bool), shape, one)
    if heat is not None:
        fmap = _plane(heat, what, "heat", (torch.uint8, torch.float32), shape, one)
        fill = K.CS_RENDER_FILL_HEAT_F32 if fmap.dtype == torch.float32 else K.CS_RENDER_FILL_HEAT_U8
    if fill == K.CS_RENDER_FILL_HEAT_F32:
        if isinstance(threshold, bool) or not isinstance(threshold, (int, float, np.integer, np.floating)) or threshold != threshold:
            raise ValueError(f"compose: float32 heat needs a threshold (h = p > threshold ? uint8(255 p) : 0), got {threshold!r}")
    elif threshold is not None:
        raise ValueError("compose: threshold goes with float32 heat only")
    if heat is None:
        if colormap is not None:
            raise ValueError("compose: colormap goes with heat only")
    else:
        colormap = _table(jet() if colormap is None else colormap, what, "colormap", 256)
    labels = None
    if outlines is not None:
        Rg._check_connectivity(connectivity)
        labels = _plane(outlines, what, "outlines", (torch.int32, torch.bool), shape, one)
        if palette is not None:
            palette = _table(palette, what, "palette", (1, 256))
    elif palette is not None:
        raise ValueError("compose: palette goes with outlines only")
    K._render_rgb(what, "outline_color", outline_color)
    if out is not None:
        want = shape[1:] + (3,) if one else shape + (3,)
        if not (torch.is_tensor(out) and out.dtype == torch.uint8 and tuple(out.shape) == want and out.is_cuda and out.is_contiguous()):
            raise ValueError(f"compose: out must be a contiguous device uint8 tensor shaped {want}")
    dev = _device(t, out)
    t = t.to(dev).contiguous()
    if labels is not None:
        labels = (Rg.label(labels.to(dev), connectivity) if labels.dtype == torch.bool else labels.to(dev)).contiguous()
    res = K.render_compose(t, fill, None if fmap is None else _u8(fmap, dev), 0.0 if threshold is None else float(threshold), invert,
                           None if heat is None else colormap.to(dev).contiguous(), labels, outline_color,
                           None if palette is None else palette.to(dev).contiguous(), out=None if out is None else out.view(t.shape))
    return out if out is not None else res[0] if one else res


def _point_args(what, points, offsets, limits, N, tail):
    """the points of N images in the forms ``regions.split`` takes them -> their PointSet (nothing keeps them inside the image)"""
    # a sequence is one point array per image, as in regions.split; for ONE image it may also be that image's (row, col) pairs
    per_image = isinstance(points, (list, tuple)) and offsets is None and (N != 1 or (len(points) and np.ndim(points[0]) == 2))
    ps = PointSet(points, offsets, limits, N, what, per_image=per_image)
    if tail and ps.lim is None:
        raise ValueError(f"{what}: tail draws the points from limits[n] on: it needs limits")
    return ps


def _check_mark(what, radius, thickness):
    for name, v in (("radius", radius), ("thickness", thickness)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise TypeError(f"{what}: {name} must be an integer, got {v!r}")
    if not 0 <= radius <= MAX_RADIUS:
        raise ValueError(f"{what}: radius must be in [0, {MAX_RADIUS}], got {radius}")
    if thickness == 0 or thickness > 2 * radius:
        raise ValueError(f"{what}: thickness must be negative (filled) or a ring's 1 <= t <= 2 radius = {2 * radius}, got {thickness}")


def draw_points(canvas_u8, points, offsets=None, limits=None, radius=4, color=(255, 0, 0), thickness=-1, xy=False, tail=False):
    """Draw a dot (``thickness < 0``) or a ring of ``thickness`` at every point, in place on ``canvas_u8`` -- a contiguous device uint8
    ``[N, H, W, 3]`` or ``[H, W, 3]`` tensor, which is returned.  ``points``, ``offsets`` and ``limits`` are the triple that
    ``regions.split`` and ``spatial.nearest`` take: (row, col) pairs as the detector returns them, or (x, y) with ``xy=True`` as
    ``dotting`` takes them; ``limits`` draws the first ``limits[n]`` points of image n, and with ``tail=True`` the points from
    ``limits[n]`` on instead (the reference's ``new_grids[cell_count:]``, the discarded points).  Points may lie anywhere; pixels
    outside the image are skipped.  ``radius <= 64``, ``1 <= thickness <= 2 radius`` for a ring.  The raster rule is the module's own
    (see its docstring), not OpenCV's.  A call with no points launches nothing."""
    what = "draw_points"
    if not torch.is_tensor(canvas_u8) or canvas_u8.dtype != torch.uint8:
        raise TypeError("draw_points: the canvas must be a uint8 torch tensor (it is drawn on in place)")
    if canvas_u8.dim() not in (3, 4) or canvas_u8.shape[-1] != 3 or canvas_u8.numel() == 0:
        raise ValueError(f"draw_points: the canvas must be shaped [H, W, 3] or [N, H, W, 3], got {tuple(canvas_u8.shape)}")
    c4 = canvas_u8 if canvas_u8.dim() == 4 else canvas_u8.unsqueeze(0)
    N, H, W, _ = c4.shape
    if N > 65535 or N * H * W >= 1 << 31:
        raise ValueError(f"draw_points: a call takes up to 65535 images of fewer than 2^31 pixels in all, got {(N, H, W)}")
    _check_mark(what, radius, thickness)
    K._render_rgb(what, "color", color)
    ps = _point_args(what, points, offsets, limits, N, tail)
    if not canvas_u8.is_cuda or not canvas_u8.is_contiguous():
        raise ValueError("draw_points: the canvas must be a contiguous device tensor")
    if ps.rows:
        ps.upload(canvas_u8.device)
        K.render_points(c4, ps.pts_dev, ps.off_dev, ps.lim_dev, int(radius), color, int(thickness), xy=bool(xy), tail=bool(tail))
    return canvas_u8


# ---- the reference's names ------------------------------------------------------------------------------------------------------
def overlap_mask(img, img_bin, postprocess=True, min_object_size=300, hole_area_threshold=100):
    """utils/image_processing.py:20-28 -> device uint8: ``regions.remove_small_regions`` of the boolean ``img_bin`` (with
    ``postprocess``), then the half-white mask fill over ``img``.  The input image is not written to."""
    from . import regions as Rg
    t, one = _images_arg(img, "overlap_mask")
    m = _plane(img_bin, "overlap_mask", "img_bin", (torch.bool,), tuple(t.shape[:3]), one)
    if postprocess:
        m = Rg.remove_small_regions(m, min_object_size, hole_area_threshold)
    return compose(t[0] if one else t, mask=m[0] if one else m)


def _stacked(x):
    """a list of per-image arrays, as the reference passes them -> one array"""
    if isinstance(x, (list, tuple)) and len(x):
        return torch.stack([_tensor(v) for v in x]) if all(isinstance(v, (np.ndarray, torch.Tensor)) for v in x) else x
    return x


def save_images_with_masks(images, masks, threshold, soft=False):
    """utils/image_processing.py:170-189 without the files: ``images`` uint8 ``[N, H, W, 3]`` (or a list of ``[H, W, 3]``), ``masks``
    float32 probability maps ``[N, H, W]`` (or a list).  ``soft=False`` -> the mask fill with ``masks > threshold`` (the reference's
    ``test_*.png``).  ``soft=True`` -> ``(blended, soft)``: the uint8 soft maps ``uint8(255 * masks * (masks > threshold))`` (its
    ``soft/*.png``) and the images blended with ``jet()[255 - soft]`` (its ``test_*.png``; see ``jet`` for the colours)."""
    from . import regions as Rg
    what = "save_images_with_masks"
    t, one = _images_arg(_stacked(images), what)
    p = _plane(_stacked(masks), what, "masks", (torch.float32,), tuple(t.shape[:3]), one)
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float, np.integer, np.floating)) or threshold != threshold:
        raise ValueError(f"{what}: threshold must be a number, got {threshold!r}")
    p = p.to(_device(t, p)).contiguous()
    classes = Rg.threshold(p, threshold)
    img = t[0] if one else t
    if not soft:
        return compose(img, mask=classes[0] if one else classes)
    softmap = K.detect_quantize(p) * classes.view(torch.uint8)
    softmap = softmap[0] if one else softmap
    return compose(img, heat=softmap), softmap


def _canvas(img, what, copy):
    """one uint8 image, host or device -> a device tensor to draw on (the device tensor itself unless ``copy``)"""
    t, one = _images_arg(img, what)
    if not one:
        raise ValueError(f"{what}: expected one image shaped [H, W, 3], got shape {tuple(t.shape)}")
    if t.is_cuda:
        return img if t.is_contiguous() and not copy else t[0].clone(memory_format=torch.contiguous_format)
    t = t[0]
    return t.to(_device()).contiguous()


def dotting(img, points, radius=4, color=(255, 0, 0), thickness=-1):
    """utils/image_processing.py:31-34 -> device uint8 ``[H, W, 3]``: a mark at every ``(x, y)`` of ``points``.  A contiguous device
    ``img`` is drawn on in place, as ``cv2.circle`` draws on its argument; a host image is copied to the device first."""
    _check_mark("dotting", radius, thickness)
    K._render_rgb("dotting", "color", color)
    pts = _point_args("dotting", points, None, None, 1, False).pts
    return draw_points(_canvas(img, "dotting", copy=False), pts, radius=radius, color=color, thickness=thickness, xy=True)


def _dots(canvas, grids, discarded):
    """red filled r = 4 dots at ``grids``, then blue ones at ``discarded``: (row, col) points of the one image ``canvas``"""
    draw_points(canvas, grids, radius=4, color=RED)
    if discarded is not None and len(discarded):
        draw_points(canvas, discarded, radius=4, color=BLUE)
    return canvas


def locate_cells(image, grids, discarded_grids=None):
    """utils/image_processing.py:37-49 for an image already in memory -> device uint8 ``[H, W, 3]``, a copy of ``image`` with a red
    filled dot of radius 4 at every (row, col) of ``grids``, then a blue one at every discarded point, in that order."""
    g = _point_args("locate_cells", grids, None, None, 1, False).pts
    d = None if discarded_grids is None else _point_args("locate_cells", discarded_grids, None, None, 1, False).pts
    return _dots(_canvas(image, "locate_cells", copy=True), g, d)


def render_detections(result, images_u8, **compose_args):
    """``DetectResult.render``: ``compose(images_u8, **compose_args)``, then the kept points of every map (``cell_counts`` as the
    limit) as red dots and the discarded ones as blue dots, read from the result's device points where it has them."""
    N = len(result.offsets) - 1
    t, one = _images_arg(images_u8, "render")
    if t.shape[0] != N:
        raise ValueError(f"render: {N} maps but {t.shape[0]} images")
    canvas = compose(images_u8, **compose_args)
    pts, off = result._own_points()
    limits = result.cell_counts
    draw_points(canvas, pts, off, limits, radius=4, color=RED)
    if limits is not None:
        draw_points(canvas, pts, off, limits, radius=4, color=BLUE, tail=True)
    return canvas
