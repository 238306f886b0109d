"""inference_tiles / sample / inference_image / inference_seg with the reference's signatures
(inference.py:9-153), on the HIP path.

* ``inference_tiles``: eval forward + on-device softmax prob of class 1, written into ONE device
  buffer and copied to the host once at the end (the reference copies every batch).
* ``sample``: the adaptive top-k.  Host logic only builds the per-tile k and the run offsets from
  ``trainset.tileIDX`` / ``trainset.labels``; sorting + selection run in the segmented top-k HIP
  kernel, bit-exact with ``np.lexsort`` + the reference's wrap-around predicate.
"""
from dataclasses import dataclass

import numpy as np
import torch

from . import kernels as K
from ._args import _device, _images, _tensor

try:
    from tqdm import tqdm
except ImportError:  # pragma: no cover
    def tqdm(x, **kw):
        return x


def inference_tiles(loader, model, device, epoch=None, total_epochs=None, mode='train'):
    """Forward inference to obtain instance classification probs -> np.ndarray[float32, len(dataset)]."""
    model.eval()
    probs = torch.zeros((len(loader.dataset),), dtype=torch.float32, device=device)
    with torch.no_grad():
        for i, input in enumerate(tqdm(loader, desc="tile forwarding")):
            if mode == 'train':
                input = input[0]
            output = model(input.to(device))
            n = input.size(0)
            probs[i * loader.batch_size:i * loader.batch_size + n] = K.softmax_prob1(output.contiguous())
    return probs.cpu().numpy()


def selection_plan(tile_idx, labels, tiles_per_pos, topk_neg):
    """Host half of ``sample``: per-tile k and run offsets (inference.py:38-39 semantics).
    labels may be a dict or a sequence indexed by group id."""
    groups = np.asarray(tile_idx)
    if groups.ndim != 1 or len(groups) == 0:
        raise ValueError("tileIDX must be a non-empty 1-D sequence")
    if np.any(groups[1:] < groups[:-1]):
        raise ValueError("tileIDX must be non-decreasing (tiles of one image are contiguous, dataset/dataset.py:120-140)")
    lab = np.asarray([labels[g] for g in groups], dtype=np.int64)
    k = np.where(lab == 0, topk_neg, lab * tiles_per_pos).astype(np.int32)
    starts = np.flatnonzero(np.r_[True, groups[1:] != groups[:-1]])
    offsets = np.r_[starts, len(groups)].astype(np.int64)
    return groups.astype(np.int32), k, offsets


def select_topk(probs, tile_idx, labels, tiles_per_pos, topk_neg, device=None):
    """order[index] of inference.py:34-42 as a python list of ints."""
    groups, k, offsets = selection_plan(tile_idx, labels, tiles_per_pos, topk_neg)
    if device is None:
        device = probs.device if torch.is_tensor(probs) else torch.device("cuda")
    p = probs if torch.is_tensor(probs) else torch.from_numpy(np.ascontiguousarray(probs, dtype=np.float32))
    p = p.to(device=device, dtype=torch.float32).contiguous()
    out, cnt = K.segmented_topk(p, torch.from_numpy(groups).to(device), torch.from_numpy(k).to(device),
                                torch.from_numpy(offsets).to(device), int(np.diff(offsets).max()))
    n = int(cnt.item())
    return out[:n].cpu().tolist()


def sample(trainset, probs, tiles_per_pos, topk_neg, pos_neg_ratio):
    """Select top-k tiles per image to create the instance training set (inference.py:31-43)."""
    selected = select_topk(probs, trainset.tileIDX, trainset.labels, tiles_per_pos, topk_neg)
    p, n = trainset.make_train_data(selected, pos_neg_ratio)
    print("Training data is sampled. (Pos samples: {} | Neg samples: {})".format(p, n))


def inference_image(loader, model, device, epoch=None, total_epochs=None, mode='train', cls_limit=False, return_id=False,
                    categorize=None, de_categorize=None):
    """Image-level class + rounded count (inference.py:46-101).  ``categorize``/``de_categorize`` are the dataset helpers the
    reference imports at module level (inference.py:6, dataset/dataset.py:745-780); only needed with cls_limit, and then taken
    from the caller's ``dataset`` module when not passed."""
    if cls_limit and (categorize is None or de_categorize is None):
        import dataset as _dataset                       # the reference's (or the user's) dataset module, as inference.py:6
        categorize = categorize or _dataset.categorize
        de_categorize = de_categorize or _dataset.de_categorize
    model.eval()
    ids, cats, counts = [], [], []
    with torch.no_grad():
        for i, data in enumerate(tqdm(loader, desc="image forwarding")):
            if mode == 'train':
                data = data[0]
            else:
                batch_ids, data = data
                ids.append(np.asarray(batch_ids))
            output = model(data.to(device))
            cat_labels = K.softmax_argmax(output[0].float().contiguous()).cpu().numpy()      # argmax of the PROBABILITIES (:72-76)
            output_reg = np.round(output[1][:, 0].cpu().numpy()).astype(int)
            if cls_limit:
                for j, x in enumerate(output_reg):
                    if categorize(x) > cat_labels[j]:
                        output_reg[j] = de_categorize(cat_labels[j])[1]
                    elif categorize(x) < cat_labels[j]:
                        output_reg[j] = de_categorize(cat_labels[j])[0]
            cats.append(cat_labels.astype(np.float64))
            counts.append(output_reg.astype(np.float64))
    cats = np.concatenate(cats) if cats else np.array(())
    counts = np.concatenate(counts) if counts else np.array(())
    if return_id:
        return (np.concatenate(ids) if ids else np.array(())), cats, counts
    return cats, counts


def inference_image_cls(loader, model, device, epoch=None, total_epochs=None, mode='train'):
    """Image-level class only (inference.py:104-120): argmax of the 7-way head."""
    model.eval()
    cats = []
    with torch.no_grad():
        for i, data in enumerate(tqdm(loader, desc="image forwarding")):
            if mode == 'train':
                data = data[0]
            output = model(data.to(device))
            cats.append(K.softmax_argmax(output[0].float().contiguous()).cpu().numpy().astype(np.float64))     # :118-119
    return np.concatenate(cats) if cats else np.array(())


def inference_image_reg(loader, model, device, epoch=None, total_epochs=None, mode='train'):
    """Image-level count only (inference.py:123-137): the raw regression output, float32 [len(dataset)]."""
    model.eval()
    nums = []
    with torch.no_grad():
        for i, data in enumerate(tqdm(loader, desc="image forwarding")):
            if mode == 'train':
                data = data[0]
            output = model(data.to(device))
            nums.append(output[1].detach()[:, 0].float().cpu())
    return torch.cat(nums, dim=0).numpy() if nums else torch.tensor(()).numpy()


def inference_seg(loader, model, device, mode='train'):
    """inference.py:140-153"""
    model.eval()
    masks = []
    with torch.no_grad():
        for i, data in enumerate(tqdm(loader, desc="image segmenting")):
            output = model(data.to(device))
            if mode == 'test':
                output = K.softmax_channel_fwd(output.contiguous(), 1)
            masks.append(output.cpu().numpy())
    return np.concatenate(masks)


def detect_cells(loader, model, device, eps=11, reg_limit=False, method="gaussianblur", thr_for_dt=10, **blur):
    """Cell locations per image (test_seg.py cell_detect + meanshift_cluster, one map per image): segment-mode forward, softmax
    channel 1, quantise, then detect.detect_points with the remaining keyword arguments (thr, window_size, interval, ksize, sigmaX,
    ...).  method="distancetransform" smooths by the exact distance transform of ``u8 > thr_for_dt`` instead of the blur (ksize and
    sigma are then not consulted); either way the fp32 probabilities go straight into the smoothing kernel.  With reg_limit the
    image-mode count rint(reg) caps each image's list (test_seg.py:217-221; the model is set back to segment mode afterwards).  Returns [(points, discarded)] per image, as meanshift_cluster."""
    from . import detect as D
    opts = _detect_options("detect_cells", eps, method, thr_for_dt, **blur)
    model.eval()
    out = []
    with torch.no_grad():
        for i, data in enumerate(tqdm(loader, desc="cell detecting")):
            probs, reg = _segment_batch(model, data.to(device), reg_limit, False)     # the count only caps the list
            out.extend(D._detect(probs, reg.cpu().numpy().astype(int) if reg_limit else None, opts).per_image())
    return out


def _detect_options(what, eps, method, thr_for_dt, **blur):
    """the detection arguments of a driver -> detect.DetectOptions: every argument error that needs no image, before the model is
    touched.  ``blur``: the driver's remaining keyword arguments."""
    from . import detect as D
    unknown = set(blur) - {"thr", "window_size", "interval", "ksize", "sigmaX", "sigmaY", "max_iter"}
    if unknown:
        raise TypeError(f"{what}: unexpected arguments {sorted(unknown)}")
    return D.DetectOptions(eps=eps, method=method, thr_for_dt=thr_for_dt, **blur)


def _rounded_counts(model, x):
    """rint(reg) of an image-mode forward -> device fp32 [n]"""
    return torch.round(model(x)[1].detach()[:, 0].float())


def _segment_batch(model, x, want_counts, zero_empty):
    """One batch through the model in segment mode -> (probs, reg): probs fp32 [n, H, W] = softmax channel 1; reg = the image-mode
    counts rint(reg) of a second forward as a device fp32 [n] tensor, None without ``want_counts`` (the model is set back to
    segment mode).  ``zero_empty``: the map of an image whose count is 0 is zeroed (test_seg.py:518-524)."""
    probs = K.softmax_channel_fwd(model(x).contiguous(), 1)
    reg = None
    if want_counts:
        model.setmode("image")
        reg = _rounded_counts(model, x)
        model.setmode("segment")
        if zero_empty:
            probs = probs * (reg != 0).to(probs.dtype)[:, None, None]
    return probs, reg


@dataclass
class SlideResult:
    """One slide of ``detect_slide``: ``points`` / ``discarded`` int64 [n, 2] (row, col) as ``meanshift_cluster`` returns them
    (``discarded`` is ``[]`` without a cap), ``cell_count`` the summed per-patch counts, ``mask`` the stitched uint8 [H, W] device
    tensor, ``tissue`` the ``tissue.TissueResult`` of a run with ``tissue=`` (None without).  ``stain``: the slide's own
    ``stain.StainEstimate`` of a run with ``stain=`` (None without); an attribute that ``detect_slide`` sets, not an argument of
    the constructor, so that the record's positional fields stay the five they were.  ``roi``: the device uint8 [H, W] mask of 0 / 1
    of a run with ``roi=`` (None without), an attribute set the same way; with ``tissue=`` as well, ``tissue.mask`` is the tissue mask
    cut to the ROI and ``tissue.coverage`` counts that."""
    points: np.ndarray
    discarded: object
    cell_count: int
    mask: torch.Tensor
    tissue: object = None
    stain = None
    roi = None


def _check_blend(blend, tta, ph, pw):
    """``blend=`` / ``tta=`` of detect_slide -> (taps, codes): the ``(row taps, column taps)`` pair of ``detect.StitchBlend`` and the
    flip codes of the views, un-flipped first; every error on the host."""
    from . import detect as D
    codes = (0,)
    if tta is not None:
        try:
            codes = tuple(tta)
        except TypeError:
            raise TypeError(f"detect_slide: tta must be a sequence of flip codes, got {tta!r}") from None
        if any(isinstance(c, bool) or not isinstance(c, (int, np.integer)) or not 0 <= c <= 3 for c in codes):
            raise ValueError(f"detect_slide: a tta flip code is 0 (none), 1 (horizontal), 2 (vertical) or 3 (both), got {tta!r}")
        if len(set(codes)) != len(codes) or 0 not in codes:
            raise ValueError(f"detect_slide: tta must hold distinct flip codes, the un-flipped view 0 among them, got {tta!r}")
        codes = (0,) + tuple(int(c) for c in codes if c != 0)
        if blend is None:
            blend = True
    if blend is True:
        blend = {}
    elif isinstance(blend, str):
        blend = {"window": blend}
    elif not isinstance(blend, dict):
        raise TypeError(f"detect_slide: blend must be None, True, 'linear', 'uniform' or a dict with window and ramp, got {blend!r}")
    unknown = set(blend) - {"window", "ramp"}
    if unknown:
        raise TypeError(f"detect_slide: blend has no entries {sorted(unknown)}")
    return D._blend_windows(blend.get("window", "linear"), blend.get("ramp"), ph, pw), codes


def _blended_loop(model, img, ti, rc, size, batch_size, dtype, total, taps, codes):
    """detect_slide's loop with blending on -> the blended uint8 [H, W] mask.  Per batch of corners and per view of ``codes``: stage
    (view 0 by ``tiles.gather_tiles`` as in the plain loop, a flipped view by ``augment.stage_tiles``' kernel with that flip code
    for every tile), segment forward, ``StitchBlend.add`` with the view's code; the image-mode counts of view 0 alone are added to
    ``total``.  Every operand is a device tensor made before the loop, so nothing in it synchronises; ``finish`` runs once after
    it."""
    from . import detect as D
    from . import tiles as T
    sb = D.StitchBlend(img.shape[1:3], (size, size), taps, device=img.device)
    if len(rc) * len(codes) * sb._wmax >= 1 << 31:                         # add would raise part of the way through the slide
        raise OverflowError(f"detect_slide: {len(rc)} patches in {len(codes)} views of weight up to {sb._wmax} could overflow the "
                            "int32 weight sum of the blend; pass a smaller ramp (blend={'ramp': 16})")
    flips = {c: torch.full((batch_size,), c, dtype=torch.int8, device=img.device) for c in codes if c}
    with torch.no_grad():
        for i in range(0, len(rc), batch_size):
            bi, brc = ti[i:i + batch_size], rc[i:i + batch_size]
            for code in codes:
                fl = flips[code][:len(brc)] if code else None
                x = K.stage_augmented(img, bi, brc, size, size, flips=fl, dtype=dtype) if code else T.gather_tiles(img, bi, brc, size, dtype)
                model.setmode("segment")
                sb.add(model(x).float().contiguous(), brc, fl, 1)
                if not code:
                    model.setmode("image")
                    total += _rounded_counts(model, x).sum(dtype=torch.float64)
    return sb.finish()


def detect_slide(image_u8, model, device=None, batch_size=16, patch_size=299, interval=None, eps=11, reg_limit=True,
                 method="gaussianblur", thr_for_dt=10, tissue=None, stain=None, blend=None, tta=None, roi=None, **blur):
    """The loop of ``cell_detect`` (test_seg.py:182-316) for one slide or ROI, streamed on the device -> SlideResult.

    image_u8: uint8 [H, W, 3], numpy or torch; it is moved to the device once.  ``tiles.sample_patches`` gives the (row, col) patch
    corners (the reference's ROI mode indexes ``image[x:x+ph, y:y+pw]``); per batch of ``batch_size`` corners ``tiles.gather_tiles``
    stages the patches, the segment-mode forward's logits go through ``detect.stitch_logits`` into one zeroed uint8 [H, W] mask
    (later patches overwrite earlier ones, as ``whole_image_mask[...] = mask`` does), and ``rint(reg)`` of the image-mode forward of
    the same staged batch is added to a device accumulator.  Nothing inside the loop synchronises with the host.  The stitched mask
    then goes through ``detect._detect`` with the summed count as the cap (reg_limit=True, as ``cell_detect`` always caps, :240,265;
    False returns every point).  ``method``, ``thr_for_dt`` and the keyword arguments thr, window_size, ksize, sigmaX, sigmaY, max_iter are
    those of ``detect_cells``; ``interval`` is the patch grid's here, so the seed grid keeps ``meanshift_cluster``'s default of 10, as
    in ``cell_detect``.  ``patch_size`` must be square here (gather_tiles cuts square tiles; ``sample_patches`` itself is general).  The model is left in segment mode and ``eval()``.

    ``tissue`` (not in the reference, which runs every patch): None, the default, reaches none of it.  ``True`` or a
    ``tissue.TissueOptions`` first decides on the device which patches hold tissue (``tissue.select_patches``: a tissue mask by
    Otsu's threshold, the tissue pixels under every patch, the patches with enough of them) and runs the loop over those only, in
    the order of ``sample_patches`` and in batches of ``batch_size`` of the kept list.  Mask pixels that no kept patch covers stay
    0, the count sums over the kept patches, and ``SlideResult.tissue`` holds the ``TissueResult``.  That costs two small
    synchronisations before the loop and none inside it; with no patch kept the loop does not run.

    ``stain`` (not in the reference either): None, the default, reaches none of it.  ``True``, a ``stain.StainOptions`` or an
    ``(options, target)`` pair estimates the slide's stain vectors once (``stain.estimate``, over the tissue mask when ``tissue`` is
    given as well -- the tissue decision itself is taken on the slide as scanned) and writes a Macenko-normalised copy of the slide
    on the device (``stain.normalize`` towards ``target``, by default ``stain.TARGET_HDAB``); ``gather_tiles`` then reads that copy.
    ``SlideResult.stain`` holds the slide's own ``StainEstimate``.  The estimate's three small copies to the host happen before
    the loop; there is none inside it.

    ``blend`` (not in the reference, whose last writer wins every overlap): None, the default, reaches none of it.  ``True``
    (linear window, full ramp), ``"linear"``, ``"uniform"`` or a dict with ``window`` and ``ramp`` (``detect.blend_taps``; ``window``
    may also be an explicit pair of tap sequences) feeds the logits of every batch to a ``detect.StitchBlend`` instead: per pixel
    the weighted integer mean of every patch that covers it, the weight falling towards a patch's edge, so that no seam is left
    where patches meet and a smaller ``interval`` buys a smoother mask.  The mask is its ``finish()``, taken once after the loop,
    and does not depend on ``batch_size``; a pixel that one patch covers holds the byte it holds without ``blend``.  The two
    accumulators take 12 bytes per slide pixel while the loop runs.

    ``tta``: None, or a sequence of distinct flip codes with 0 among them, e.g. ``(0, 1, 2, 3)`` (``augment``'s codes: 1 horizontal,
    2 vertical, 3 both): every batch also runs through the segment forward once per flipped view, staged by
    ``augment.stage_tiles``' kernel, and the view's logits are added to the same ``StitchBlend`` with its code, which puts every
    pixel back where it belongs on the slide.  ``tta`` alone turns on ``blend=True``.  ``cell_count`` still sums ``rint(reg)`` of
    the un-flipped view only, so the count and the cap it puts on the points do not depend on ``tta``.  Both compose with
    ``tissue`` and ``stain`` unchanged; pixels that no kept patch covers are 0.

    ``roi`` (the reference's QuPath flow crops the region on the host): None, the default, reaches none of it.  A
    ``polygons.PolygonSet`` of one image, a GeoJSON object (read by ``polygons.from_geojson`` with its defaults) or a uint8 / bool
    [H, W] mask (non-zero = inside) restricts the run to the region a pathologist drew.  The ROI becomes a device mask once
    (``polygons.rasterize``); the patches with at least one ROI pixel under them are kept, in the order of ``sample_patches``
    (``tissue_coverage`` and ``tissue_select``, one small synchronisation); with ``tissue`` as well the tissue mask is ANDed with
    the ROI before the windows are counted.  After the loop the stitched mask is zeroed outside the ROI, so no point lies outside
    it; inside it every patch that covers a pixel has run, in the same order, so the mask there is the mask of the run without
    ``roi``.  ``cell_count`` sums the kept patches whole and therefore over-counts at the ROI's border, where a patch reaches
    beyond it.  ``SlideResult.roi`` holds the mask.  It composes with ``stain``, ``blend`` and ``tta`` unchanged.

    Not done here: reading ``.svs`` / ``.png`` files (OpenSlide is not a dependency), writing the CSV and PNG files, and the
    ``name-<xoffset>`` file-name convention -- the caller adds the offset to ``points[:, 1]``.  ``meanshift_cluster(...,
    "distancetransform")`` keeps raising ``NotImplementedError``; method="distancetransform" here goes through ``detect._detect``."""
    from . import detect as D
    from . import tiles as T
    opts = _detect_options("detect_slide", eps, method, thr_for_dt, **blur)   # ``interval`` is the patch grid's: never in blur
    if tissue is not None:
        from . import tissue as Ts
        tissue = Ts._check_options(tissue, "detect_slide: tissue")
    if stain is not None:
        from . import stain as St
        stain = St._check_slide_argument(stain, "detect_slide: stain")
    ph, pw = T._pair(patch_size, "patch_size")
    if ph != pw:
        raise ValueError(f"detect_slide cuts square patches (tiles.gather_tiles), got patch_size {(ph, pw)}")
    if int(batch_size) < 1:
        raise ValueError(f"batch_size must be positive, got {batch_size!r}")
    blended = None if blend is None and tta is None else _check_blend(blend, tta, ph, pw)
    img = _tensor(image_u8)
    if not torch.is_tensor(img) or img.dtype != torch.uint8 or img.dim() != 3 or img.shape[-1] != 3:
        raise TypeError("detect_slide expects a uint8 image shaped [H, W, 3] (numpy or torch)")
    H, W = int(img.shape[0]), int(img.shape[1])
    corners = np.asarray(T.sample_patches((H, W), (ph, pw), interval), dtype=np.int32).reshape(-1, 2)
    if roi is not None:                                                    # checked here, made on the device below
        from . import polygons as Pg
        roi = Pg.roi_mask(roi, (H, W))
    if device is None:
        device = _device(img)
    img = img.to(device).contiguous()[None]
    rc = torch.from_numpy(corners).to(device)                              # every corner of the slide, uploaded once
    ti = torch.zeros((len(corners),), dtype=torch.int32, device=device)
    kept = None
    if roi is not None:
        roi = roi(device)
    if tissue is not None:                                                 # the patches that hold tissue, in the order of the grid
        kept = Ts._select(img, corners, ti, rc, ph, pw, tissue, roi)
        rc, ti = rc.index_select(0, kept.selected.long()), ti[:kept.n_selected]
    elif roi is not None:                                                  # the patches over at least one pixel of the ROI
        selected, n_selected = K.tissue_select(K.tissue_coverage(roi[None], ti, rc, ph, pw), 1)
        n = int(n_selected.item())
        rc, ti = rc.index_select(0, selected[:n].long()), ti[:n]
    source = None
    if stain is not None:                                                  # the loop reads the normalised copy from here on
        img, source = St._normalize_slide(img, None if kept is None else kept.mask[None], *stain)
    total = torch.zeros((), dtype=torch.float64, device=device)
    dtype = getattr(model, "compute_dtype", torch.float32)
    model.eval()
    if blended is None:
        mask = torch.zeros((H, W), dtype=torch.uint8, device=device)
        with torch.no_grad():
            for i in range(0, len(rc), int(batch_size)):
                x = T.gather_tiles(img, ti[i:i + batch_size], rc[i:i + batch_size], ph, dtype)
                model.setmode("segment")
                K.stitch_logits(mask, model(x).float().contiguous(), rc[i:i + batch_size], 1)
                model.setmode("image")
                total += _rounded_counts(model, x).sum(dtype=torch.float64)
    else:
        mask = _blended_loop(model, img, ti, rc, ph, int(batch_size), dtype, total, *blended)
    model.setmode("segment")
    if roi is not None:
        mask *= roi                                                        # 0 / 1: nothing is left outside the ROI
    count = int(total.item())                                              # the first synchronisation of the slide's loop
    points, discarded = D._detect(mask[None], count if reg_limit else None, opts).per_image()[0]
    result = SlideResult(points, discarded, count, mask, kept)
    result.stain = source
    result.roi = roi
    return result


def detect_slides(slides, model, device=None, blend=None, tta=None, roi=None, **kwargs):
    """``detect_slide`` for every image of an iterable -> a generator of SlideResult, one per slide, in order.  ``blend`` and ``tta``
    (blended overlaps, flip test-time augmentation), ``roi`` (one region for every slide) and the ``kwargs`` are ``detect_slide``'s,
    ``tissue=`` and ``stain=`` among them."""
    for image_u8 in slides:
        yield detect_slide(image_u8, model, device, blend=blend, tta=tta, roi=roi, **kwargs)


def render_slide(image_u8, result, fill="mask", thr_u8=127, outlines=None, **compose):
    """The annotated slide of a ``SlideResult`` -> device uint8 [H, W, 3]: ``render.compose`` of ``image_u8`` (uint8 [H, W, 3], numpy or
    torch) over ``result.mask``, then the dots of ``render.locate_cells``: red at ``result.points``, blue at ``result.discarded``.
    ``fill``: ``"mask"`` is the half-white overlay of ``result.mask > thr_u8``; ``"heat"`` takes ``result.mask`` itself as the uint8 heat
    map; ``None`` skips the fill.  ``outlines`` and the other keyword arguments (colormap, invert, outline_color, palette,
    connectivity, out) are ``compose``'s.  The image is not written to unless it is ``out``."""
    from . import render as Rd
    from .tissue import _check_threshold
    if not isinstance(result, SlideResult):
        raise TypeError(f"render_slide: expected a SlideResult, got {type(result).__name__}")
    if fill not in ("mask", "heat", None):
        raise ValueError(f"render_slide: fill must be 'mask', 'heat' or None, got {fill!r}")
    for name in ("mask", "heat", "threshold"):
        if name in compose:
            raise TypeError(f"render_slide: {name} is not an argument here: the fill comes from result.mask")
    thr_u8 = _check_threshold(thr_u8, "thr_u8")
    t, one = Rd._images_arg(image_u8, "render_slide")
    if not one or tuple(t.shape[1:3]) != tuple(result.mask.shape):
        raise ValueError(f"render_slide: expected one image shaped {tuple(result.mask.shape) + (3,)}, got shape {tuple(np.shape(image_u8))}")
    if fill == "mask":
        compose["mask"] = result.mask > thr_u8
    elif fill == "heat":
        compose["heat"] = result.mask
    return Rd._dots(Rd.compose(image_u8, outlines=outlines, **compose), result.points, result.discarded)


def _opened(classes, opening_radius):
    """``morph.binary_opening(classes, opening_radius, border_value=0)`` when the radius is positive, else ``classes`` itself"""
    if not opening_radius:
        return classes
    from . import morph as M
    return M.binary_opening(classes, opening_radius, border_value=0)


def _cleaned_batch(model, x, threshold, mo, ho, want_counts, zero_empty, opening_radius=0):
    """test_seg.py:515-527 for one batch on the device: ``_segment_batch`` -> (probs fp32 [n, H, W], cleaned classes bool [n, H, W],
    reg).  A positive ``opening_radius`` opens the thresholded masks by that disk before the clean-up."""
    from . import regions as Rg
    probs, reg = _segment_batch(model, x, want_counts, zero_empty)
    classes = _opened(Rg.threshold(probs, threshold), opening_radius)
    return probs, Rg.remove_small_regions(classes, mo, ho, out=classes), reg


def segment_classes(loader, model, device, threshold, min_object_size=300, hole_area_threshold=100, reg_limit=False, opening_radius=0):
    """Cleaned binary masks per image (test_seg.py:515-527): segment-mode forward, softmax channel 1, ``> threshold`` (compared in
    float32, as numpy does for a float32 map), ``remove_small_regions(., 300, 100)``.  With reg_limit the map of an image whose
    image-mode count rint(reg) is 0 is zeroed first (:518-524; the model is set back to segment mode afterwards).  A positive
    ``opening_radius`` runs ``morph.binary_opening(., opening_radius, border_value=0)`` between the threshold and the clean-up (not
    in the reference; 0, the default, reaches none of it).  Returns a device ``torch.bool`` tensor [len(dataset), H, W], ready for
    ``metrics.dice_coef``."""
    from . import regions as Rg
    _check_opening("segment_classes", opening_radius)
    mo, ho = Rg._check_size(min_object_size, "min_object_size"), Rg._check_size(hole_area_threshold, "hole_area_threshold")
    model.eval()
    out = []
    with torch.no_grad():
        for i, data in enumerate(tqdm(loader, desc="image segmenting")):
            out.append(_cleaned_batch(model, data.to(device), threshold, mo, ho, reg_limit, reg_limit, opening_radius)[1])
    return torch.cat(out) if out else torch.zeros((0,), dtype=torch.bool, device=device)


def measure_cells(loader, model, device, threshold, min_object_size=300, hole_area_threshold=100, reg_limit=False, connectivity=1,
                  max_regions=None, shape=False, hull=False, opening_radius=0, contours=False, max_vertices=None):
    """One row per segmented cell: the per-batch body of ``segment_classes``, then ``regions.measure`` of the cleaned masks with
    ``detect.quantize`` of the probabilities (uint8 ``trunc(255 p)``) as the intensity.  Returns the ``RegionTable.per_image``
    dicts of all batches in dataset order (area, bbox, centroid, intensity_sum / _mean / _max per cell).  With ``max_regions``
    given nothing synchronises inside the loop: the tables are read back after the last batch.  ``shape=True`` runs
    ``regions.shape`` on every batch instead and the dicts are those of ``ShapeTable.per_image``: the same keys with the same
    values, plus moments, tallies, central_moments, axis_lengths, eccentricity, orientation, perimeter, equivalent_diameter, extent
    and circularity per cell.  ``hull=True`` adds the columns of ``HullTable.per_image`` (hull, convex_area, solidity,
    feret_diameter_max, feret_diameter_min, n_vertices, too_large) in the same way; with both, every batch is labelled and measured
    once and ``regions.shape_labels`` and ``regions.hull_labels`` share that one ``RegionTable``.  ``opening_radius`` as in
    ``segment_classes``.  ``contours=True`` takes that label-once path too and adds the columns of ``ContourTable.per_image``
    (contour, polygon, n_vertices, too_large, truncated, is_simple, crack_perimeter, enclosed_area, hole_area) from
    ``regions.contour_labels`` with this ``connectivity`` and ``max_vertices`` (None: every batch reads its largest vertex count
    back, so that no polygon is truncated); together with ``hull=True`` the hull keeps ``n_vertices`` and ``too_large`` and the
    contour's two go by ``contour_n_vertices`` and ``contour_too_large``."""
    from . import detect as D
    from . import regions as Rg
    _check_opening("measure_cells", opening_radius)
    mo, ho = Rg._check_size(min_object_size, "min_object_size"), Rg._check_size(hole_area_threshold, "hole_area_threshold")
    model.eval()
    tables = []
    with torch.no_grad():
        for data in tqdm(loader, desc="cell measuring"):
            probs, classes, _ = _cleaned_batch(model, data.to(device), threshold, mo, ho, reg_limit, reg_limit, opening_radius)
            if hull or contours:                                          # label and measure once; the tables hang on that one
                lab = Rg.label(classes, connectivity)
                table = Rg.measure_labels(lab, intensity=D.quantize(probs), max_regions=max_regions)
                parts = [Rg.shape_labels(lab, table=table)] if shape else []
                if contours:
                    parts.append(Rg.contour_labels(lab, table=table, connectivity=connectivity, max_vertices=max_vertices))
                if hull:
                    parts.append(Rg.hull_labels(lab, table=table))
            else:
                measure = Rg.shape if shape else Rg.measure
                parts = [measure(classes, intensity=D.quantize(probs), connectivity=connectivity, max_regions=max_regions)]
            tables.append(parts)
    def per_image(part):
        dicts = part.per_image()
        if hull and isinstance(part, Rg.ContourTable):                    # the two names that HullTable.per_image has as well
            for d in dicts:
                d.update(contour_n_vertices=d.pop("n_vertices"), contour_too_large=d.pop("too_large"))
        return dicts

    out = []
    for parts in tables:
        dicts = per_image(parts[0])
        for more in parts[1:]:
            for d, extra in zip(dicts, per_image(more)):
                d.update(extra)
        out += dicts
    return out


def measure_slide(mask_u8, thr_u8=127, min_object_size=300, hole_area_threshold=100, connectivity=1, max_regions=None, opening_radius=0):
    """One row per cell of a stitched uint8 [H, W] map such as ``SlideResult.mask``: foreground = ``mask_u8 > thr_u8``, opened by the
    disk of ``opening_radius`` when that is positive (``morph.binary_opening``, ``border_value=0``), cleaned by
    ``remove_small_regions``, measured with the map itself as the intensity -> the one-image ``RegionTable`` (device tensors)."""
    from . import regions as Rg
    t, fg = _slide_foreground("measure_slide", mask_u8, thr_u8, min_object_size, hole_area_threshold, connectivity, opening_radius)
    return Rg.measure(fg, intensity=t, connectivity=connectivity, max_regions=max_regions)


def _check_opening(what, opening_radius):
    """the argument errors of ``opening_radius`` under the caller's name, before the model runs"""
    from .score import radius_squared
    try:
        radius_squared(opening_radius)
    except (TypeError, ValueError) as e:
        raise type(e)(f"{what}: opening_radius: {e}") from None


def _slide_foreground(what, mask_u8, thr_u8, min_object_size, hole_area_threshold, connectivity, opening_radius=0):
    """a stitched uint8 [H, W] map -> (the map on the device, its cleaned foreground ``map > thr_u8`` as device bool, opened first
    when ``opening_radius`` is positive)"""
    from . import regions as Rg
    _check_opening(what, opening_radius)
    if isinstance(thr_u8, bool) or int(thr_u8) != thr_u8 or not 0 <= thr_u8 <= 255:
        raise ValueError(f"{what}: thr_u8 must be an integer in [0, 255], got {thr_u8!r}")
    try:
        t = _images(mask_u8, what, torch.uint8, "a uint8 map, got {}", ranks=(2,), to_device=True).contiguous()
    except (TypeError, ValueError):                                         # one message, one type, whatever is wrong with the map
        raise TypeError(f"{what}: expected a uint8 [H, W] map") from None
    fg = _opened(t > int(thr_u8), opening_radius)
    return t, Rg.remove_small_regions(fg, min_object_size, hole_area_threshold, connectivity, out=fg)


def measure_slide_cells(result, thr_u8=127, min_object_size=300, hole_area_threshold=100, connectivity=1, max_regions=None,
                        opening_radius=0, geodesic=False, intensity=None):
    """One row per DETECTED cell of a ``SlideResult``: ``measure_slide``'s thresholding and clean-up of ``result.mask``, then
    ``regions.split`` of the foreground at ``result.points`` and ``regions.measure_labels`` with the map as the intensity ->
    ``(RegionTable, SplitResult)`` of one image.  Row k is ``result.points[k]`` (all zero where the point is not live: on the
    background after the clean-up, or a second point on one pixel); the rows from ``len(result.points)`` on are cells that no
    detection claimed.  ``max_regions`` and ``opening_radius`` as in ``measure_slide``: an int ``max_regions`` means no
    synchronisation.  ``geodesic``: ``regions.split_geodesic`` in its exact mode instead of ``regions.split``, so that every cell is
    one connected piece (it reads a flag back: a synchronisation of its own).  ``intensity``: a uint8 ``[H, W]`` map of the mask's
    shape that takes the place of ``result.mask`` as the intensity of ``measure_labels`` -- the labels still come from the mask --,
    for example the DAB concentration ``stain.separate(slide, dtype="u8")[..., 1]``."""
    from . import regions as Rg
    if not isinstance(result, SlideResult):
        raise TypeError("measure_slide_cells: expected the SlideResult of detect_slide")
    if intensity is not None:
        intensity = _tensor(intensity)
        if not torch.is_tensor(intensity) or intensity.dtype != torch.uint8 or tuple(intensity.shape) != tuple(result.mask.shape):
            raise TypeError(f"measure_slide_cells: intensity must be a uint8 map shaped {tuple(result.mask.shape)}")
    t, fg = _slide_foreground("measure_slide_cells", result.mask, thr_u8, min_object_size, hole_area_threshold, connectivity,
                              opening_radius)
    pts = np.asarray(result.points, np.int64).reshape(-1, 2)
    parts = (Rg.split_geodesic if geodesic else Rg.split)(fg, pts, connectivity=connectivity)
    if intensity is not None:
        t = intensity.to(t.device).contiguous()
    return Rg.measure_labels(parts.labels, intensity=t, max_regions=max_regions, counts=parts.counts), parts


def slide_contacts(result, distance=None, connectivity=1, max_pairs=None, **measure_kwargs):
    """Which DETECTED cells of a ``SlideResult`` touch which, on the device: ``measure_slide_cells(result, connectivity=connectivity,
    **measure_kwargs)``, whose split labels go to ``regions.adjacency_labels`` with ``counts=parts.counts`` and the region table's
    capacity -> ``(AdjacencyTable, RegionTable, SplitResult)`` of one image.  Row k of every table is ``result.points[k]``.
    ``distance``: cells whose gap ``morph.expand_labels`` closes at that distance count as touching (the adjacency table then
    describes the expanded labels, the region table the cells as split).  ``connectivity`` serves the clean-up, the split and the
    adjacency alike: with 2, cells that meet at a pixel corner are neighbours.  ``max_pairs`` as in ``adjacency_labels``; with it
    and ``max_regions`` both integers nothing synchronises."""
    from . import regions as Rg
    if not isinstance(result, SlideResult):
        raise TypeError("slide_contacts: expected the SlideResult of detect_slide")
    conn = Rg._check_connectivity(connectivity)
    Rg._check_max_pairs(max_pairs)
    if distance is not None:
        from .score import radius_squared
        radius_squared(distance)
    table, parts = measure_slide_cells(result, connectivity=conn, **measure_kwargs)
    contacts = Rg.adjacency_labels(parts.labels, conn, distance=distance, max_regions=table.capacity, max_pairs=max_pairs,
                                   counts=parts.counts)
    return contacts, table, parts


def slide_positivity(result, image_u8, stains=None, thresholds=(0.2, 0.4, 0.6), distance=None, stain=1, options=None, **measure_kwargs):
    """Which DETECTED cells of a ``SlideResult`` are stained and how strongly, on the device: ``measure_slide_cells(result,
    **measure_kwargs)``, whose split labels go to ``stain.quantify_labels`` over ``image_u8`` (uint8 RGB ``[H, W, 3]`` of the mask's
    shape) with ``counts=parts.counts`` and the region table's capacity -> ``(PositivityScore, StainTable, RegionTable,
    SplitResult)`` of one image.  Row k of every table is ``result.points[k]``.  ``stains``: a [3, 2] matrix or a ``StainEstimate``;
    None estimates the slide (``stain.estimate``).  ``thresholds``: 1 to 3 increasing concentrations of stain ``stain`` (1 = DAB)
    that a cell's mean level must reach for the classes 1+, 2+, 3+ (``StainTable.classify``).  ``distance``: the cells are grown by
    ``morph.expand_labels`` at that distance and the ring is tabulated as compartment 1 (it is then also the compartment that is
    classified, as a cytoplasmic stain asks for); None classifies the cells as split.  The score is read back; with an int
    ``max_regions`` and given ``stains`` nothing else synchronises."""
    from . import stain as St
    if not isinstance(result, SlideResult):
        raise TypeError("slide_positivity: expected the SlideResult of detect_slide")
    opts = St._options(options, "slide_positivity")
    St.class_thresholds(thresholds, opts.conc_max)
    img = _tensor(image_u8)
    if not torch.is_tensor(img) or img.dtype != torch.uint8 or tuple(img.shape) != tuple(result.mask.shape) + (3,):
        raise TypeError(f"slide_positivity: image_u8 must be a uint8 RGB image shaped {tuple(result.mask.shape) + (3,)}")
    if stains is not None:
        St.quantised_matrix(stains, False, opts.conc_max)
    if distance is not None:
        from .score import radius_squared
        radius_squared(distance)
    table, parts = measure_slide_cells(result, **measure_kwargs)
    img = img.to(parts.labels.device)
    if stains is None:
        stains = St.estimate(img, options=opts)
    ring = None
    if distance is not None:
        from . import morph
        ring = morph.expand_labels(parts.labels, distance)
    cells = St.quantify_labels(img, parts.labels, stains, expanded=ring, table=table, options=opts)
    return cells.score(thresholds, stain, 0 if ring is None else 1), cells, table, parts


def slide_texture(result, image_u8, stains=None, stain=0, levels=16, distance=1, options=None, **measure_kwargs):
    """How a stain is arranged inside the DETECTED cells of a ``SlideResult``, on the device: ``measure_slide_cells(result,
    **measure_kwargs)``, whose split labels go to ``stain.texture_labels`` over ``image_u8`` (uint8 RGB ``[H, W, 3]`` of the mask's
    shape) with the region table -> ``(TextureTable, RegionTable, SplitResult)`` of one image.  Row k of every table is
    ``result.points[k]``.  ``stains``: a [3, 2] matrix or a ``StainEstimate``; None estimates the slide (``stain.estimate``).
    ``stain``: the stain whose level is the grey value (0 = haematoxylin: chromatin texture); ``levels`` and ``distance`` as in
    ``regions.texture_labels``.  With an int ``max_regions`` and given ``stains`` nothing synchronises."""
    from . import regions as Rg
    from . import stain as St
    if not isinstance(result, SlideResult):
        raise TypeError("slide_texture: expected the SlideResult of detect_slide")
    opts = St._options(options, "slide_texture")
    Rg._check_texture(levels, distance)
    if isinstance(stain, bool) or not isinstance(stain, (int, np.integer)) or not 0 <= stain < 2:
        raise ValueError(f"stain must be an integer in [0, 2), got {stain!r}")
    img = _tensor(image_u8)
    if not torch.is_tensor(img) or img.dtype != torch.uint8 or tuple(img.shape) != tuple(result.mask.shape) + (3,):
        raise TypeError(f"slide_texture: image_u8 must be a uint8 RGB image shaped {tuple(result.mask.shape) + (3,)}")
    if stains is not None:
        St.quantised_matrix(stains, False, opts.conc_max)
    Rg._check_texture_size("slide_texture", tuple(result.mask.shape))
    table, parts = measure_slide_cells(result, **measure_kwargs)
    img = img.to(parts.labels.device)
    if stains is None:
        stains = St.estimate(img, options=opts)
    cells = St.texture_labels(img, parts.labels, stains, stain=stain, levels=levels, distance=distance, table=table, options=opts)
    return cells, table, parts


def slide_neighbors(result, k=1, radii=(), other=None, other_xy=False):
    """Neighbourhood statistics of the detected cells of a ``SlideResult``, on the device: ``result.points`` is uploaded once and
    queried on the bucket grid of ``spatial`` with the mask's shape as the image -> ``(NeighborTable or None, WithinCounts or
    None)``: the ``k`` nearest detections of every detection (``k=0``: not asked for) and the number of detections within each of
    ``radii`` of it (empty: not asked for).  ``other``: an integer [m, 2] point set (annotations, another cell class; ``other_xy``
    as in ``score.score_points``) to query against instead of the detections themselves.  Both tables stay device tensors, row i
    being ``result.points[i]``; nothing synchronises."""
    from . import spatial as Sp
    from ._points import points as _points
    if not isinstance(result, SlideResult):
        raise TypeError("slide_neighbors: expected the SlideResult of detect_slide")
    hw = tuple(int(v) for v in result.mask.shape)
    pts = np.asarray(result.points, np.int64).reshape(-1, 2)
    kw = {}
    if other is not None:
        kw = {"other": _points(other, "slide_neighbors: other")[0], "other_xy": other_xy}
    radii = [radii] if np.isscalar(radii) else list(radii)
    dev_pts = torch.from_numpy(pts).to(result.mask.device)
    near = Sp.nearest(dev_pts, hw, k, **kw) if k else None
    within = Sp.count_within(dev_pts, hw, radii, **kw) if radii else None
    return near, within


def slide_clusters(result, eps, min_samples=5):
    """The aggregates of the detected cells of a ``SlideResult``, on the device: ``result.points`` is uploaded once and clustered by
    ``spatial.cluster`` (DBSCAN; its docstring has the rules) with the mask's shape as the image -> ``spatial.ClusterTable``: the
    cluster number of every detection (-1: noise), ``n_clusters`` [1], and size, core count, centroid sums and bounding box of
    cluster c in row c of the tables.  Everything stays a device tensor, row i being ``result.points[i]``; nothing synchronises."""
    from . import spatial as Sp
    if not isinstance(result, SlideResult):
        raise TypeError("slide_clusters: expected the SlideResult of detect_slide")
    hw = tuple(int(v) for v in result.mask.shape)
    pts = np.asarray(result.points, np.int64).reshape(-1, 2)
    return Sp.cluster(torch.from_numpy(pts).to(result.mask.device), hw, eps, min_samples)


def _batch_points(points, n):
    """the annotations of a batch as the loader yields them -> a list of n [k, 2] arrays: a list of per-image arrays, or the
    [n, k, 2] tensor the default collate makes of equally long lists (batch size 1 in the reference)"""
    if isinstance(points, (list, tuple)):
        per = list(points)
    else:
        if points.ndim != 3:
            raise ValueError(f"evaluate_detection: expected annotations shaped [n, k, 2], got {tuple(points.shape)}")
        per = [points[i] for i in range(points.shape[0])]
    if len(per) != n:
        raise ValueError(f"evaluate_detection: {n} images but {len(per)} annotation arrays")
    return per


def evaluate_detection(loader, model, device, threshold=0.5, eps=11, reg_limit=False, method="gaussianblur", thr_for_dt=10,
                       min_object_size=300, hole_area_threshold=100, radius=16, **blur):
    """The evaluation loop of test_seg.py ``test()`` (:511-543) with its localisation block (:530-536) active, a batch at a time
    on the device.  The loader yields ``(images, masks, points, ...)`` as ``PointTestset`` does: masks uint8 0 / 255 [n, H, W],
    points a list of [k, 2] (x, y) arrays or one [n, k, 2] tensor.  Per batch: one segment-mode forward and softmax channel 1; the
    image-mode count rint(reg) (always, it is the ``count`` column; with reg_limit a count of 0 zeroes the map and the count caps
    the detection list); detect._detect and DetectResult.score against the annotations within ``radius``; ``> threshold``,
    remove_small_regions and dice_coef against ``mask / 255``.  Returns a dict of numpy arrays ``count, tp, fp, fn, p, r, f1,
    dice`` (the columns of center.csv) and ``mean`` = the averages (p, r, f1, dice) that ``MetricGroup.avg()`` prints.  The model
    is left in segment mode."""
    from . import detect as D
    from . import metrics as M
    from . import regions as Rg
    from . import score as S
    opts = _detect_options("evaluate_detection", eps, method, thr_for_dt, **blur)
    mo, ho = Rg._check_size(min_object_size, "min_object_size"), Rg._check_size(hole_area_threshold, "hole_area_threshold")
    S.radius_squared(radius)
    model.setmode("segment")
    model.eval()
    cols = {k: [] for k in ("count", "tp", "fp", "fn", "p", "r", "f1", "dice")}
    with torch.no_grad():
        for i, batch in enumerate(tqdm(loader, desc="testing")):
            images, masks, points = batch[0], batch[1], batch[2]
            x = images.to(device)
            probs, classes, reg = _cleaned_batch(model, x, threshold, mo, ho, True, reg_limit)       # the count column: always
            counts = reg.cpu().numpy().astype(int)
            sc = D._detect(probs, counts if reg_limit else None, opts).score(_batch_points(points, x.shape[0]), gt_xy=True, radius=radius)
            truth = torch.as_tensor(masks).to(device=device, dtype=torch.float32) / 255
            dice = M.dice_coef(classes.float(), truth.reshape(classes.shape))
            for k, v in zip(cols, (counts, sc.tp, sc.fp, sc.fn, sc.precision, sc.recall, sc.f1, dice.cpu().numpy().astype(np.float64))):
                cols[k].append(v)
    return _columns(cols, mean=("p", "r", "f1", "dice"))


def _columns(cols, **means):
    """the tail of the ``evaluate_*`` drivers: per-batch column pieces -> a dict of numpy arrays (empty float64 for an empty loader),
    plus under every name of ``means`` the tuple of the averages of the columns it lists (0.0 for an empty column)"""
    out = {k: (np.concatenate(v) if v else np.zeros((0,), np.float64)) for k, v in cols.items()}
    for name, keys in means.items():
        out[name] = tuple(float(out[k].mean()) if len(out[k]) else 0.0 for k in keys)
    return out


def evaluate_instances(loader, model, device, threshold=0.5, iou_threshold=0.5, eps=11, reg_limit=False, method="gaussianblur",
                       thr_for_dt=10, min_object_size=300, hole_area_threshold=100, connectivity=1, overlap=False, hausdorff=False,
                       geodesic=False, **blur):
    """The instance-level sibling of ``evaluate_detection``: every image's cells -- the cleaned segmentation split at the detected
    points -- against ground-truth instances, matched by IoU on the device (``regions.match_labels``).  The loader yields ``(images,
    masks, ...)``: masks uint8 0 / 255 [n, H, W], whose connected components (``regions.label(masks != 0, connectivity)``) are the
    truth instances, or int32 label images [n, H, W], used as they are.  Per batch: the body of ``segment_classes`` (with reg_limit
    a count of 0 zeroes the map); detect._detect on the probabilities (with reg_limit capped by the image-mode count, as in
    ``evaluate_detection``); ``regions.split`` of the cleaned classes at the device-resident detections; ``match_labels`` and
    ``MatchTable.score(iou_threshold)``.  Returns a dict of numpy arrays ``n_pred, n_truth, tp, fp, fn, p, r, f1, sq, pq`` (one
    entry per image) and ``mean`` = the averages (p, r, f1, sq, pq).  ``overlap=True`` also runs ``regions.overlap_labels`` on the
    same label pair and adds the columns ``aji`` and ``dice_obj`` (``score.overlap_score``) and ``mean_overlap`` = their averages
    (aji, dice_obj); without it nothing more is launched and the keys are the ones above.  ``hausdorff=True`` also runs
    ``regions.hausdorff_labels`` on the same label pair -- on the overlap tables of ``overlap=True`` where both are asked for, which
    are then made once -- and adds the column ``hausdorff_obj`` (``score.hausdorff_score``; ``inf`` for an image with objects on
    one side only), ``mean_hausdorff`` = its average over the images where it is finite (0.0 without one) and
    ``hausdorff_undefined`` = the number of the others; without it nothing more is launched either.  ``geodesic=True`` splits with
    ``regions.split_geodesic`` in its exact mode instead, so that every predicted cell is one connected piece; the keys are the
    same.  The model is left in segment mode."""
    from . import detect as D
    from . import regions as Rg
    from . import score as S
    opts = _detect_options("evaluate_instances", eps, method, thr_for_dt, **blur)
    mo, ho = Rg._check_size(min_object_size, "min_object_size"), Rg._check_size(hole_area_threshold, "hole_area_threshold")
    conn = Rg._check_connectivity(connectivity)
    S.check_iou_threshold(iou_threshold)
    model.setmode("segment")
    model.eval()
    names = {"n_pred": "n_pred", "n_truth": "n_truth", "tp": "tp", "fp": "fp", "fn": "fn", "p": "precision", "r": "recall", "f1": "f1",
             "sq": "sq", "pq": "pq"}
    cols = {k: [] for k in names}
    if overlap:
        cols.update(aji=[], dice_obj=[])
    if hausdorff:
        cols.update(hausdorff_obj=[])
    with torch.no_grad():
        for batch in tqdm(loader, desc="testing"):
            images, masks = batch[0], batch[1]
            probs, classes, reg = _cleaned_batch(model, images.to(device), threshold, mo, ho, reg_limit, reg_limit)
            parts = D._detect(probs, reg.cpu().numpy().astype(int) if reg_limit else None, opts).split(classes, connectivity=conn,
                                                                                                          geodesic=geodesic)
            truth = torch.as_tensor(masks)
            if truth.dtype == torch.uint8:
                truth = Rg.label(truth.to(device).reshape(classes.shape) != 0, conn)
            elif truth.dtype != torch.int32:
                raise TypeError(f"evaluate_instances: masks must be uint8 0 / 255 or int32 label images, got {truth.dtype}")
            sc = Rg.match_labels(parts.labels, truth.reshape(classes.shape), pred_counts=parts.counts).score(iou_threshold)
            for k, field in names.items():
                cols[k].append(getattr(sc, field))
            if overlap or hausdorff:
                table = Rg.overlap_labels(parts.labels, truth.reshape(classes.shape), pred_counts=parts.counts)
            if overlap:
                ov = table.score()
                cols["aji"].append(ov.aji)
                cols["dice_obj"].append(ov.dice_obj)
            if hausdorff:
                cols["hausdorff_obj"].append(Rg.hausdorff_labels(parts.labels, truth.reshape(classes.shape), overlap=table).score().hausdorff_obj)
    out = _columns(cols, mean=("p", "r", "f1", "sq", "pq"), **({"mean_overlap": ("aji", "dice_obj")} if overlap else {}))
    if hausdorff:
        finite = out["hausdorff_obj"][np.isfinite(out["hausdorff_obj"])]
        out["mean_hausdorff"] = float(finite.mean()) if len(finite) else 0.0
        out["hausdorff_undefined"] = int(len(out["hausdorff_obj"]) - len(finite))
    return out
