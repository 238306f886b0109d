"""Tissue detection on the GPU (csrc/tissue.hip): the four launches bit for bit against the numpy restatement tests/tissue_ref.py on
the pinned vectors and on shapes that take the kernels' other paths, and inference.detect_slide(tissue=...) against the loop
composed here from gather_tiles, the model and stitch_logits over the restatement's selected corners."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import tissue_ref as R  # noqa: E402
from shifted import shifted  # noqa: E402
from cellsegmentation_amd import detect as D  # noqa: E402
from cellsegmentation_amd import kernels as K  # noqa: E402
from cellsegmentation_amd import tiles, tissue  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(ROOT, "tests", "golden", "tissue_vectors.npz"), allow_pickle=False)
NAMES = [str(n) for n in GOLD["names"]]


@pytest.mark.parametrize("name", NAMES)
def test_pinned_cases_bit_equal(dev, name):
    images = GOLD[f"{name}.images"]
    size = GOLD[f"{name}.size"].tolist()
    size = size[0] if len(size) == 1 else tuple(size)
    ti, rc = GOLD[f"{name}.tile_img"], GOLD[f"{name}.tile_rc"]
    given = int(GOLD[f"{name}.given_threshold"]) if f"{name}.given_threshold" in GOLD.files else None
    batch = images if images.ndim == 4 else images[None]
    for c, ch in enumerate(R.CHANNELS):
        hist = tissue.histogram(images, ch)
        assert hist.is_cuda and hist.dtype == torch.int64 and np.array_equal(hist.cpu().numpy(), GOLD[f"{name}.hist"][c])
        assert np.array_equal(np.asarray(tissue.otsu(hist)), GOLD[f"{name}.thr"][c]) or given is not None
        m = tissue.mask(torch.from_numpy(images), given, ch)
        assert m.is_cuda and m.dtype == torch.uint8 and np.array_equal(m.cpu().numpy(), GOLD[f"{name}.mask"][c])
        cover = tissue.coverage(m, ti, rc, size)
        assert cover.dtype == torch.int32 and np.array_equal(cover.cpu().numpy(), GOLD[f"{name}.cover"][c])
        for k, need in enumerate(GOLD[f"{name}.needs"]):
            sel, n = K.tissue_select(cover, int(need))
            assert np.array_equal(sel.cpu().numpy(), GOLD[f"{name}.selected"][c, k]) and int(n) == GOLD[f"{name}.n_selected"][c, k]
        # the same images and masks at every kind of address: the single pixels before the first 16-byte boundary, the three stores
        thr = torch.from_numpy(np.atleast_1d(GOLD[f"{name}.thr"][c]).astype(np.int32)).to(dev)
        for shift_in, shift_out in ((1, 0), (7, 4), (12, 3), (0, 9)):
            x = shifted(batch, shift_in, dev)[0]
            assert np.array_equal(K.tissue_histogram(x, c).cpu().numpy(), np.atleast_2d(GOLD[f"{name}.hist"][c]))
            out = shifted(np.full(batch.shape[:3], 7, np.uint8), shift_out, dev)[0]
            assert K.tissue_mask(x, thr, c, out=out) is out
            assert np.array_equal(out.cpu().numpy().reshape(GOLD[f"{name}.mask"][c].shape), GOLD[f"{name}.mask"][c])
            got = K.tissue_coverage(out, torch.from_numpy(ti).to(dev), torch.from_numpy(rc).to(dev), *np.broadcast_to(GOLD[f"{name}.size"], (2,)).tolist())
            assert np.array_equal(got.cpu().numpy(), GOLD[f"{name}.cover"][c])


def _mixed(h, w, seed):
    """noise, a constant region and a run of one value that straddles rows: every path of the run counter"""
    rng = np.random.RandomState(seed)
    img = rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    img[h // 3:2 * h // 3] = (236, 228, 231)
    img[2 * h // 3:, : w // 2] = rng.randint(200, 204, size=(h - 2 * h // 3, w // 2, 1))
    return img


def test_several_workgroups_301x517(dev):
    img = _mixed(301, 517, 3)[None]
    x = torch.from_numpy(img).to(dev)
    for ch in R.CHANNELS:
        want = R.histogram(img, ch)
        assert want.sum() == 301 * 517
        assert np.array_equal(tissue.histogram(x, ch).cpu().numpy(), want)
        thr = R.otsu(want)
        assert np.array_equal(tissue.mask(x, None, ch).cpu().numpy(), R.mask(img, thr, ch))
        assert np.array_equal(tissue.mask(x, 128, ch).cpu().numpy(), R.mask(img, 128, ch))


def test_grid_cap_strides_over_a_large_image(dev):
    """2912 x 2903 pixels are more runs of 16 than the capped grid has threads: some threads take two, run carried over"""
    img = _mixed(2912, 2903, 4)
    assert img.size // 3 // 16 > 2048 * 256
    x = torch.from_numpy(img).to(dev)
    want = R.histogram(img, "chroma")
    assert np.array_equal(tissue.histogram(x, "chroma").cpu().numpy(), want)
    got = tissue.mask(x, 40, "chroma")
    assert np.array_equal(got.cpu().numpy(), R.mask(img, 40, "chroma"))
    corners = tiles.sample_patches(img.shape[:2], 299)
    ti = np.zeros(len(corners), np.int32)
    assert np.array_equal(tissue.coverage(got, ti, corners, 299).cpu().numpy(), R.coverage(got.cpu().numpy(), ti, corners, 299))


def test_constant_batch_counts_are_exact(dev):
    img = np.empty((3, 64, 64, 3), np.uint8)
    img[0], img[1], img[2] = (255, 255, 255), (200, 120, 90), (0, 0, 0)
    h = tissue.histogram(img, "chroma").cpu().numpy()
    assert h[0, 0] == 4096 and h[1, 110] == 4096 and h[2, 0] == 4096 and h.sum() == 3 * 4096
    h = tissue.histogram(img, "darkness").cpu().numpy()
    assert h[0, 0] == 4096 and h[2, 255] == 4096 and h.sum() == 3 * 4096 and np.array_equal(h, R.histogram(img, "darkness"))
    assert not tissue.mask(img).any()                                      # single-valued images: nothing is tissue
    assert tissue.mask(img, [-1, 109, 0]).cpu().numpy().reshape(3, -1).sum(axis=1).tolist() == [4096, 4096, 0]


def test_runs_repeat_and_the_histogram_accumulates(dev):
    img = _mixed(97, 131, 5)[None].repeat(2, axis=0)
    img[1] = img[1, ::-1]
    x = torch.from_numpy(img).to(dev)
    first = K.tissue_histogram(x, K.CS_TISSUE_CHROMA)
    for _ in range(3):
        assert torch.equal(K.tissue_histogram(x, K.CS_TISSUE_CHROMA), first)
    assert torch.equal(first[0], first[1]) and np.array_equal(first.cpu().numpy(), R.histogram(img, "chroma"))
    seed = torch.arange(512, dtype=torch.int64, device=dev).reshape(2, 256) * (1 << 33) + 5      # beyond 32 bits: 64-bit adds
    acc = seed.clone()
    assert K.tissue_histogram(x, K.CS_TISSUE_CHROMA, hist=acc) is acc and torch.equal(acc, seed + first)
    K.tissue_histogram(x, K.CS_TISSUE_CHROMA, hist=acc)
    assert torch.equal(acc, seed + 2 * first)
    thr = torch.tensor([30, 90], dtype=torch.int32, device=dev)
    m = K.tissue_mask(x, thr, K.CS_TISSUE_CHROMA)
    assert torch.equal(K.tissue_mask(x, thr, K.CS_TISSUE_CHROMA), m) and np.array_equal(m.cpu().numpy(), R.mask(img, [30, 90], "chroma"))


@pytest.mark.parametrize("T", [1, 255, 256, 257, 1000])
def test_select_at_the_chunk_boundaries(dev, T):
    rng = np.random.RandomState(T)
    for cover in (rng.randint(0, 100, T), np.zeros(T, np.int64), np.full(T, 50), np.arange(T) % 2 * 50, (np.arange(T) >= T - 1) * 50):
        cover = cover.astype(np.int32)
        sel, n = K.tissue_select(torch.from_numpy(cover).to(dev), 50)
        want, want_n = R.select(cover, 50)
        assert int(n) == want_n and np.array_equal(sel.cpu().numpy(), want)
    sel, n = K.tissue_select(torch.from_numpy(cover).to(dev), 0)
    assert int(n) == T and sel.cpu().tolist() == list(range(T))


def test_empty_tables_and_clamped_windows(dev):
    sel, n = K.tissue_select(torch.zeros((0,), dtype=torch.int32, device=dev), 0)
    assert sel.numel() == 0 and int(n) == 0
    m = (np.random.RandomState(6).randint(0, 3, size=(2, 23, 31)) * 100).astype(np.uint8)          # non-zero values other than 1 count once
    assert tissue.coverage(m, np.zeros(0, np.int32), np.zeros((0, 2), np.int32), 4).numel() == 0
    # device tables are not read back: windows that leave the image are clamped, an image index outside the batch counts 0
    ti = np.asarray([0, 1, 1, 0, 1, 2, -1, 0, 1], np.int32)
    rc = np.asarray([(-3, -2), (20, 28), (5, 29), (23, 0), (0, 31), (0, 0), (0, 0), (-9, 3), (-2 ** 31, 2 ** 31 - 1)], np.int32)
    for size in ((7, 5), (9, 9), (40, 40)):
        got = tissue.coverage(torch.from_numpy(m).to(dev), torch.from_numpy(ti).to(dev), torch.from_numpy(rc).to(dev), size)
        assert np.array_equal(got.cpu().numpy(), R.coverage(m, ti, rc, size))
    assert np.array_equal(tissue.coverage(m.astype(bool), [1], [(0, 0)], (23, 31)).cpu().numpy(), [np.count_nonzero(m[1])])


def test_clean_up_reuses_the_region_and_disk_passes(dev):
    from cellsegmentation_amd import morph, regions
    slide = R.blob_slide(seed=33)
    plain = tissue.select_patches(slide, 64, 48)
    opts = tissue.TissueOptions(opening_radius=1, min_object_size=12, hole_area_threshold=4, min_pixels=41)
    got = tissue.select_patches(slide, 64, 48, options=opts)
    want = regions.remove_small_regions(morph.binary_opening(plain.mask.bool(), 1, border_value=0), 12, 4)
    assert got.threshold == plain.threshold and torch.equal(got.mask.bool(), want) and not torch.equal(got.mask, plain.mask)
    corners = got.corners
    assert np.array_equal(got.coverage.cpu().numpy(), R.coverage(want.cpu().numpy(), np.zeros(len(corners), np.int32), corners, 64))


# ---- end to end -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(dev):
    from cellsegmentation_amd import synth
    from cellsegmentation_amd.model import resnet as RN
    m = RN.MILresnet18()
    sd = m.state_dict()
    synth.fill_state_dict(sd)
    m.load_state_dict(sd)
    return m.to(dev).set_compute_dtype(torch.float32)


def _composed(img, m, dev, corners, batch):
    """detect_slide's loop over the given corners, from the existing pieces"""
    H, W = img.shape[:2]
    rc = torch.from_numpy(np.asarray(corners, np.int32).reshape(-1, 2)).to(dev)
    d = torch.from_numpy(img).to(dev)[None]
    mask = torch.zeros((H, W), dtype=torch.uint8, device=dev)
    count = torch.zeros((), dtype=torch.float64, device=dev)
    m.eval()
    with torch.no_grad():
        for i in range(0, len(rc), batch):
            x = tiles.gather_tiles(d, np.zeros(len(rc[i:i + batch]), np.int32), rc[i:i + batch], 64, torch.float32)
            m.setmode("segment")
            K.stitch_logits(mask, m(x).float().contiguous(), rc[i:i + batch], 1)
            m.setmode("image")
            count += torch.round(m(x)[1][:, 0].float()).sum(dtype=torch.float64)
    m.setmode("segment")
    return mask, int(count.item())


@pytest.mark.parametrize("channel", R.CHANNELS)
def test_detect_slide_runs_the_tissue_patches_only(dev, model, channel):
    from cellsegmentation_amd import inference
    slide = R.blob_slide(seed=31)
    ref = R.select_patches(slide, 64, 48, channel, need=41)
    assert ref["corners"].tolist() == [[r, c] for r in (0, 48, 86) for c in (0, 48, 96, 106)]
    assert ref["selected"].tolist() == ([5, 6, 7, 9, 10, 11] if channel == "chroma" else [0, 5, 6, 7, 9, 10, 11])
    opts = tissue.TissueOptions(channel=channel)                            # min_fraction 0.01 of 64 x 64: 41 pixels
    assert opts.pixels(64, 64) == 41
    want_mask, want_count = _composed(slide, model, dev, ref["selected_corners"], 4)
    want = D.detect_points(want_mask, cell_counts=want_count, eps=11, thr=-0.01).per_image()[0]
    got = inference.detect_slide(slide, model, dev, batch_size=4, patch_size=64, interval=48, eps=11, thr=-0.01, tissue=opts)
    print(f"{channel}: {got.tissue.n_selected} of {len(got.tissue.corners)} patches, count {got.cell_count}, {len(got.points)} points")
    # (a) the composed loop
    assert torch.equal(got.mask, want_mask) and got.cell_count == want_count and model.mode == "segment" and not model.training
    assert np.array_equal(got.points, want[0]) and np.array_equal(got.discarded, want[1]) and len(want[0]) + len(want[1]) > 0
    # (e) the selection is the restatement's
    t = got.tissue
    assert isinstance(t, tissue.TissueResult) and t.n_selected == ref["n_selected"] and t.threshold == ref["threshold"] and t.min_pixels == 41
    assert np.array_equal(t.selected_corners, ref["selected_corners"]) and np.array_equal(t.selected.cpu().numpy(), ref["selected"])
    assert np.array_equal(t.corners, ref["corners"]) and np.array_equal(t.coverage.cpu().numpy(), ref["coverage"])
    assert t.mask.shape == (150, 170) and np.array_equal(t.mask.cpu().numpy(), ref["mask"])
    # (c) pixels that no selected patch covers stay 0
    covered = np.zeros((150, 170), bool)
    for r, c in ref["selected_corners"]:
        covered[r:r + 64, c:c + 64] = True
    assert not covered.all() and not got.mask.cpu().numpy()[~covered].any() and got.mask.any()
    # True is the default options; detect_slides passes the argument on
    if channel == "chroma":
        for again in (inference.detect_slide(slide, model, dev, batch_size=4, patch_size=64, interval=48, eps=11, thr=-0.01, tissue=True),
                      next(inference.detect_slides([slide], model, dev, batch_size=4, patch_size=64, interval=48, eps=11, thr=-0.01, tissue=opts))):
            assert torch.equal(again.mask, got.mask) and again.cell_count == got.cell_count and np.array_equal(again.points, got.points)
        alone = tissue.select_patches(slide, 64, 48, opts, dev)
        assert alone.n_selected == t.n_selected and torch.equal(alone.selected, t.selected) and torch.equal(alone.mask, t.mask)


def test_everything_selected_equals_no_selection(dev, model):
    from cellsegmentation_amd import inference
    slide = R.blob_slide(seed=31)
    kw = dict(batch_size=5, patch_size=64, interval=48, eps=11, thr=-0.01)
    plain = inference.detect_slide(slide, model, dev, **kw)
    every = inference.detect_slide(slide, model, dev, tissue=tissue.TissueOptions(min_pixels=0), **kw)
    assert plain.tissue is None and every.tissue.n_selected == 12 and every.tissue.selected.cpu().tolist() == list(range(12))
    assert torch.equal(every.mask, plain.mask) and every.cell_count == plain.cell_count                  # (b)
    assert np.array_equal(every.points, plain.points) and np.array_equal(every.discarded, plain.discarded)
    assert len(plain.points) + len(plain.discarded) > 0
    mask, count = _composed(slide, model, dev, tiles.sample_patches((150, 170), 64, 48), 5)              # and both are the parent's loop
    assert torch.equal(plain.mask, mask) and plain.cell_count == count


def test_a_white_slide_runs_no_patch(dev, model):
    from cellsegmentation_amd import inference
    white = np.full((150, 170, 3), 255, np.uint8)

    class Counting(torch.nn.Module):
        calls = 0
        mode, training, compute_dtype = "segment", False, torch.float32

        def setmode(self, mode):
            self.mode = mode

        def forward(self, x):
            Counting.calls += 1
            return model(x)

    got = inference.detect_slide(white, Counting(), dev, batch_size=4, patch_size=64, interval=48, eps=11, tissue=True)
    assert Counting.calls == 0                                             # (d): the loop does not run
    assert got.tissue.n_selected == 0 and got.tissue.selected.numel() == 0 and got.tissue.selected_corners.shape == (0, 2)
    assert got.tissue.threshold == 0 and not got.tissue.mask.any() and not got.tissue.coverage.any()
    assert got.cell_count == 0 and not got.mask.any() and len(got.points) == 0 and len(got.discarded) == 0
