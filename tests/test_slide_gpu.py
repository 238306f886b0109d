"""Whole-slide streaming on the GPU: detect.stitch_logits (csrc/detect.hip, one launch per batch of segment logits, ownership from the
corners alone) bit for bit against the resident path softmax_channel_fwd -> quantize -> stitch_patches and against the numpy
restatement tests/detect_ref.py, and inference.detect_slide against the same loop composed from the existing pieces."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import detect_ref as R  # noqa: E402
from cellsegmentation_amd import detect as D  # noqa: E402
from cellsegmentation_amd import kernels as K  # noqa: E402
from cellsegmentation_amd import tiles  # noqa: E402

pytestmark = pytest.mark.gpu


def _splits(n, sizes):
    assert sum(sizes) == n
    edges = np.cumsum([0] + list(sizes))
    return list(zip(edges[:-1].tolist(), edges[1:].tolist()))


def _streamed(logits, grid, hw, sizes, ch=1, fill=0):
    mask = torch.full(hw, fill, dtype=torch.uint8, device=logits.device)
    for s, e in _splits(len(grid), sizes):
        out = D.stitch_logits(mask, logits[s:e], grid[s:e], ch)
        assert out is mask
    return mask.cpu().numpy()


def _sequential(q, grid, hw, fill=0):
    """the reference's write order in numpy: whole_image_mask[r:r+ph, c:c+pw] = patch, one patch after the other"""
    out = np.full(hw, fill, np.uint8)
    ph, pw = q.shape[1:]
    for p, (r, c) in zip(q, grid):
        out[r:r + ph, c:c + pw] = p
    return out


class _Case:
    """logits on the device, and the resident path's result computed once: device probabilities, their quantisation, the stitch"""

    def __init__(self, dev, grid, hw, C, ph, pw, ch, seed):
        g = torch.Generator().manual_seed(seed)
        self.grid, self.hw, self.ch = grid, hw, ch
        self.logits = (4 * torch.randn((len(grid), C, ph, pw), generator=g)).to(dev)
        probs = K.softmax_channel_fwd(self.logits, ch)
        self.parent = D.stitch_patches(D.quantize(probs), grid, hw).cpu().numpy()
        self.numpy = R.stitch(R.quantize(probs.cpu().numpy()), grid, hw)


@pytest.fixture(scope="module")
def grid_case(dev):
    """the shape of test_stitch_overlapping_patches: 16-px overlaps, border-aligned last row and column, an uncovered strip"""
    grid = [(r, c) for r in (0, 48, 96, 136) for c in (0, 48, 96, 150, 186)]
    return _Case(dev, grid, (210, 260), 2, 64, 64, 1, seed=11)


@pytest.fixture(scope="module")
def odd_case(dev):
    """odd patch and mask sizes, odd corners, three channels: unaligned rows, byte tails, the general channel count"""
    grid = tiles.sample_patches((101, 131), (37, 53), (21, 37)) + [(1, 3), (7, 77), (63, 5), (33, 41), (64, 78), (11, 1), (5, 43)]
    return _Case(dev, grid, (101, 131), 3, 37, 53, 2, seed=12)


@pytest.mark.parametrize("sizes", [[20], [1] * 20, [3, 7, 10], [6, 6, 6, 2]])
def test_streamed_batches_equal_the_resident_stitch(grid_case, sizes):
    c = grid_case
    assert np.array_equal(c.parent, c.numpy)
    got = _streamed(c.logits, c.grid, c.hw, sizes)
    assert np.array_equal(got, c.parent)
    assert np.array_equal(got, c.numpy)
    assert (got[200:] == 0).all() and (got[:, 250:] == 0).all() and got.any()       # the uncovered strip stays zero


@pytest.mark.parametrize("sizes", [[27], [1] * 27, [4, 9, 14], [5, 5, 5, 5, 5, 2]])
def test_odd_shapes_three_channels(odd_case, sizes):
    c = odd_case
    assert len(c.grid) == 27 and np.array_equal(c.parent, c.numpy)
    got = _streamed(c.logits, c.grid, c.hw, sizes, ch=c.ch)
    assert np.array_equal(got, c.parent)
    assert np.array_equal(got, c.numpy)


def test_arbitrary_corners_in_one_batch(dev):
    """12 corners in ONE launch, random but for two identical pairs and one patch that four later ones cover between them: the
    sequential numpy write"""
    rng = np.random.RandomState(5)
    ph, pw, hw = 29, 43, (90, 120)
    grid = [(int(rng.randint(0, hw[0] - ph + 1)), int(rng.randint(0, hw[1] - pw + 1))) for _ in range(12)]
    grid[4] = grid[1]                                                        # the same corner twice: index 4 wins everywhere
    grid[11] = grid[7]
    grid[2], grid[5], grid[6], grid[8], grid[9] = (30, 40), (25, 30), (25, 45), (35, 30), (35, 45)   # patch 2 ends up with no pixel
    logits = (4 * torch.randn((12, 2, ph, pw), generator=torch.Generator().manual_seed(6))).to(dev)
    q = D.quantize(K.softmax_channel_fwd(logits, 1)).cpu().numpy()
    want = _sequential(q, grid, hw)
    got = _streamed(logits, grid, hw, [12])
    assert np.array_equal(got, want)
    assert np.array_equal(_streamed(logits, grid, hw, [1] * 12), want)
    other = q.copy()
    other[2] = 255 - q[2]
    assert np.array_equal(_sequential(other, grid, hw), want)                # ... so what it holds does not matter
    r, c = grid[11]
    assert np.array_equal(got[r:r + ph, c:c + pw], q[11]) and not np.array_equal(q[7], q[11])
    rev = _streamed(logits.flip(0).contiguous(), grid[::-1], hw, [12])       # the index decides, not the position
    assert np.array_equal(rev, _sequential(q[::-1], grid[::-1], hw))


def test_saturation_and_nan(dev):
    ph = pw = 8
    logits = torch.zeros((3, 2, ph, pw), dtype=torch.float32)
    logits[0, 1], logits[0, 0] = 40., -40.
    logits[1, 1], logits[1, 0] = -40., 40.
    logits[2] = torch.randn((2, ph, pw), generator=torch.Generator().manual_seed(7))
    logits[2, 1, 3, 4] = float("nan")
    logits[2, 0, 5, 6] = float("nan")
    logits = logits.to(dev)
    grid = [(0, 0), (0, 9), (9, 3)]
    got = _streamed(logits, grid, (20, 20), [3], fill=99)
    assert (got[0:8, 0:8] == 255).all() and (got[0:8, 9:17] == 0).all()
    want = D.quantize(K.softmax_channel_fwd(logits, 1)).cpu().numpy()       # a NaN logit: whatever quantize makes of the NaN probability
    assert np.array_equal(got[9:17, 3:11], want[2])
    assert got[8, 0] == 99 and got[0, 8] == 99


def test_mask_is_not_cleared_and_runs_repeat(grid_case):
    c = grid_case
    covered = _sequential(np.ones((20, 64, 64), np.uint8), c.grid, c.hw) == 1
    a = _streamed(c.logits, c.grid, c.hw, [6, 6, 6, 2], fill=7)
    assert (a[~covered] == 7).all() and (~covered).sum() == 210 * 260 - 200 * 250
    assert np.array_equal(a[covered], c.parent[covered])
    # a batch that covers part of the mask leaves the rest of an earlier result alone
    part = torch.from_numpy(c.parent).to(c.logits.device).clone()
    D.stitch_logits(part, c.logits[7:9].flip(1).contiguous(), c.grid[7:9])          # channels swapped: 1 - p
    part = part.cpu().numpy()
    touched = _sequential(np.ones((2, 64, 64), np.uint8), c.grid[7:9], c.hw) == 1
    assert np.array_equal(part[~touched], c.parent[~touched]) and not np.array_equal(part[touched], c.parent[touched])
    b = _streamed(c.logits, c.grid, c.hw, [6, 6, 6, 2], fill=7)
    assert np.array_equal(a, b)


def test_slide_sized_mask_needs_no_workspace(dev):
    """one batch of 16 patches of 299^2 into a 4096^2 mask: the peak rises by the corner table, not by an owner map (64 MiB in
    stitch_patches) or resident patches.  299-wide rows at these columns take the dword and the byte stores."""
    H = W = 4096
    grid = tiles.sample_patches((H, W))[14 * 15 + 10:14 * 15 + 15] + tiles.sample_patches((H, W))[:11]   # the end of the border-aligned last row, the start of the first
    assert len(grid) == 16
    logits = (4 * torch.randn((16, 2, 299, 299), generator=torch.Generator().manual_seed(8))).to(dev)
    mask = torch.zeros((H, W), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    D.stitch_logits(mask, logits, grid)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"peak rise of one stitch_logits call: {rise} bytes")
    assert rise <= 64 * 1024
    want = D.stitch_patches(D.quantize(K.softmax_channel_fwd(logits, 1)), grid, (H, W))
    assert torch.equal(mask, want)


def test_offsets_past_2_31(dev):
    """a mask of more than 2^31 pixels: the patches at its far end are addressed with 64-bit offsets"""
    H = W = 46400
    assert H * W > 1 << 31
    mask = torch.zeros((H, W), dtype=torch.uint8, device=dev)
    ph, pw = 21, 30
    grid = [(H - ph, W - pw), (H - ph - 10, W - pw - 17), (H - 2 * ph, 5), (46340, 46341)]
    logits = (4 * torch.randn((4, 2, ph, pw), generator=torch.Generator().manual_seed(9))).to(dev)
    D.stitch_logits(mask, logits, grid)
    q = D.quantize(K.softmax_channel_fwd(logits, 1)).cpu().numpy()
    r0 = H - 64
    want = np.zeros((64, W), np.uint8)
    for p, (r, c) in zip(q, grid):
        want[r - r0:r - r0 + ph, c:c + pw] = p
    assert np.array_equal(mask[r0:].cpu().numpy(), want)
    assert int(torch.count_nonzero(mask[:r0])) == 0                          # nothing wrapped round to the front of the mask


def _blob_slide(H, W, seed):
    """uint8 [H, W, 3]: dark Gaussian blobs on a light ground, a little different per channel"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    p = np.zeros((H, W), np.float32)
    for cy, cx in zip(rng.randint(0, H, 14), rng.randint(0, W, 14)):
        r = rng.uniform(3, 7)
        p = np.maximum(p, np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * r * r)).astype(np.float32))
    img = np.stack([235 - 150 * p, 225 - 170 * p, 230 - 90 * p], -1) + rng.randint(-6, 7, size=(H, W, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def _composed(img, m, dev, batch):
    """cell_detect's loop from the existing pieces, with detect_slide's batch boundaries"""
    H, W = img.shape[:2]
    corners = tiles.sample_patches((H, W), 64, 48)
    rc = np.asarray(corners, dtype=np.int32)
    d = torch.from_numpy(img).to(dev)[None]
    probs, count = [], torch.zeros((), dtype=torch.float64, device=dev)
    m.eval()
    with torch.no_grad():
        for i in range(0, len(rc), batch):
            x = tiles.gather_tiles(d, np.zeros(len(rc[i:i + batch]), np.int32), rc[i:i + batch], 64, torch.float32)
            m.setmode("segment")
            probs.append(K.softmax_channel_fwd(m(x).contiguous(), 1))
            m.setmode("image")
            count += torch.round(m(x)[1][:, 0].float()).sum(dtype=torch.float64)
    m.setmode("segment")
    mask = D.stitch_patches(D.quantize(torch.cat(probs)), corners, (H, W))
    return corners, mask, int(count.item())


def test_detect_slide_end_to_end_resnet18(dev):
    from cellsegmentation_amd import inference, synth
    from cellsegmentation_amd.model import resnet as RN
    m = RN.MILresnet18()
    sd = m.state_dict()
    synth.fill_state_dict(sd)
    m.load_state_dict(sd)
    m = m.to(dev).set_compute_dtype(torch.float32)
    m.setmode("image")
    m.train()
    slides = [_blob_slide(150, 170, 31), _blob_slide(150, 170, 32)]
    corners, mask, count = _composed(slides[0], m, dev, 5)
    assert corners == [(r, c) for r in (0, 48, 86) for c in (0, 48, 96, 106)]       # batches of 5, 5 and 2 cut rows of four
    want = {lim: D.detect_points(mask, cell_counts=count if lim else None, eps=11).per_image()[0] for lim in (True, False)}
    print(f"count {count}, {len(want[False][0])} cells, mask max {int(mask.max())}")
    m.setmode("image")
    m.train()
    for lim in (True, False):
        got = inference.detect_slide(slides[0], m, dev, batch_size=5, patch_size=64, interval=48, eps=11, reg_limit=lim)
        assert isinstance(got, inference.SlideResult) and m.mode == "segment" and not m.training
        assert got.mask.is_cuda and got.mask.dtype == torch.uint8 and torch.equal(got.mask, mask)
        assert got.cell_count == count
        assert got.points.dtype == np.int64 and np.array_equal(got.points, want[lim][0])
        if lim:
            assert np.array_equal(got.discarded, want[lim][1]) and len(got.points) + len(got.discarded) == len(want[False][0])
        else:
            assert got.discarded == []
    # every seed window kept (thr < 0), so that the point lists are not empty whatever the random weights make of the slide
    every = D.detect_points(mask, cell_counts=count, eps=11, thr=-0.01).per_image()[0]
    got = inference.detect_slide(slides[0], m, dev, batch_size=5, patch_size=64, interval=48, eps=11, thr=-0.01)
    print(f"thr -0.01: {len(every[0])} kept, {len(every[1])} discarded")
    assert len(every[0]) + len(every[1]) > 0
    assert np.array_equal(got.points, every[0]) and np.array_equal(got.discarded, every[1]) and torch.equal(got.mask, mask)
    default = inference.detect_slide(torch.from_numpy(slides[0]), m, batch_size=5, patch_size=64, interval=48)   # caps by default
    assert np.array_equal(default.points, want[True][0]) and np.array_equal(default.discarded, want[True][1])
    one = inference.detect_slide(slides[0], m, dev, batch_size=12, patch_size=64, interval=48)   # other boundaries, the same mask
    assert torch.equal(one.mask, mask)
    gen = inference.detect_slides(slides, m, dev, batch_size=5, patch_size=64, interval=48, eps=11)
    both = list(gen)
    assert len(both) == 2
    for img, got in zip(slides, both):
        single = inference.detect_slide(img, m, dev, batch_size=5, patch_size=64, interval=48, eps=11)
        assert torch.equal(got.mask, single.mask) and got.cell_count == single.cell_count
        assert np.array_equal(got.points, single.points) and np.array_equal(got.discarded, single.discarded)
    assert torch.equal(both[0].mask, mask) and not torch.equal(both[1].mask, mask)
    assert m.mode == "segment"
