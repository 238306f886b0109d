"""Blended whole-slide stitching on the GPU: detect.StitchBlend (csrc/detect.hip: stitch_blend_add_kernel, one launch per batch, the
lowest covering patch of the batch owning a pixel's update; stitch_blend_finish_kernel) bit for bit against the numpy restatement
tests/blend_ref.py applied to K.softmax_channel_fwd of the same logits, and inference.detect_slide(blend=, tta=) against the same
loop composed from the existing pieces.  Every comparison is array_equal."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import blend_ref as BR  # noqa: E402
from cellsegmentation_amd import augment  # noqa: E402
from cellsegmentation_amd import detect as D  # noqa: E402
from cellsegmentation_amd import kernels as K  # noqa: E402
from cellsegmentation_amd import tiles  # noqa: E402

pytestmark = pytest.mark.gpu


def _splits(n, sizes):
    assert sum(sizes) == n
    edges = np.cumsum([0] + list(sizes))
    return list(zip(edges[:-1].tolist(), edges[1:].tolist()))


def _blended(logits, grid, hw, sizes, ch=1, window="linear", flips=None):
    sb = D.StitchBlend(hw, logits.shape[-2:], window, device=logits.device)
    for s, e in _splits(len(grid), sizes):
        assert sb.add(logits[s:e], grid[s:e], None if flips is None else flips[s:e], ch) is sb
    assert sb.n_added == len(grid)
    return sb.finish().cpu().numpy()


def _cover(grid, hw, ph, pw):
    n = np.zeros(hw, np.int64)
    for r, c in grid:
        n[r:r + ph, c:c + pw] += 1
    return n


class _Case:
    """logits on the device and their probabilities on the host, computed once"""

    def __init__(self, dev, grid, hw, C, ph, pw, ch, seed):
        g = torch.Generator().manual_seed(seed)
        self.grid, self.hw, self.ch, self.patch = grid, hw, ch, (ph, pw)
        self.logits = (4 * torch.randn((len(grid), C, ph, pw), generator=g)).to(dev)
        self.probs = K.softmax_channel_fwd(self.logits, ch).cpu().numpy()
        self.want = {w: BR.blend(self.probs, grid, hw, None, BR.taps(ph, w), BR.taps(pw, w)) for w in ("linear", "uniform")}


@pytest.fixture(scope="module")
def grid_case(dev):
    """the 20-patch grid of test_slide_gpu.py: 16-px overlaps, border-aligned last row and column, an uncovered strip"""
    grid = [(r, c) for r in (0, 48, 96, 136) for c in (0, 48, 96, 150, 186)]
    return _Case(dev, grid, (210, 260), 2, 64, 64, 1, seed=11)


@pytest.fixture(scope="module")
def odd_case(dev):
    """the 27-patch odd case of test_slide_gpu.py: odd patch and mask sizes, odd corners, three channels"""
    grid = tiles.sample_patches((101, 131), (37, 53), (21, 37)) + [(1, 3), (7, 77), (63, 5), (33, 41), (64, 78), (11, 1), (5, 43)]
    return _Case(dev, grid, (101, 131), 3, 37, 53, 2, seed=12)


def _every_split_and_order(c, window, splits):
    want = c.want[window]
    rev_logits, rev_grid = c.logits.flip(0).contiguous(), c.grid[::-1]
    for sizes in splits:
        assert np.array_equal(_blended(c.logits, c.grid, c.hw, sizes, c.ch, window), want), sizes
        assert np.array_equal(_blended(rev_logits, rev_grid, c.hw, sizes, c.ch, window), want), ("reversed", sizes)
    return want


@pytest.mark.parametrize("window", ["linear", "uniform"])
def test_grid_any_split_any_order(grid_case, window):
    want = _every_split_and_order(grid_case, window, [[20], [1] * 20, [3, 7, 10], [6, 6, 6, 2]])
    assert (want[200:] == 0).all() and (want[:, 250:] == 0).all() and want.any()       # the uncovered strip is zero


@pytest.mark.parametrize("window", ["linear", "uniform"])
def test_odd_shapes_three_channels_any_split_any_order(odd_case, window):
    assert len(odd_case.grid) == 27
    _every_split_and_order(odd_case, window, [[27], [1] * 27, [4, 9, 14], [5, 5, 5, 5, 5, 2]])


def test_the_windows_differ_and_blend(grid_case):
    c = grid_case
    n = _cover(c.grid, c.hw, 64, 64)
    assert not np.array_equal(c.want["linear"][n > 1], c.want["uniform"][n > 1])
    assert np.array_equal(c.want["linear"][n == 1], c.want["uniform"][n == 1])


def test_single_cover_is_the_streamed_stitch(grid_case):
    c = grid_case
    apart = [0, 2, 4, 10, 12, 14]                                            # corners 96 px apart: nothing overlaps
    grid = [c.grid[i] for i in apart]
    assert _cover(grid, c.hw, 64, 64).max() == 1
    logits = c.logits[apart].contiguous()
    streamed = D.stitch_logits(torch.zeros(c.hw, dtype=torch.uint8, device=logits.device), logits, grid).cpu().numpy()
    for window in ("linear", "uniform"):
        assert np.array_equal(_blended(logits, grid, c.hw, [6], 1, window), streamed)
        assert np.array_equal(_blended(logits, grid, c.hw, [2, 4], 1, window), streamed)
    # on the overlapping grid: the pixels that one patch covers hold the bytes stitch_logits writes
    streamed = D.stitch_logits(torch.zeros(c.hw, dtype=torch.uint8, device=logits.device), c.logits, c.grid).cpu().numpy()
    once = _cover(c.grid, c.hw, 64, 64) == 1
    assert once.sum() > 10000
    got = _blended(c.logits, c.grid, c.hw, [20])
    assert np.array_equal(got[once], streamed[once]) and not np.array_equal(got[~once], streamed[~once])


def test_flipped_views_land_where_they_belong(odd_case):
    c = odd_case
    ph, pw = c.patch
    tr, tc = np.arange(1, ph + 1), (np.arange(pw) * 7) % 255 + 1           # asymmetric taps: a view put back wrongly changes the bytes
    M = 6
    logits, grid = c.logits[:M].contiguous(), c.grid[:M]
    views = torch.cat([logits, logits.flip(-1), logits.flip(-2), logits.flip(-2, -1)]).contiguous()
    codes = [0] * M + [1] * M + [2] * M + [3] * M
    base = BR.blend(c.probs[:M], grid, c.hw, None, tr, tc)
    probs = K.softmax_channel_fwd(views, c.ch).cpu().numpy()
    assert np.array_equal(BR.blend(probs, grid * 4, c.hw, codes, tr, tc), base)

    def run(flips, sizes, device_flips=False):
        sb = D.StitchBlend(c.hw, (ph, pw), window=(tr, tc), device=views.device)
        for s, e in _splits(4 * M, sizes):
            fl = flips[s:e]
            sb.add(views[s:e], grid4[s:e], torch.tensor(fl, dtype=torch.uint8, device=views.device) if device_flips else fl, c.ch)
        return sb.finish().cpu().numpy()

    grid4 = grid * 4
    assert np.array_equal(run(codes, [4 * M]), base)                         # one launch: the same corner four times, four codes
    assert np.array_equal(run(codes, [M] * 4), base)                         # a launch per view
    assert np.array_equal(run(codes, [5, 7, 1, 11], device_flips=True), base)
    assert not np.array_equal(run([0] * (4 * M), [4 * M]), base)             # without the codes the flipped views land mirrored
    alone = D.StitchBlend(c.hw, (ph, pw), window=(tr, tc), device=views.device).add(logits, grid, None, c.ch).finish().cpu().numpy()
    assert np.array_equal(alone, base)
    one_shot = D.stitch_blend(views, grid4, c.hw, flips=codes, ch=c.ch, window=(tr, tc))
    assert one_shot.is_cuda and one_shot.dtype == torch.uint8 and np.array_equal(one_shot.cpu().numpy(), base)


def test_arbitrary_corners_in_one_batch(dev):
    """the 12 corners of test_slide_gpu.py in ONE launch: two identical pairs, one patch that four others cover between them"""
    rng = np.random.RandomState(5)
    ph, pw, hw = 29, 43, (90, 120)
    grid = [(int(rng.randint(0, hw[0] - ph + 1)), int(rng.randint(0, hw[1] - pw + 1))) for _ in range(12)]
    grid[4] = grid[1]
    grid[11] = grid[7]
    grid[2], grid[5], grid[6], grid[8], grid[9] = (30, 40), (25, 30), (25, 45), (35, 30), (35, 45)
    logits = (4 * torch.randn((12, 2, ph, pw), generator=torch.Generator().manual_seed(6))).to(dev)
    probs = K.softmax_channel_fwd(logits, 1).cpu().numpy()
    for window in ("linear", "uniform"):
        want = BR.blend(probs, grid, hw, None, BR.taps(ph, window), BR.taps(pw, window))
        assert np.array_equal(_blended(logits, grid, hw, [12], 1, window), want)
        assert np.array_equal(_blended(logits, grid, hw, [1] * 12, 1, window), want)
    assert _cover(grid, hw, ph, pw).max() >= 5
    dcorners = torch.tensor(grid, dtype=torch.int32, device=dev)             # corners already on the device: taken as they are
    sb = D.StitchBlend(hw, (ph, pw), device=dev).add(logits, dcorners)
    assert np.array_equal(sb.finish().cpu().numpy(), BR.blend(probs, grid, hw, None, BR.taps(ph), BR.taps(pw)))


def test_accumulator_width_saturation_and_nan(dev):
    ph = pw = 8
    full = ([255] * ph, [255] * pw)
    one = torch.zeros((80, 2, ph, pw), dtype=torch.float32)
    one[:, 1], one[:, 0] = 40., -40.                                         # p == 1 in fp32
    grid = [(3, 5)] * 80
    for logits, value in ((one, 255), (one.flip(1).contiguous(), 0)):
        sb = D.StitchBlend((20, 20), (ph, pw), window=full, device=dev).add(logits.to(dev), grid)
        got = sb.finish().cpu().numpy()
        assert (got[3:11, 5:13] == value).all() and got.sum() == value * 64
        assert int(sb.den.max()) == 80 * 255 * 255
        if value:
            assert int(sb.num.max()) == 80 * 255 * 255 * 65280 > 1 << 32     # the sum needs its 64 bits
    # a NaN logit: that patch's level is 0 at the pixel, its weight still counts
    logits = torch.zeros((3, 2, ph, pw), dtype=torch.float32)
    logits[:2, 1], logits[:2, 0] = 40., -40.
    logits[2] = torch.randn((2, ph, pw), generator=torch.Generator().manual_seed(7))
    logits[1, 1, 3, 4] = float("nan")
    logits[2, 0, 5, 6] = float("nan")
    logits = logits.to(dev)
    grid = [(0, 0), (0, 0), (9, 3)]
    probs = K.softmax_channel_fwd(logits, 1).cpu().numpy()
    assert np.isnan(probs[1, 3, 4]) and np.isnan(probs[2, 5, 6])
    got = D.StitchBlend((20, 20), (ph, pw), window=full, device=dev).add(logits, grid).finish().cpu().numpy()
    assert np.array_equal(got, BR.blend(probs, grid, (20, 20), None, *full))
    assert got[3, 4] == 127 and got[3, 5] == 255 and got[9 + 5, 3 + 6] == 0


def test_finish_reset_and_the_overflow_guard(grid_case):
    c = grid_case
    dev = c.logits.device
    sb = D.StitchBlend(c.hw, (64, 64), device=dev)
    sb.add(c.logits[:8], c.grid[:8])
    first = sb.finish()
    want8 = BR.blend(c.probs[:8], c.grid[:8], c.hw, None, BR.taps(64), BR.taps(64))
    assert np.array_equal(first.cpu().numpy(), want8) and torch.equal(sb.finish(), first)       # finish only reads
    out = torch.full(c.hw, 9, dtype=torch.uint8, device=dev)
    assert sb.finish(out=out) is out and torch.equal(out, first)
    sb.add(c.logits[8:], c.grid[8:])                                         # add after finish continues the sums
    assert np.array_equal(sb.finish().cpu().numpy(), c.want["linear"]) and sb.n_added == 20
    assert sb.reset() is sb and sb.n_added == 0 and int(sb.den.max()) == 0 and int(sb.num.max()) == 0
    assert int(sb.finish().max()) == 0
    assert np.array_equal(sb.add(c.logits[:8], c.grid[:8]).finish().cpu().numpy(), want8)
    # the den bound is kept on the host: it raises before anything is enqueued
    sb.n_added = (1 << 31) // (32 * 32) - 2
    sb.add(c.logits[:1], c.grid[:1])
    before = (sb.num.clone(), sb.den.clone())
    with pytest.raises(OverflowError):
        sb.add(c.logits[:1], c.grid[:1])
    assert torch.equal(sb.num, before[0]) and torch.equal(sb.den, before[1])


@pytest.mark.parametrize("offset", [0, 1])
def test_finish_is_the_floor_division(dev, offset):
    """stitch_blend_finish on accumulators written here: quotients at either side of every byte step, the largest den, den == 0;
    offset 1 moves the buffers off their 16-byte alignment (the element-by-element path), 37 x 23 pixels leave a tail."""
    H, W = 37, 23
    rng = np.random.RandomState(21)
    den = rng.randint(1, 1 << 31, size=H * W).astype(np.int64)
    den[:5] = [1, 2, (1 << 31) - 1, 255 * 255, 0]
    byte = rng.randint(0, 256, size=H * W).astype(np.int64)
    num = byte * 256 * den + rng.choice([-1, 0, 1], size=H * W) * (byte > 0)                 # one below a step: the byte before
    num = np.minimum(np.maximum(num, 0), 255 * 256 * den)
    num[4] = 12345                                                                            # den == 0: the byte is 0 whatever num holds
    want = BR.finish(num.reshape(H, W), den.reshape(H, W))
    assert want.ravel()[4] == 0 and want.min() == 0 and want.max() == 255 and len(np.unique(want)) > 200
    nbuf, dbuf = torch.zeros(H * W + 1, dtype=torch.int64, device=dev), torch.zeros(H * W + 1, dtype=torch.int32, device=dev)
    nbuf[offset:offset + H * W] = torch.from_numpy(num).to(dev)
    dbuf[offset:offset + H * W] = torch.from_numpy(den.astype(np.int32)).to(dev)
    got = K.stitch_blend_finish(nbuf[offset:offset + H * W].view(H, W), dbuf[offset:offset + H * W].view(H, W))
    assert np.array_equal(got.cpu().numpy(), want)


def _blob_slide(H, W, seed):
    """uint8 [H, W, 3]: dark Gaussian blobs on a light ground, a little different per channel (as in test_slide_gpu.py)"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    p = np.zeros((H, W), np.float32)
    for cy, cx in zip(rng.randint(0, H, 14), rng.randint(0, W, 14)):
        r = rng.uniform(3, 7)
        p = np.maximum(p, np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * r * r)).astype(np.float32))
    img = np.stack([235 - 150 * p, 225 - 170 * p, 230 - 90 * p], -1) + rng.randint(-6, 7, size=(H, W, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def _composed(img, m, dev, batch, codes):
    """the loop from the existing pieces with detect_slide's batch boundaries -> (corners, {code: probs [M, 64, 64] on the host},
    count of the un-flipped view)"""
    H, W = img.shape[:2]
    corners = tiles.sample_patches((H, W), 64, 48)
    rc = np.asarray(corners, dtype=np.int32)
    d = torch.from_numpy(img).to(dev)[None]
    probs, count = {c: [] for c in codes}, torch.zeros((), dtype=torch.float64, device=dev)
    m.eval()
    with torch.no_grad():
        for i in range(0, len(rc), batch):
            brc = rc[i:i + batch]
            zeros = np.zeros(len(brc), np.int32)
            for code in codes:
                if code:
                    x = augment.stage_tiles(d, zeros, brc, 64, flips=np.full(len(brc), code), dtype=torch.float32)
                else:
                    x = tiles.gather_tiles(d, zeros, brc, 64, torch.float32)
                m.setmode("segment")
                probs[code].append(K.softmax_channel_fwd(m(x).contiguous(), 1).cpu().numpy())
                if not code:
                    m.setmode("image")
                    count += torch.round(m(x)[1][:, 0].float()).sum(dtype=torch.float64)
    m.setmode("segment")
    return corners, {c: np.concatenate(p) for c, p in probs.items()}, int(count.item())


def test_detect_slide_blend_and_tta_end_to_end_resnet18(dev):
    from cellsegmentation_amd import inference, synth
    from cellsegmentation_amd.model import resnet as RN
    m = RN.MILresnet18()
    sd = m.state_dict()
    synth.fill_state_dict(sd)
    m.load_state_dict(sd)
    m = m.to(dev).set_compute_dtype(torch.float32)
    slide = _blob_slide(150, 170, 31)
    hw, t64 = (150, 170), BR.taps(64)
    kw = dict(patch_size=64, interval=48, eps=11)
    corners, probs, count = _composed(slide, m, dev, 5, (0, 1, 2, 3))
    assert corners == [(r, c) for r in (0, 48, 86) for c in (0, 48, 96, 106)]
    # blend=None: the mask it always was
    plain = D.stitch_patches(D.quantize(torch.from_numpy(probs[0]).to(dev)), corners, hw)
    got = inference.detect_slide(slide, m, dev, batch_size=5, **kw)
    assert torch.equal(got.mask, plain) and got.cell_count == count
    # blend=True against the composition; the points are detect_points of that mask with the same count
    want = BR.blend(probs[0], corners, hw, None, t64, t64)
    assert not np.array_equal(want, plain.cpu().numpy())
    m.setmode("image")
    m.train()
    got = inference.detect_slide(slide, m, dev, batch_size=5, blend=True, thr=-0.01, **kw)
    assert isinstance(got, inference.SlideResult) and m.mode == "segment" and not m.training
    assert got.mask.is_cuda and got.mask.dtype == torch.uint8 and np.array_equal(got.mask.cpu().numpy(), want)
    assert got.cell_count == count
    pts = D.detect_points(torch.from_numpy(want).to(dev), cell_counts=count, eps=11, thr=-0.01).per_image()[0]
    assert len(pts[0]) + len(pts[1]) > 0
    assert np.array_equal(got.points, pts[0]) and np.array_equal(got.discarded, pts[1])
    for batch in (5, 12):                                                    # other boundaries, the same bytes
        assert np.array_equal(inference.detect_slide(slide, m, dev, batch_size=batch, blend=True, **kw).mask.cpu().numpy(), want)
    assert np.array_equal(inference.detect_slide(slide, m, dev, batch_size=5, blend="linear", **kw).mask.cpu().numpy(), want)
    uni = inference.detect_slide(slide, m, dev, batch_size=5, blend={"window": "uniform"}, **kw)
    assert np.array_equal(uni.mask.cpu().numpy(), BR.blend(probs[0], corners, hw, None, BR.taps(64, "uniform"), BR.taps(64, "uniform")))
    r16 = inference.detect_slide(slide, m, dev, batch_size=5, blend={"ramp": 16}, **kw)
    assert np.array_equal(r16.mask.cpu().numpy(), BR.blend(probs[0], corners, hw, None, BR.taps(64, ramp=16), BR.taps(64, ramp=16)))
    # four views
    codes = (0, 1, 2, 3)
    allp = np.concatenate([probs[c] for c in codes])
    flips = [c for c in codes for _ in corners]
    want4 = BR.blend(allp, corners * 4, hw, flips, t64, t64)
    assert not np.array_equal(want4, want)
    for batch in (5, 12):
        got4 = inference.detect_slide(slide, m, dev, batch_size=batch, tta=codes, **kw)     # tta alone turns blending on
        assert np.array_equal(got4.mask.cpu().numpy(), want4) and got4.cell_count == count
    two = inference.detect_slide(slide, m, dev, batch_size=5, blend=True, tta=(2, 0), **kw)
    assert np.array_equal(two.mask.cpu().numpy(), BR.blend(np.concatenate([probs[0], probs[2]]), corners * 2, hw,
                                                           [0] * 12 + [2] * 12, t64, t64))
    assert two.cell_count == count
    every = list(inference.detect_slides([slide], m, dev, batch_size=5, tta=codes, **kw))
    assert len(every) == 1 and np.array_equal(every[0].mask.cpu().numpy(), want4)
    assert m.mode == "segment"
