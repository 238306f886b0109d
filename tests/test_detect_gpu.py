"""Cell localisation on the GPU (csrc/detect.hip through cellsegmentation_amd.detect), bit-exact against the numpy restatement
tests/detect_ref.py: quantise, blur, mean shift, both clustering paths, order and cut, batching, stitching, repeatability and the
end-to-end inference.detect_cells on a random-weight ResNet-18."""
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

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden", "detect_vectors.npz")


def blobs(H, W, n, seed, radius=(3, 7)):
    """float32 probability map with n Gaussian-ish blobs (some on the borders)."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    p = np.zeros((H, W), np.float32)
    centres = list(zip(rng.randint(0, H, n), rng.randint(0, W, n))) + [(0, 0), (H - 1, W - 1), (0, W // 2)]
    for cy, cx in centres:
        r = rng.uniform(*radius)
        p = np.maximum(p, np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * r * r)).astype(np.float32))
    return p


def test_quantize_bit_exact(dev):
    rng = np.random.RandomState(1)
    k = np.arange(256, dtype=np.float32)
    below = np.nextafter((k / np.float32(255)).astype(np.float32), np.float32(0))
    p = np.concatenate([rng.rand(10001).astype(np.float32), below, k / np.float32(255), np.float32([0.0, 1.0, 1.0, 0.5])])
    got = D.quantize(torch.from_numpy(p).to(dev)).cpu().numpy()
    assert np.array_equal(got, R.quantize(p))
    q = D.quantize(torch.from_numpy(p[:7]).to(dev)).cpu().numpy()       # tail shorter than one 16-byte load
    assert np.array_equal(q, R.quantize(p[:7]))


@pytest.mark.parametrize("hw", [(299, 299), (512, 512), (17, 40), (64, 16), (5, 3), (130, 97)])
def test_blur_bit_exact(dev, hw):
    rng = np.random.RandomState(hw[0] * 7 + hw[1])
    u8 = rng.randint(0, 256, size=(3,) + hw).astype(np.uint8)
    u8[1] = 173                                                             # constant
    u8[2] = 0
    u8[2, hw[0] // 2, hw[1] // 2] = 255                                     # impulse
    got = D.gaussian_blur(torch.from_numpy(u8).to(dev), (15, 15), 3.).cpu().numpy()
    for n in range(3):
        assert np.array_equal(got[n], R.blur(u8[n])), n
    assert (got[1] == 173).all()
    # fused quantise + blur from fp32 probabilities, and a non-square kernel
    p = rng.rand(2, *hw).astype(np.float32)
    fused = K.detect_blur(torch.from_numpy(p).to(dev), D.gaussian_taps(15, 3.), D.gaussian_taps(15, 3.)).cpu().numpy()
    for n in range(2):
        assert np.array_equal(fused[n], R.blur(R.quantize(p[n])))
    g2 = D.gaussian_blur(u8[0], (5, 9), 1.2, 2.5).cpu().numpy()
    assert np.array_equal(g2, R.blur(u8[0], (5, 9), 1.2, 2.5))


@pytest.mark.parametrize("hw,thr,max_iter", [((299, 299), 0.2, 100), ((299, 299), -0.01, 100), ((512, 512), 0.2, 100),
                                             ((299, 299), 0.2, 2), ((40, 300), 0.1, 100)])
def test_meanshift_end_points(dev, hw, thr, max_iter):
    u8 = R.quantize(blobs(*hw, n=hw[0] * hw[1] // 1500, seed=hw[0]))
    u8[: hw[0] // 3, : hw[1] // 3] = 0                                      # empty corner: zero-mass windows when thr < 0
    b = R.blur(u8)
    pts, n_pts = K.detect_meanshift(torch.from_numpy(b[None]).to(dev), 10, 16, thr * 255.0, max_iter)
    corners = R.seeds(b, thr, 16, 10)
    assert int(n_pts[0]) == len(corners)
    want = R.meanshift(b, corners, 16, max_iter)
    assert np.array_equal(pts[0, :len(corners)].cpu().numpy().astype(np.int64), want)


def test_meanshift_iteration_counts(dev):
    """Windows between two blobs, stopped after 1, 2, 3, 7 and 100 steps: the GPU stops where the restatement stops.  (A 2-cycle,
    which must run all max_iter steps, was not found by a host search over small random images, so none is pinned here.)"""
    H, W = 64, 64
    u8 = np.zeros((H, W), np.uint8)
    u8[20:24, 4:8] = 255
    u8[20:24, 20:24] = 255
    for it in (1, 2, 3, 7, 100):
        pts, _ = K.detect_meanshift(torch.from_numpy(u8[None]).to(dev), 10, 16, -1.0, it)
        corners = R.seeds(u8, -1.0 / 255, 16, 10)
        want = R.meanshift(u8, corners, 16, it)
        assert np.array_equal(pts[0, :len(corners)].cpu().numpy().astype(np.int64), want), it


def _golden_sets():
    z = np.load(GOLDEN)
    o = z["offsets"]
    return [(z["points"][o[i]:o[i + 1]], float(z["eps"][i])) for i in range(len(o) - 1)]


@pytest.mark.parametrize("force_global", [False, True])
def test_clustering_designed_and_random_sets(dev, force_global):
    rng = np.random.RandomState(4)
    weights = rng.randint(0, 4, size=(2048, 2048)).astype(np.uint8)       # few levels: many ties, so the label order matters
    sets = [(p, e) for p, e in _golden_sets()] + [(rng.randint(0, 299, size=(900, 2)), 11.0), (np.zeros((0, 2), np.int64), 11.0)]
    for eps in sorted({e for _, e in sets}):
        group = [p for p, e in sets if e == eps]
        cap = max(1, max(len(p) for p in group))
        pts = np.zeros((len(group), cap, 2), np.int32)
        for i, p in enumerate(group):
            pts[i, :len(p)] = p
        n_pts = torch.tensor([len(p) for p in group], dtype=torch.int32, device=dev)
        bl = torch.from_numpy(np.repeat(weights[None], len(group), 0)).to(dev)
        out_pts, out_w, off = K.detect_cluster(torch.from_numpy(pts).to(dev), n_pts, eps, bl, force_global=force_global)
        off = off.cpu().numpy()
        out_pts, out_w = out_pts.cpu().numpy(), out_w.cpu().numpy()
        for i, p in enumerate(group):
            want_p, want_w = R.cluster(p, eps, weights)
            assert np.array_equal(out_pts[off[i]:off[i + 1]], want_p), (eps, i)
            assert np.array_equal(out_w[off[i]:off[i + 1]], want_w), (eps, i)


def test_meanshift_cluster_counts(dev):
    u8 = R.quantize(blobs(299, 299, 60, seed=3))
    full, _ = R.detect(u8, None, eps=11)
    assert len(full) > 5
    got, rest = D.meanshift_cluster(u8, "gaussianblur", None, eps=11, ksize=(15, 15), sigmaX=3.)
    assert rest == [] and got.dtype == np.int64 and got.shape == full.shape and np.array_equal(got, full)
    for c in (0, 3, len(full), 10 * len(full)):
        a, b = D.meanshift_cluster(torch.from_numpy(u8).to(dev), "gaussianblur", c, eps=11, ksize=(15, 15), sigmaX=3.)
        wa, wb = R.detect(u8, c, eps=11)
        assert np.array_equal(a, wa) and np.array_equal(b, wb) and a.shape[1:] == (2,) and b.shape[1:] == (2,)
    empty, _ = D.meanshift_cluster(np.zeros((64, 64), np.uint8), "gaussianblur", ksize=(15, 15), sigmaX=3.)
    assert empty.shape == (0, 2) and empty.dtype == np.int64


def test_batch_of_64_equals_single_calls_and_global_path(dev):
    maps = np.stack([R.quantize(blobs(299, 299, 20 + (i % 9) * 8, seed=100 + i)) for i in range(64)])
    counts = [i % 7 * 5 for i in range(64)]
    res = D.detect_points(torch.from_numpy(maps).to(dev), cell_counts=counts, eps=11)
    glob = D.detect_points(torch.from_numpy(maps[:8]).to(dev), cell_counts=counts[:8], eps=11, _force_global=True)
    per = res.per_image()
    for i in range(64):
        one = D.detect_points(maps[i], eps=11)
        want, w = R.detect(maps[i], None, eps=11, with_weights=True)
        pts_i = res.points[res.offsets[i]:res.offsets[i + 1]]
        assert np.array_equal(pts_i, one.points) and np.array_equal(pts_i, want[0]), i
        assert np.array_equal(res.weights[res.offsets[i]:res.offsets[i + 1]], w)
        assert np.array_equal(per[i][0], want[0][:counts[i]]) and np.array_equal(per[i][1], want[0][counts[i]:])
        assert res.n_kept[i] == len(R.seeds(R.blur(maps[i])))
        if i < 8:
            assert np.array_equal(glob.points[glob.offsets[i]:glob.offsets[i + 1]], pts_i)


def test_stitch_overlapping_patches(dev):
    rng = np.random.RandomState(8)
    ph = pw = 64
    grid = [(r, c) for r in (0, 48, 96, 136) for c in (0, 48, 96, 150, 186)]       # 16-px overlaps, border-aligned last ones
    patches = rng.randint(1, 256, size=(len(grid), ph, pw)).astype(np.uint8)
    hw = (210, 260)                                                                 # leaves an uncovered strip (zeros)
    got = D.stitch_patches(torch.from_numpy(patches).to(dev), grid, hw).cpu().numpy()
    assert np.array_equal(got, R.stitch(patches, grid, hw))
    with pytest.raises(ValueError):
        D.stitch_patches(patches[:1], [(200, 0)], hw)


def test_two_runs_identical(dev):
    maps = np.stack([R.quantize(blobs(512, 512, 150, seed=50 + i)) for i in range(4)])
    a = D.detect_points(maps, eps=11)
    b = D.detect_points(maps, eps=11)
    c = D.detect_points(maps, eps=11, _force_global=True)
    for x in (b, c):
        assert np.array_equal(a.points, x.points) and np.array_equal(a.weights, x.weights) and np.array_equal(a.offsets, x.offsets)


def test_detect_cells_end_to_end_resnet18(dev):
    from cellsegmentation_amd import inference, synth
    from cellsegmentation_amd.model import resnet as RN
    m = RN.MILresnet18()
    sd = m.state_dict()
    synth.fill_state_dict(sd)
    m.load_state_dict(sd)
    m = m.to(dev).set_compute_dtype(torch.float32)
    m.setmode("segment")
    x = synth.normalise(synth.ihc_tiles(16, 299, seed=21))
    loader = [x[:8], x[8:]]
    probs = inference.inference_seg(loader, m, dev, mode="test")
    got = inference.detect_cells(loader, m, dev, eps=11)
    assert len(got) == 16
    for i in range(16):
        want = R.detect(R.quantize(probs[i]), None, eps=11)
        assert np.array_equal(got[i][0], want[0]) and got[i][1] == [], i
    limited = inference.detect_cells(loader, m, dev, eps=11, reg_limit=True)
    assert m.mode == "segment"
    m.setmode("image")
    with torch.no_grad():
        reg = np.concatenate([np.round(m(b.to(dev))[1][:, 0].float().cpu().numpy()).astype(int) for b in loader])
    m.setmode("segment")
    for i in range(16):
        assert np.array_equal(limited[i][0], got[i][0][:reg[i]]) and np.array_equal(limited[i][1], got[i][0][reg[i]:])
