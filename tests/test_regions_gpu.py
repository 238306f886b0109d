"""Small-region clean-up on the GPU (csrc/regions.hip through cellsegmentation_amd.regions), exact against the numpy restatement
tests/regions_ref.py: degenerate and ragged sizes, components across tile edges and corners (tiles are 64 x 64), long union
chains, the strict area bounds, border pockets, objects inside holes, batches, in-place, repeatability, graph replay, the
float32 threshold, the HSV gate / preprocess_masks and the end-to-end inference.segment_classes."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import regions_ref as R  # noqa: E402
from cellsegmentation_amd import kernels as K  # noqa: E402
from cellsegmentation_amd import regions as G  # noqa: E402
from cellsegmentation_amd import stage  # noqa: E402

pytestmark = pytest.mark.gpu
TILE = 64


def _np(t):
    return t.cpu().numpy()


def check_all(m, connectivity, sizes=((3, 2),)):
    """label, areas, both filters and the fused call of m ([H,W] or [N,H,W] bool numpy) against the restatement"""
    lab = _np(G.label(m, connectivity))
    assert lab.dtype == np.int32 and np.array_equal(lab, R.batched(R.label, m, connectivity))
    assert np.array_equal(_np(G.component_areas(m, connectivity)), R.batched(R.component_areas, m, connectivity))
    for mo, ho in sizes:
        assert np.array_equal(_np(G.remove_small_objects(m, mo, connectivity)), R.batched(R.remove_small_objects, m, mo, connectivity))
        assert np.array_equal(_np(G.remove_small_holes(m, ho, connectivity)), R.batched(R.remove_small_holes, m, ho, connectivity))
        got = G.remove_small_regions(m, mo, ho, connectivity)
        assert got.dtype == torch.bool and got.is_cuda and tuple(got.shape) == m.shape
        assert np.array_equal(_np(got), R.batched(R.remove_small_regions, m, mo, ho, connectivity))


@pytest.mark.parametrize("connectivity", [1, 2])
@pytest.mark.parametrize("hw", [(1, 1), (1, 37), (41, 1), (5, 3), (TILE, TILE), (TILE + 1, TILE + 1), (130, 97)])
def test_degenerate_and_ragged_sizes(dev, hw, connectivity):
    rng = np.random.RandomState(hw[0] * 131 + hw[1])
    for m in (rng.rand(*hw) > 0.45, rng.rand(*hw) > 0.8, np.zeros(hw, bool), np.ones(hw, bool)):
        check_all(m, connectivity, sizes=((3, 2), (0, 0), (hw[0] * hw[1], hw[0] * hw[1] + 1)))


def test_components_across_tile_edges_and_corners(dev):
    m = np.zeros((130, 200), bool)
    m[10, 50:80] = True                       # crosses the vertical edge at column 64
    m[50:80, 20] = True                       # crosses the horizontal edge at row 64
    m[63, 63] = m[64, 64] = True              # meet only at the corner of four tiles (main diagonal)
    m[63, 128] = m[64, 127] = True            # the same on the anti-diagonal at (64, 128)
    m[100, 63] = m[101, 64] = True            # diagonal across a vertical edge only
    m[63, 150] = m[64, 151] = True            # diagonal across a horizontal edge only
    lab1, lab2 = _np(G.label(m, 1)), _np(G.label(m, 2))
    assert lab1.max() == 2 + 8 and lab2.max() == 2 + 4
    assert lab1[63, 63] != lab1[64, 64] and lab2[63, 63] == lab2[64, 64] and lab2[63, 128] == lab2[64, 127]
    a1 = _np(G.component_areas(m, 1))
    assert a1[10, 50] == 30 and a1[79, 20] == 30 and a1[63, 63] == 1
    assert _np(G.component_areas(m, 2))[64, 64] == 2
    for conn in (1, 2):
        check_all(m, conn, sizes=((2, 2), (30, 5), (31, 5)))
        check_all(~m, conn, sizes=((2, 2), (30, 31)))


@pytest.mark.parametrize("connectivity", [1, 2])
def test_long_union_chains_small(dev, connectivity):
    s = R.serpentine(150, 131)
    for m in (s, s.T.copy(), ~s):
        check_all(m, connectivity, sizes=((131, 130), (130, 131)))


def test_long_union_chain_1024(dev):
    H = W = 1024
    s = torch.from_numpy(R.serpentine(H, W)).to(dev)
    for conn in (1, 2):
        lab = G.label(s, conn)
        assert int(lab.max()) == 1 and torch.equal(lab > 0, s)
        areas = G.component_areas(s, conn)
        assert bool((areas[s] == (H // 2) * W + H // 2).all()) and bool((areas[~s] == W - 1).all())
        holes = G.label(~s, conn)
        assert int(holes.max()) == H // 2
        # every odd row's background is one component, numbered from the top
        rows = torch.arange(H, device=dev)[:, None].expand(H, W)
        assert torch.equal(holes[~s], (rows[~s] // 2 + 1).to(torch.int32))
        assert torch.equal(G.remove_small_regions(s, 0, W - 1, conn), s)
        assert bool(G.remove_small_regions(s, 0, W, conn).all())


def test_checkerboard(dev):
    H, W = 66, 70
    m = (np.indices((H, W)).sum(0) % 2).astype(bool)
    lab1 = _np(G.label(m, 1))
    assert lab1.max() == H * W // 2 and np.array_equal(lab1[m], np.arange(1, H * W // 2 + 1))
    assert _np(G.label(m, 2)).max() == 1
    assert (_np(G.component_areas(m, 1)) == 1).all() and (_np(G.component_areas(m, 2)) == H * W // 2).all()
    assert not _np(G.remove_small_regions(m, 2, 0, 1)).any()
    assert _np(G.remove_small_regions(m, 0, 2, 1)).all()
    assert np.array_equal(_np(G.remove_small_regions(m, 2, 2, 2)), m)


@pytest.mark.parametrize("connectivity", [1, 2])
def test_area_bounds_are_strict(dev, connectivity):
    size = 9
    m = np.zeros((40, 140), bool)
    for k, area in enumerate((size - 1, size, size + 1)):
        m[2, 5 + 20 * k:5 + 20 * k + area] = True                   # objects of 8, 9, 10 pixels
    m[10:30, 50:136] = True
    for k, area in enumerate((size - 1, size, size + 1)):
        m[15, 58 + 20 * k:58 + 20 * k + area] = False               # holes of 8, 9, 10 pixels (the first one spans a tile edge)
    obj = _np(G.remove_small_objects(m, size, connectivity))
    assert not obj[2, 5] and obj[2, 25] and obj[2, 45]
    holes = _np(G.remove_small_holes(m, size, connectivity))
    assert holes[15, 58] and not holes[15, 78] and not holes[15, 98]
    both = _np(G.remove_small_regions(m, size, size, connectivity))
    assert not both[2, 5] and both[2, 25] and both[15, 58] and not both[15, 78]
    check_all(m, connectivity, sizes=((size, size), (size + 1, size + 1), (size + 2, size + 2)))


def test_border_pocket_is_filled(dev):
    m = np.ones((70, 70), bool)
    m[0, 0:3] = False                          # touches the top border
    m[30:32, 69] = False                       # touches the right border
    m[69, 60:70] = False                       # ten pixels: stays with a threshold of 10
    got = _np(G.remove_small_holes(m, 10))
    assert got[0, 0] and got[30, 69] and not got[69, 65]
    check_all(m, 1, sizes=((0, 10), (0, 11)))


def test_objects_go_before_holes(dev):
    m = np.zeros((80, 80), bool)
    m[20:70, 20:70] = True
    m[60:65, 62:66] = False                    # a 20-pixel hole across the tile corner at (64, 64)
    m[30:35, 30:35] = False                    # a 25-pixel hole ...
    m[32, 31:34] = True                        # ... with a 3-pixel object inside: 22 hole pixels
    got = _np(G.remove_small_regions(m, 5, 24))
    # the object goes first, so the hole has 25 pixels when it is measured and stays; holes first would have filled it
    assert not got[30:35, 30:35].any() and got[60:65, 62:66].all()
    assert np.array_equal(got, R.remove_small_regions(m, 5, 24))
    check_all(m, 2, sizes=((5, 24), (5, 26), (3, 23)))


def test_nothing_leaks_across_images(dev):
    m = np.zeros((3, 10, 12), bool)
    m[0, 9] = m[1, 0] = True                   # image 0 ends and image 1 begins with a full row
    m[1, 9, 4:] = True
    m[2, 0, :5] = True                         # aligned with the end of image 1's last row in memory
    assert np.array_equal(_np(G.label(m)).reshape(3, -1).max(1), [1, 2, 1])
    a = _np(G.component_areas(m))
    assert a[0, 9, 0] == 12 and a[1, 0, 0] == 12 and a[1, 9, 11] == 8 and a[2, 0, 0] == 5
    assert not _np(G.remove_small_objects(m, 13)).any()
    for conn in (1, 2):
        check_all(m, conn, sizes=((12, 100), (9, 109)))


@pytest.fixture(scope="module")
def blob_case():
    """3 x 299^2 blobs and the restatement's answers for the reference's two parameter pairs"""
    m = R.blobs(3, 299, 299, seed=7)
    want = {p: R.batched(R.remove_small_regions, m, *p) for p in ((300, 100), (400, 120))}
    return m, want


def test_random_blobs_299(dev, blob_case):
    m, want = blob_case
    assert all((w != m).sum() > 500 for w in want.values())            # both filters have work to do
    d = torch.from_numpy(m).to(dev)
    for (mo, ho), w in want.items():
        got = G.remove_small_regions(d, mo, ho)
        assert np.array_equal(_np(got), w) and np.array_equal(_np(d), m)
        assert np.array_equal(_np(G.remove_small_regions(m[1], mo, ho)), w[1])           # one image, from the host
        buf = d.clone()
        assert G.remove_small_regions(buf, mo, ho, out=buf) is buf and torch.equal(buf, got)        # in place
        other = torch.empty_like(d)
        G.remove_small_regions(d, mo, ho, out=other)
        assert torch.equal(other, got)
    check_all(m, 1, sizes=((300, 100),))
    check_all(m[:2], 2, sizes=((400, 120),))


def test_raw_filter_in_place_and_workspace_reuse(dev, blob_case):
    m, want = blob_case
    d = torch.from_numpy(m).to(dev).view(torch.uint8)
    ws = K.regions_workspace(3, 299, 299, dev)
    ws.fill_(0xAB)                                                      # stale contents must not matter
    a = K.regions_remove_small(d, 300, 100, ws=ws)
    buf = (d * 255).contiguous()                                        # any non-zero value is foreground
    K.regions_remove_small(buf, 300, 100, out=buf, ws=ws)
    assert torch.equal(a, buf) and np.array_equal(_np(a).astype(bool), want[(300, 100)])
    with pytest.raises(RuntimeError):
        K.regions_remove_small(d, 300, 100, ws=ws[:-16].clone())        # workspace too small: refused, nothing launched
    with pytest.raises(RuntimeError):
        K.regions_filter(d, 1, 5, connectivity=3, ws=ws)


def test_batches_are_cut_into_chunks(dev, monkeypatch):
    m = R.blobs(5, 70, 90, seed=3, density=1 / 150.0)
    want = _np(G.remove_small_regions(m, 30, 10))
    lab = _np(G.label(m))
    monkeypatch.setattr(G, "_MAX_PIXELS", 2 * 70 * 90 + 5)             # two images per call: 2 + 2 + 1
    assert [b - a for a, b in G._chunks(torch.empty(5, 70, 90))] == [2, 2, 1]
    assert np.array_equal(_np(G.remove_small_regions(m, 30, 10)), want)
    assert np.array_equal(_np(G.label(m)), lab)
    assert np.array_equal(want, R.batched(R.remove_small_regions, m, 30, 10))


def test_two_runs_identical_and_graph_replay(dev, blob_case):
    m, want = blob_case
    d = torch.from_numpy(m).to(dev)
    a, b = G.remove_small_regions(d, 300, 100), G.remove_small_regions(d, 300, 100)
    assert torch.equal(a, b) and torch.equal(G.label(d, 2), G.label(d, 2))
    static_in = torch.zeros_like(d)
    static_out = torch.empty_like(d)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        G.remove_small_regions(static_in, 300, 100, out=static_out)                       # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        G.remove_small_regions(static_in, 300, 100, out=static_out)
    static_in.copy_(d)
    graph.replay()
    assert torch.equal(static_out, a)
    other = torch.from_numpy(R.blobs(3, 299, 299, seed=8)).to(dev)
    static_in.copy_(other)
    graph.replay()
    assert torch.equal(static_out, G.remove_small_regions(other, 300, 100))


def test_threshold_compares_in_float32(dev):
    t32 = np.float32(0.3)                      # 0.30000001192..., above the double 0.3
    p = np.array([t32, np.nextafter(t32, np.float32(1)), np.nextafter(t32, np.float32(0)), 0.0, 1.0, np.nan], np.float32)
    p = np.concatenate([p, np.random.RandomState(0).rand(1000).astype(np.float32)]).reshape(2, -1)
    want = p > np.float32(0.3)
    assert not want[0, 0] and want[0, 1] and bool(p.astype(np.float64)[0, 0] > 0.3)      # a float64 compare would keep p[0, 0]
    assert np.array_equal(p > 0.3, want)                                                  # numpy's own float32-array compare
    assert np.array_equal(_np(G.threshold(p, 0.3)), want)
    assert np.array_equal(_np(G.threshold(torch.from_numpy(p).to(dev), 0.3)), want)


def test_hsv_gate_and_preprocess_masks(dev):
    rng = np.random.RandomState(5)
    img = rng.randint(120, 256, size=(3, 70, 90, 3)).astype(np.uint8)
    img[0, :, :45] = rng.randint(0, 171, size=(70, 45, 3))             # a dark half: passes the gate
    img[1, 10, 10] = (170, 0, 170)
    img[1, 10, 11] = (171, 0, 0)
    img[1, 10, 12] = (0, 0, 171)
    masks = R.blobs(3, 70, 90, seed=6, density=1 / 100.0, holes=False)
    masks[1, 10, 10:13] = True
    gate = R.hsv_gate(img, masks)
    assert gate[1, 10, 10] and not gate[1, 10, 11] and not gate[1, 10, 12]
    got = K.regions_hsv_gate(torch.from_numpy(img).to(dev), torch.from_numpy(masks.view(np.uint8)).to(dev))
    assert np.array_equal(_np(got).astype(bool), gate)
    for mo, ho in ((400, 120), (20, 8)):
        want = R.preprocess_masks(img, masks, mo, ho)
        got = stage.preprocess_masks(img, masks.view(np.uint8), mo, ho)
        assert got.dtype == torch.bool and np.array_equal(_np(got), want)
        assert np.array_equal(_np(stage.preprocess_masks(torch.from_numpy(img).to(dev), torch.from_numpy(masks).to(dev), mo, ho)), want)
    assert np.array_equal(_np(stage.preprocess_masks(img[0], masks[0], 20, 8)), R.preprocess_masks(img[0], masks[0], 20, 8))
    assert (R.preprocess_masks(img, masks, 20, 8) != gate).any()


def test_generate_masks_with_preprocess(dev):
    rng = np.random.RandomState(9)
    n_images, hw, tile = 3, (96, 120), 32
    grid = [(r, c) for r in range(0, hw[0] - tile + 1, 16) for c in range(0, hw[1] - tile + 1, 22)]
    tile_idx = np.repeat(np.arange(n_images), len(grid))
    tiles = np.tile(np.asarray(grid), (n_images, 1))
    selected = np.sort(rng.choice(len(tile_idx), 14, replace=False))
    img = np.full((n_images,) + hw + (3,), 150, np.uint8)
    for n, r, c, h, w in zip(rng.randint(0, n_images, 60), rng.randint(0, hw[0], 60), rng.randint(0, hw[1], 60), rng.randint(2, 14, 60),
                             rng.randint(2, 14, 60)):
        img[n, r:r + h, c:c + w, rng.randint(3)] = 220                 # bright patches: cut out of the painted squares by the gate
    plain = stage.generate_masks(n_images, hw, tile, tile_idx, tiles, selected, device=dev)
    again = stage.generate_masks(n_images, hw, tile, tile_idx, tiles, selected, device=dev, preprocess=None)
    assert plain.dtype == torch.uint8 and torch.equal(plain, again)
    got = stage.generate_masks(n_images, hw, tile, tile_idx, tiles, selected, device=dev, preprocess=img)
    assert got.dtype == torch.uint8 and tuple(got.shape) == tuple(plain.shape)
    assert torch.equal(got.view(torch.bool), stage.preprocess_masks(img, plain))
    assert np.array_equal(_np(got).astype(bool), R.preprocess_masks(img, _np(plain)))
    small = stage.generate_masks(n_images, hw, tile, tile_idx, tiles, selected, device=dev, preprocess=img, min_object_size=30,
                                 hole_area_threshold=9)
    assert np.array_equal(_np(small).astype(bool), R.preprocess_masks(img, _np(plain), 30, 9))


def test_segment_classes_end_to_end_resnet18(dev):
    from cellsegmentation_amd import inference, metrics, synth
    from cellsegmentation_amd.model import resnet as RN
    m = RN.MILresnet18()
    sd = m.state_dict()
    synth.fill_state_dict(sd)
    m.load_state_dict(sd)
    m = m.to(dev).set_compute_dtype(torch.float32)
    m.setmode("segment")
    x = synth.normalise(synth.ihc_tiles(4, 299, seed=23))
    loader = [x[:3], x[3:]]
    probs = inference.inference_seg(loader, m, dev, mode="test")
    assert probs.dtype == np.float32
    thr = float(np.median(probs))                                      # a threshold that splits this model's output
    for mo, ho in ((300, 100), (40, 15)):
        got = inference.segment_classes(loader, m, dev, thr, mo, ho)
        assert got.dtype == torch.bool and got.is_cuda and tuple(got.shape) == probs.shape
        want = R.batched(R.remove_small_regions, probs > np.float32(thr), mo, ho)
        assert np.array_equal(_np(got), want)
    limited = inference.segment_classes(loader, m, dev, thr, 40, 15, reg_limit=True)
    assert m.mode == "segment"
    m.setmode("image")
    with torch.no_grad():
        reg = np.concatenate([np.round(m(b.to(dev))[1][:, 0].float().cpu().numpy()).astype(int) for b in loader])
    m.setmode("segment")
    zeroed = probs * (reg != 0)[:, None, None].astype(np.float32)
    assert np.array_equal(_np(limited), R.batched(R.remove_small_regions, zeroed > np.float32(thr), 40, 15))
    dice = metrics.dice_coef(got.float(), torch.from_numpy(want).to(dev).float())       # device masks go straight into the metric
    assert np.allclose(_np(dice), 1.0, atol=1e-6)
