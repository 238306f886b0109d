"""cellsegmentation_amd.morph on the GPU (csrc/morph.hip), bit-exact against the numpy restatement tests/morph_ref.py and the scipy
vectors tests/golden/morph_vectors.npz: the nearest-site transform in both polarities, the four binary operations with both border
values, label expansion, the distance transform of detect on the same core, Pythagorean ties, adversarial maps, batching and input
forms, repeatability, graph capture, and the ``opening_radius`` option of the segmentation pipeline."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import detect_ref as DR  # noqa: E402
import edt_ref as E  # noqa: E402
import morph_ref as MR  # noqa: E402
import regions_ref as RR  # noqa: E402
from cellsegmentation_amd import detect as D  # noqa: E402
from cellsegmentation_amd import kernels as K  # noqa: E402
from cellsegmentation_amd import morph as M  # noqa: E402
from cellsegmentation_amd import regions as G  # noqa: E402
from test_edt_gpu import three_maps  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "morph_vectors.npz"), allow_pickle=False)
MASK_NAMES = sorted(k[len("mask/"):-len(".mask")] for k in GOLD.files if k.startswith("mask/") and k.endswith(".mask"))
LABEL_NAMES = sorted(k[len("labels/"):-len(".labels")] for k in GOLD.files if k.endswith(".labels"))
GOLD_R2S = (0, 1, 2, 4, 5, 13, 25, 56)

# (3, 33001): a row of packed words beyond 64 KiB of LDS, several trips of a workgroup over its row
SHAPES = [(5, 3), (1, 70), (70, 1), (17, 40), (64, 16), (130, 97), (299, 299), (3, 33001)]
R2S = (0, 1, 2, 5, 25)
OPS = ("dilation", "erosion", "opening", "closing")


def _np(t):
    return t.cpu().numpy()


def three_masks(hw):
    """blobs, 50 % noise, 2 % noise -> bool [3, H, W]"""
    H, W = hw
    return np.stack([E.blob_mask(H, W, seed=H + W) > 10, E.random_mask(H, W, 0.5, seed=H * 3 + W) > 10,
                     E.random_mask(H, W, 0.98, seed=H * 5 + W) > 10])


def labels_of(masks, seed):
    """int32 label image of every mask: an arbitrary nonzero value under every True pixel (neighbours differ, some are negative), so
    that the site a pixel takes shows in the label it gets"""
    rng = np.random.RandomState(seed)
    v = rng.randint(1, 1000, size=masks.shape).astype(np.int32)
    v = np.where(rng.rand(*masks.shape) < 0.1, -v, v)
    return np.where(masks, v, 0).astype(np.int32)


_REF = {}


def ref(hw):
    """everything expected of a shape, computed once: masks, labels, and the reference results by name"""
    if hw not in _REF:
        masks = three_masks(hw)
        labels = labels_of(masks, hw[0] * 7 + hw[1])
        wide = hw[1] > 30000
        want = {}
        for bg in (False, True):
            if wide:                                               # the unbounded search: the 50 % map only
                want["nearest", bg] = [MR.nearest(masks[1] ^ bg)]
            else:
                want["nearest", bg] = [MR.nearest(m ^ bg) for m in masks]
        for op, r2, bv in itertools.product(OPS, R2S, (0, 1)):
            want[op, r2, bv] = np.stack([getattr(MR, f"binary_{op}")(m, r2, bv) for m in masks])
        for r2 in (2, 25):
            want["expand", r2] = np.stack([MR.expand_labels(lab, r2) for lab in labels])
        for a in [masks, labels] + [v for v in want.values() if isinstance(v, np.ndarray)]:
            a.setflags(write=False)
        _REF[hw] = (masks, labels, want)
    return _REF[hw]


@pytest.mark.parametrize("hw", SHAPES)
def test_nearest_sites_bit_exact(dev, hw):
    masks, labels, want = ref(hw)
    pick = slice(1, 2) if hw[1] > 30000 else slice(0, 3)
    d = torch.from_numpy(masks[pick].copy()).to(dev)
    for bg in (False, True):
        d2, site = M.nearest_sites(d, background=bg)
        assert d2.dtype == torch.int32 and site.dtype == torch.int32 and d2.is_cuda and tuple(d2.shape) == tuple(d.shape)
        for n, (wd, ws) in enumerate(want["nearest", bg]):
            assert np.array_equal(_np(d2[n]), wd), (bg, n)
            assert np.array_equal(_np(site[n]), ws), (bg, n)
    # a label image: its nonzero pixels are the sites
    d2, site = M.nearest_sites(torch.from_numpy(labels[pick].copy()).to(dev))
    for n, (wd, ws) in enumerate(want["nearest", False]):
        assert np.array_equal(_np(d2[n]), wd) and np.array_equal(_np(site[n]), ws), n


@pytest.mark.parametrize("hw", SHAPES)
def test_binary_operations_bit_exact(dev, hw):
    masks, _, want = ref(hw)
    d = torch.from_numpy(masks.copy()).to(dev)
    for op, r2, bv in itertools.product(OPS, R2S, (0, 1)):
        got = getattr(M, f"binary_{op}")(d, radius_sq=r2, border_value=bv)
        assert got.dtype == torch.bool and got.is_cuda and tuple(got.shape) == masks.shape
        assert np.array_equal(_np(got), want[op, r2, bv]), (op, r2, bv)
    assert torch.equal(M.binary_dilation(d, 2.3), M.binary_dilation(d, radius_sq=5))         # floor(2.3^2) = 5
    assert torch.equal(M.binary_erosion(d, 0), d) and torch.equal(M.binary_dilation(d, 0, border_value=1), d)


@pytest.mark.parametrize("hw", SHAPES)
def test_expand_labels_bit_exact(dev, hw):
    _, labels, want = ref(hw)
    d = torch.from_numpy(labels.copy()).to(dev)
    for r2 in (2, 25):
        got = M.expand_labels(d, radius_sq=r2)
        assert got.dtype == torch.int32 and got.is_cuda and tuple(got.shape) == labels.shape
        assert np.array_equal(_np(got), want["expand", r2]), r2
    assert torch.equal(M.expand_labels(d, 5), M.expand_labels(d, radius_sq=25))
    assert torch.equal(M.expand_labels(d, 0), d)


# ---- the distance transform of detect and the nearest-site transform share one core ---------------------------------------------------
EDT_SHAPES = [(5, 3), (1, 70), (70, 1), (64, 16), (130, 97), (3, 33001)]
_EDT_REF = {}


def edt_ref(hw, thr):
    """(uint8 maps: the three of test_edt_gpu and one all-foreground map, expected D2 by edt_ref alone), computed once"""
    if (hw, thr) not in _EDT_REF:
        maps = np.concatenate([three_maps(hw), np.full((1,) + hw, 255, np.uint8)])
        want = np.stack([E.edt_sq(m, thr) for m in maps])
        maps.setflags(write=False)
        want.setflags(write=False)
        _EDT_REF[hw, thr] = (maps, want)
    return _EDT_REF[hw, thr]


@pytest.mark.parametrize("thr", (10, 0, 254))
@pytest.mark.parametrize("hw", EDT_SHAPES)
def test_distance_transform_equals_nearest_sites_of_the_background(dev, hw, thr):
    maps, want = edt_ref(hw, thr)
    edt = _np(D.distance_transform_sq(torch.from_numpy(maps.copy()).to(dev), thr))
    near = _np(M.nearest_sites(torch.from_numpy(maps > thr), background=True)[0])
    assert np.array_equal(edt, near)
    for n in range(len(maps)):
        assert np.array_equal(edt[n], want[n]) and np.array_equal(near[n], want[n]), n
    assert (edt[3] == -1).all() and (near[3] == -1).all()                               # all foreground: no site
    if hw == (130, 97):                                                                 # the same maps as fp32 probabilities k / 255
        p = maps.astype(np.float32) / np.float32(255)
        assert np.array_equal(DR.quantize(p), maps)
        f32 = _np(K.detect_edt_sq(torch.from_numpy(p).to(dev), thr))
        assert np.array_equal(f32, edt) and np.array_equal(f32, want)


# ---- Pythagorean ties ---------------------------------------------------------------------------------------------------------------
TWELVE = [(5, 0), (-5, 0), (0, 5), (0, -5)] + [(sy * a, sx * b) for a, b in ((3, 4), (4, 3)) for sy in (1, -1) for sx in (1, -1)]
SUBSETS = [[(0, 5), (3, 4)],            # the site on the centre's own row is met last, at d * d == best: a `d * d < best` exit misses it
           [(-3, 4), (0, -5)],
           [(3, 4), (4, 3)], [(5, 0), (0, 5)], [(4, -3), (3, 4), (0, 5)], [(3, -4), (3, 4)], [(5, 0), (4, 3), (4, -3)], TWELVE]


@pytest.mark.parametrize("centre", [(10, 10), (0, 10), (10, 0)])
def test_pythagorean_ties_go_to_the_lowest_row_major_site(dev, centre):
    cy, cx = centre
    maps, expected = [], []
    for subset in SUBSETS:
        lab = np.zeros((21, 21), np.int32)
        inside = [(cy + dy, cx + dx) for dy, dx in subset if 0 <= cy + dy < 21 and 0 <= cx + dx < 21]
        if not inside:
            continue
        for k, (y, x) in enumerate(inside):
            lab[y, x] = 100 + k                                    # every site its own label
        maps.append(lab)
        expected.append(min(inside))                               # (row, col) tuples order as row-major indices do
    assert len(maps) >= 5
    maps = np.stack(maps)
    d2, site = M.nearest_sites(maps)
    grown = _np(M.expand_labels(maps, 5))
    short = _np(M.expand_labels(maps, radius_sq=24))
    d2, site = _np(d2), _np(site)
    for i, (y, x) in enumerate(expected):
        assert d2[i, cy, cx] == 25 and site[i, cy, cx] == y * 21 + x, (i, y, x)
        assert grown[i, cy, cx] == maps[i, y, x] and short[i, cy, cx] == 0, i
        wd, ws = MR.nearest_brute(maps[i] != 0)
        assert np.array_equal(d2[i], wd) and np.array_equal(site[i], ws), i
        assert np.array_equal(grown[i], MR.expand_labels(maps[i], 25)), i


# ---- adversarial maps ---------------------------------------------------------------------------------------------------------------
def frame(H, W, k):
    """True within k pixels of the image edge"""
    yy, xx = np.mgrid[0:H, 0:W]
    return np.minimum(np.minimum(yy, H - 1 - yy), np.minimum(xx, W - 1 - xx)) < k


@pytest.mark.parametrize("hw", [(299, 299), (257, 1025)])
def test_adversarial_maps(dev, hw):
    H, W = hw
    none, full = np.zeros(hw, bool), np.ones(hw, bool)
    corner = none.copy()
    corner[H - 1, 0] = True
    columns = none.copy()
    columns[:, 1::2] = True
    batch = torch.from_numpy(np.stack([none, full, corner, columns])).to(dev)          # a map without a site among ordinary ones
    d2, site = (_np(t) for t in M.nearest_sites(batch))
    yy, xx = np.mgrid[0:H, 0:W]
    flat = (yy * W + xx).astype(np.int32)
    assert (d2[0] == -1).all() and (site[0] == -1).all()
    assert not d2[1].any() and np.array_equal(site[1], flat)
    assert np.array_equal(d2[2], (yy - (H - 1)) ** 2 + xx ** 2) and (site[2] == (H - 1) * W).all()
    assert np.array_equal(d2[3], (xx % 2 == 0).astype(np.int32))
    assert np.array_equal(site[3], np.where(xx % 2 == 1, flat, np.where(xx == 0, flat + 1, flat - 1)))   # the left neighbour: lower index
    alone = M.nearest_sites(none)
    assert (_np(alone[0]) == -1).all() and (_np(alone[1]) == -1).all()
    for r2 in (1, 5, 25):
        k = int(np.sqrt(r2))
        dil0, dil1 = _np(M.binary_dilation(batch, radius_sq=r2)), _np(M.binary_dilation(batch, radius_sq=r2, border_value=1))
        ero0, ero1 = _np(M.binary_erosion(batch, radius_sq=r2)), _np(M.binary_erosion(batch, radius_sq=r2, border_value=1))
        assert not dil0[0].any() and np.array_equal(dil1[0], frame(H, W, k))            # nothing to grow but the outside
        assert np.array_equal(ero0[1], ~frame(H, W, k)) and ero1[1].all()               # eaten from the edge only
        assert dil0[1].all() and not ero0[0].any() and not ero1[0].any()
        assert np.array_equal(dil0[2], (yy - (H - 1)) ** 2 + xx ** 2 <= r2)
        assert dil0[3].all() and not ero1[3].any()
        for i in range(4):
            m = _np(batch[i])
            assert np.array_equal(dil1[i], MR.binary_dilation(m, r2, 1)) and np.array_equal(ero0[i], MR.binary_erosion(m, r2, 0)), (r2, i)
    # a radius larger than the image
    r2 = H * H + W * W
    assert np.array_equal(_np(M.binary_dilation(batch, radius_sq=r2)), np.stack([none, full, full, full]))
    assert not _np(M.binary_erosion(batch, radius_sq=r2)).any()
    assert np.array_equal(_np(M.binary_erosion(batch, radius_sq=r2, border_value=1)), np.stack([none, full, none, none]))
    lab = np.zeros((2,) + hw, np.int32)
    lab[1, H - 1, 0] = 7
    lab[1, 0, W - 1] = -3
    grown = _np(M.expand_labels(lab, radius_sq=r2))
    to_7, to_3 = (yy - (H - 1)) ** 2 + xx ** 2, yy ** 2 + (xx - (W - 1)) ** 2
    assert not grown[0].any() and np.array_equal(grown[1], np.where(to_3 <= to_7, -3, 7))        # a tie: (0, W - 1) has the lower index


# ---- batching and inputs ------------------------------------------------------------------------------------------------------------
def test_batches_and_input_forms(dev, monkeypatch):
    masks, labels, want = ref((130, 97))
    mixed = np.concatenate([masks[:1], np.zeros((1, 130, 97), bool), masks[1:]])
    got = _np(M.binary_opening(mixed, radius_sq=5))
    d2, site = M.nearest_sites(mixed)
    for i, j in ((0, 0), (2, 1), (3, 2)):
        assert np.array_equal(got[i], want["opening", 5, 0][j])
        one = M.binary_opening(mixed[i], radius_sq=5)                                   # numpy [H, W] in -> [H, W] out
        assert tuple(one.shape) == (130, 97) and one.is_cuda and np.array_equal(_np(one), got[i])
        assert np.array_equal(_np(d2[i]), want["nearest", False][j][0]) and np.array_equal(_np(site[i]), want["nearest", False][j][1])
    assert not got[1].any() and (_np(d2[1]) == -1).all()
    one = M.nearest_sites(masks[0].copy())
    assert tuple(one[0].shape) == (130, 97) and np.array_equal(_np(one[1]), want["nearest", False][0][1])
    assert tuple(M.expand_labels(labels[0].copy(), radius_sq=2).shape) == (130, 97)
    # chunks of whole images
    monkeypatch.setattr(G, "_MAX_PIXELS", 2 * 130 * 97 + 5)
    assert [b - a for a, b in G._chunks(torch.empty(3, 130, 97))] == [2, 1]
    assert np.array_equal(_np(M.binary_closing(masks.copy(), radius_sq=25, border_value=1)), want["closing", 25, 1])
    assert np.array_equal(_np(M.expand_labels(labels.copy(), radius_sq=25)), want["expand", 25])
    assert np.array_equal(_np(M.nearest_sites(masks.copy(), background=True)[1]), np.stack([w[1] for w in want["nearest", True]]))
    monkeypatch.undo()
    # non-contiguous and offset device views
    big = torch.zeros((4, 131, 200), dtype=torch.bool, device=dev)
    big[1:, 1:, 3:100] = torch.from_numpy(masks.copy()).to(dev)
    view = big[1:, 1:, 3:100]
    assert not view.is_contiguous() and view.data_ptr() % 16 != 0
    assert np.array_equal(_np(M.binary_erosion(view, radius_sq=2)), want["erosion", 2, 0])
    lbig = torch.zeros((3, 130, 2 * 97), dtype=torch.int32, device=dev)
    lbig[:, :, ::2] = torch.from_numpy(labels.copy()).to(dev)
    assert np.array_equal(_np(M.expand_labels(lbig[:, :, ::2], radius_sq=2)), want["expand", 2])
    assert np.array_equal(_np(M.expand_labels(torch.from_numpy(labels.copy()).to(dev)[1:], radius_sq=2)), want["expand", 2][1:])


def test_two_runs_identical(dev):
    masks, labels, _ = ref((299, 299))
    d, lab = torch.from_numpy(masks.copy()).to(dev), torch.from_numpy(labels.copy()).to(dev)
    a, b = M.nearest_sites(d), M.nearest_sites(d)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(M.binary_opening(d, 2), M.binary_opening(d, 2)) and torch.equal(M.binary_closing(d, 3, 1), M.binary_closing(d, 3, 1))
    assert torch.equal(M.expand_labels(lab, 4), M.expand_labels(lab, 4))


# ---- golden vectors -----------------------------------------------------------------------------------------------------------------
def gold_bits(key, W):
    return np.unpackbits(GOLD[key], axis=1)[:, :W].astype(bool)


@pytest.mark.parametrize("name", MASK_NAMES)
def test_masks_equal_scipy_vectors(dev, name):
    H, W = GOLD[f"mask/{name}.shape"]
    m = gold_bits(f"mask/{name}.mask", W)
    d = torch.from_numpy(m).to(dev)
    assert np.array_equal(_np(M.nearest_sites(d)[0]), GOLD[f"mask/{name}.d2_true"])
    assert np.array_equal(_np(M.nearest_sites(d, background=True)[0]), GOLD[f"mask/{name}.d2_false"])
    for op, r2, bv in itertools.product(OPS, GOLD_R2S, (0, 1)):
        got = _np(getattr(M, f"binary_{op}")(d, radius_sq=r2, border_value=bv))
        assert np.array_equal(got, gold_bits(f"mask/{name}.{op}.{r2}.{bv}", W)), (op, r2, bv)


@pytest.mark.parametrize("name", LABEL_NAMES)
def test_labels_equal_scipy_vectors(dev, name):
    labels = GOLD[f"labels/{name}.labels"]
    W = labels.shape[1]
    r2 = int(GOLD[f"labels/{name}.r2"])
    filled, ambiguous = gold_bits(f"labels/{name}.filled", W), gold_bits(f"labels/{name}.ambiguous", W)
    got = _np(M.expand_labels(labels, radius_sq=r2))
    assert np.array_equal(got[labels != 0], labels[labels != 0])
    assert np.array_equal((got != 0) & (labels == 0), filled)
    sure = filled & ~ambiguous                                       # the tie rule shows on the ambiguous pixels alone
    assert ambiguous.sum() <= 0.03 * filled.sum() and np.array_equal(got[sure], GOLD[f"labels/{name}.under"][sure])
    assert np.array_equal(got, MR.expand_labels(labels, r2))         # ... and there it is this project's own: nothing skipped


# ---- labels -------------------------------------------------------------------------------------------------------------------------
def test_expanded_labels_keep_their_table(dev):
    masks = RR.blobs(3, 130, 97, seed=11, density=1 / 300.0, holes=False)
    lab = G.label(masks)
    before = G.measure_labels(lab, max_regions=64)
    grown = M.expand_labels(lab, 4)
    assert torch.equal(grown[lab != 0], lab[lab != 0]) and int((grown != 0).sum()) > int((lab != 0).sum())
    after = G.measure_labels(grown, max_regions=64, counts=before.counts)
    assert torch.equal(after.counts, before.counts) and int(before.counts.min()) > 0
    assert bool((after.area >= before.area).all()) and bool((after.area > before.area).any())
    own = G.measure_labels(grown, max_regions=64)                    # no label appeared or disappeared
    assert torch.equal(own.counts, before.counts) and torch.equal(own.area, after.area)
    assert np.array_equal(_np(grown), np.stack([MR.expand_labels(x, 16) for x in _np(lab)]))


# ---- pipeline -----------------------------------------------------------------------------------------------------------------------
def test_segment_classes_with_an_opening_resnet18(dev):
    from cellsegmentation_amd import inference, synth
    from cellsegmentation_amd.model import resnet as RN
    m = RN.MILresnet18()
    sd = m.state_dict()
    synth.fill_state_dict(sd)
    m.load_state_dict(sd)
    m = m.to(dev).set_compute_dtype(torch.float32)
    m.setmode("segment")
    x = synth.normalise(synth.ihc_tiles(2, 299, seed=21))
    loader = [x]
    probs = inference.inference_seg(loader, m, dev, mode="test")
    thr = float(np.median(probs))                                    # a threshold that splits this model's output
    classes = probs > np.float32(thr)
    opened = np.stack([MR.binary_opening(c, 4, 0) for c in classes])
    assert (opened != classes).any()
    got = inference.segment_classes(loader, m, dev, thr, 40, 15, opening_radius=2)
    assert got.dtype == torch.bool and np.array_equal(_np(got), RR.batched(RR.remove_small_regions, opened, 40, 15))
    plain = inference.segment_classes(loader, m, dev, thr, 40, 15)
    zero = inference.segment_classes(loader, m, dev, thr, 40, 15, opening_radius=0)
    assert _np(plain).tobytes() == _np(zero).tobytes()
    assert np.array_equal(_np(plain), RR.batched(RR.remove_small_regions, classes, 40, 15))
    # the stitched-map entry points take the same option
    u8 = (np.clip(probs[0], 0, 1) * 255).astype(np.uint8)
    t8 = int(np.median(u8))
    table = inference.measure_slide(u8, thr_u8=t8, min_object_size=40, hole_area_threshold=15, max_regions=512, opening_radius=2)
    want = RR.remove_small_regions(MR.binary_opening(u8 > t8, 4, 0), 40, 15)
    n = RR.label(want)[1]
    assert 0 < n <= 512 and int(table.counts[0]) == n and int(table.area.sum()) == int(want.sum())


# ---- graph capture ------------------------------------------------------------------------------------------------------------------
def test_graph_capture_and_replay(dev):
    masks, labels, want = ref((130, 97))
    d, lab = torch.from_numpy(masks.copy()).to(dev), torch.from_numpy(labels.copy()).to(dev)
    eager = (M.binary_opening(d, 2), M.expand_labels(lab, 5))
    static_m, static_l = torch.zeros_like(d), torch.zeros_like(lab)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        M.binary_opening(static_m, 2), M.expand_labels(static_l, 5)                     # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_m, out_l = M.binary_opening(static_m, 2), M.expand_labels(static_l, 5)
    static_m.copy_(d)
    static_l.copy_(lab)
    graph.replay()
    assert torch.equal(out_m, eager[0]) and torch.equal(out_l, eager[1])
    assert np.array_equal(_np(out_m), np.stack([MR.binary_opening(m, 4, 0) for m in masks]))
    assert np.array_equal(_np(out_l), want["expand", 25])
    static_m.copy_(~d)
    graph.replay()
    assert torch.equal(out_m, M.binary_opening(~d, 2)) and torch.equal(out_l, eager[1])
