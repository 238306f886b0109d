"""The distance-transform smoothing on the GPU (csrc/detect.hip edt_* through cellsegmentation_amd.detect), bit-exact against the
numpy restatement tests/edt_ref.py and the scipy vectors tests/golden/edt_vectors.npz: squared distances, the integer
normalisation, fp32 input, adversarial maps, batching, repeatability, detect_points / inference.detect_cells with
method="distancetransform"."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import detect_ref as R  # noqa: E402
import edt_ref as E  # noqa: E402
from cellsegmentation_amd import detect as D  # noqa: E402
from cellsegmentation_amd import kernels as K  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "edt_vectors.npz"), allow_pickle=False)
GOLD_NAMES = sorted(k[:-len(".mask")] for k in GOLD.files if k.endswith(".mask"))

# (3, 33001): a row of 16-bit column distances beyond 64 KiB of LDS
SHAPES = [(5, 3), (1, 70), (70, 1), (17, 40), (64, 16), (130, 97), (299, 299), (300, 1100), (3, 33001)]


def three_maps(hw):
    """blobs, noise with 50 % background, noise with 2 % background"""
    H, W = hw
    return np.stack([E.blob_mask(H, W, seed=H + W), E.random_mask(H, W, 0.5, seed=H * 3 + W), E.random_mask(H, W, 0.02, seed=H * 5 + W)])


_REF = {}


def ref_sq(hw):
    """(maps, expected D2) of a shape, computed once"""
    if hw not in _REF:
        maps = three_maps(hw)
        want = np.stack([E.edt_sq(m) for m in maps])
        maps.setflags(write=False)
        want.setflags(write=False)
        _REF[hw] = (maps, want)
    return _REF[hw]


@pytest.mark.parametrize("hw", SHAPES)
def test_squared_distance_bit_exact(dev, hw):
    maps, want = ref_sq(hw)
    got = D.distance_transform_sq(torch.from_numpy(maps.copy()).to(dev))
    assert got.dtype == torch.int32 and tuple(got.shape) == maps.shape and got.is_cuda
    assert np.array_equal(got.cpu().numpy(), want)
    one = D.distance_transform_sq(maps[0].copy())                           # numpy in, [H, W] in -> [H, W] out
    assert tuple(one.shape) == hw and np.array_equal(one.cpu().numpy(), want[0])


@pytest.mark.parametrize("hw", SHAPES)
def test_smoothed_map_bit_exact(dev, hw):
    maps, want = ref_sq(hw)
    got = D.distance_smooth(torch.from_numpy(maps.copy()).to(dev))
    assert got.dtype == torch.uint8 and tuple(got.shape) == maps.shape
    got = got.cpu().numpy()
    for n in range(3):
        assert np.array_equal(got[n], E.normalise(want[n])), n
        assert got[n].max() == (255 if want[n].max() > 0 else 0)


@pytest.mark.parametrize("name", GOLD_NAMES)
def test_squared_distance_equals_scipy_vectors(dev, name):
    H, W = GOLD[f"{name}.shape"]
    fg = np.unpackbits(GOLD[f"{name}.mask"], axis=1)[:, :W].astype(bool)
    got = D.distance_transform_sq(np.where(fg, 11, 10).astype(np.uint8)).cpu().numpy()
    assert np.array_equal(got, GOLD[f"{name}.d2"])


def one_background_pixel(H, W, y0, x0):
    """all foreground but (y0, x0): the distances are the definition itself"""
    m = np.full((H, W), 255, np.uint8)
    m[y0, x0] = 0
    yy, xx = np.mgrid[0:H, 0:W]
    return m, ((yy - y0) ** 2 + (xx - x0) ** 2).astype(np.int32)


def adversarial(H, W):
    """[(name, map, expected D2)] at the default threshold"""
    out = [("corner",) + one_background_pixel(H, W, H - 1, 0), ("centre",) + one_background_pixel(H, W, H // 2, W // 2)]
    out.append(("no background", np.full((H, W), 11, np.uint8), np.full((H, W), -1, np.int32)))
    out.append(("all background", np.full((H, W), 10, np.uint8), np.zeros((H, W), np.int32)))
    m = np.zeros((H, W), np.uint8)
    m[H // 3, W - 2] = 200
    d = np.zeros((H, W), np.int32)
    d[H // 3, W - 2] = 1
    out.append(("one foreground pixel", m, d))
    m = np.full((H, W), 10, np.uint8)
    m[:, 1::2] = 11                                                       # 10 | 11 | 10 | 11: every other column is foreground
    out.append(("10 and 11", m, (m == 11).astype(np.int32)))
    return out


@pytest.mark.parametrize("hw", [(299, 299), (257, 1025), (3, 33001)])
def test_adversarial_maps(dev, hw):
    cases = adversarial(*hw)
    maps = np.stack([c[1] for c in cases])
    t = torch.from_numpy(maps).to(dev)
    got = D.distance_transform_sq(t).cpu().numpy()
    sm = D.distance_smooth(t).cpu().numpy()                               # one batch: a map without background among ordinary ones
    for i, (name, _, want) in enumerate(cases):
        assert np.array_equal(got[i], want), name
        assert np.array_equal(sm[i], E.normalise(want)), name
    assert not sm[2].any() and not sm[3].any() and sm[4].sum() == 255
    # alone as well: the per-map flag and maximum of a one-map call
    assert (D.distance_transform_sq(maps[2]).cpu().numpy() == -1).all() and not D.distance_smooth(maps[2]).cpu().numpy().any()


@pytest.mark.parametrize("hw", [(299, 299), (257, 1025)])
def test_threshold_values(dev, hw):
    m = np.random.RandomState(hw[1]).randint(0, 256, size=hw).astype(np.uint8)
    m[:7, :9] = 255                                                       # a patch deeper than one pixel
    for thr in (0, 255, 254, 100, -1, 10.5):
        got = D.distance_transform_sq(m, thr_for_dt=thr).cpu().numpy()
        ithr = int(np.floor(thr))
        assert np.array_equal(got, E.edt_sq(m, ithr)), thr
        assert np.array_equal(D.distance_smooth(m, thr_for_dt=thr).cpu().numpy(), E.smooth(m, ithr)), thr
    assert not D.distance_transform_sq(m, thr_for_dt=255).cpu().numpy().any()
    assert (D.distance_transform_sq(m, thr_for_dt=-1).cpu().numpy() == -1).all()


def test_every_map_is_scaled_by_its_own_maximum(dev):
    big = np.zeros((69, 69), np.uint8)
    big[1:68, 1:68] = 200                                                 # M = 34^2: 22.5 -> 22, 37.5 -> 38, 52.5 -> 52
    small = np.zeros((69, 69), np.uint8)
    small[30:33, 40:43] = 50                                              # M = 4: D2 = 1 gives 127.5 -> 128
    full = np.full((69, 69), 255, np.uint8)
    maps = np.stack([big, small, full, np.zeros((69, 69), np.uint8), small, big])
    got = D.distance_smooth(maps).cpu().numpy()
    for n in range(len(maps)):
        assert np.array_equal(got[n], E.smooth(maps[n])), n
    assert got[0, 34, 34] == 255 and got[0, 3, 34] == 22 and got[0, 5, 34] == 38 and got[0, 7, 34] == 52
    assert got[1, 31, 41] == 255 and got[1, 30, 40] == 128 and got[1, 31, 40] == 128
    assert not got[2].any() and not got[3].any()
    d2 = D.distance_transform_sq(maps).cpu().numpy()
    assert d2[0].max() == 1156 and d2[1].max() == 4 and (d2[2] == -1).all() and not d2[3].any()
    tie = np.full((5, 5), 255, np.uint8)
    tie[0, :] = tie[-1, :] = 0
    tie[:, 0] = tie[:, -1] = 0
    assert np.array_equal(D.distance_smooth(tie).cpu().numpy(), E.smooth(tie)) and E.smooth(tie)[1, 1] == 128


def test_fp32_probabilities(dev):
    rng = np.random.RandomState(12)
    p = (rng.rand(3, 37, 53) ** 4).astype(np.float32)                     # 37 * 53 * 4 bytes per map: not a multiple of 16
    k = np.arange(256, dtype=np.float32) / np.float32(255)
    p[0, 0, :40] = np.nextafter(k[:40], np.float32(0))                    # just below k / 255: quantises to k - 1
    p[0, 1, :40] = k[:40]
    t = torch.from_numpy(p).to(dev)
    q = R.quantize(p)
    for thr in (10, 0, 37):
        sm = K.detect_edt_smooth(t, thr).cpu().numpy()
        sq = K.detect_edt_sq(t, thr).cpu().numpy()
        for n in range(3):
            assert np.array_equal(sq[n], E.edt_sq(q[n], thr)), (thr, n)
            assert np.array_equal(sm[n], E.smooth(q[n], thr)), (thr, n)
    view = t[1:]                                                          # starts 7844 bytes into the buffer
    assert view.data_ptr() % 16 != 0
    assert np.array_equal(K.detect_edt_smooth(view, 10).cpu().numpy(), np.stack([E.smooth(q[1]), E.smooth(q[2])]))
    assert np.array_equal(K.detect_edt_smooth(torch.from_numpy(q).to(dev), 10).cpu().numpy(), K.detect_edt_smooth(t, 10).cpu().numpy())


def mixed_batch(H, W):
    maps = [E.blob_mask(H, W, seed=H, density=1 / 1500.0, radius=(3, 7)), E.blob_mask(H, W, seed=W + 1, density=1 / 400.0, radius=(2, 5)),
            np.full((H, W), 255, np.uint8), np.zeros((H, W), np.uint8)]
    touching = np.zeros((H, W), np.uint8)                                 # two overlapping discs: what the method is offered for
    yy, xx = np.mgrid[0:H, 0:W]
    for cy, cx in ((H // 2, W // 2 - 9), (H // 2, W // 2 + 9)):
        touching[(yy - cy) ** 2 + (xx - cx) ** 2 <= 144] = 180
    return np.stack(maps + [touching])


@pytest.mark.parametrize("hw", [(299, 299), (512, 512), (40, 300)])
def test_detect_points_distancetransform(dev, hw):
    maps = mixed_batch(*hw)
    counts = [3, 0, 5, 5, 1]
    res = D.detect_points(torch.from_numpy(maps).to(dev), cell_counts=counts, eps=11, method="distancetransform")
    glob = D.detect_points(maps, cell_counts=counts, eps=11, method="distancetransform", _force_global=True)
    again = D.detect_points(maps, cell_counts=counts, eps=11, method="distancetransform", thr_for_dt=10, ksize=None, sigmaX=None)
    per = res.per_image()
    assert len(res.offsets) == len(maps) + 1 and res.offsets[0] == 0
    for i, m in enumerate(maps):
        (want, w, kept) = E.detect(m, None, eps=11, with_weights=True, with_kept=True)
        pts = res.points[res.offsets[i]:res.offsets[i + 1]]
        assert np.array_equal(pts, want[0]) and pts.dtype == np.int64, i
        assert np.array_equal(res.weights[res.offsets[i]:res.offsets[i + 1]], w), i
        assert res.n_kept[i] == kept, i
        assert np.array_equal(per[i][0], want[0][:counts[i]]) and np.array_equal(per[i][1], want[0][counts[i]:]), i
    assert res.offsets[3] - res.offsets[2] == 0 and res.offsets[4] - res.offsets[3] == 0       # no background / no foreground: no cells
    assert res.offsets[1] > 0
    for other in (glob, again):
        assert np.array_equal(other.points, res.points) and np.array_equal(other.weights, res.weights)
        assert np.array_equal(other.offsets, res.offsets) and np.array_equal(other.n_kept, res.n_kept)
    other_thr = D.detect_points(maps[:2], eps=11, method="distancetransform", thr_for_dt=128)
    for i in range(2):
        want = E.detect(maps[i], None, eps=11, thr_for_dt=128)
        assert np.array_equal(other_thr.points[other_thr.offsets[i]:other_thr.offsets[i + 1]], want[0]), i


def test_default_method_is_the_blur(dev):
    maps = mixed_batch(299, 299)[:2]
    a = D.detect_points(maps, eps=11)
    b = D.detect_points(maps, eps=11, method="gaussianblur", thr_for_dt=200)
    for i in range(2):
        want, w = R.detect(maps[i], None, eps=11, with_weights=True)
        assert np.array_equal(a.points[a.offsets[i]:a.offsets[i + 1]], want[0]) and np.array_equal(a.weights[a.offsets[i]:a.offsets[i + 1]], w)
    assert np.array_equal(a.points, b.points) and np.array_equal(a.weights, b.weights) and np.array_equal(a.offsets, b.offsets)
    assert np.array_equal(a.n_kept, b.n_kept)


def test_two_runs_identical(dev):
    maps = torch.from_numpy(np.stack([E.blob_mask(512, 512, seed=60 + i, density=1 / 700.0) for i in range(4)])).to(dev)
    a, b = D.distance_transform_sq(maps), D.distance_transform_sq(maps)
    assert torch.equal(a, b)
    sa, sb = D.distance_smooth(maps), D.distance_smooth(maps)
    assert torch.equal(sa, sb)
    ra = D.detect_points(maps, eps=11, method="distancetransform")
    rb = D.detect_points(maps, eps=11, method="distancetransform")
    assert ra.points.tobytes() == rb.points.tobytes() and ra.weights.tobytes() == rb.weights.tobytes()
    assert ra.offsets.tobytes() == rb.offsets.tobytes() and len(ra.points) > 10


def test_detect_cells_distancetransform_resnet18(dev):
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
    q = R.quantize(probs)
    # the default threshold, and the median level of the model's own maps (random weights need not straddle 10)
    for thr_for_dt in (10, int(np.median(q))):
        got = inference.detect_cells(loader, m, dev, eps=11, method="distancetransform", thr_for_dt=thr_for_dt)
        assert len(got) == 2
        for i in range(2):
            want = E.detect(q[i], None, eps=11, thr_for_dt=thr_for_dt)
            assert np.array_equal(got[i][0], want[0]) and got[i][1] == [], (thr_for_dt, i)
    blur = inference.detect_cells(loader, m, dev, eps=11)
    explicit = inference.detect_cells(loader, m, dev, eps=11, method="gaussianblur")
    for i in range(2):
        assert np.array_equal(blur[i][0], explicit[i][0]) and np.array_equal(blur[i][0], R.detect(q[i], None, eps=11)[0])
