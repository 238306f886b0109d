"""Stain separation and normalisation on the GPU (csrc/stain.hip) against the float64 restatement tests/stain_ref.py: the integer
moments bit for bit, the two histograms and the estimate to one bin width, apply and the uint8 separation to one level, the fp32
separation to its rounding bound; detect_slide(stain=...) against detect_slide on the normalised slide and against the loop
composed here; measure_slide_cells(intensity=...) against measure_labels."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import stain_ref as R  # noqa: E402
import tissue_ref as TR  # noqa: E402
from shifted import shifted  # noqa: E402
from cellsegmentation_amd import detect as D  # noqa: E402
from cellsegmentation_amd import kernels as K  # noqa: E402
from cellsegmentation_amd import stain, tiles, tissue  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(ROOT, "tests", "golden", "stain_vectors.npz"), allow_pickle=False)
NAMES = [str(n) for n in GOLD["names"]]
BIG = "synth_96x96_seed0"
OPTS = stain.StainOptions()
ANGLE_BIN = math.pi / OPTS.angle_bins
CONC_BIN = OPTS.conc_max / OPTS.conc_bins
MAX_OD = math.log(256.0)                                                   # 5.55: no optical density is larger


def batch_of(name):
    images = GOLD[f"{name}.images"]
    return images if images.ndim == 4 else images[None]


def gold(name, key):
    a = GOLD[f"{name}.{key}"]
    return a if GOLD[f"{name}.images"].ndim == 4 else a[None]


def _od(dev):
    return torch.from_numpy(stain.od_table(OPTS.Io)).to(dev)


def _f32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def _shifted(a, shift, dev):
    return shifted(a, shift, dev)[0]


def _mask_for(shape, seed):
    m = (np.random.RandomState(seed).randint(0, 3, size=shape) * 100).astype(np.uint8)     # non-zero values other than 1 keep as well
    return m


@pytest.fixture(scope="module")
def big():
    """the reference's estimate of the 96x96 case, computed once and shared"""
    return R.estimate(GOLD[f"{BIG}.images"])


@pytest.fixture(scope="module")
def dense():
    """(the dense fixture, the reference's estimate of it): the blobs of the 96x96 case repeated 22 x 22 times under fresh floor and
    noise.  tests/test_stain_host.py shows on the reference alone that its angles and concentrations are dense enough around the
    chosen order statistics for a tolerance of one bin width; no 96x96 image is."""
    image = R.synth_hdab(96, 96, seed=0, tile=R.DENSE_TILE)
    return image, R.estimate(image)


# ---- moments ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_moments_bit_equal_on_the_pinned_cases(dev, name):
    images = batch_of(name)
    x, od = torch.from_numpy(images).to(dev), _od(dev)
    got = K.stain_moments(x, od, OPTS.beta_q)
    assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), gold(name, "moments"))
    mask = _mask_for(images.shape[:3], 5)
    want = R.moments(images, mask)
    assert np.array_equal(K.stain_moments(x, od, OPTS.beta_q, torch.from_numpy(mask).to(dev)).cpu().numpy(), want)
    assert (want[:, 0] <= gold(name, "moments")[:, 0]).all()
    # the same bytes at other addresses: the single pixels before the first 16-byte boundary, the three kinds of mask load
    for shift_in, shift_mask in ((1, 0), (7, 4), (12, 3), (0, 9)):
        got = K.stain_moments(_shifted(images, shift_in, dev), od, OPTS.beta_q, _shifted(mask, shift_mask, dev))
        assert np.array_equal(got.cpu().numpy(), want), (shift_in, shift_mask)


def test_moments_several_workgroups_301x517(dev):
    img = R.synth_hdab(301, 517, seed=7, n_h=300, n_dab=150)
    assert 517 % 16 and 301 * 517 // 16 > 256
    mask = _mask_for((301, 517), 8)
    od = _od(dev)
    for m in (None, mask):
        want = R.moments(img, m)
        got = K.stain_moments(torch.from_numpy(img).to(dev)[None], od, OPTS.beta_q, None if m is None else torch.from_numpy(m).to(dev)[None])
        assert want[0] > 1000 and np.array_equal(got.cpu().numpy()[0], want)
    other = stain.StainOptions(Io=255, beta=0.3)                            # another table and threshold
    got = K.stain_moments(torch.from_numpy(img).to(dev)[None], torch.from_numpy(stain.od_table(255)).to(dev), other.beta_q)
    assert np.array_equal(got.cpu().numpy()[0], R.moments(img, None, 255, 0.3))


def test_grid_cap_strides_over_a_large_image(dev):
    """2912 x 2903 pixels are more runs of 16 than the capped grid has threads: some threads take two"""
    rng = np.random.RandomState(4)
    img = rng.randint(0, 256, size=(2912, 2903, 3)).astype(np.uint8)
    img[1000:2000] = (236, 228, 231)
    assert img.size // 3 // 16 > 2048 * 256
    x, od = torch.from_numpy(img).to(dev)[None], _od(dev)
    want = R.moments(img)
    assert np.array_equal(K.stain_moments(x, od, OPTS.beta_q).cpu().numpy()[0], want)
    assert int(K.stain_angle_hist(x, od, OPTS.beta_q, _f32(R.HDAB[None], dev), 64).sum()) == want[0]
    assert int(K.stain_conc_hist(x, od, OPTS.beta_q, _f32(np.linalg.pinv(R.HDAB)[None], dev), 64, 4.0).sum()) == 2 * want[0]
    A = R.normalizer(R.HDAB, (1.5, 0.7))
    diff = K.stain_apply(x, od, _f32(A[None], dev), OPTS.Io).cpu().numpy()[0].astype(np.int16) - R.apply(img, A)[0]
    assert np.abs(diff).max() <= 1
    u8 = K.stain_separate(x, od, _f32(np.linalg.pinv(R.HDAB)[None], dev), True, 8.0).cpu().numpy()[0].astype(np.int16)
    assert np.abs(u8 - R.separate_u8(img, R.HDAB)).max() <= 1


def test_moments_of_an_image_one_byte_into_a_buffer_and_accumulation(dev):
    img = GOLD["odd_37x53.images"]
    od = _od(dev)
    buf = torch.zeros((img.size + 64,), dtype=torch.uint8, device=dev)
    view = buf[1:1 + img.size].view(1, 37, 53, 3)
    view.copy_(torch.from_numpy(img))
    first = K.stain_moments(view, od, OPTS.beta_q)
    assert np.array_equal(first.cpu().numpy()[0], GOLD["odd_37x53.moments"])
    seed = torch.arange(10, dtype=torch.int64, device=dev).reshape(1, 10) * (1 << 40) + 3       # beyond 32 bits: 64-bit adds
    acc = seed.clone()
    assert K.stain_moments(view, od, OPTS.beta_q, out=acc) is acc and torch.equal(acc, seed + first)
    K.stain_moments(view, od, OPTS.beta_q, out=acc)
    assert torch.equal(acc, seed + 2 * first)


# ---- the two histograms, given the reference's V and P ------------------------------------------------------------------------------
def _angles_selected(dev, image, ref):
    """the angle histogram of one image with the reference's V: its total is the kept count, the bins that hold the two order
    statistics have their centres within one bin width of the reference's -> (the histogram tensor, its numpy copy)"""
    x, od = torch.from_numpy(image).to(dev)[None], _od(dev)
    hist = K.stain_angle_hist(x, od, OPTS.beta_q, _f32(ref["V"][None], dev), OPTS.angle_bins)
    assert hist.dtype == torch.int64 and tuple(hist.shape) == (1, OPTS.angle_bins)
    h = hist.cpu().numpy()[0]
    assert h.sum() == ref["n_kept"]
    for k in (ref["k_lo"], ref["k_hi"]):
        phi = -math.pi / 2 + (stain.order_bin(h, k) + 0.5) * ANGLE_BIN
        print(f"{image.shape[0]}x{image.shape[1]} rank {k}: bin centre {phi:.6f}, reference {ref['phi'][k]:.6f}, "
              f"{abs(phi - ref['phi'][k]) / ANGLE_BIN:.3f} bins apart")
        assert abs(phi - ref["phi"][k]) <= ANGLE_BIN
    return x, od, hist, h


def test_angle_histogram_selects_the_reference_angles(dev, big, dense):
    _angles_selected(dev, *dense)                                          # the fixture whose density the tolerance rests on
    x, od, hist, h = _angles_selected(dev, GOLD[f"{BIG}.images"], big)
    assert h.sum() == GOLD[f"{BIG}.n_kept"]
    again = K.stain_angle_hist(x, od, OPTS.beta_q, _f32(big["V"][None], dev), OPTS.angle_bins, out=hist)
    assert again is hist and np.array_equal(hist.cpu().numpy()[0], 2 * h)   # it adds, and repeats itself
    mask = _mask_for((1, 96, 96), 9)
    hm = K.stain_angle_hist(x, od, OPTS.beta_q, _f32(big["V"][None], dev), 300, torch.from_numpy(mask).to(dev)).cpu().numpy()[0]
    assert hm.shape == (300,) and hm.sum() == R.moments(GOLD[f"{BIG}.images"], mask[0])[0]


def _max_conc_selected(dev, image, ref):
    """the concentration histogram of one image with the reference's P: both totals are the kept count, max_conc from it is within
    one bin width of the reference's -> (x, od, its numpy copy)"""
    x, od = torch.from_numpy(image).to(dev)[None], _od(dev)
    hist = K.stain_conc_hist(x, od, OPTS.beta_q, _f32(ref["P"][None], dev), OPTS.conc_bins, OPTS.conc_max)
    assert hist.dtype == torch.int64 and tuple(hist.shape) == (1, 2, OPTS.conc_bins)
    h = hist.cpu().numpy()[0]
    assert h[0].sum() == ref["n_kept"] and h[1].sum() == ref["n_kept"]
    got = stain.max_conc_of_hist(h, OPTS.conc_max)
    print(f"{image.shape[0]}x{image.shape[1]} max_conc", got, "reference", ref["max_conc"], "bins apart", np.abs(got - ref["max_conc"]) / CONC_BIN)
    assert np.abs(got - ref["max_conc"]).max() <= CONC_BIN
    return x, od, h


def test_concentration_histogram_selects_the_reference_max_conc(dev, big, dense):
    _max_conc_selected(dev, *dense)                                        # the fixture whose density the tolerance rests on
    x, od, h = _max_conc_selected(dev, GOLD[f"{BIG}.images"], big)
    assert h[:, 0].min() > 0                                               # concentrations below 0 land in bin 0
    few = K.stain_conc_hist(x, od, OPTS.beta_q, _f32(big["P"][None], dev), 7, 2.0).cpu().numpy()[0]
    assert few.shape == (2, 7) and (few.sum(axis=1) == big["n_kept"]).all() and few[:, 6].min() > 0      # and above conc_max in the last


# ---- estimate -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_estimate_equals_its_stages_and_the_reference(dev, name):
    images = batch_of(name)
    x, od = torch.from_numpy(images).to(dev), _od(dev)
    got = stain.estimate(images)
    got = got if isinstance(got, list) else [got]
    assert len(got) == len(images)
    moments = K.stain_moments(x, od, OPTS.beta_q).cpu().numpy()
    for i, e in enumerate(got):
        assert isinstance(e, stain.StainEstimate) and e.n_kept == gold(name, "n_kept")[i] == moments[i, 0] and e.ok == bool(gold(name, "ok")[i])
        if not e.ok:
            assert np.array_equal(e.vectors, stain.HDAB) and e.max_conc.tolist() == [1, 1]
            continue
        one = x[i:i + 1]
        V = stain.plane_of_moments(moments[i])
        angles = K.stain_angle_hist(one, od, OPTS.beta_q, _f32(V[None], dev), OPTS.angle_bins).cpu().numpy()[0]
        S = stain.vectors_of_hist(V, angles, OPTS.alpha)
        conc = K.stain_conc_hist(one, od, OPTS.beta_q, _f32(np.linalg.pinv(S)[None], dev), OPTS.conc_bins, OPTS.conc_max).cpu().numpy()[0]
        assert np.array_equal(e.vectors, S) and np.array_equal(e.max_conc, stain.max_conc_of_hist(conc, OPTS.conc_max))
        off = [R.angle_between(e.vectors[:, k], gold(name, "vectors")[i][:, k]) for k in range(2)]
        print(f"{name}[{i}]: {e.n_kept} kept, vectors {off[0] / ANGLE_BIN:.3f} and {off[1] / ANGLE_BIN:.3f} bins from the reference's")
        assert max(off) <= ANGLE_BIN and abs(np.linalg.norm(e.vectors, axis=0) - 1).max() < 1e-12 and e.vectors[0, 0] >= e.vectors[0, 1]


def test_estimate_under_a_mask_and_on_the_device(dev):
    img = GOLD[f"{BIG}.images"]
    mask = np.zeros((96, 96), bool)
    mask[:, 40:] = True
    e = stain.estimate(torch.from_numpy(img).to(dev), mask=mask)
    ref = R.estimate(img, mask)
    assert e.ok and e.n_kept == ref["n_kept"] < GOLD[f"{BIG}.n_kept"]
    assert max(R.angle_between(e.vectors[:, k], ref["vectors"][:, k]) for k in range(2)) <= ANGLE_BIN
    assert stain.estimate(img, mask=np.zeros((96, 96), np.uint8)).ok is False


# ---- apply and normalize ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_apply_within_one_level_of_the_reference(dev, name):
    images, A = batch_of(name), gold(name, "A")
    got = K.stain_apply(torch.from_numpy(images).to(dev), _od(dev), _f32(A, dev), OPTS.Io)
    assert got.dtype == torch.uint8 and tuple(got.shape) == images.shape
    diff = np.abs(got.cpu().numpy().astype(np.int32) - gold(name, "normalized").astype(np.int32))
    print(f"{name}: {np.count_nonzero(diff)} of {diff.size} bytes differ, by at most {diff.max()}")
    assert diff.max() <= 1
    want = got.cpu().numpy()
    for shift_in, shift_out in ((1, 0), (7, 4), (12, 3), (0, 9)):           # the 16-byte, dword and byte stores
        out = _shifted(np.full(images.shape, 7, np.uint8), shift_out, dev)
        assert K.stain_apply(_shifted(images, shift_in, dev), _od(dev), _f32(A, dev), OPTS.Io, out=out) is out
        assert np.array_equal(out.cpu().numpy(), want), (shift_in, shift_out)


def test_apply_several_workgroups_and_clamps(dev):
    img = R.synth_hdab(301, 517, seed=7, n_h=300, n_dab=150)
    for A in (R.normalizer(R.HDAB, (1.5, 0.7)), -0.2 * np.eye(3), 40 * np.eye(3)):             # the last two clamp at 255 and at 0
        got = K.stain_apply(torch.from_numpy(img).to(dev)[None], _od(dev), _f32(A[None], dev), OPTS.Io).cpu().numpy()[0]
        want, exact = R.apply(img, A)
        diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
        assert diff.max() <= 1 and (np.abs(exact.clip(0, 255) - got)[diff > 0] > 0.49).all()      # only a rounding tie differs


def test_normalize_is_apply_with_its_own_estimate(dev):
    for name in (BIG, "batch_of_three", "all_white"):
        images = GOLD[f"{name}.images"]
        got = stain.normalize(images)
        est = stain.estimate(images)
        est = est if isinstance(est, list) else [est]
        A = np.stack([stain.normalizer(e, stain.TARGET_HDAB) for e in est])
        want = K.stain_apply(torch.from_numpy(batch_of(name)).to(dev), _od(dev), _f32(A, dev), OPTS.Io)
        assert got.is_cuda and tuple(got.shape) == images.shape and torch.equal(got.reshape(want.shape), want)
        diff = np.abs(got.cpu().numpy().astype(np.int32) - GOLD[f"{name}.normalized"].astype(np.int32))
        print(f"{name}: normalize differs from the reference's by at most {diff.max()} levels, mean {diff.mean():.4f}")
    img = GOLD[f"{BIG}.images"]
    mine = stain.StainEstimate(R.HDAB[:, ::-1], [2.0, 1.5])
    est = stain.estimate(img)
    given = stain.normalize(img, source=est, target=mine)                   # a given source and a target of the caller's
    want = K.stain_apply(torch.from_numpy(img).to(dev)[None], _od(dev), _f32(stain.normalizer(est, mine)[None], dev), OPTS.Io)
    assert torch.equal(given, want[0]) and not torch.equal(given, stain.normalize(img))
    out = torch.empty((1, 96, 96, 3), dtype=torch.uint8, device=dev)
    assert stain.normalize(img, source=mine, target=mine, out=out) is out
    assert (out[0].cpu().numpy().astype(np.int32) - R.apply(img, R.HDAB[:, ::-1] @ np.linalg.pinv(R.HDAB[:, ::-1]))[0]).__abs__().max() <= 1


# ---- separate -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_separate_against_the_reference(dev, name):
    images = GOLD[f"{name}.images"]
    for residual, key, Kn in ((False, "sep", 2), (True, "sep3", 3)):
        P = np.linalg.pinv(R.stain_matrix(R.HDAB, residual))
        bound = 4 * 2.0 ** -23 * np.abs(P).sum(axis=1) * MAX_OD            # three fp32 products and two adds per concentration
        got = stain.separate(images, dtype="float", residual=residual)
        assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == images.shape[:-1] + (Kn,)
        err = np.abs(got.cpu().numpy().astype(np.float64) - GOLD[f"{name}.{key}"]).reshape(-1, Kn).max(axis=0)
        print(f"{name} K={Kn}: fp32 error {err} of the bound {bound}")
        assert (err <= bound).all()
        u8 = stain.separate(torch.from_numpy(images), stains=stain.TARGET_HDAB, dtype="u8", residual=residual)
        assert u8.dtype == torch.uint8 and tuple(u8.shape) == images.shape[:-1] + (Kn,)
        assert np.abs(u8.cpu().numpy().astype(np.int32) - GOLD[f"{name}.{key}_u8"].astype(np.int32)).max() <= 1
        # the stores of the other alignments: fp32 is at least dword aligned
        x, Pd = batch_of(name), _f32(np.repeat(P[None], len(batch_of(name)), axis=0), dev)
        for shift_in, shift_f, shift_b in ((1, 0, 0), (7, 4, 4), (12, 8, 3), (0, 12, 9)):
            of = _shifted(np.zeros(x.shape[:3] + (Kn,), np.float32), shift_f, dev)
            ob = _shifted(np.zeros(x.shape[:3] + (Kn,), np.uint8), shift_b, dev)
            K.stain_separate(_shifted(x, shift_in, dev), _od(dev), Pd, False, out=of)
            K.stain_separate(_shifted(x, shift_in, dev), _od(dev), Pd, True, OPTS.conc_max, out=ob)
            assert torch.equal(of.reshape(got.shape), got) and torch.equal(ob.reshape(u8.shape), u8), (shift_in, shift_f, shift_b)


def test_separate_with_an_estimate_and_another_range(dev):
    img = R.synth_hdab(301, 517, seed=7, n_h=300, n_dab=150)
    est = stain.estimate(img)
    want, P = R.separate(img, est.vectors)
    got = stain.separate(img, stains=est)
    assert (np.abs(got.cpu().numpy() - want).reshape(-1, 2).max(axis=0) <= 4 * 2.0 ** -23 * np.abs(P).sum(axis=1) * MAX_OD).all()
    u8 = stain.separate(img, stains=est, dtype="u8", options=stain.StainOptions(conc_max=2.5)).cpu().numpy()
    assert np.abs(u8.astype(np.int32) - R.separate_u8(img, est.vectors, conc_max=2.5)).max() <= 1 and u8.max() == 255 and u8.min() == 0


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(dev):
    from cellsegmentation_amd import synth
    from cellsegmentation_amd.model import resnet as RN
    m = RN.MILresnet18()
    sd = m.state_dict()
    synth.fill_state_dict(sd)
    m.load_state_dict(sd)
    return m.to(dev).set_compute_dtype(torch.float32)


KW = dict(batch_size=4, patch_size=64, interval=48, eps=11, thr=-0.01)


def _same(a, b):
    assert torch.equal(a.mask, b.mask) and a.cell_count == b.cell_count
    assert np.array_equal(a.points, b.points) and np.array_equal(a.discarded, b.discarded)


def test_detect_slide_normalises_the_slide_first(dev, model):
    from cellsegmentation_amd import inference
    slide = TR.blob_slide(seed=31)
    plain = inference.detect_slide(slide, model, dev, **KW)
    none = inference.detect_slide(slide, model, dev, stain=None, **KW)
    assert plain.stain is None and none.stain is None
    _same(none, plain)                                                      # stain=None is the parent's path
    norm = stain.normalize(slide)
    assert not torch.equal(norm.cpu(), torch.from_numpy(slide))
    want = inference.detect_slide(norm, model, dev, **KW)
    got = inference.detect_slide(slide, model, dev, stain=True, **KW)
    _same(got, want)
    assert len(got.points) + len(got.discarded) > 0 and got.tissue is None and model.mode == "segment" and not model.training
    est = stain.estimate(slide)
    assert isinstance(got.stain, stain.StainEstimate) and got.stain.ok and got.stain.n_kept == est.n_kept > 100
    assert np.array_equal(got.stain.vectors, est.vectors) and np.array_equal(got.stain.max_conc, est.max_conc)
    # options and a target of the caller's; detect_slides passes the argument on
    opts, target = stain.StainOptions(alpha=2.0, beta=0.2), stain.StainEstimate(R.HDAB[:, ::-1], [1.2, 0.8])
    want = inference.detect_slide(stain.normalize(slide, target=target, options=opts), model, dev, **KW)
    _same(inference.detect_slide(slide, model, dev, stain=(opts, target), **KW), want)
    _same(next(inference.detect_slides([slide], model, dev, stain=(opts, target), **KW)), want)
    _same(inference.detect_slide(slide, model, dev, stain=stain.StainOptions(), **KW), got)


def test_detect_slide_with_stain_and_tissue(dev, model):
    """the tissue decision is taken on the slide as scanned, the estimate over its mask, the loop reads the normalised copy"""
    from cellsegmentation_amd import inference
    slide = TR.blob_slide(seed=31)
    sel = tissue.select_patches(slide, 64, 48)
    assert 0 < sel.n_selected < len(sel.corners)
    norm = stain.normalize(slide, mask=sel.mask)
    rc = torch.from_numpy(np.asarray(sel.selected_corners, np.int32).reshape(-1, 2)).to(dev)
    mask = torch.zeros((150, 170), dtype=torch.uint8, device=dev)
    count = torch.zeros((), dtype=torch.float64, device=dev)
    model.eval()
    with torch.no_grad():
        for i in range(0, len(rc), 4):
            x = tiles.gather_tiles(norm[None], np.zeros(len(rc[i:i + 4]), np.int32), rc[i:i + 4], 64, torch.float32)
            model.setmode("segment")
            K.stitch_logits(mask, model(x).float().contiguous(), rc[i:i + 4], 1)
            model.setmode("image")
            count += torch.round(model(x)[1][:, 0].float()).sum(dtype=torch.float64)
    model.setmode("segment")
    want = D.detect_points(mask, cell_counts=int(count.item()), eps=11, thr=-0.01).per_image()[0]
    got = inference.detect_slide(slide, model, dev, stain=True, tissue=True, **KW)
    assert torch.equal(got.mask, mask) and got.cell_count == int(count.item())
    assert np.array_equal(got.points, want[0]) and np.array_equal(got.discarded, want[1]) and got.mask.any()
    assert got.tissue.n_selected == sel.n_selected and torch.equal(got.tissue.mask, sel.mask) and torch.equal(got.tissue.selected, sel.selected)
    masked = stain.estimate(slide, mask=sel.mask)
    assert np.array_equal(got.stain.vectors, masked.vectors) and got.stain.n_kept == masked.n_kept <= stain.estimate(slide).n_kept
    alone = inference.detect_slide(slide, model, dev, tissue=True, **KW)    # tissue alone is the parent's path
    assert alone.stain is None and torch.equal(alone.tissue.selected, sel.selected)


def test_measure_slide_cells_takes_an_intensity_map(dev):
    from cellsegmentation_amd import inference, regions
    img = R.synth_hdab(120, 140, seed=12)
    dab = stain.separate(img, dtype="u8", options=stain.StainOptions(conc_max=3.0))[..., 1].contiguous()
    assert dab.dtype == torch.uint8 and tuple(dab.shape) == (120, 140) and dab.max() > 100
    yy, xx = np.mgrid[0:120, 0:140]
    centres = np.asarray([(30, 30), (30, 90), (80, 50), (90, 110), (83, 56)], np.int64)
    prob = np.zeros((120, 140), np.uint8)
    for r, c in centres:
        prob[(yy - r) ** 2 + (xx - c) ** 2 <= 81] = 200
    res = inference.SlideResult(centres, [], len(centres), torch.from_numpy(prob).to(dev))
    kw = dict(min_object_size=20, hole_area_threshold=0)
    base, base_parts = inference.measure_slide_cells(res, **kw)
    for given in (dab, dab.cpu().numpy()):
        table, parts = inference.measure_slide_cells(res, intensity=given, **kw)
        assert torch.equal(parts.labels, base_parts.labels) and torch.equal(table.area, base.area)       # the labels come from the mask
        want = regions.measure_labels(parts.labels, intensity=dab, counts=parts.counts)
        for f in ("counts", "area", "bbox", "sum_rc", "intensity_sum", "intensity_max"):
            assert torch.equal(getattr(table, f), getattr(want, f)), f
    assert not torch.equal(table.intensity_sum, base.intensity_sum) and int(table.area.sum()) > 0
    lab = parts.labels.cpu().numpy().reshape(120, 140)
    k = int(np.argmax(table.area.cpu().numpy()[0]))
    assert int(table.intensity_sum[0, k]) == int(dab.cpu().numpy()[lab == k + 1].astype(np.int64).sum())
