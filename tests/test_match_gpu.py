"""Object-level matching of label images on the GPU (csrc/regions.hip through cellsegmentation_amd.regions.match_labels), exact
against the dense-table statement tests/match_ref.py and the vectors of tests/golden/match_vectors.npz.  Every table is compared by
value (they are integers) and every ``LabelScore`` field bit for bit.  Shapes are tiny: widths either side of the 64-lane wave,
heights 1 and 3, and a few blob batches with ragged last segments."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import match_ref as M  # noqa: E402
import regions_ref as R  # noqa: E402
import split_ref as SR  # noqa: E402
from cellsegmentation_amd import inference  # noqa: E402
from cellsegmentation_amd import regions as G  # noqa: E402
from cellsegmentation_amd import score as S  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "match_vectors.npz"), allow_pickle=False)
NAMES = sorted(k[:-len(".pred")] for k in GOLD.files if k.endswith(".pred"))
THRESHOLDS = (0.5, 0.75, 1.0)


def _np(t):
    return t.cpu().numpy()


def assert_tables(got, ref):
    assert isinstance(got, G.MatchTable) and (got.cap_pred, got.cap_truth) == (ref["cap_pred"], ref["cap_truth"])
    for key in M.TABLES:
        t = getattr(got, key)
        assert t.is_cuda and t.dtype == torch.int32 and tuple(t.shape) == ref[key].shape, key
        assert np.array_equal(_np(t), ref[key]), key
    over = (ref["counts_pred"] > ref["cap_pred"]) | (ref["counts_truth"] > ref["cap_truth"])
    assert got.overflowed().dtype == torch.bool and np.array_equal(_np(got.overflowed()), over)


def assert_scores(got, ref, thresholds=THRESHOLDS):
    for thr in thresholds:
        s, want = got.score(thr), M.score(ref, thr)
        assert isinstance(s, S.LabelScore)
        for key in M.SCORES:
            a = getattr(s, key)
            assert a.dtype == want[key].dtype and a.tobytes() == want[key].tobytes(), (thr, key)


def check(pred, truth, max_regions=None, **kw):
    """match_labels on the device against the reference with the same capacities -> (MatchTable, reference)"""
    caps = (None, None) if max_regions is None else max_regions if isinstance(max_regions, tuple) else (max_regions, max_regions)
    ref = M.match(pred, truth, *caps)
    got = G.match_labels(pred, truth, max_regions=max_regions, **kw)
    assert_tables(got, ref)
    assert_scores(got, ref)
    return got, ref


@pytest.mark.parametrize("name", NAMES)
def test_golden_vectors(dev, name):
    pred, truth = GOLD[f"{name}.pred"], GOLD[f"{name}.truth"]
    got = G.match_labels(torch.from_numpy(pred).to(dev), truth, max_regions=tuple(int(c) for c in GOLD[f"{name}.caps"]))
    for key in M.TABLES:
        assert np.array_equal(_np(getattr(got, key)), GOLD[f"{name}.{key}"]), key
    for thr in THRESHOLDS:
        s = got.score(thr)
        for key in M.SCORES:
            assert getattr(s, key).tobytes() == GOLD[f"{name}.score{thr}.{key}"].tobytes(), (thr, key)


def test_hand_worked_known_answers(dev):
    def one(name):
        pred, truth, cp, ct = M.hand_cases()[name]
        caps = None if ct is None else (1, ct)
        return check(pred, truth, caps)[0]                              # a 2-D pair: one image of one row

    t = one("half_twice")                                               # IoU exactly 1/2, twice
    s = t.score()
    assert not _np(t.match).any() and not _np(t.match_truth).any() and (s.tp[0], s.fp[0], s.fn[0]) == (0, 1, 2)
    t = one("two_thirds")
    assert _np(t.match).tolist() == [[1]] and _np(t.inter).tolist() == [[2]] and _np(t.match_truth).tolist() == [[1]]
    assert t.score(0.5).tp[0] == 1 and t.score(0.75).tp[0] == 0 and t.score(0.75).fp[0] == 1
    t = one("false_candidate")                                          # the votes spell 3, which covers 40 %
    assert not _np(t.match).any() and not _np(t.inter).any() and _np(t.area_truth).tolist() == [[3, 3, 4]]
    t = one("out_of_range_candidate")                                   # the votes spell 7 with cap_truth = 6
    assert t.cap_truth == 6 and not _np(t.match).any() and not _np(t.match_truth).any()
    assert not _np(one("background_majority").match).any()
    t = one("identical_with_empty")
    s = t.score(1.0)
    assert _np(t.match).tolist() == [[1, 0, 3]] and _np(t.counts_pred).tolist() == [3]
    assert (s.n_pred[0], s.n_truth[0], s.tp[0], s.fp[0], s.fn[0], s.sq[0], s.pq[0]) == (2, 2, 2, 0, 0, 1.0, 1.0)


def test_many_labels_need_eleven_vote_bits(dev):
    b = M.blocks()
    cleared = b.copy()
    cleared[1::2, 1::2] = 0
    t, _ = check(b, cleared)
    assert t.cap_truth == 1024 and np.array_equal(_np(t.match)[0], np.arange(1, 1025)) and (_np(t.inter) == 3).all()
    assert (_np(t.iou()) == 0.75).all() and t.score(0.75).tp[0] == 1024
    t, _ = check(b, np.roll(b, 1, axis=1))                              # IoU 1/3 everywhere
    assert not _np(t.match).any() and t.score().fp[0] == 1024 and t.score().fn[0] == 1024


def _edge_pair(H, W, kind):
    pred, truth = np.zeros((H, W), np.int32), np.zeros((H, W), np.int32)
    lo, hi = max(0, 64 - 5), min(W, 64 + 7)
    if kind == "run_across_64":                                         # one run of both labels over the wave boundary
        pred[:, lo:hi], truth[:, max(0, lo - 1):hi] = 1, 2
    elif kind == "pred_changes_at_64":                                  # ... under a constant truth label
        pred[:, lo:64], truth[:, lo:hi] = 1, 1
        pred[:, 64:hi] = 2
    elif kind == "truth_changes_at_64":
        truth[:, lo:64], pred[:, lo:hi] = 1, 1
        truth[:, 64:hi] = 2
    elif kind == "two_pred_under_one_truth":                            # adjacent pred labels inside one wave: the run must break
        k = max(1, min(W, 40) // 3)
        pred[:, :k], pred[:, k:3 * k] = 1, 2
        truth[:, :3 * k] = 1
    elif kind == "two_truth_under_one_pred":
        k = max(1, min(W, 40) // 3)
        truth[:, :k], truth[:, k:3 * k] = 1, 2
        pred[:, :3 * k] = 1
    elif kind == "full":                                                # first and last lane, every segment
        pred[:], truth[:] = 1, 1
        truth[:, W - 1] = 2
    elif kind == "alternating":                                         # runs of one
        pred[:, 0::2], truth[:, 0::2] = 1, 1
        truth[:, 1::2] = 2
    if H > 1:
        pred[1], truth[1] = np.roll(pred[1], 1), np.where(truth[1] > 0, 3, 0)
    return pred, truth


@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("W", [1, 63, 64, 65, 129])
def test_wave_and_run_edges(dev, H, W):
    kinds = ("run_across_64", "pred_changes_at_64", "truth_changes_at_64", "two_pred_under_one_truth", "two_truth_under_one_pred",
             "full", "alternating")
    pairs = [_edge_pair(H, W, k) for k in kinds]
    check(np.stack([p for p, _ in pairs]), np.stack([t for _, t in pairs]))          # one batch of all of them
    for p, t in pairs[:3]:
        check(p, t, max_regions=(2, 3))


BLOBS = [((5, 70), 1 / 40.0, 23), ((63, 65), 1 / 150.0, 21), ((130, 67), 1 / 150.0, 22), ((97, 200), 1 / 150.0, 23)]
_PAIRS = {}


def blob_pair(shape):
    """(pred, truth) int32 [3, H, W] for a shape of BLOBS, made once: label of random discs, and of the same mask rolled and
    noised"""
    if shape not in _PAIRS:
        density, seed = next((d, s) for sh, d, s in BLOBS if sh == shape)
        masks = R.blobs(3, *shape, seed=seed, density=density)
        _PAIRS[shape] = M.noisy_pair(masks, seed + 10, lambda m: R.label(m, 1)[0])
    return _PAIRS[shape]


@pytest.mark.parametrize("shape", [b[0] for b in BLOBS])
def test_random_blobs_in_a_batch(dev, shape):
    pred, truth = blob_pair(shape)
    got, ref = check(pred, truth)
    objects, matched = int((ref["area_pred"] > 0).sum()), int((ref["match"] > 0).sum())
    print(f"{shape}: the reference matches {matched} of {objects} objects")
    assert 0 < matched < objects                                        # both sides of the decision are exercised
    assert np.array_equal(_np(G.label(torch.from_numpy(pred > 0).to(dev), 1)), pred)     # (pred is what the device labels, too)
    # pred from a split at random seeds: dead seeds and doubles leave empty labels
    masks = pred > 0
    pts, off = SR.random_seeds(masks, 7, seed=shape[1])
    pts[off[1] + 1] = pts[off[1]]                                       # two seeds on one pixel
    parts = G.split(masks, pts, off)
    lab = _np(parts.labels)
    assert np.array_equal(lab, SR.split(masks, pts, off)["labels"])
    check(lab, truth)                                                   # the counts found on the device: the largest labels
    counts = _np(parts.counts)                                          # ... and split's own, which also count empty last labels
    ref = M.match(lab, truth, max(1, int(counts.max())), None)
    ref["counts_pred"] = counts
    got = G.match_labels(parts.labels, truth, pred_counts=parts.counts)
    assert_tables(got, ref)
    assert_scores(got, ref)
    present = np.zeros((3, got.cap_pred + 1), bool)
    for n in range(3):
        present[n, np.unique(lab[n])] = True
    assert (~present[:, 1:] & (np.arange(1, got.cap_pred + 1) <= _np(parts.counts)[:, None])).any()       # an empty label below the count
    assert np.array_equal(_np(got.area_pred) > 0, present[:, 1:])
    assert np.array_equal(got.score().n_pred, present[:, 1:].sum(axis=1))               # empty labels are no false positives


def test_capacity(dev):
    pred, truth = blob_pair((63, 65))
    full = M.match(pred, truth)
    cp, ct = full["cap_pred"], full["cap_truth"]
    assert cp > 4 and ct > 4
    for caps in ((3, ct), (cp, 4), (3, 4), (cp + 5, ct + 9), 5):
        got, ref = check(pred, truth, caps)
        assert np.array_equal(_np(got.counts_pred), full["counts_pred"]) and np.array_equal(_np(got.counts_truth), full["counts_truth"])
    got, _ = check(pred, truth, (3, 4))
    assert _np(got.overflowed()).any()
    # the rows are those of the images with the over-capacity labels taken for background
    clipped = M.match(np.where(pred > 3, 0, pred), np.where(truth > 4, 0, truth), 3, 4)
    for key in M.TABLES[2:]:
        assert np.array_equal(_np(getattr(got, key)), clipped[key]), key
    free, exact = G.match_labels(pred, truth), G.match_labels(pred, truth, max_regions=(cp, ct))
    assert (free.cap_pred, free.cap_truth) == (cp, ct) and not _np(free.overflowed()).any()
    for key in M.TABLES:
        assert torch.equal(getattr(free, key), getattr(exact, key)), key
    empty = G.match_labels(np.zeros((2, 3, 4), np.int32), np.full((2, 3, 4), -7, np.int32))          # no label at all: capacity 1
    assert (empty.cap_pred, empty.cap_truth) == (1, 1) and not _np(empty.area_pred).any() and empty.score().pq.tolist() == [0.0, 0.0]
    assert empty.score().precision.tolist() == [1.0, 1.0]


def test_batches_cut_into_chunks(dev, monkeypatch):
    pred, truth = blob_pair((63, 65))
    pred, truth = np.concatenate([pred, pred[:2]]), np.concatenate([truth, truth[1:]])
    whole, _ = check(pred, truth)
    monkeypatch.setattr(G, "_MAX_PIXELS", 2 * 63 * 65 + 40)             # two images per call: 2 + 2 + 1
    assert [b - a for a, b in G._chunks(torch.empty(5, 63, 65))] == [2, 2, 1]
    for kw in ({}, {"max_regions": (whole.cap_pred, 7)}):
        got, _ = check(pred, truth, **kw)
        if not kw:
            for key in M.TABLES:
                assert torch.equal(getattr(got, key), getattr(whole, key)), key


def test_two_runs_identical_and_graph_replay(dev):
    pred, truth = blob_pair((130, 67))
    a, b = G.match_labels(pred, truth), G.match_labels(pred, truth)
    for key in M.TABLES:
        assert _np(getattr(a, key)).tobytes() == _np(getattr(b, key)).tobytes(), key
    caps = (a.cap_pred + 3, a.cap_truth + 3)
    dp, dt = torch.from_numpy(pred).to(dev), torch.from_numpy(truth).to(dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        G.match_labels(dp, dt, max_regions=caps)                        # warm-up
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = G.match_labels(dp, dt, max_regions=caps)
    # new contents of the same shape: the images swap sides and the batch is reversed
    new_pred, new_truth = np.ascontiguousarray(truth[::-1]), np.ascontiguousarray(pred[::-1])
    new_truth = np.where(new_truth > a.cap_pred - 2, 0, new_truth)      # (keep both sides within the captured capacities)
    dp.copy_(torch.from_numpy(new_pred))
    dt.copy_(torch.from_numpy(new_truth))
    graph.replay()
    torch.cuda.synchronize()
    ref = M.match(new_pred, new_truth, *caps)
    assert_tables(got, ref)
    assert_scores(got, ref)
    assert ref["counts_pred"].max() > caps[0] and _np(got.overflowed()).any()         # the replayed pred side overflows its capacity


def test_iou_and_threshold_sweep(dev):
    pred, truth = blob_pair((97, 200))
    got, ref = check(pred, truth)
    q, want = _np(got.iou()), M.iou(ref)
    assert got.iou().is_cuda and q.dtype == np.float64 and q.shape == want.shape
    assert np.array_equal(q == 0, want == 0) and (np.abs(q - want) <= np.spacing(want)).all()       # within 1 ulp
    assert ((want > 0.5) == (ref["match"] > 0)).all()
    sweep = [got.score(t).tp.sum() for t in THRESHOLDS]
    assert sweep[0] >= sweep[1] >= sweep[2] and sweep[0] > sweep[2]


@pytest.mark.parametrize("reg_limit", [False, True])
def test_evaluate_instances_resnet18(dev, reg_limit):
    import detect_ref
    from cellsegmentation_amd import synth
    from cellsegmentation_amd.model import resnet as RN
    m = RN.MILresnet18()
    sd = m.state_dict()
    synth.fill_state_dict(sd)
    m.load_state_dict(sd)
    m = m.to(dev).set_compute_dtype(torch.float32)
    m.setmode("segment")
    x = synth.normalise(synth.ihc_tiles(2, 299, seed=21))
    images = [x[:1], x[1:]]
    probs = inference.inference_seg(images, m, dev, mode="test")
    thr = float(np.median(probs))
    thr_for_dt = int(np.median(detect_ref.quantize(probs)))             # random weights need not straddle the default 10
    kw = dict(eps=11, method="distancetransform", thr_for_dt=thr_for_dt)
    # truth: the cleaned segmentation itself, rolled a little, as uint8 0 / 255 masks and as the label images they stand for
    classes = _np(inference.segment_classes(images, m, dev, thr, reg_limit=reg_limit))
    masks = np.stack([np.roll(c, (2, -3), axis=(0, 1)) for c in classes]).astype(np.uint8) * 255
    labels = np.stack([R.label(k != 0, 1)[0] for k in masks]).astype(np.int32)
    cells = inference.detect_cells(images, m, dev, reg_limit=reg_limit, **kw)
    parts = [SR.split(classes[i], cells[i][0]) for i in range(2)]
    for truth, iou_thr in ((masks, 0.5), (labels, 0.9)):
        loader = [(images[0], torch.from_numpy(truth[:1]), "unused"), (images[1], torch.from_numpy(truth[1:]))]
        out = inference.evaluate_instances(loader, m, dev, threshold=thr, iou_threshold=iou_thr, reg_limit=reg_limit, **kw)
        assert m.mode == "segment"
        assert sorted(out) == sorted(["n_pred", "n_truth", "tp", "fp", "fn", "p", "r", "f1", "sq", "pq", "mean"])
        for i in range(2):
            want = M.score(M.match(parts[i]["labels"], labels[i]), iou_thr)
            for key, name in zip(("n_pred", "n_truth", "tp", "fp", "fn", "p", "r", "f1", "sq", "pq"), M.SCORES):
                assert out[key][i:i + 1].tobytes() == want[name].tobytes(), (key, i)
        assert out["mean"] == tuple(float(out[k].mean()) for k in ("p", "r", "f1", "sq", "pq"))
    if not reg_limit:
        assert out["n_pred"].sum() > 0 and out["n_truth"].sum() > 0
