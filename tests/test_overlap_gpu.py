"""Overlap tables of label images on the GPU (csrc/regions.hip through cellsegmentation_amd.regions.overlap_labels), exact against
the dense-table statement tests/overlap_ref.py and the vectors of tests/golden/overlap_vectors.npz: every integer table and the
sorted pair list by value, the floats of ``OverlapTable.score`` within 1e-12 (sums of at most a few thousand float64 terms in
[0, 1]).  Shapes are the smallest at which each mechanism can go wrong: one-row hand cases, widths either side of the 64-lane
segments, 1024 labels with four partners each, tables filled to the brim and beyond."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import match_ref as M  # noqa: E402
import overlap_ref as O  # noqa: E402
import regions_ref as R  # noqa: E402
import split_ref as SR  # noqa: E402
from cellsegmentation_amd import inference  # noqa: E402
from cellsegmentation_amd import kernels as K  # noqa: E402
from cellsegmentation_amd import regions as G  # noqa: E402
from cellsegmentation_amd import score as S  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "overlap_vectors.npz"), allow_pickle=False)
NAMES = sorted(k[:-len(".pred")] for k in GOLD.files if k.endswith(".pred"))
TOL = 1e-12
PARTNERS = O.TABLES[5:]
_REFS = {}


def _np(t):
    return t.cpu().numpy()


def assert_pairs(got, want):
    pairs = got.pairs()
    assert len(pairs) == 4
    for key, a, b in zip(O.PAIRS, pairs, want):
        assert a.dtype == np.int64 and np.array_equal(a, b), key


def assert_tables(got, ref):
    assert isinstance(got, G.OverlapTable) and (got.cap_pred, got.cap_truth) == (ref["cap_pred"], ref["cap_truth"])
    for key in O.TABLES:
        t = getattr(got, key)
        assert t.is_cuda and t.dtype == torch.int32 and tuple(t.shape) == ref[key].shape, key
        assert np.array_equal(_np(t), ref[key]), key
    assert got.dropped.dtype == torch.int32 and not _np(got.dropped).any()
    assert_pairs(got, ref["pairs"])
    over = (ref["counts_pred"] > ref["cap_pred"]) | (ref["counts_truth"] > ref["cap_truth"])
    assert got.overflowed().dtype == torch.bool and got.overflowed().is_cuda and np.array_equal(_np(got.overflowed()), over)


def assert_scores(got, ref):
    s, want = got.score(), O.score(ref)
    assert isinstance(s, S.OverlapScore)
    for key in O.SCORES:
        a = getattr(s, key)
        assert a.dtype == want[key].dtype and a.shape == want[key].shape, key
        if a.dtype == np.int64:
            assert np.array_equal(a, want[key]), key
        else:
            assert (np.abs(a - want[key]) <= TOL).all(), (key, a, want[key])


def check(pred, truth, max_regions=None, max_pairs=None, **kw):
    """overlap_labels on the device against the reference with the same capacities -> (OverlapTable, reference)"""
    caps = (None, None) if max_regions is None else max_regions if isinstance(max_regions, tuple) else (max_regions, max_regions)
    ref = O.overlap(pred, truth, *caps)
    got = G.overlap_labels(pred, truth, max_regions=max_regions, max_pairs=max_pairs, **kw)
    assert_tables(got, ref)
    assert_scores(got, ref)
    return got, ref


@pytest.mark.parametrize("name", NAMES)
def test_golden_vectors(dev, name):
    pred, truth = GOLD[f"{name}.pred"], GOLD[f"{name}.truth"]
    got = G.overlap_labels(torch.from_numpy(pred).to(dev), truth, max_regions=tuple(int(c) for c in GOLD[f"{name}.caps"]))
    for key in O.TABLES:
        assert np.array_equal(_np(getattr(got, key)), GOLD[f"{name}.{key}"]), key
    assert_pairs(got, [GOLD[f"{name}.pair_{key}"] for key in O.PAIRS])
    s = got.score()
    for key in O.SCORES:
        want = GOLD[f"{name}.score.{key}"]
        assert np.array_equal(getattr(s, key), want) if want.dtype == np.int64 else (np.abs(getattr(s, key) - want) <= TOL).all(), key


def test_hand_cases_alone_and_as_one_ragged_batch(dev):
    for name, (pred, truth) in O.hand_cases().items():
        check(pred, truth)                                              # a 2-D pair: one image of one row
        check(pred, truth, max_regions=(7, 6), max_pairs=16)
    names, pred, truth = O.stacked()
    got, ref = check(pred, truth)                                       # different counts per image, negative labels among them
    s = got.score()
    i = names.index("iou_vs_inter")
    assert _np(got.iou_partner)[i, 0] == 1 and _np(got.inter_partner_truth)[i, 0] == 2
    assert (s.aji_inter[i], s.aji_union[i]) == (2, 36) and abs(s.dice_obj[i] - 17 / 96) <= TOL
    i = names.index("iou_tie")
    assert _np(got.iou_partner)[i, 0] == 1 and abs(s.aji[i] - 1 / 3) <= TOL
    i = names.index("shared_pred")
    assert (s.aji_inter[i], s.aji_union[i], s.aji[i]) == (6, 12, 0.5)
    i = names.index("both_empty")
    assert (s.aji[i], s.dice_obj[i]) == (1.0, 1.0)
    i = names.index("pred_empty")
    assert (s.aji[i], s.dice_obj[i]) == (0.0, 0.0)
    i = names.index("negative")
    assert _np(got.area_pred)[i].tolist()[:2] == [3, 2] and _np(got.n_pairs)[i] == 2


@pytest.mark.parametrize("shape", [(1, 70), (3, 130)])
def test_runs_across_segments_and_rows_meet_in_one_slot(dev, shape):
    H, W = shape
    at = np.arange(H * W).reshape(H, W)
    pred, truth = (1 + (at // 45) % 3).astype(np.int32), (1 + (at // 31) % 2).astype(np.int32)     # runs over row ends and lane 63 / 64
    pred[:, W // 2] = 0
    got, ref = check(pred, truth)
    assert ref["n_pairs"][0] >= 2 and int(ref["pairs"][3].sum()) == H * (W - 1)
    full = np.ones((H, W), np.int32)                                    # one pair fed by every wave
    got, _ = check(full, full * 2)
    assert [c.tolist() for c in got.pairs()] == [[0], [1], [2], [H * W]]


@pytest.mark.parametrize("W", [1, 63, 64, 65, 129])
@pytest.mark.parametrize("H", [1, 3])
def test_both_sides_accounted_alike_by_match_overlap_and_measure(dev, H, W):
    """The accounting that match_labels and overlap_labels share (label maxima, clamp to the capacities, areas), at the widths
    either side of a wave's 64-column segment, with labels below 1 and labels above both capacities, against measure_labels of each
    side and the dense statement."""
    rng = np.random.RandomState(1000 * H + W)
    pred, truth = (rng.randint(-1, 10, size=(2, H, W)).astype(np.int32) for _ in range(2))
    ref = O.overlap(pred, truth, 6, 7)
    m = G.match_labels(pred, truth, max_regions=(6, 7))
    o = G.overlap_labels(pred, truth, max_regions=(6, 7), max_pairs=64)     # at most 6 x 7 pairs: nothing is dropped
    assert not _np(o.dropped).any()
    for key in ("counts_pred", "counts_truth", "area_pred", "area_truth"):
        a, b = getattr(m, key), getattr(o, key)
        assert a.dtype == torch.int32 and torch.equal(a, b), key
        assert np.array_equal(_np(a), ref[key]), key
    assert torch.equal(G.measure_labels(pred, max_regions=6).area, m.area_pred)
    assert torch.equal(G.measure_labels(truth, max_regions=7).area, m.area_truth)


def blocks_ref():
    if "blocks" not in _REFS:
        truth = M.blocks(64, 64)
        pred = np.roll(truth, (1, 1), axis=(0, 1))
        _REFS["blocks"] = (pred, truth, O.overlap(pred, truth))
    return _REFS["blocks"]


def test_many_labels_few_partners_and_automatic_capacity(dev, monkeypatch):
    pred, truth, ref = blocks_ref()
    assert ref["cap_pred"] == 1024 and ref["n_pairs"][0] == 4096 and (ref["inter_truth"] == 1).all()
    got = G.overlap_labels(pred, truth)                                 # max_pairs=None: min(4 (1024 + 1024), H W) holds them at once
    assert_tables(got, ref)
    assert_scores(got, ref)
    assert got.slot_keys.shape == (1, 8192)
    # 32 x 32 labels that all meet: 1024 pairs against a first table of 4 (32 + 32) = 256 pairs, 512 slots -- it has to double,
    # and the 1024 slots it ends with are exactly full
    r, c = np.mgrid[:32, :32]
    pred, truth = (r + 1).astype(np.int32), (c + 1).astype(np.int32)
    calls = []
    inner = K.regions_overlap_labels
    monkeypatch.setattr(K, "regions_overlap_labels", lambda *a, **kw: calls.append(a[4]) or inner(*a, **kw))
    got, ref = check(pred, truth, max_regions=32)
    assert calls == [256, 512] and got.slot_keys.shape == (1, 1024) and (_np(got.slot_keys) != 0).all()
    low = G.overlap_labels(pred, truth, max_regions=32, max_pairs=256)  # the first of the two, on its own: flagged, not exact
    assert _np(low.dropped)[0] > 0 and _np(low.n_pairs)[0] == 512 and _np(low.overflowed()).all()
    assert np.array_equal(_np(low.area_pred), ref["area_pred"])


def test_noisy_blobs_agree_with_match_labels(dev):
    import scipy.ndimage
    masks = R.blobs(3, 96, 96, seed=31, density=1 / 150.0)
    pred, truth = M.noisy_pair(masks, 41, lambda m: scipy.ndimage.label(m)[0])
    got, ref = check(pred, truth)
    assert ref["n_pairs"].min() > 0
    m = G.match_labels(pred, truth)
    match, inter = _np(m.match), _np(m.inter)
    assert (match > 0).any() and (match == 0).any()
    iou_partner, iou_inter = _np(got.iou_partner), _np(got.iou_inter)
    for n, p in zip(*np.nonzero(match)):
        g = match[n, p] - 1
        assert iou_partner[n, g] == p + 1 and iou_inter[n, g] == inter[n, p], (n, p)
    assert np.array_equal(_np(m.area_pred), _np(got.area_pred)) and np.array_equal(_np(m.area_truth), _np(got.area_truth))


def test_probing_a_nearly_full_table(dev):
    pred, truth = O.hand_cases()["six_pairs"]
    for max_pairs in (8, 4, 3):                                         # 6 pairs in 16, 8 and 8 slots
        got, _ = check(pred, truth, max_regions=(3, 4), max_pairs=max_pairs)
        assert got.slot_keys.shape == (1, K.regions_overlap_slots(max_pairs)) and int((_np(got.slot_keys) != 0).sum()) == 6
    pred, truth = O.hand_cases()["five_labels"]                         # 9 pairs in 16 slots
    got, _ = check(pred, truth, max_regions=5, max_pairs=5)
    assert got.slot_keys.shape == (1, 16)
    grid = np.arange(64, dtype=np.int32).reshape(1, 64)                  # 64 pairs in exactly 64 slots: every chain ends somewhere
    got, _ = check(1 + grid // 8, 1 + grid % 8, max_regions=8, max_pairs=32)
    assert got.slot_keys.shape == (1, 64) and (_np(got.slot_keys) != 0).all()


def test_overflow_is_reported_and_the_images_that_fit_are_exact(dev):
    names, pred, truth = O.stacked()
    ref = O.overlap(pred, truth, 5, 5)
    got = G.overlap_labels(pred, truth, max_regions=5, max_pairs=2)     # 4 slots per image
    torch.cuda.synchronize()                                            # the call returned and the work ends
    fits = ref["n_pairs"] <= 4
    assert not fits[names.index("six_pairs")] and not fits[names.index("five_labels")] and fits.sum() == len(names) - 2
    dropped, n_pairs, over = _np(got.dropped), _np(got.n_pairs), _np(got.overflowed())
    assert np.array_equal(over, ~fits) and np.array_equal(dropped > 0, ~fits) and (n_pairs <= 4).all() and (n_pairs[~fits] == 4).all()
    for key in O.TABLES:                                                # the areas and counts of every image, the rest where it fits
        rows = slice(None) if key in O.TABLES[:4] else fits
        assert np.array_equal(_np(getattr(got, key))[rows], ref[key][rows]), key
    image, p, g, inter = got.pairs()
    keep = fits[ref["pairs"][0]]
    want = [c[keep] for c in ref["pairs"]]
    mine = fits[image]
    for a, b in zip((image, p, g, inter), want):
        assert np.array_equal(a[mine], b)
    # what an overflowed image does hold is true: a subset of its pairs, none counted beyond its intersection
    truth_of = {(int(n), int(i), int(j)): int(c) for n, i, j, c in zip(*ref["pairs"])}
    for n, i, j, c in zip(image[~mine], p[~mine], g[~mine], inter[~mine]):
        assert 0 < c <= truth_of[(int(n), int(i), int(j))]


def test_capacities_below_the_largest_label(dev):
    pred, truth = O.hand_cases()["five_labels"]
    got, ref = check(pred, truth, max_regions=(3, 2), max_pairs=8)
    assert _np(got.counts_pred).tolist() == [5] and _np(got.counts_truth).tolist() == [5] and _np(got.overflowed()).tolist() == [True]
    assert [c.tolist() for c in got.pairs()[1:]] == [[1, 1, 2], [1, 2, 2], [1, 1, 1]]
    clipped = O.overlap(np.where(pred > 3, 0, pred), np.where(truth > 2, 0, truth), 3, 2)
    for key in O.TABLES[2:]:
        assert np.array_equal(_np(getattr(got, key)), clipped[key]), key


def test_caller_supplied_counts(dev):
    names, pred, truth = O.stacked()
    found, ref = check(pred, truth)
    cp, ct = torch.from_numpy(ref["counts_pred"]).to(dev), torch.from_numpy(ref["counts_truth"]).to(dev)
    for kw in ({"pred_counts": cp}, {"truth_counts": ct}, {"pred_counts": cp, "truth_counts": ct}):
        for fixed in ({}, {"max_regions": (found.cap_pred, found.cap_truth), "max_pairs": 16}):
            got = G.overlap_labels(pred, truth, **kw, **fixed)
            assert_tables(got, ref)
            for key in O.TABLES:
                assert torch.equal(getattr(got, key), getattr(found, key)), key
    more = cp + 2                                                       # counts may exceed the labels in use (split's empty last cells)
    got = G.overlap_labels(pred, truth, pred_counts=more)
    assert got.cap_pred == found.cap_pred + 2 and torch.equal(got.counts_pred, more)
    assert torch.equal(got.area_pred[:, :found.cap_pred], found.area_pred) and not _np(got.area_pred[:, found.cap_pred:]).any()
    assert_pairs(got, ref["pairs"])


def _table(r, cp, ct):
    return G.OverlapTable(r["counts_pred"], r["counts_truth"], cp, ct, *(r[k] for k in ("area_pred", "area_truth", "n_pairs", "dropped")
                                                                          + PARTNERS), r["slot_keys"], r["slot_counts"])


def test_two_runs_identical_and_graph_replay(dev):
    pred, truth, ref = blocks_ref()
    a, b = G.overlap_labels(pred, truth, max_regions=1024, max_pairs=4096), G.overlap_labels(pred, truth, max_regions=1024, max_pairs=4096)
    for key in O.TABLES + ("dropped",):
        assert _np(getattr(a, key)).tobytes() == _np(getattr(b, key)).tobytes(), key
    for x, y in zip(a.pairs(), b.pairs()):
        assert x.tobytes() == y.tobytes()
    assert_tables(a, ref)
    # one call at the kernels' level, everything preallocated, captured and replayed on new contents of the same shape
    masks = R.blobs(3, 70, 67, seed=5, density=1 / 150.0)
    pred, truth = M.noisy_pair(masks, 6, lambda m: R.label(m, 1)[0])
    cp, ct, mp = int(pred.max()) + 2, int(truth.max()) + 2, 128
    dp, dt = torch.from_numpy(pred).to(dev), torch.from_numpy(truth).to(dev)
    ws = K.regions_overlap_workspace(3, cp, ct, mp, dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = K.regions_overlap_labels(dp, dt, cp, ct, mp, ws=ws)       # warm-up; its outputs are reused below
    torch.cuda.current_stream().wait_stream(side)
    given = {k: v for k, v in out.items() if k not in ("slot_keys", "slot_counts")}
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = K.regions_overlap_labels(dp, dt, cp, ct, mp, ws=ws, **given)
    assert all(got[k] is given[k] for k in given) and got["slot_keys"].data_ptr() == ws.data_ptr()
    new_pred, new_truth = np.ascontiguousarray(truth[::-1]), np.ascontiguousarray(pred[::-1])        # sides swapped, batch reversed
    dp.copy_(torch.from_numpy(new_pred))
    dt.copy_(torch.from_numpy(new_truth))
    graph.replay()
    torch.cuda.synchronize()
    want = O.overlap(new_pred, new_truth, cp, ct)
    table = _table(got, cp, ct)
    assert_tables(table, want)
    assert_scores(table, want)
    assert want["n_pairs"].max() <= 2 * mp and want["n_pairs"].min() > 0


def test_batches_cut_into_chunks(dev, monkeypatch):
    names, pred, truth = O.stacked()
    whole, ref = check(pred, truth)
    W = pred.shape[2]
    monkeypatch.setattr(G, "_MAX_PIXELS", 4 * W + 3)                    # four one-row images per call
    assert [b - a for a, b in G._chunks(torch.empty(len(names), 1, W))] == [4] * (len(names) // 4) + [len(names) % 4] * (len(names) % 4 > 0)
    for kw in ({}, {"max_regions": (whole.cap_pred, whole.cap_truth), "max_pairs": 16}):
        got, _ = check(pred, truth, **kw)
        for key in O.TABLES:
            assert torch.equal(getattr(got, key), getattr(whole, key)), key


def test_evaluate_instances_with_overlap(dev):
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
    classes = _np(inference.segment_classes(images, m, dev, thr))
    labels = np.stack([R.label(np.roll(c, (2, -3), axis=(0, 1)) != 0, 1)[0] for c in classes]).astype(np.int32)
    cells = inference.detect_cells(images, m, dev, **kw)
    parts = [SR.split(classes[i], cells[i][0]) for i in range(2)]
    loader = [(images[0], torch.from_numpy(labels[:1])), (images[1], torch.from_numpy(labels[1:]))]
    plain = inference.evaluate_instances(loader, m, dev, threshold=thr, **kw)
    assert sorted(plain) == sorted(["n_pred", "n_truth", "tp", "fp", "fn", "p", "r", "f1", "sq", "pq", "mean"])
    out = inference.evaluate_instances(loader, m, dev, threshold=thr, overlap=True, **kw)
    assert sorted(out) == sorted(list(plain) + ["aji", "dice_obj", "mean_overlap"])
    for key in plain:
        assert out[key].tobytes() == plain[key].tobytes() if key != "mean" else out[key] == plain[key], key
    for i in range(2):
        want = O.score(O.overlap(parts[i]["labels"], labels[i]))
        assert abs(out["aji"][i] - want["aji"][0]) <= TOL and abs(out["dice_obj"][i] - want["dice_obj"][0]) <= TOL, i
    assert out["mean_overlap"] == (float(out["aji"].mean()), float(out["dice_obj"].mean()))
    assert out["n_pred"].sum() > 0 and out["n_truth"].sum() > 0 and 0 < out["aji"].max() < 1
