"""Object-level Hausdorff tables of label images on the GPU (csrc/regions.hip through cellsegmentation_amd.regions.hausdorff_labels),
exact against the dense statement tests/hausdorff_ref.py and the vectors of tests/golden/hausdorff_vectors.npz: every integer table
by value, the floats of ``HausdorffTable.score`` within 1e-12 relative to max(1, value) (sums of at most a few thousand float64
terms, the bound and reasoning of test_overlap_gpu.py).  Shapes are the smallest at which each mechanism can go wrong: hand cases of
one row, widths either side of the 64-column segments, a comb with more runs than one stage holds, objects that overlap nothing."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import hausdorff_ref as HR  # noqa: E402
import match_ref as M  # noqa: E402
import regions_ref as R  # noqa: E402
import split_ref as SR  # noqa: E402
from cellsegmentation_amd import inference  # noqa: E402
from cellsegmentation_amd import kernels as K  # noqa: E402
from cellsegmentation_amd import regions as G  # noqa: E402
from cellsegmentation_amd import score as S  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "hausdorff_vectors.npz"), allow_pickle=False)
NAMES = sorted(k[:-len(".pred")] for k in GOLD.files if k.endswith(".pred"))
TOL = 1e-12
_REFS = {}


def _np(t):
    return t.cpu().numpy()


def close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    fin = np.isfinite(b)
    return a.shape == b.shape and np.array_equal(a[~fin], b[~fin]) and bool((np.abs(a[fin] - b[fin]) <= TOL * np.maximum(1.0, np.abs(b[fin]))).all())


def assert_tables(got, ref):
    assert isinstance(got, G.HausdorffTable) and (got.cap_pred, got.cap_truth) == (ref["cap_pred"], ref["cap_truth"])
    for key in HR.CARRIED + HR.TABLES:
        t = getattr(got, key)
        assert t.is_cuda and t.dtype == torch.int32 and tuple(t.shape) == ref[key].shape, key
        assert np.array_equal(_np(t), ref[key]), (key, _np(t), ref[key])
    over = (ref["counts_pred"] > ref["cap_pred"]) | (ref["counts_truth"] > ref["cap_truth"])
    assert got.overflowed().dtype == torch.bool and got.overflowed().is_cuda and np.array_equal(_np(got.overflowed()), over)


def assert_scores(got, ref):
    s, want = got.score(), HR.score(ref)
    assert isinstance(s, S.HausdorffScore)
    for key in HR.SCORES:
        a = getattr(s, key)
        assert a.dtype == want[key].dtype and (np.array_equal(a, want[key]) if a.dtype == np.int64 else close(a, want[key])), (key, a, want[key])


def check(pred, truth, max_regions=None, max_pairs=None, **kw):
    """hausdorff_labels on the device against the reference with the same capacities -> (HausdorffTable, reference)"""
    caps = (None, None) if max_regions is None else max_regions if isinstance(max_regions, tuple) else (max_regions, max_regions)
    ref = HR.hausdorff(pred, truth, *caps)
    got = G.hausdorff_labels(pred, truth, max_regions=max_regions, max_pairs=max_pairs, **kw)
    assert_tables(got, ref)
    assert_scores(got, ref)
    return got, ref


@pytest.mark.parametrize("name", NAMES)
def test_golden_vectors(dev, name):
    got = G.hausdorff_labels(torch.from_numpy(GOLD[f"{name}.pred"]).to(dev), GOLD[f"{name}.truth"])
    for key in ("area_pred", "area_truth") + HR.TABLES:
        assert np.array_equal(_np(getattr(got, key)), GOLD[f"{name}.{key}"]), key
    s = got.score()
    for key in ("term_truth", "term_pred", "hausdorff_obj"):
        assert close(getattr(s, key), GOLD[f"{name}.score.{key}"]), key


def test_one_row_hand_cases(dev):
    pred, truth = HR.hand_cases()["apart"]                              # pred on columns 0..2, truth on column 5: no overlap
    got, _ = check(pred, truth)
    assert _np(got.partner_truth).tolist() == [[1]] and _np(got.partner_pred).tolist() == [[1]]
    assert _np(got.d2_truth).tolist() == [[25]] and _np(got.d2_pred).tolist() == [[25]] and got.score().hausdorff_obj.tolist() == [5.0]
    got, _ = check(*HR.hand_cases()["identical"])
    assert _np(got.d2_truth).tolist() == [[-1, 0]] and _np(got.d2_pred).tolist() == [[-1, 0]] and got.score().hausdorff_obj.tolist() == [0.0]
    for name, (pred, truth) in HR.hand_cases().items():
        check(pred, truth)
        check(pred, truth, max_regions=(5, 3), max_pairs=8)


def test_the_maximum_lies_inside_the_object(dev):
    sq, frame = HR.square_in_frame()
    for pred, truth in ((sq, frame), (frame, sq)):
        got, _ = check(pred, truth)                                     # 16 at the square's centre; its boundary reaches 4, the frame 8
        assert _np(got.d2_truth).tolist() == [[16]] and _np(got.d2_pred).tolist() == [[16]] and got.score().hausdorff_obj.tolist() == [4.0]
    ring = sq.copy()
    ring[3:6, 3:6] = 0                                                  # the square's boundary alone: the shortcut's answer
    got, _ = check(ring, frame)
    assert _np(got.d2_truth).tolist() == [[8]]


@pytest.mark.parametrize("W", [63, 64, 65, 129])
def test_objects_across_the_segment_ends(dev, W):
    """every object's box starts at another column, so the 64-column segments of its walk end inside the other objects' runs: long
    runs, runs that end on the last column and one-pixel runs, each as source and as target, with and without overlap"""
    H = 5
    pred, truth = np.zeros((H, W), np.int32), np.zeros((H, W), np.int32)
    pred[0, :] = 1                                                       # one run over every segment end
    pred[1, 1:W - 1] = 2
    pred[2, ::2] = 3                                                     # one-pixel runs, 32 to a full segment
    pred[4, W - 2:] = 4
    truth[0, W // 2:] = 1                                                # overlaps pred 1
    truth[1:3, 0] = 2                                                    # overlaps pred 3 on one pixel
    truth[3, 3:W] = 3                                                    # overlaps nothing
    truth[4, 1::2] = 4                                                   # overlaps pred 4 on the last odd column
    got, ref = check(pred, truth)
    assert (ref["overlap"]["inter_partner_truth"][0] == 0).tolist() == [False, False, True, False]
    check(truth, pred)
    check(np.stack([pred, truth]), np.stack([truth, pred]), max_regions=4, max_pairs=16)


def comb_ref():
    if "comb" not in _REFS:
        cap = K.regions_hausdorff_stage_runs()
        W = 130
        rows = cap // (W // 2) + 1                                      # rows 65 + 1 runs > cap, in the smallest such image
        comb = HR.comb(rows, W)
        other = np.zeros_like(comb)
        other[rows // 2:rows // 2 + 3, 60:70] = 1                        # overlaps the comb
        other[rows, 1:9:2] = 2                                           # between the last teeth: overlaps nothing
        _REFS["comb"] = (comb, other, rows * (W // 2) + 1, HR.hausdorff(comb, other), HR.hausdorff(other, comb))
    return _REFS["comb"]


@pytest.mark.parametrize("as_pred", [True, False])
def test_more_runs_than_one_stage(dev, as_pred):
    """the comb is source and target of its partner's job and of every candidate job of the object that overlaps nothing"""
    comb, other, n_runs, ref_pred, ref_truth = comb_ref()
    assert n_runs > K.regions_hausdorff_stage_runs() and comb.shape[0] * comb.shape[1] < 3 * n_runs
    got = G.hausdorff_labels(comb, other) if as_pred else G.hausdorff_labels(other, comb)
    ref = ref_pred if as_pred else ref_truth
    assert_tables(got, ref)
    assert_scores(got, ref)
    lone = _np(got.partner_truth if as_pred else got.partner_pred)[0]
    assert lone.tolist() == [1, 1] and ref["overlap"]["inter_partner_truth" if as_pred else "inter_partner_pred"][0].tolist() == [1, 0]


def test_source_in_several_turns_against_a_target_in_several_stages(dev):
    """comb against shifted comb: the source's box takes several turns of the workgroup and the target is staged anew in each"""
    comb = comb_ref()[0]
    shifted = np.roll(comb, (1, 1), axis=(0, 1))
    got, ref = check(comb, shifted)
    assert ref["d2_truth"].tolist() == [[1]] and comb.size > 1024


def test_partner_rules(dev):
    for name in ("larger_intersection", "mirror_tie", "nearest_candidate"):
        pred, truth = HR.hand_cases()[name]
        ov = G.overlap_labels(pred, truth)
        got, ref = check(pred, truth)
        given = _np(ov.inter_partner_truth)
        assert np.array_equal(_np(got.partner_truth)[given > 0], given[given > 0])
        given = _np(ov.inter_partner_pred)
        assert np.array_equal(_np(got.partner_pred)[given > 0], given[given > 0])
    got, _ = check(*HR.hand_cases()["larger_intersection"])
    assert _np(got.partner_truth).tolist() == [[2]] and _np(got.d2_truth).tolist() == [[36]]         # not pred 1 at 16
    got, _ = check(*HR.hand_cases()["nearest_candidate"])
    assert _np(got.partner_truth).tolist() == [[2]] and _np(got.d2_truth).tolist() == [[9]]          # not pred 1 at 49
    got, _ = check(*HR.hand_cases()["mirror_tie"])
    assert _np(got.partner_truth).tolist() == [[1]] and _np(got.d2_truth).tolist() == [[16]]         # pred 3 is as near
    pred, truth = HR.hand_cases()["mirror_tie"]
    got, _ = check(np.ascontiguousarray(pred[:, ::-1]), np.ascontiguousarray(truth[:, ::-1]))          # mirrored: still the lower label
    assert _np(got.partner_truth).tolist() == [[1]]


def test_more_candidates_than_one_workgroup_holds_at_a_time(dev):
    """320 one-pixel pred objects on a grid, none under a truth pixel: every object of either side goes through the candidates, 256
    labels at a time, and the four nearest of a truth pixel are equally far, on both sides of label 256"""
    pred, truth = np.zeros((20, 64), np.int32), np.zeros((20, 64), np.int32)
    pred[::2, ::2] = np.arange(1, 321).reshape(10, 32)
    truth[15, 41], truth[17, 61] = 1, 2
    got, ref = check(pred, truth)
    assert ref["overlap"]["n_pairs"].tolist() == [0]
    assert _np(got.partner_truth).tolist() == [[245, 287]] and _np(got.d2_truth).tolist() == [[2, 2]]      # 245 246 277 278; 287 288 319 320
    assert set(_np(got.partner_pred)[0].tolist()) == {1, 2}
    check(truth, pred, max_regions=(2, 320), max_pairs=4)


def test_edge_rows(dev):
    names, pred, truth = HR.stacked()
    got, ref = check(pred, truth)
    s = got.score()
    i = names.index("both_empty")
    assert not _np(got.partner_truth)[i].any() and (_np(got.d2_pred)[i] == -1).all() and s.hausdorff_obj[i] == 0.0
    i = names.index("pred_empty")
    assert _np(got.area_truth)[i, 0] == 3 and _np(got.partner_truth)[i, 0] == 0 and _np(got.d2_truth)[i, 0] == -1
    assert s.hausdorff_obj[i] == np.inf and s.term_truth[i] == np.inf and s.term_pred[i] == 0.0
    i = names.index("truth_empty")
    assert s.hausdorff_obj[i] == np.inf and (s.n_pred[i], s.n_truth[i]) == (1, 0)
    i = names.index("mirror_tie")                                       # pred label 2 owns nothing: no row and no candidate
    assert _np(got.area_pred)[i].tolist() == [2, 0, 2, 1] and _np(got.partner_pred)[i].tolist() == [1, 0, 1, 1]
    assert _np(got.d2_pred)[i].tolist() == [16, -1, 16, 64] and not _np(got.overflowed()).any()
    # labels above the capacity are background: pred 3 and 4 are no candidates any more, and the image is flagged
    pred, truth = HR.hand_cases()["mirror_tie"]
    got, ref = check(pred, truth, max_regions=(2, 1), max_pairs=4)
    assert _np(got.counts_pred).tolist() == [4] and _np(got.overflowed()).tolist() == [True]
    assert _np(got.partner_pred).tolist() == [[1, 0]] and _np(got.d2_pred).tolist() == [[16, -1]]
    got, ref = check(truth, pred, max_regions=(1, 2), max_pairs=4)
    assert _np(got.overflowed()).tolist() == [True] and _np(got.partner_truth).tolist() == [[1, 0]]


def blobs_ref():
    if "blobs" not in _REFS:
        import scipy.ndimage
        masks = R.blobs(3, 48, 80, seed=19, density=1 / 70.0)   # discs merge: 9 to 16 blobs a side, and specks of noise in truth
        pred, truth = M.noisy_pair(masks, 23, lambda m: scipy.ndimage.label(m)[0])
        _REFS["blobs"] = (pred, truth, HR.hausdorff(pred, truth))
    return _REFS["blobs"]


def test_random_pairs(dev):
    pred, truth, ref = blobs_ref()
    assert pred.shape == (3, 48, 80) and ref["cap_pred"] >= 10
    ov = ref["overlap"]
    assert ((ref["area_truth"] > 0) & (ov["inter_partner_truth"] == 0)).any() and (ov["inter_partner_truth"] > 0).any()
    got = G.hausdorff_labels(pred, truth)
    assert_tables(got, ref)
    assert_scores(got, ref)


def test_batches_and_inputs(dev):
    pred, truth, ref = blobs_ref()                                      # N = 3 images of different contents, numpy inputs
    a = G.hausdorff_labels(torch.from_numpy(pred).to(dev), torch.from_numpy(truth))      # a device and a host tensor
    b = G.hausdorff_labels(pred, truth, max_regions=(ref["cap_pred"], ref["cap_truth"]), max_pairs=512)
    assert_tables(a, ref)
    for key in HR.CARRIED + HR.TABLES:                                  # two runs give equal bits
        assert _np(getattr(a, key)).tobytes() == _np(getattr(b, key)).tobytes(), key
    ov = G.overlap_labels(pred, truth)
    c = G.hausdorff_labels(pred, truth, overlap=ov)                     # a given OverlapTable and a self-made one agree
    assert c.area_pred is ov.area_pred and c.counts_truth is ov.counts_truth
    for key in HR.TABLES:
        assert torch.equal(getattr(c, key), getattr(a, key)), key
    with pytest.raises(ValueError, match="against an OverlapTable of capacities"):
        G.hausdorff_labels(pred, truth, overlap=ov, max_regions=ref["cap_pred"] + 1)
    with pytest.raises(ValueError, match="an OverlapTable of 3 images"):
        G.hausdorff_labels(pred[:2], truth[:2], overlap=ov)
    swapped = G.hausdorff_labels(truth, pred)                           # the sides swapped: the tables swapped
    for mine, theirs in (("partner_truth", "partner_pred"), ("d2_truth", "d2_pred"), ("partner_pred", "partner_truth"),
                         ("d2_pred", "d2_truth"), ("area_pred", "area_truth")):
        assert torch.equal(getattr(swapped, mine), getattr(a, theirs)), mine
    assert close(swapped.score().hausdorff_obj, a.score().hausdorff_obj)
    one = G.hausdorff_labels(pred[1], truth[1])                         # a 2-D pair: one image
    want = HR.hausdorff(pred[1], truth[1])
    assert_tables(one, want)
    assert_scores(one, want)


def test_batches_cut_into_chunks(dev, monkeypatch):
    names, pred, truth = HR.stacked()
    whole, ref = check(pred, truth)
    H, W = pred.shape[1:]
    monkeypatch.setattr(G, "_MAX_PIXELS", 4 * H * W + 3)                # four images per call
    assert [b - a for a, b in G._chunks(torch.empty(len(names), H, W))][:2] == [4, 4]
    for kw in ({}, {"max_regions": (whole.cap_pred, whole.cap_truth), "max_pairs": 16}):
        got, _ = check(pred, truth, **kw)
        for key in HR.TABLES:
            assert torch.equal(getattr(got, key), getattr(whole, key)), key


def test_graph_replay_on_new_contents(dev):
    pred, truth, _ = blobs_ref()
    cp = ct = max(int(pred.max()), int(truth.max())) + 2
    mp = 256
    dp, dt = torch.from_numpy(pred).to(dev), torch.from_numpy(truth).to(dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        G.hausdorff_labels(dp, dt, max_regions=(cp, ct), max_pairs=mp)  # warm-up
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                       # the whole call: nothing in it synchronises
        got = G.hausdorff_labels(dp, dt, max_regions=(cp, ct), max_pairs=mp)
    new_pred, new_truth = np.ascontiguousarray(truth[::-1]), np.ascontiguousarray(pred[::-1])        # sides swapped, batch reversed
    dp.copy_(torch.from_numpy(new_pred))
    dt.copy_(torch.from_numpy(new_truth))
    graph.replay()
    torch.cuda.synchronize()
    want = HR.hausdorff(new_pred, new_truth, cp, ct)
    assert want["overlap"]["n_pairs"].max() <= mp
    assert_tables(got, want)
    assert_scores(got, want)


def test_evaluate_instances_with_hausdorff(dev):
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
    assert sorted(inference.evaluate_instances(loader, m, dev, threshold=thr, hausdorff=False, **kw)) == sorted(plain)
    extra = ["hausdorff_obj", "mean_hausdorff", "hausdorff_undefined"]
    out = inference.evaluate_instances(loader, m, dev, threshold=thr, hausdorff=True, **kw)
    assert sorted(out) == sorted(list(plain) + extra)
    both = inference.evaluate_instances(loader, m, dev, threshold=thr, overlap=True, hausdorff=True, **kw)
    assert sorted(both) == sorted(list(plain) + extra + ["aji", "dice_obj", "mean_overlap"])
    for key in plain:
        assert out[key].tobytes() == plain[key].tobytes() if key != "mean" else out[key] == plain[key], key
    assert both["hausdorff_obj"].tobytes() == out["hausdorff_obj"].tobytes()
    for i in range(2):
        want = G.hausdorff_labels(parts[i]["labels"].astype(np.int32), labels[i]).score().hausdorff_obj
        assert close(out["hausdorff_obj"][i:i + 1], want), i
    fin = np.isfinite(out["hausdorff_obj"])
    assert out["hausdorff_undefined"] == int((~fin).sum()) and isinstance(out["mean_hausdorff"], float)
    assert close([out["mean_hausdorff"]], [out["hausdorff_obj"][fin].mean() if fin.any() else 0.0])
    assert out["n_pred"].sum() > 0 and out["n_truth"].sum() > 0 and fin.any() and out["hausdorff_obj"][fin].max() > 0
