"""CPU: the numpy statement of the label matcher (tests/match_ref.py) against tests/golden/match_vectors.npz and against answers
worked by hand; the argument errors of ``regions.match_labels`` / ``MatchTable.score`` (raised before any device work); the new
entry points in the library; ``score.label_score`` on hand-made integer tables."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import match_ref as M  # noqa: E402
from cellsegmentation_amd import _lib, inference  # noqa: E402
from cellsegmentation_amd import regions as G  # noqa: E402
from cellsegmentation_amd import score as S  # noqa: E402

GOLD = np.load(os.path.join(ROOT, "tests", "golden", "match_vectors.npz"), allow_pickle=False)
NAMES = sorted(k[:-len(".pred")] for k in GOLD.files if k.endswith(".pred"))
THRESHOLDS = (0.5, 0.75, 1.0)


def test_golden_file_is_what_the_maker_writes():
    import make_match_golden as MG
    assert NAMES == sorted(name for name, _ in MG.cases()) and MG.THRESHOLDS == THRESHOLDS
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "match_vectors.npz")) < 256 * 1024


@pytest.mark.parametrize("name", NAMES)
def test_reference_equals_golden(name):
    cp, ct = (int(c) for c in GOLD[f"{name}.caps"])
    t = M.match(GOLD[f"{name}.pred"], GOLD[f"{name}.truth"], cp, ct)
    for key in M.TABLES:
        assert t[key].dtype == np.int32 and np.array_equal(t[key], GOLD[f"{name}.{key}"]), key
    for thr in THRESHOLDS:
        s = M.score(t, thr)
        for key in M.SCORES:
            assert s[key].tobytes() == GOLD[f"{name}.score{thr}.{key}"].tobytes(), (thr, key)


def _one(name):
    pred, truth, cp, ct = M.hand_cases()[name]
    t = M.match(pred, truth, cp, ct)
    return t, {thr: M.score(t, thr) for thr in THRESHOLDS}


def _counts(s):
    return tuple(int(s[k][0]) for k in ("n_pred", "n_truth", "tp", "fp", "fn"))


def test_hand_worked_answers():
    t, s = _one("half_twice")                                           # IoU 2 / 4 with either truth label: no match
    assert t["match"].tolist() == [[0]] and t["match_truth"].tolist() == [[0, 0]] and t["inter"].tolist() == [[0]]
    assert t["area_pred"].tolist() == [[4]] and t["area_truth"].tolist() == [[2, 2]] and _counts(s[0.5]) == (1, 2, 0, 1, 2)
    t, s = _one("two_thirds")
    assert t["match"].tolist() == [[1]] and t["inter"].tolist() == [[2]] and t["match_truth"].tolist() == [[1]]
    assert _counts(s[0.5]) == (1, 1, 1, 0, 0) and _counts(s[0.75]) == (1, 1, 0, 1, 1)
    assert s[0.5]["sq"][0] == 2 / 3 and s[0.5]["pq"][0] == 2 / 3 and s[0.75]["sq"][0] == 0.0
    t, s = _one("false_candidate")                                      # bit 0: 4 + 3 of 10, bit 1: 4 + 3 of 10 -> 3, which holds 4
    assert t["match"].tolist() == [[0]] and t["area_truth"].tolist() == [[3, 3, 4]] and _counts(s[0.5]) == (1, 3, 0, 1, 3)
    t, s = _one("out_of_range_candidate")                               # bits 0, 1, 2 have 6, 6, 8 of 10 -> 7 > cap_truth
    assert t["cap_truth"] == 6 and t["match"].tolist() == [[0]] and t["area_truth"].tolist() == [[0, 0, 2, 0, 4, 4]]
    t, s = _one("background_majority")
    assert t["match"].tolist() == [[0]] and _counts(s[0.5]) == (1, 1, 0, 1, 1)
    t, s = _one("identical_with_empty")
    assert t["counts_pred"].tolist() == [3] and t["match"].tolist() == [[1, 0, 3]] and t["inter"].tolist() == [[3, 0, 4]]
    for thr in THRESHOLDS:
        assert _counts(s[thr]) == (2, 2, 2, 0, 0) and s[thr]["sq"][0] == 1.0 and s[thr]["pq"][0] == 1.0
    b = M.blocks()
    cleared = b.copy()
    cleared[1::2, 1::2] = 0
    t = M.match(b, cleared)
    assert t["cap_pred"] == 1024 and (t["match"] == np.arange(1, 1025)).all() and (t["inter"] == 3).all()
    assert (M.iou(t) == 0.75).all() and int(M.score(t, 0.75)["tp"][0]) == 1024 and int(M.score(t, 1.0)["tp"][0]) == 0
    assert not M.match(b, np.roll(b, 1, axis=1))["match"].any()         # IoU 2 / 6


def test_label_score_from_integer_tables():
    # image 0: labels 1 (IoU 3 / 4), 2 (empty), 3 (IoU 1), 4 (unmatched); truth label 4 unmatched.  image 1: nothing at all.
    area_pred = np.asarray([[3, 0, 5, 2], [0, 0, 0, 0]], np.int32)
    area_truth = np.asarray([[4, 5, 0, 7], [0, 0, 0, 0]], np.int32)
    match = np.asarray([[1, 0, 2, 0], [0, 0, 0, 0]], np.int32)
    inter = np.asarray([[3, 0, 5, 0], [0, 0, 0, 0]], np.int32)
    s = S.label_score(area_pred, area_truth, match, inter)
    assert isinstance(s, S.LabelScore)
    for k in ("n_pred", "n_truth", "tp", "fp", "fn"):
        assert getattr(s, k).dtype == np.int64
    assert (s.n_pred.tolist(), s.n_truth.tolist(), s.tp.tolist(), s.fp.tolist(), s.fn.tolist()) == ([3, 0], [3, 0], [2, 0], [1, 0], [1, 0])
    assert s.precision.tolist() == [2 / 3, 1.0] and s.recall.tolist() == [2 / 3, 1.0]
    assert s.f1.tobytes() == np.asarray([(2 * (2 / 3) * (2 / 3)) / (2 / 3 + 2 / 3), 1.0]).tobytes()
    assert s.sq.tolist() == [(0.75 + 1.0) / 2, 0.0] and s.pq.tobytes() == (s.sq * s.f1).tobytes()
    hi = S.label_score(area_pred, area_truth, match, inter, 0.75)       # >= : 3 / 4 still counts
    assert hi.tp.tolist() == [2, 0]
    one = S.label_score(area_pred, area_truth, match, inter, 1)
    assert one.tp.tolist() == [1, 0] and one.fp.tolist() == [2, 0] and one.sq.tolist() == [1.0, 0.0] and one.pq[0] == one.f1[0]
    ref = M.score({"area_pred": area_pred, "area_truth": area_truth, "match": match, "inter": inter}, 0.75)
    for k in M.SCORES:
        assert getattr(hi, k).tobytes() == ref[k].tobytes(), k
    for bad in (0.49, 1.01, -1, float("nan"), "0.5", None, True):
        with pytest.raises(ValueError, match="iou_threshold"):
            S.label_score(area_pred, area_truth, match, inter, bad)
    with pytest.raises(ValueError, match="label_score"):
        S.label_score(area_pred, area_truth, match[:, :3], inter)


def test_argument_errors_before_any_device_work():
    lab = np.zeros((4, 5), np.int32)
    with pytest.raises(TypeError, match="numpy array or a torch tensor"):
        G.match_labels([[1]], lab)
    with pytest.raises(TypeError, match="int32 label image"):
        G.match_labels(lab.astype(np.int64), lab)
    with pytest.raises(TypeError, match="int32 label image"):
        G.match_labels(lab, lab > 0)
    with pytest.raises(ValueError, match=r"\[H, W\] or \[N, H, W\]"):
        G.match_labels(lab[0], lab[0])
    with pytest.raises(ValueError, match="empty label image"):
        G.match_labels(lab[:0], lab[:0])
    with pytest.raises(ValueError, match="against truth of shape"):
        G.match_labels(lab, lab[:, :4])
    with pytest.raises(ValueError, match="against truth of shape"):
        G.match_labels(lab, lab[None])
    with pytest.raises(ValueError, match="2\\^31 pixels"):
        big = torch.zeros((1, 1), dtype=torch.int32).expand(1 << 16, 1 << 15)
        G.match_labels(big, big)
    for bad in (0, -3, 2.5, True, (4,), (4, 0), (1, 2, 3), (None, 4)):
        with pytest.raises(ValueError, match="max_regions"):
            G.match_labels(lab, lab, max_regions=bad)
    for kw in ({"pred_counts": torch.zeros(2, dtype=torch.int32)}, {"truth_counts": torch.zeros(1, dtype=torch.int64)},
               {"pred_counts": np.zeros(1, np.int32)}):
        with pytest.raises(TypeError, match="counts must be an int32 tensor of shape"):
            G.match_labels(lab, lab, **kw)
    z = torch.zeros((1, 2), dtype=torch.int32)
    table = G.MatchTable(torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), 2, 2, z, z, z, z, z)
    for bad in (0.25, 1.5, "x", None, float("nan")):
        with pytest.raises(ValueError, match="iou_threshold"):
            table.score(bad)
    with pytest.raises(ValueError, match="iou_threshold"):
        inference.evaluate_instances([], None, None, iou_threshold=0.3)
    with pytest.raises(TypeError, match="unexpected arguments"):
        inference.evaluate_instances([], None, None, bogus=1)


def test_match_table_scores_host_tables_and_caches_them():
    """the table's tensors may live anywhere: score() reads them once and keeps the copy"""
    t = M.match(*M.hand_cases()["two_thirds"][:2])
    table = G.MatchTable(*(torch.from_numpy(t[k]) if isinstance(t[k], np.ndarray) else t[k] for k in
                           ("counts_pred", "counts_truth", "cap_pred", "cap_truth", "area_pred", "area_truth", "match", "inter",
                            "match_truth")))
    assert not table.overflowed().any() and table.iou().tolist() == [[2 / 3]]
    s = table.score()
    assert (s.tp.tolist(), s.fp.tolist(), s.fn.tolist()) == ([1], [0], [0]) and s.sq[0] == 2 / 3
    kept = table._host
    table.area_pred = None                                              # a second threshold touches no tensor
    assert table.score(0.75).tp.tolist() == [0] and table._host is kept


def test_library_has_the_entry_points():
    lib = _lib.load()
    assert hasattr(lib, "cs_regions_match_labels") and hasattr(lib, "cs_regions_match_workspace")
    assert lib.cs_abi_version() == 10
    # 4 N cap_pred (B + 1) bytes, B = bit_length(cap_truth); every part 16-byte aligned
    assert lib.cs_regions_match_workspace(1, 4, 1) == 16 + 16
    assert lib.cs_regions_match_workspace(3, 1000, 1024) == 3 * 1000 * 11 * 4 + 3 * 1000 * 4
    assert lib.cs_regions_match_workspace(2, 10000, 10000) == 2 * 10000 * 15 * 4         # far from 2 x 10^4 x 10^4 x 4
    for bad in ((0, 1, 1), (65536, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1 << 30, 4), (1, 1, -1)):
        assert lib.cs_regions_match_workspace(*bad) == 0, bad
    # the call refuses what the workspace function refuses, before anything is launched
    import ctypes
    buf = ctypes.create_string_buffer(64)
    ptr = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    args = lambda N, H, W, cp, ct: (ptr, ptr, N, H, W, cp, ct, None, None, ptr, ptr, ptr, ptr, ptr, ptr, 1 << 20, None)  # noqa: E731
    assert lib.cs_regions_match_labels(*args(1, 4, 4, 0, 1)) == -1 and b"capacities" in lib.cs_last_error()
    assert lib.cs_regions_match_labels(*args(0, 4, 4, 1, 1)) == -1 and b"N H W" in lib.cs_last_error()
    small = list(args(1, 4, 4, 8, 8))
    small[15] = 16
    assert lib.cs_regions_match_labels(*small) == -1 and b"workspace too small" in lib.cs_last_error()
