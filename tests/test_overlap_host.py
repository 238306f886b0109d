"""CPU: the numpy statement of the overlap tables (tests/overlap_ref.py) against answers worked by hand and against
tests/golden/overlap_vectors.npz; ``score.overlap_score`` against that statement on the same integer tables (integers equal,
floats within 1e-12: each is a sum of at most a few thousand float64 terms in [0, 1]); the argument errors of
``regions.overlap_labels`` (raised before any device work); the new entry points in the library."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import overlap_ref as O  # noqa: E402
from cellsegmentation_amd import _lib, inference  # noqa: E402
from cellsegmentation_amd import kernels as K  # noqa: E402
from cellsegmentation_amd import regions as G  # noqa: E402
from cellsegmentation_amd import score as S  # noqa: E402

GOLD = np.load(os.path.join(ROOT, "tests", "golden", "overlap_vectors.npz"), allow_pickle=False)
NAMES = sorted(k[:-len(".pred")] for k in GOLD.files if k.endswith(".pred"))
TOL = 1e-12
HOST_TABLES = ("area_pred", "area_truth", "iou_partner", "iou_inter", "inter_partner_truth", "inter_truth", "inter_partner_pred",
               "inter_pred", "n_pairs")


def test_golden_file_is_what_the_maker_writes():
    import make_overlap_golden as MG
    assert NAMES == sorted(name for name, _ in MG.cases())
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "overlap_vectors.npz")) < 256 * 1024


@pytest.mark.parametrize("name", NAMES)
def test_reference_equals_golden(name):
    cp, ct = (int(c) for c in GOLD[f"{name}.caps"])
    t = O.overlap(GOLD[f"{name}.pred"], GOLD[f"{name}.truth"], cp, ct)
    for key in O.TABLES:
        assert t[key].dtype == np.int32 and np.array_equal(t[key], GOLD[f"{name}.{key}"]), key
    for key, col in zip(O.PAIRS, t["pairs"]):
        assert col.dtype == np.int64 and np.array_equal(col, GOLD[f"{name}.pair_{key}"]), key
    s = O.score(t)
    for key in O.SCORES:
        assert s[key].tobytes() == GOLD[f"{name}.score.{key}"].tobytes(), key


def _one(name):
    t = O.overlap(*O.hand_cases()[name])
    return t, O.score(t)


def _pairs(t):
    return [tuple(int(c[k]) for c in t["pairs"][1:]) for k in range(len(t["pairs"][0]))]


def test_hand_worked_answers():
    t, s = _one("iou_vs_inter")
    assert _pairs(t) == [(1, 1, 2), (2, 1, 3)] and t["area_pred"].tolist() == [[2, 30]] and t["area_truth"].tolist() == [[6]]
    assert t["iou_partner"].tolist() == [[1]] and t["iou_inter"].tolist() == [[2]]              # 2/6 beats 3/33
    assert t["inter_partner_truth"].tolist() == [[2]] and t["inter_truth"].tolist() == [[3]]
    assert t["inter_partner_pred"].tolist() == [[1, 1]] and t["inter_pred"].tolist() == [[2, 3]]
    assert (s["aji_inter"][0], s["aji_union"][0]) == (2, 36) and abs(s["aji"][0] - 2 / 36) <= TOL
    assert abs(s["dice_obj"][0] - 17 / 96) <= TOL and (s["n_pred"][0], s["n_truth"][0], s["n_pairs"][0]) == (2, 1, 2)
    t, s = _one("iou_tie")                                              # 2/4 and 2/4: the lower pred label
    assert t["iou_partner"].tolist() == [[1]] and t["inter_partner_truth"].tolist() == [[1]]
    assert (s["aji_inter"][0], s["aji_union"][0]) == (2, 6) and abs(s["aji"][0] - 1 / 3) <= TOL and abs(s["dice_obj"][0] - 2 / 3) <= TOL
    t, s = _one("shared_pred")
    assert t["iou_partner"].tolist() == [[1, 1]] and t["inter_partner_pred"].tolist() == [[1]] and s["n_pairs"][0] == 2
    assert (s["aji_inter"][0], s["aji_union"][0]) == (6, 12) and s["aji"][0] == 0.5 and abs(s["dice_obj"][0] - 2 / 3) <= TOL
    t, s = _one("both_empty")
    assert (t["cap_pred"], t["cap_truth"]) == (1, 1) and len(t["pairs"][0]) == 0
    assert (s["aji"][0], s["dice_obj"][0], s["aji_union"][0], s["n_pred"][0], s["n_truth"][0]) == (1.0, 1.0, 0, 0, 0)
    t, s = _one("pred_empty")
    assert (s["aji"][0], s["dice_obj"][0], s["aji_inter"][0], s["aji_union"][0]) == (0.0, 0.0, 0, 3)
    t, s = _one("truth_empty")
    assert (s["aji"][0], s["dice_obj"][0], s["aji_union"][0]) == (0.0, 0.0, 3) and t["counts_pred"].tolist() == [2]
    t, s = _one("six_pairs")
    assert _pairs(t) == [(1, 1, 2), (1, 2, 1), (2, 2, 2), (2, 3, 1), (3, 3, 2), (3, 4, 1)] and t["n_pairs"].tolist() == [6]
    assert t["iou_partner"].tolist() == [[1, 2, 3, 3]] and t["inter_partner_pred"].tolist() == [[1, 2, 3]]
    t, s = _one("negative")                                             # negative labels are background
    assert _pairs(t) == [(1, 1, 1), (2, 2, 2)] and t["area_pred"].tolist() == [[3, 2]] and t["area_truth"].tolist() == [[3, 2]]
    t, s = _one("inter_tie")                                            # I = 2 with truth 1 and truth 2: the lower truth label
    assert t["inter_partner_pred"].tolist() == [[1]] and t["inter_pred"].tolist() == [[2]] and t["iou_partner"].tolist() == [[1, 1]]
    pred, truth = O.hand_cases()["five_labels"]
    t = O.overlap(pred, truth, 3, 2)                                    # labels above the capacity are background
    assert t["counts_pred"].tolist() == [5] and t["counts_truth"].tolist() == [5]
    assert _pairs(t) == [(1, 1, 1), (1, 2, 1), (2, 2, 1)] and t["area_pred"].tolist() == [[2, 2, 2]] and t["area_truth"].tolist() == [[1, 2]]


def _assert_scores(got, want):
    assert isinstance(got, S.OverlapScore)
    for key in O.SCORES:
        a = getattr(got, key)
        assert a.dtype == want[key].dtype and a.shape == want[key].shape, key
        if a.dtype == np.int64:
            assert np.array_equal(a, want[key]), key
        else:
            assert (np.abs(a - want[key]) <= TOL).all(), key


@pytest.mark.parametrize("name", NAMES)
def test_overlap_score_equals_reference_on_golden_tables(name):
    t = {k: GOLD[f"{name}.{k}"] for k in O.TABLES}
    _assert_scores(S.overlap_score(*(t[k] for k in HOST_TABLES)), O.score(t))
    s = S.overlap_score(*(t[k] for k in HOST_TABLES))
    for key in O.SCORES:
        want = GOLD[f"{name}.score.{key}"]
        assert np.array_equal(getattr(s, key), want) if want.dtype == np.int64 else (np.abs(getattr(s, key) - want) <= TOL).all(), key


def test_overlap_score_hand_cases_and_errors():
    _, pred, truth = O.stacked()
    t = O.overlap(pred, truth)
    s = S.overlap_score(*(t[k] for k in HOST_TABLES))
    _assert_scores(s, O.score(t))
    names = list(O.hand_cases())
    i = names.index("iou_vs_inter")
    assert abs(s.aji[i] - 2 / 36) <= TOL and abs(s.dice_obj[i] - 17 / 96) <= TOL
    assert s.aji[names.index("both_empty")] == 1.0 and s.dice_obj[names.index("both_empty")] == 1.0
    assert s.aji[names.index("pred_empty")] == 0.0 and s.dice_obj[names.index("pred_empty")] == 0.0
    args = [t[k] for k in HOST_TABLES]
    with pytest.raises(ValueError, match="overlap_score"):
        S.overlap_score(*args[:2], args[2][:, :1], *args[3:])
    with pytest.raises(ValueError, match="overlap_score"):
        S.overlap_score(*args[:8], args[8][:1])
    bad = args[2].copy()
    bad[0, 0] = t["cap_pred"] + 1
    with pytest.raises(ValueError, match="outside"):
        S.overlap_score(*args[:2], bad, *args[3:])


def test_argument_errors_before_any_device_work():
    lab = np.zeros((4, 5), np.int32)
    with pytest.raises(TypeError, match="numpy array or a torch tensor"):
        G.overlap_labels([[1]], lab)
    with pytest.raises(TypeError, match="int32 label image"):
        G.overlap_labels(lab.astype(np.int64), lab)
    with pytest.raises(TypeError, match="int32 label image"):
        G.overlap_labels(lab, lab > 0)
    with pytest.raises(ValueError, match=r"\[H, W\] or \[N, H, W\]"):
        G.overlap_labels(lab[0], lab[0])
    with pytest.raises(ValueError, match="empty label image"):
        G.overlap_labels(lab[:0], lab[:0])
    with pytest.raises(ValueError, match="against truth of shape"):
        G.overlap_labels(lab, lab[:, :4])
    with pytest.raises(ValueError, match="against truth of shape"):
        G.overlap_labels(lab, lab[None])
    with pytest.raises(ValueError, match="2\\^31 pixels"):
        big = torch.zeros((1, 1), dtype=torch.int32).expand(1 << 16, 1 << 15)
        G.overlap_labels(big, big)
    for bad in (0, -3, 2.5, True, (4,), (4, 0), (1, 2, 3), (None, 4)):
        with pytest.raises(ValueError, match="max_regions"):
            G.overlap_labels(lab, lab, max_regions=bad)
    for bad in (0, -1, 1.5, True, (1 << 29) + 1):
        with pytest.raises(ValueError, match="max_pairs"):
            G.overlap_labels(lab, lab, max_regions=4, max_pairs=bad)
    for kw in ({"pred_counts": torch.zeros(2, dtype=torch.int32)}, {"truth_counts": torch.zeros(1, dtype=torch.int64)},
               {"pred_counts": np.zeros(1, np.int32)}):
        with pytest.raises(TypeError, match="counts must be an int32 tensor of shape"):
            G.overlap_labels(lab, lab, **kw)
    with pytest.raises(TypeError, match="unexpected arguments"):
        inference.evaluate_instances([], None, None, overlap=True, bogus=1)


def test_overlap_table_on_host_tensors_pairs_score_and_cache():
    """the table's tensors may live anywhere: pairs() sorts the raw slots, score() reads the tables once and keeps the copy"""
    t = O.overlap(*O.hand_cases()["iou_vs_inter"])
    keys = torch.tensor([[0, (2 << 32) | 1, 0, (1 << 32) | 1]], dtype=torch.int64)      # out of order, with empty slots
    counts = torch.tensor([[0, 3, 0, 2]], dtype=torch.int32)
    z = torch.zeros(1, dtype=torch.int32)
    table = G.OverlapTable(torch.from_numpy(t["counts_pred"]), torch.from_numpy(t["counts_truth"]), t["cap_pred"], t["cap_truth"],
                           torch.from_numpy(t["area_pred"]), torch.from_numpy(t["area_truth"]), torch.from_numpy(t["n_pairs"]), z,
                           *(torch.from_numpy(t[k]) for k in O.TABLES[5:]), keys, counts)
    got = table.pairs()
    for a, b in zip(got, t["pairs"]):
        assert a.dtype == np.int64 and np.array_equal(a, b)
    assert not table.overflowed().any()
    table.dropped = torch.ones(1, dtype=torch.int32)
    assert table.overflowed().tolist() == [True]
    s = table.score()
    assert s.aji_inter.tolist() == [2] and s.aji_union.tolist() == [36] and abs(s.dice_obj[0] - 17 / 96) <= TOL
    kept = table._host
    table.area_pred = None                                              # a second call touches no tensor
    assert table.score().aji_union.tolist() == [36] and table._host is kept


def test_library_has_the_entry_points():
    lib = _lib.load()
    assert hasattr(lib, "cs_regions_overlap_labels") and hasattr(lib, "cs_regions_overlap_workspace")
    assert lib.cs_abi_version() == 10
    # 12 N slots + 8 N (2 cap_truth + cap_pred) bytes, slots = the power of two >= 2 max_pairs; every part 16-byte aligned
    assert [K.regions_overlap_slots(m) for m in (1, 2, 3, 4, 5, 8, 9, 5000)] == [2, 4, 8, 8, 16, 16, 32, 16384]
    assert lib.cs_regions_overlap_workspace(1, 4, 1, 1) == 16 + 16 + 2 * 16 + 32
    assert lib.cs_regions_overlap_workspace(3, 1000, 1024, 5000) == 12 * 3 * 16384 + 8 * 3 * (2 * 1024 + 1000)
    assert lib.cs_regions_overlap_workspace(2, 10000, 10000, 30000) == 12 * 2 * 65536 + 8 * 2 * 30000     # far from 2 x 10^4 x 10^4 x 4
    for bad in ((0, 1, 1, 1), (65536, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (1, 1, 1, -1), (1, 1, 1, (1 << 29) + 1),
                (4, 1, 1, 1 << 28), (2, 1 << 30, 1, 1), (2, 1, 1 << 30, 1)):
        assert lib.cs_regions_overlap_workspace(*bad) == 0, bad
    # the call refuses what the workspace function refuses, before anything is launched
    import ctypes
    buf = ctypes.create_string_buffer(64)
    ptr = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    args = lambda N, H, W, cp, ct, mp: (ptr, ptr, N, H, W, cp, ct, mp, None, None) + (ptr,) * 11 + (1 << 20, None)  # noqa: E731
    assert lib.cs_regions_overlap_labels(*args(1, 4, 4, 0, 1, 1)) == -1 and b"capacities" in lib.cs_last_error()
    assert lib.cs_regions_overlap_labels(*args(1, 4, 4, 1, 1, 0)) == -1 and b"max_pairs" in lib.cs_last_error()
    assert lib.cs_regions_overlap_labels(*args(0, 4, 4, 1, 1, 1)) == -1 and b"N H W" in lib.cs_last_error()
    small = list(args(1, 4, 4, 8, 8, 8))
    small[21] = 16
    assert lib.cs_regions_overlap_labels(*small) == -1 and b"workspace too small" in lib.cs_last_error()
    missing = list(args(1, 4, 4, 8, 8, 8))
    missing[12] = None                                                  # n_pairs
    assert lib.cs_regions_overlap_labels(*missing) == -1 and b"NULL" in lib.cs_last_error()
    with pytest.raises(ValueError, match="max_pairs"):
        K.regions_overlap_workspace(1, 1, 1, 0, "cpu")
