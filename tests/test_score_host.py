"""CPU: the numpy restatement of the point scoring (tests/score_ref.py) and score.precision_recall against the vectors the
reference's own get_prf1 produced (tests/golden/make_score_golden.py), the argument errors of cellsegmentation_amd.score, which
are raised before the library is loaded, and the ABI additions."""
import os
import re

import numpy as np
import pytest
import torch

import score_ref as R
from cellsegmentation_amd import _lib, detect, kernels, score

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "score_vectors.npz"), allow_pickle=False)
NAMES = [str(n) for n in GOLD["names"]]


def test_golden_holds_the_pinned_cases():
    assert len(NAMES) == 41 and NAMES[0] == "random_00" and NAMES[27] == "random_27"
    assert set(NAMES) >= {"both_empty", "tie_goes_to_index_0", "d2_257_is_outside", "d2_244_is_inside", "duplicate_annotations",
                          "duplicate_detections", "stolen_neighbour_next_inside", "stolen_neighbour_next_outside", "order_a_tp1",
                          "order_b_tp2", "chain_30_shifted_by_8"}
    assert tuple(GOLD["order_a_tp1.counts"]) == (1, 1, 1) and tuple(GOLD["order_b_tp2.counts"]) == (2, 0, 0)
    assert np.array_equal(np.sort(GOLD["order_a_tp1.hat"], axis=0), np.sort(GOLD["order_b_tp2.hat"], axis=0))
    assert tuple(GOLD["both_empty.prf"]) == (1.0, 1.0, 1.0) and tuple(GOLD["no_detections_one_annotation.prf"]) == (1.0, 0.0, 0.0)
    assert sum(int(GOLD[f"{n}.counts"][0]) for n in NAMES[:28]) > 100            # the random cases do match points


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_reference_vectors(name):
    hat, gt = GOLD[f"{name}.hat"], GOLD[f"{name}.gt"]
    tp, fp, fn, match = R.score(hat, gt)
    assert [tp, fp, fn] == GOLD[f"{name}.counts"].tolist()
    assert R.prf(tp, fp, fn).tobytes() == GOLD[f"{name}.prf"].tobytes()
    assert match.dtype == np.int32 and len(match) == len(hat) and (match >= 0).sum() == tp and (match == -1).sum() == fp
    taken = match[match >= 0]
    assert len(set(taken.tolist())) == tp and len(gt) - tp == fn


def test_restatement_match_limits_and_radius():
    gt = [(0, 0), (0, 10)]
    assert R.score([(0, 1), (0, 2)], gt)[3].tolist() == [0, 1]
    assert R.score([(0, 1), (0, 2)], [(0, 0), (0, 30)])[3].tolist() == [0, -1]
    assert R.score([(0, 0)], [(0, 16), (16, 0)])[3].tolist() == [0]
    hat = [(0, 1), (0, 2), (50, 50)]
    for lim, kept in ((0, 0), (1, 1), (3, 3), (8, 3), (-1, 2), (-3, 0), (-4, 0)):
        tp, fp, fn, m = R.score(hat, gt, lim)
        assert tp + fp == kept and (m == -2).sum() == 3 - kept and np.array_equal(m[:kept], R.score(hat[:kept], gt)[3])
    assert R.score([(0, 0)], [(4, 16)], radius2=272)[0] == 1 and R.score([(0, 0)], [(4, 16)], radius2=271)[0] == 0
    assert R.score([(3, 3)], [(3, 3)], radius2=0)[0] == 1 and R.score([(3, 3)], [(3, 4)], radius2=0)[0] == 0
    big = [(1 << 31, 0), (0, 0)]                                          # a coordinate outside int32 matches nothing
    assert R.score(big, [((1 << 31) - 1, 0), (0, 0)])[3].tolist() == [-1, 1]
    c, p, m = R.score_batch(*R.ragged([hat, [], hat]), *R.ragged([gt, gt, []]), limits=[-1, 2, 1])
    assert c.tolist() == [[2, 0, 0], [0, 0, 2], [0, 1, 0]] and m.tolist() == [0, 1, -2, -1, -2, -2]
    assert p[1].tolist() == [1.0, 0.0, 0.0] and p[2].tolist() == [0.0, 1.0, 0.0]


def test_precision_recall_bits():
    counts = np.stack([GOLD[f"{n}.counts"] for n in NAMES])
    want = np.stack([GOLD[f"{n}.prf"] for n in NAMES])
    p, r, f1 = score.precision_recall(counts[:, 0], counts[:, 1], counts[:, 2], return_f1=True)
    assert p.dtype == r.dtype == f1.dtype == np.float64
    assert np.stack([p, r, f1], axis=1).tobytes() == want.tobytes()
    for (tp, fp, fn), w in zip(counts.tolist(), want):
        got = score.precision_recall(tp, fp, fn, return_f1=True)
        assert all(isinstance(v, np.float64) for v in got) and np.asarray(got).tobytes() == w.tobytes()
        assert np.asarray(score.precision_recall(tp, fp, fn)).tobytes() == w[:2].tobytes()
    assert score.precision_recall(0, 0, 0, True) == (1.0, 1.0, 1.0) and score.precision_recall(0, 0, 3, True) == (1.0, 0.0, 0.0)
    assert score.precision_recall(0, 2, 0, True) == (0.0, 1.0, 0.0) and score.precision_recall(0, 2, 3, True) == (0.0, 0.0, 0.0)
    assert score.precision_recall(1, 2, 0, True)[2] == (2 * (1 / 3) * 1.0) / (1 / 3 + 1.0)
    with pytest.raises(TypeError):
        score.precision_recall(1.0, 0, 0)
    with pytest.raises(ValueError):
        score.precision_recall(np.asarray([1, -1]), np.asarray([0, 0]), np.asarray([0, 0]))


def test_radius_squared():
    assert [score.radius_squared(r) for r in (0, 16, 16.5, np.float32(2.5), np.int64(3), 46340)] == [0, 256, 272, 6, 9, 46340 ** 2]
    for bad in (-1, -0.5, float("nan"), float("inf"), 46341):
        with pytest.raises(ValueError):
            score.radius_squared(bad)
    for bad in ("16", None, True, [16]):
        with pytest.raises(TypeError):
            score.radius_squared(bad)


def test_argument_errors_come_before_the_library_is_loaded(monkeypatch):
    def no_load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_load)
    monkeypatch.setattr(score, "_device", no_load)
    hat, gt = np.asarray([(0, 0), (5, 5)]), np.asarray([(0, 1)])
    for kw in ({"radius": -1}, {"radius": "16"}, {"radius": float("nan")}, {"radius": 1e6}):
        with pytest.raises((TypeError, ValueError)):
            score.score_points(hat, gt, **kw)
    for bad in (hat.astype(np.float64), hat.astype(np.float32), torch.zeros(2, 2), torch.zeros(2, 2, dtype=torch.bool)):
        with pytest.raises(TypeError):
            score.score_points(bad, gt)
        with pytest.raises(TypeError):
            score.score_points(hat, bad)
    for bad in (np.zeros((2, 3), np.int64), np.zeros(4, np.int64), np.zeros((1, 2, 2), np.int64), torch.zeros(2, 3, dtype=torch.int64)):
        with pytest.raises(ValueError):
            score.score_points(bad, gt)
        with pytest.raises(ValueError):
            score.score_points(hat, bad)
    for bad in ([0, 1], [0, 3], [1, 2], [0, 2, 1, 2], [0], np.asarray([0.0, 2.0])):
        with pytest.raises(ValueError):
            score.score_points(hat, gt, hat_offsets=bad, offsets=[0, 1] if len(bad) == 2 else [0, 0, 1, 1])
    with pytest.raises(ValueError):
        score.score_points(hat, gt, hat_offsets=[0, 1, 2], offsets=[0, 1])            # two images of detections, one of annotations
    with pytest.raises(ValueError):
        score.score_points(hat, np.asarray([(0, 1 << 31)]))                            # does not fit int32
    with pytest.raises(ValueError):
        score.score_points(hat, np.asarray([(-(1 << 31) - 1, 0)]))
    with pytest.raises(ValueError):
        score.score_points(hat, np.asarray([(1 << 31, 0)]), gt_xy=True)
    with pytest.raises(TypeError):
        score.score_points(hat, gt, limits=1.5)
    with pytest.raises(ValueError):
        score.score_points(hat, gt, limits=[1, 2])
    many = np.zeros(65537, np.int64)                                      # 65536 images
    with pytest.raises(ValueError, match="65535"):
        score.score_points(hat, gt, hat_offsets=np.r_[many[:-1], 2], offsets=np.r_[many[:-1], 1])
    # the raw binding refuses host tensors, wrong dtypes and wrong shapes before it loads anything either
    t = torch.zeros(2, 2, dtype=torch.int64)
    off = torch.tensor([0, 2])
    with pytest.raises(ValueError):
        kernels.score_points(t, off, t.int(), off)
    with pytest.raises((TypeError, ValueError)):
        kernels.score_points(t, off.int(), t.int(), off)
    # DetectResult.score: the annotations must say which map they belong to
    res = detect.DetectResult(np.zeros((3, 2), np.int64), np.zeros(3, np.int64), np.asarray([0, 1, 3]), np.asarray([1, 2]))
    for bad in (gt, [gt], [gt, gt, gt], np.zeros((3, 4, 2), np.int64)):
        with pytest.raises(ValueError):
            res.score(bad)
    with pytest.raises(TypeError):
        res.score([gt, gt.astype(np.float32)])
    with pytest.raises(ValueError):
        res.score([gt, gt], radius=-2)


def test_new_symbols_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "cellseg_hip.h")).read()
    for name in ("cs_score_workspace", "cs_score_points"):
        assert re.search(rf"^(size_t|int) {name}\(", header, re.M), name
        assert name in _lib._SIGNATURES and name in _lib.exported_symbols()
    assert len(_lib._SIGNATURES["cs_score_points"][1]) == 13 and _lib._SIGNATURES["cs_score_workspace"][0] is _lib.c_size_t
    lib = _lib.load()
    assert lib.cs_abi_version() == 10
    assert lib.cs_score_workspace(0, 10) == 0 and lib.cs_score_workspace(65536, 10) == 0 and lib.cs_score_workspace(1, -1) == 0
    assert lib.cs_score_workspace(1, 0) == 16 and lib.cs_score_workspace(300, 1 << 20) >= ((1 << 20) // 32 + 300) * 4
    # refused before any launch (no GPU needed): N, a NULL offset table, a negative radius2, unknown flag bits
    for args in ((0, 256, 0), (65536, 256, 0), (1, -1, 0), (1, 256, 2)):
        assert lib.cs_score_points(None, None, None, None, None, args[0], args[1], args[2], None, None, None, 0, None) != 0
    assert b"score_points" in lib.cs_last_error()


def test_detect_result_keeps_its_five_positional_fields():
    pts = np.asarray([(1, 1), (2, 2), (3, 3)], np.int64)
    res = detect.DetectResult(pts, np.asarray([9, 8, 7]), np.asarray([0, 1, 3]), np.asarray([1, 2]), [1, 1])
    assert res.device_points is None and res.device_offsets is None
    per = res.per_image()
    assert np.array_equal(per[0][0], pts[:1]) and np.array_equal(per[1][0], pts[1:2]) and np.array_equal(per[1][1], pts[2:])
    import dataclasses
    assert [f.name for f in dataclasses.fields(res)][:5] == ["points", "weights", "offsets", "n_kept", "cell_counts"]
    assert detect.DetectResult(pts, res.weights, res.offsets, res.n_kept).per_image()[1][1] == []
