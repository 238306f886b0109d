"""CPU: the numpy statement of the object-level Hausdorff tables (tests/hausdorff_ref.py) against answers worked by hand, against
tests/golden/hausdorff_vectors.npz (made by distance transforms: another route) and against scipy's ``directed_hausdorff``;
``score.hausdorff_score`` against that statement on the same integer tables (floats within 1e-12 relative to max(1, value): each is
a sum of at most a few thousand float64 terms); the argument errors of ``regions.hausdorff_labels`` that need no device; the new
entry points in the library."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import hausdorff_ref as HR  # noqa: E402
from cellsegmentation_amd import _lib, inference  # noqa: E402
from cellsegmentation_amd import kernels as K  # noqa: E402
from cellsegmentation_amd import regions as G  # noqa: E402
from cellsegmentation_amd import score as S  # noqa: E402

GOLD = np.load(os.path.join(ROOT, "tests", "golden", "hausdorff_vectors.npz"), allow_pickle=False)
NAMES = sorted(k[:-len(".pred")] for k in GOLD.files if k.endswith(".pred"))
TOL = 1e-12


def close(a, b):
    """float64 arrays: equal where either is not finite, within TOL relative to max(1, |b|) elsewhere"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    fin = np.isfinite(b)
    return a.shape == b.shape and np.array_equal(a[~fin], b[~fin]) and bool((np.abs(a[fin] - b[fin]) <= TOL * np.maximum(1.0, np.abs(b[fin]))).all())


def test_golden_file_is_what_the_maker_writes():
    import make_hausdorff_golden as MG
    assert NAMES == sorted(name for name, _ in MG.cases())
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "hausdorff_vectors.npz")) < 64 * 1024
    for name, (pred, truth) in MG.cases():
        assert np.array_equal(pred, GOLD[f"{name}.pred"]) and np.array_equal(truth, GOLD[f"{name}.truth"])


@pytest.mark.parametrize("name", NAMES)
def test_reference_equals_golden(name):
    t = HR.hausdorff(GOLD[f"{name}.pred"], GOLD[f"{name}.truth"])
    for key in ("area_pred", "area_truth") + HR.TABLES:
        assert t[key].dtype == np.int32 and np.array_equal(t[key], GOLD[f"{name}.{key}"]), key
    s = HR.score(t)
    for key in ("term_truth", "term_pred", "hausdorff_obj"):
        assert close(s[key], GOLD[f"{name}.score.{key}"]), key
    if name == "blobs":                                                 # both partner rules are at work in it
        ov = t["overlap"]
        assert ((t["area_truth"] > 0) & (ov["inter_partner_truth"] == 0)).any() and (ov["inter_partner_truth"] > 0).any()
        assert ((t["area_pred"] > 0) & (ov["inter_partner_pred"] == 0)).any() and (ov["inter_partner_pred"] > 0).any()


def test_reference_against_scipy_directed_hausdorff():
    from scipy.spatial.distance import directed_hausdorff
    rng = np.random.RandomState(7)
    for _ in range(40):
        H, W = rng.randint(1, 12, size=2)
        a, b = rng.rand(H, W) < rng.uniform(0.05, 0.6), rng.rand(H, W) < rng.uniform(0.05, 0.6)
        if not a.any() or not b.any():
            continue
        pa, pb = np.argwhere(a).astype(np.int64), np.argwhere(b).astype(np.int64)
        for x, y in ((pa, pb), (pb, pa)):
            d = directed_hausdorff(x.astype(np.float64), y.astype(np.float64))[0]
            assert HR.directed(x, y) == int(np.rint(d * d))
        t = HR.hausdorff(a.astype(np.int32), b.astype(np.int32))      # one object a side: partners whether they overlap or not
        want = max(HR.directed(pa, pb), HR.directed(pb, pa))
        assert t["d2_truth"].tolist() == [[want]] and t["d2_pred"].tolist() == [[want]]
        assert t["partner_truth"].tolist() == [[1]] and t["partner_pred"].tolist() == [[1]]


def _one(name):
    t = HR.hausdorff(*HR.hand_cases()[name])
    return t, HR.score(t)


def test_hand_worked_answers():
    t, s = _one("apart")
    assert t["overlap"]["n_pairs"].tolist() == [0]                      # nothing overlaps: the partners are the nearest objects
    assert t["partner_truth"].tolist() == [[1]] and t["partner_pred"].tolist() == [[1]]
    assert t["d2_truth"].tolist() == [[25]] and t["d2_pred"].tolist() == [[25]] and s["hausdorff_obj"].tolist() == [5.0]
    t, s = _one("identical")
    assert t["partner_truth"].tolist() == [[0, 2]] and t["d2_truth"].tolist() == [[-1, 0]] and t["d2_pred"].tolist() == [[-1, 0]]
    assert s["hausdorff_obj"].tolist() == [0.0] and s["n_pred"].tolist() == [1]
    sq, frame = (np.argwhere(m > 0).astype(np.int64) for m in HR.square_in_frame())
    assert HR.directed(sq, frame) == 16 and HR.directed(frame, sq) == 8
    edge = np.asarray([p for p in sq if 2 in p or 6 in p])             # the square's boundary pixels reach 4 only
    assert len(edge) == 16 and HR.directed(edge, frame) == 4
    for name in ("square_in_frame", "frame_in_square"):
        t, s = _one(name)
        assert t["overlap"]["n_pairs"].tolist() == [0] and t["d2_truth"].tolist() == [[16]] and t["d2_pred"].tolist() == [[16]]
        assert s["hausdorff_obj"].tolist() == [4.0]
    t, s = _one("both_empty")
    assert t["d2_truth"].tolist() == [[-1]] and t["partner_pred"].tolist() == [[0]] and s["hausdorff_obj"].tolist() == [0.0]
    t, s = _one("pred_empty")
    assert t["partner_truth"].tolist() == [[0]] and t["d2_truth"].tolist() == [[-1]] and t["area_truth"].tolist() == [[3]]
    assert s["hausdorff_obj"].tolist() == [np.inf] and s["term_truth"].tolist() == [np.inf] and s["term_pred"].tolist() == [0.0]
    t, s = _one("truth_empty")
    assert t["partner_pred"].tolist() == [[0, 0]] and t["d2_pred"].tolist() == [[-1, -1]] and s["hausdorff_obj"].tolist() == [np.inf]
    t, s = _one("larger_intersection")
    assert t["partner_truth"].tolist() == [[2]] and t["d2_truth"].tolist() == [[36]]
    assert t["partner_pred"].tolist() == [[1, 1]] and t["d2_pred"].tolist() == [[16, 36]]
    assert close(s["hausdorff_obj"], [(6.0 + (2 / 5 * 4 + 3 / 5 * 6)) / 2])
    t, s = _one("mirror_tie")
    assert t["area_pred"].tolist() == [[2, 0, 2, 1]]
    assert t["partner_truth"].tolist() == [[1]] and t["d2_truth"].tolist() == [[16]]                 # pred 1 and pred 3 both at 16
    assert t["partner_pred"].tolist() == [[1, 0, 1, 1]] and t["d2_pred"].tolist() == [[16, -1, 16, 64]]
    t, s = _one("nearest_candidate")
    assert t["partner_truth"].tolist() == [[2]] and t["d2_truth"].tolist() == [[9]] and t["d2_pred"].tolist() == [[49, 9]]
    t = HR.hausdorff(*HR.hand_cases()["mirror_tie"], 2, 1)              # pred 3 and 4 above the capacity: background
    assert t["counts_pred"].tolist() == [4] and t["partner_pred"].tolist() == [[1, 0]] and t["d2_pred"].tolist() == [[16, -1]]


def test_comb_has_the_runs_it_says():
    m = HR.comb(3, 9)
    assert m.shape == (4, 9) and m[0].all() and m[1:, ::2].all() and not m[1:, 1::2].any()
    starts = (m > 0) & ~np.pad(m > 0, ((0, 0), (1, 0)))[:, :-1]
    assert int(starts.sum()) == 3 * 5 + 1


def test_hausdorff_score_equals_the_reference():
    for pred, truth in [HR.stacked()[1:]] + [(GOLD[f"{n}.pred"], GOLD[f"{n}.truth"]) for n in NAMES]:
        t = HR.hausdorff(pred, truth)
        got, want = S.hausdorff_score(t["area_pred"], t["area_truth"], t["d2_truth"], t["d2_pred"]), HR.score(t)
        assert isinstance(got, S.HausdorffScore)
        for key in HR.SCORES:
            a = getattr(got, key)
            assert a.dtype == want[key].dtype and (np.array_equal(a, want[key]) if a.dtype == np.int64 else close(a, want[key])), key


def test_hausdorff_score_on_hand_tables():
    # image 0: truth areas 3, 1 at d2 16, 0; pred area 4 at d2 9.  image 1: nothing.  image 2: truth only.  image 3: pred only.
    ap = np.asarray([[4, 0], [0, 0], [0, 0], [0, 7]])
    at = np.asarray([[3, 1], [0, 0], [5, 0], [0, 0]])
    dt = np.asarray([[16, 0], [-1, -1], [-1, -1], [-1, -1]])
    dp = np.asarray([[9, -1], [-1, -1], [-1, -1], [-1, -1]])
    s = S.hausdorff_score(ap, at, dt, dp)
    assert s.n_pred.tolist() == [1, 0, 0, 1] and s.n_truth.tolist() == [2, 0, 1, 0]
    assert s.term_truth.tolist() == [3.0, 0.0, np.inf, 0.0] and s.term_pred.tolist() == [3.0, 0.0, 0.0, np.inf]
    assert s.hausdorff_obj.tolist() == [3.0, 0.0, np.inf, np.inf] and s.hausdorff_obj.dtype == np.float64
    with pytest.raises(ValueError, match="hausdorff_score: expected"):
        S.hausdorff_score(ap, at, dt[:, :1], dp)
    with pytest.raises(ValueError, match="hausdorff_score: expected"):
        S.hausdorff_score(ap[0], at[0], dt[0], dp[0])


def test_hausdorff_table_on_host_tensors_score_and_cache():
    t = HR.hausdorff(*HR.hand_cases()["larger_intersection"])
    z = torch.zeros(1, dtype=torch.int32)
    table = G.HausdorffTable(torch.from_numpy(t["counts_pred"]), torch.from_numpy(t["counts_truth"]), t["cap_pred"], t["cap_truth"],
                             torch.from_numpy(t["area_pred"]), torch.from_numpy(t["area_truth"]), z,
                             *(torch.from_numpy(t[k]) for k in HR.TABLES))
    assert not table.overflowed().any()
    assert close(table.score().hausdorff_obj, HR.score(t)["hausdorff_obj"])
    kept = table._host
    table.d2_truth = None                                               # a second call touches no tensor
    assert close(table.score().hausdorff_obj, HR.score(t)["hausdorff_obj"]) and table._host is kept
    table.dropped = torch.ones(1, dtype=torch.int32)
    assert table.overflowed().tolist() == [True]
    table.dropped, table.cap_pred = z, 1
    assert table.overflowed().tolist() == [True]


def test_argument_errors_before_any_device_work():
    lab = torch.zeros((1, 4, 5), dtype=torch.int32)
    with pytest.raises(ValueError, match="against truth of shape"):
        G.hausdorff_labels(lab, lab[:, :3])
    with pytest.raises(TypeError, match="an int32 label image"):
        G.hausdorff_labels(lab, lab > 0)
    for kw in ({"pred_counts": torch.zeros(2, dtype=torch.int32)}, {"truth_counts": torch.zeros(1, dtype=torch.int64)},
               {"pred_counts": np.zeros(1, np.int32)}):
        with pytest.raises(TypeError, match="counts must be an int32 tensor of shape"):
            G.hausdorff_labels(lab, lab, **kw)
    for bad in (0, True, (4,), (None, 4)):
        with pytest.raises(ValueError, match="max_regions"):
            G.hausdorff_labels(lab, lab, max_regions=bad)
    with pytest.raises(ValueError, match="max_pairs"):
        G.hausdorff_labels(lab, lab, max_regions=4, max_pairs=0)
    with pytest.raises(TypeError, match="overlap must be an OverlapTable"):
        G.hausdorff_labels(lab, lab, overlap=object())
    # (H - 1)^2 + (W - 1)^2 has to stay below 2^31 = 46340^2 + 88048
    for shape in ((1, 46342), (46342, 1), (32769, 32769)):
        wide = torch.zeros((1, 1), dtype=torch.int32).expand(*shape)
        with pytest.raises(ValueError, match="do not fit int32"):
            G.hausdorff_labels(wide, wide)
    G._check_hausdorff_shape((1, 46341))
    G._check_hausdorff_shape((3, 2, 46341))
    G._check_hausdorff_shape((3, 297, 46341))                           # 296^2 = 87616
    with pytest.raises(ValueError, match="do not fit int32"):
        G._check_hausdorff_shape((3, 298, 46341))                       # 297^2 = 88209
    with pytest.raises(TypeError, match="unexpected arguments"):
        inference.evaluate_instances([], None, None, hausdorff=True, bogus=1)


def test_library_has_the_entry_points():
    lib = _lib.load()
    for name in ("cs_regions_hausdorff_labels", "cs_regions_hausdorff_workspace", "cs_regions_hausdorff_stage_runs"):
        assert hasattr(lib, name) and name in _lib.exported_symbols()
    assert lib.cs_abi_version() == 10
    runs = K.regions_hausdorff_stage_runs()
    assert 128 <= runs and 8 * runs <= 64 * 1024                         # 8 bytes a run: tens of KB of LDS at most
    # 16 bytes of boxes, 8 of packed minimum, 4 of list and 4 of bound per label of either side, and one counter; every part
    # 16-byte aligned
    assert lib.cs_regions_hausdorff_workspace(1, 1, 1) == 16 + 16 + 16 + 16 + 16 + 16
    assert lib.cs_regions_hausdorff_workspace(3, 1000, 1024) == 32 * 3 * 2024 + 16
    assert lib.cs_regions_hausdorff_workspace(2, 10000, 10000) == 32 * 2 * 20000 + 16     # far from 2 x 10^4 x 10^4 x 4
    for bad in ((0, 1, 1), (65536, 1, 1), (1, 0, 1), (1, 1, 0), (2, 1 << 30, 1), (2, 1, 1 << 30), (1, 1 << 30, 1 << 30)):
        assert lib.cs_regions_hausdorff_workspace(*bad) == 0, bad
    import ctypes
    buf = ctypes.create_string_buffer(64)
    ptr = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    args = lambda N, H, W, cp, ct: (ptr, ptr, N, H, W, cp, ct) + (ptr,) * 7 + (1 << 20, None)  # noqa: E731
    assert lib.cs_regions_hausdorff_labels(*args(1, 4, 4, 0, 1)) == -1 and b"capacities" in lib.cs_last_error()
    assert lib.cs_regions_hausdorff_labels(*args(0, 4, 4, 1, 1)) == -1 and b"N H W" in lib.cs_last_error()
    assert lib.cs_regions_hausdorff_labels(*args(1, 1, 46342, 1, 1)) == -1 and b"(W - 1)^2" in lib.cs_last_error()
    small = list(args(1, 4, 4, 8, 8))
    small[14] = 16
    assert lib.cs_regions_hausdorff_labels(*small) == -1 and b"workspace too small" in lib.cs_last_error()
    missing = list(args(1, 4, 4, 8, 8))
    missing[8] = None                                                   # inter_partner_pred
    assert lib.cs_regions_hausdorff_labels(*missing) == -1 and b"NULL" in lib.cs_last_error()
    with pytest.raises(ValueError, match="capacities"):
        K.regions_hausdorff_workspace(1, 0, 1, "cpu")
