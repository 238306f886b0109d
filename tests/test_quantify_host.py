"""CPU: the numpy restatement of the per-cell stain tables (tests/quantify_ref.py) against hand-worked cases, against its own
bincount form and its pinned vectors (tests/golden/make_quantify_golden.py); the integer level against the float64 uint8
concentration of tests/stain_ref.py; ``StainTable``'s methods on host tensors against the restatement; the argument errors of
``stain.quantify_labels``, ``StainTable``, ``score.positivity_score`` and ``inference.slide_positivity``, raised before the library
is loaded; the new entry point's declaration, binding and refusals (no GPU needed)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import quantify_ref as Q
import stain_ref as R
from cellsegmentation_amd import _lib, inference, kernels, regions, score, stain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "quantify_vectors.npz"), allow_pickle=False)
NAMES = [str(n) for n in GOLD["names"]]

# the hand case: four colours whose levels under HAND_MQ are worked out below
HAND_MQ = np.asarray([[[1 << 24, 0, 0], [0, 1 << 20, -(1 << 24)]]], np.int64)    # level 0 = od_q[R]; level 1 = floor(od_q[G] / 16 - od_q[B] + 1/2)
A, B, C, D = (230, 230, 239), (238, 226, 239), (0, 230, 238), (239, 239, 239)
HAND_LABELS = np.asarray([[[1, 1, 2], [1, 2, 2], [0, -1, 2]]], np.int32)
HAND_IMAGE = np.asarray([[[A, B, A], [C, A, D], [C, C, B]]], np.uint8)


@pytest.fixture()
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", refuse)


def table_of(t, conc_max=8.0, pos=True):
    """a reference dict as a StainTable of host tensors"""
    T = lambda k, dt: torch.from_numpy(t[k].astype(dt))  # noqa: E731
    return stain.StainTable(T("counts", np.int32), t["n"].shape[1], T("n", np.int32), T("sum", np.int64), T("sumsq", np.int64),
                            T("max", np.int32), T("pos", np.int32) if pos else None, T("hist", np.int32) if "hist" in t else None,
                            np.zeros((t["n"].shape[0], t["sum"].shape[-1], 3), np.int32), stain.StainOptions(conc_max=conc_max))


def test_hand_worked_levels_and_tables():
    od = Q.od_table(240)
    assert (od[239], od[238], od[230], od[226], od[0]) == (0, 17, 157, 228, 22449)
    lv = Q.levels(HAND_IMAGE, HAND_MQ[0])
    assert lv[0, 0, 0].tolist() == [157, 10]            # A: 157; floor(157 / 16 - 0 + 1/2) = floor(10.31)
    assert lv[0, 0, 1].tolist() == [17, 14]             # B: 17; floor(228 / 16 + 1/2) = floor(14.75)
    assert lv[0, 1, 0].tolist() == [255, 0]             # C: 22449 clamps to 255; floor(9.81 - 17 + 1/2) = -7 clamps to 0 (arithmetic shift)
    assert lv[0, 1, 2].tolist() == [0, 0]               # D
    for fn in (Q.quantify, Q.quantify_fast):
        t = fn(HAND_IMAGE, HAND_LABELS, HAND_MQ, 2, pos_levels=[100, 10], bins=16)
        assert t["counts"].tolist() == [2] and t["n"][0, :, 0].tolist() == [3, 4]                  # label 1: A B C, label 2: A A D B
        assert t["sum"][0, :, 0].tolist() == [[429, 24], [331, 34]]
        assert t["sumsq"][0, :, 0].tolist() == [[89963, 296], [49587, 396]]
        assert t["max"][0, :, 0].tolist() == [[255, 14], [157, 14]]
        assert t["pos"][0, :, 0].tolist() == [[2, 2], [2, 3]]
        h = t["hist"][0, :, 0]
        assert h[0, 0, [1, 9, 15]].tolist() == [1, 1, 1] and h[0, 0].sum() == 3 and h[0, 1, 0] == 3
        assert h[1, 0, [0, 1, 9]].tolist() == [1, 1, 2] and h[1, 1, 0] == 4
        short = fn(HAND_IMAGE, HAND_LABELS, HAND_MQ, 1)
        assert short["counts"].tolist() == [2] and short["n"].shape == (1, 1, 1) and short["sum"][0, 0, 0].tolist() == [429, 24]
    ring = np.asarray([[[1, 1, 2], [1, 2, 2], [1, 7, 2]]], np.int32)                               # (2, 0) joins cell 1's ring, (2, 1) is above the rows
    t = Q.quantify(HAND_IMAGE, HAND_LABELS, HAND_MQ, 2, expanded=ring)
    assert t["counts"].tolist() == [7] and t["n"][0].tolist() == [[3, 1], [4, 0]] and t["sum"][0, 0, 1].tolist() == [255, 0]


def test_reference_forms_agree_and_golden_regenerates():
    rng = np.random.RandomState(1)
    lab = np.stack([Q.blocks(13, 70, seed=s, n_labels=6) for s in range(2)])
    grown = np.stack([Q.grow(x, 2) for x in lab])
    img = rng.randint(0, 256, size=(2, 13, 70, 3)).astype(np.uint8)
    Mq = np.stack([Q.quantised_matrix(Q.HDAB, True, 2.5), Q.quantised_matrix(Q.HDAB[:, ::-1], True, 2.5)])
    for cap, ring in ((6, grown), (3, None)):
        a, b = (fn(img, lab, Mq, cap, ring, [40, 80, 0], 32) for fn in (Q.quantify, Q.quantify_fast))
        assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    assert (a["pos"][..., 2] == a["n"]).all() and a["n"].sum() > 0                                 # level >= 0 always
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_quantify_golden as G
    fresh = G.build()
    assert sorted(fresh) == sorted(GOLD.files) and NAMES == ["hand_3x3", "strip_5x129_ring", "batch3_17x65_k3", "wide_64x130_short"]
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "quantify_vectors.npz")) < 1 << 20
    for key in GOLD.files:
        assert GOLD[key].dtype == fresh[key].dtype and np.array_equal(GOLD[key], fresh[key]), key
    assert max(GOLD[f"{n}.images"].shape[1] for n in NAMES) <= 64 and max(GOLD[f"{n}.images"].shape[2] for n in NAMES) <= 130


@pytest.mark.parametrize("conc_max", [8, 2.5, 0.7])
def test_level_is_the_uint8_concentration_to_one_level(conc_max):
    img = np.random.RandomState(0).randint(0, 256, size=(64, 64, 3)).astype(np.uint8)
    for residual in (False, True):
        Mq = Q.quantised_matrix(Q.HDAB, residual, conc_max)
        assert np.array_equal(Mq, stain.quantised_matrix(stain.HDAB, residual, conc_max)) and np.abs(Mq).max() < 1 << 23
        want = R.separate_u8(img, R.HDAB, residual, 240, conc_max).astype(np.int64)
        assert np.abs(Q.levels(img, Mq) - want).max() <= 1


def test_quantised_matrix_overflow_and_thresholds(no_library):
    with pytest.raises(ValueError, match="int32"):
        stain.quantised_matrix(stain.HDAB, False, 1e-4)
    with pytest.raises(ValueError, match="int32"):
        Q.quantised_matrix(Q.HDAB, False, 1e-4)
    with pytest.raises(ValueError, match="int32"):
        stain.quantify_labels(np.zeros((4, 4, 3), np.uint8), np.zeros((4, 4), np.int32), options=stain.StainOptions(conc_max=1e-4))
    assert stain.quantised_matrix(stain.StainEstimate(stain.HDAB, np.ones(2))).dtype == np.int32
    assert stain.positive_levels(None, 2, 8.0) is None
    assert stain.positive_levels((0.0, 8.0), 2, 8.0) == (0, 255) and stain.positive_levels((-1.0, 9.0, 1.0), 3, 8.0) == (0, 256, 32)
    assert list(stain.positive_levels((0.5, 0.25), 2, 2.5)) == Q.positive_levels((0.5, 0.25), 2.5) == [51, 26]
    assert stain.class_thresholds((0.2, 0.4, 0.6), 8.0) == Q.class_thresholds((0.2, 0.4, 0.6)) == [1632, 3264, 4896]
    assert stain.class_thresholds(1.0, 8.0) == [8160]
    for bad in ((), (0.1, 0.2, 0.3, 0.4), (0.2, 0.2), (0.3, 0.2), (-0.1,), ("a",), "abc", None, (float("nan"),), (True,)):
        with pytest.raises(ValueError, match="thresholds"):
            stain.class_thresholds(bad, 8.0)
    with pytest.raises(ValueError, match="2\\^31"):
        stain.class_thresholds((1e6,), 8.0)
    for bad in ((1.0,), (1.0, 2.0, 3.0), "ab", 1.0, (1.0, "x"), (float("inf"), 1.0)):
        with pytest.raises(ValueError, match="pixel_threshold"):
            stain.positive_levels(bad, 2, 8.0)


def test_quantify_labels_argument_errors(no_library):
    img, lab = np.zeros((4, 5, 3), np.uint8), np.zeros((4, 5), np.int32)
    q = stain.quantify_labels
    for bad in (np.zeros((4, 5, 3), np.float32), "img", np.zeros((4, 5, 3), np.int32)):
        with pytest.raises(TypeError):
            q(bad, lab)
    for bad in (np.zeros((4, 5), np.uint8), np.zeros((4, 5, 4), np.uint8), np.zeros((0, 5, 3), np.uint8)):
        with pytest.raises(ValueError):
            q(bad, lab)
    for bad in (np.zeros((4, 5), np.int64), np.zeros((4, 5), bool), "lab"):
        with pytest.raises(TypeError):
            q(img, bad)
        with pytest.raises(TypeError):
            q(img, lab, expanded=bad)
    for bad in (np.zeros((5, 4), np.int32), np.zeros((2, 4, 5), np.int32)):
        with pytest.raises(ValueError, match="labels of shape"):
            q(img, bad)
        with pytest.raises(ValueError, match="expanded of shape"):
            q(img, lab, expanded=bad)
    for bad in (np.zeros((3, 3)), np.full((3, 2), np.nan), np.zeros((2, 3, 2))):
        with pytest.raises(ValueError, match="stains"):
            q(img, lab, stains=bad)
    with pytest.raises(ValueError, match="stain matrices"):
        q(img, lab, stains=[stain.HDAB, stain.HDAB])
    with pytest.raises(ValueError, match="parallel"):
        q(img, lab, stains=np.stack([Q.H_VEC, Q.H_VEC], axis=1), residual=True)
    for bad in (8, 1, 255, -16, 512, True, 16.5, None):
        with pytest.raises(ValueError, match="bins"):
            q(img, lab, bins=bad)
    for bad in ((1.0,), (1.0, 1.0, 1.0), 0.5):
        with pytest.raises(ValueError, match="pixel_threshold"):
            q(img, lab, pixel_threshold=bad)
    with pytest.raises(ValueError, match="pixel_threshold"):
        q(img, lab, residual=True, pixel_threshold=(1.0, 1.0))
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="max_regions"):
            q(img, lab, max_regions=bad)
    with pytest.raises(TypeError, match="counts"):
        q(img, lab, counts=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(TypeError, match="counts"):
        q(img, lab, counts=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(TypeError, match="StainOptions"):
        q(img, lab, options={"Io": 240})
    with pytest.raises(TypeError, match="table"):
        q(img, lab, table=object())
    z = lambda *s: torch.zeros(s, dtype=torch.int32)  # noqa: E731
    rt = regions.RegionTable(z(1), 3, z(1, 3), z(1, 3, 4), torch.zeros((1, 3, 2), dtype=torch.int64))
    with pytest.raises(ValueError, match="max_regions 4 against"):
        q(img, lab, table=rt, max_regions=4)
    with pytest.raises(ValueError, match="counts come with the table"):
        q(img, lab, table=rt, counts=z(1))
    rt2 = regions.RegionTable(z(2), 3, z(2, 3), z(2, 3, 4), torch.zeros((2, 3, 2), dtype=torch.int64))
    with pytest.raises(ValueError, match="2 images for 1"):
        q(img, lab, table=rt2)


def test_stain_table_methods_on_host_tensors():
    rng = np.random.RandomState(4)
    lab = np.stack([Q.blocks(20, 40, seed=7, n_labels=5), np.zeros((20, 40), np.int32)])
    img = rng.randint(0, 256, size=(2, 20, 40, 3)).astype(np.uint8)
    Mq = np.stack([Q.quantised_matrix(Q.HDAB, False, 2.5)] * 2)
    ref = Q.quantify_fast(img, lab, Mq, 7, np.stack([Q.grow(x, 2) for x in lab]), [50, 60], 32)
    t = table_of(ref, 2.5)
    same = lambda a, b: np.allclose(a.numpy(), b, rtol=0, atol=1e-12, equal_nan=True)  # noqa: E731
    assert same(t.mean(), Q.mean(ref)) and same(t.std(), Q.std(ref)) and same(t.positive_fraction(), Q.positive_fraction(ref))
    assert np.isnan(t.mean().numpy()[1]).all() and np.isfinite(t.mean().numpy()[0, ref["n"][0, :, 0] > 0, 0]).all()
    for qq in (0.0, 0.5, 0.9, 1.0):
        assert same(t.quantile(qq), Q.quantile(ref, qq))
    assert t.concentration(255) == 2.5 and same(t.concentration(t.mean()), Q.mean(ref) * 2.5 / 255.0)
    assert t.overflowed().tolist() == [False, False] and table_of(Q.quantify_fast(img, lab, Mq, 2), 2.5).overflowed().tolist() == [True, False]
    for thr, st, comp in (((0.2, 0.4, 0.6), 1, 0), ((0.5,), 0, 1), ((0.1, 1.0), 1, 1)):
        cls = t.classify(thr, st, comp)
        assert cls.dtype == torch.int8 and np.array_equal(cls.numpy(), Q.classify(ref, thr, st, comp, 2.5))
        got, (n, li, hs) = t.score(thr, st, comp), Q.score(ref, thr, st, comp, 2.5)
        assert np.array_equal(got.n_cells, n) and np.allclose(got.labelling_index, li, rtol=0, atol=1e-12, equal_nan=True)
        assert np.allclose(got.h_score, hs, rtol=0, atol=1e-12, equal_nan=True) and np.isnan(got.h_score[1]) and got.n_cells[1] == 0
    per = t.per_image()
    assert len(per) == 2 and per[0]["n"].shape == (int(ref["counts"][0]), 2) and per[1]["sum"].shape == (0, 2, 2)
    assert np.array_equal(per[0]["hist"], ref["hist"][0, :len(per[0]["n"])]) and same(torch.from_numpy(per[0]["std"]), Q.std(ref)[0, :len(per[0]["n"])])
    bare = table_of(Q.quantify_fast(img, lab, Mq, 7), 2.5, pos=False)
    with pytest.raises(ValueError, match="pixel_threshold"):
        bare.positive_fraction()
    with pytest.raises(ValueError, match="histogram"):
        bare.quantile(0.5)
    for kw in (dict(stain=2), dict(stain=-1), dict(compartment=1), dict(stain=True), dict(stain=1.0)):
        with pytest.raises(ValueError, match="stain|compartment"):
            bare.classify((0.2,), **kw)
    with pytest.raises(ValueError, match="q must"):
        t.quantile(1.5)


def test_classify_on_the_threshold_exactly():
    """mean level 32 = concentration 32 * 8 / 255: T = rint(65280 t / 8) = 8192 = 256 * 32, so 256 sum >= T n holds with equality"""
    t = {"counts": np.asarray([3]), "n": np.asarray([[[4], [4], [0]]]), "sum": np.asarray([[[[0, 128]], [[0, 127]], [[0, 0]]]]),
         "sumsq": np.zeros((1, 3, 1, 2), np.int64), "max": np.zeros((1, 3, 1, 2), np.int64), "pos": np.zeros((1, 3, 1, 2), np.int64)}
    thr = (32 * 8.0 / 255.0,)
    assert stain.class_thresholds(thr, 8.0) == [8192]
    assert table_of(t).classify(thr).tolist() == [[1, 0, -1]] == Q.classify(t, thr).tolist()
    s = table_of(t).score(thr)
    assert s.class_counts.tolist() == [[1, 1, 0, 0]] and s.labelling_index.tolist() == [50.0] and s.h_score.tolist() == [50.0]


def test_positivity_score_arithmetic():
    s = score.positivity_score([[10, 20, 30, 40], [0, 0, 0, 0], [5, 0, 0, 0], [0, 0, 0, 7]])
    assert isinstance(s, score.PositivityScore) and s.n_cells.tolist() == [100, 0, 5, 7]
    assert s.labelling_index[[0, 2, 3]].tolist() == [90.0, 0.0, 100.0] and s.h_score[[0, 2, 3]].tolist() == [200.0, 0.0, 300.0]
    assert np.isnan(s.labelling_index[1]) and np.isnan(s.h_score[1])
    one = score.positivity_score(np.asarray([3, 1]))
    assert one.class_counts.tolist() == [[3, 1, 0, 0]] and one.labelling_index.tolist() == [25.0] and one.h_score.tolist() == [25.0]
    n, li, hs = Q.positivity([[10, 20, 30, 40], [0, 0, 0, 0]])
    assert n.tolist() == [100, 0] and li[0] == 90.0 and hs[0] == 200.0 and np.isnan(li[1]) and np.isnan(hs[1])
    for bad in ([1.0, 2.0], [[1, -1]], [1], [1, 2, 3, 4, 5], np.zeros((1, 1, 2), np.int64), "ab"):
        with pytest.raises(ValueError, match="positivity_score"):
            score.positivity_score(bad)


def test_slide_positivity_argument_errors(no_library):
    res = inference.SlideResult(np.zeros((0, 2), np.int64), [], 0, torch.zeros(4, 4, dtype=torch.uint8))
    img = np.zeros((4, 4, 3), np.uint8)
    with pytest.raises(TypeError, match="SlideResult"):
        inference.slide_positivity(object(), img)
    for bad in (np.zeros((4, 4), np.uint8), np.zeros((4, 5, 3), np.uint8), np.zeros((4, 4, 3), np.float32), "img"):
        with pytest.raises(TypeError, match="image_u8"):
            inference.slide_positivity(res, bad)
    with pytest.raises(ValueError, match="thresholds"):
        inference.slide_positivity(res, img, thresholds=(0.4, 0.2))
    with pytest.raises(ValueError, match="stains"):
        inference.slide_positivity(res, img, stains=np.zeros((2, 3)))
    with pytest.raises(TypeError, match="radius"):
        inference.slide_positivity(res, img, distance="far")
    with pytest.raises(TypeError, match="StainOptions"):
        inference.slide_positivity(res, img, options=8.0)


def test_new_symbol_is_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "cellseg_hip.h")).read()
    name = "cs_stain_quantify_labels"
    assert re.search(rf"^int {name}\(", header, re.M)
    assert name in _lib._SIGNATURES and name in _lib.exported_symbols() and len(_lib._SIGNATURES[name][1]) == 20
    lib = _lib.load()
    assert hasattr(lib, name) and lib.cs_abi_version() == 10
    assert kernels.STAIN_QUANTIFY_BINS == stain.QUANTIFY_BINS == Q.BINS


def test_entry_point_refuses_bad_calls_without_a_gpu():
    lib = _lib.load()
    buf = (ctypes.c_int64 * 64)()                                          # host memory: nothing is launched
    base = ctypes.addressof(buf)
    base += -base % 16
    P = ctypes.c_void_p
    levels = (ctypes.c_int32 * 3)(0, 256, 10)

    def call(img=base, lab=base, exp=None, N=1, H=4, W=4, od=base, Mq=base, K=2, lv=None, bins=0, cap=2, counts=None, n=base, s=base,
             ss=base, mx=base, pos=base, hist=None):
        return lib.cs_stain_quantify_labels(P(img), P(lab), P(exp), N, H, W, P(od), P(Mq), K, lv, bins, cap, P(counts), P(n), P(s), P(ss),
                                            P(mx), P(pos), P(hist), None)

    cases = (dict(img=None), dict(lab=None), dict(od=None), dict(Mq=None), dict(n=None), dict(s=None), dict(ss=None), dict(mx=None),
             dict(pos=None), dict(N=0), dict(N=65536), dict(H=0), dict(W=-1), dict(H=46341, W=46341), dict(N=2, H=32768, W=32768),
             dict(K=1), dict(K=4), dict(bins=8), dict(bins=-16), dict(bins=48), dict(bins=512), dict(bins=16), dict(hist=base),
             dict(cap=0), dict(cap=-3), dict(N=65535, H=1, W=1, cap=1 << 30), dict(cap=1 << 22, bins=256, hist=base),
             dict(lab=base + 2), dict(exp=base + 1), dict(od=base + 2), dict(Mq=base + 3), dict(s=base + 4), dict(ss=base + 4),
             dict(lv=(ctypes.c_int32 * 2)(0, 257)), dict(lv=(ctypes.c_int32 * 2)(-1, 0)), dict(K=3, lv=(ctypes.c_int32 * 3)(0, 0, 300)))
    for kw in cases:
        assert call(**kw) == -1, kw
        assert b"stain_quantify_labels" in lib.cs_last_error(), (kw, lib.cs_last_error())
    assert levels[1] == 256                                                # (a level of 256 itself is in range: "no pixel is positive")
