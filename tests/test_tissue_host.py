"""CPU: the numpy restatement of the tissue detection (tests/tissue_ref.py) against its pinned vectors
(tests/golden/make_tissue_golden.py), exact Otsu against the float64 between-class variance, the argument errors of
cellsegmentation_amd.tissue and of detect_slide(tissue=...), which are raised before the library is loaded or the model touched,
and the ABI additions with their refusals (no GPU needed)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import tissue_ref as R
from cellsegmentation_amd import _lib, inference, kernels, tissue

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "tissue_vectors.npz"), allow_pickle=False)
NAMES = [str(n) for n in GOLD["names"]]
C, D = 0, 1                                                                # axis 0 of every recorded result: chroma, darkness


def case_size(name):
    s = GOLD[f"{name}.size"].tolist()
    return s[0] if len(s) == 1 else tuple(s)


def test_golden_holds_the_pinned_cases():
    assert len(NAMES) == 25 and NAMES[0] == "random_00" and NAMES[11] == "random_11"
    assert set(NAMES) >= {"all_white", "single_valued_non_white", "two_valued", "otsu_tie_lower_t_wins", "pixels_at_t_and_t_plus_1",
                          "black_stroke_on_white", "saturated_primary", "w_equals_1", "odd_37x53", "odd_5x7", "patch_equals_image",
                          "border_aligned_last_origins", "batch_two_thresholds"}
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "tissue_vectors.npz")) < 128 * 1024
    assert GOLD["all_white.thr"].tolist() == [0, 0] and not GOLD["all_white.mask"].any()
    assert GOLD["all_white.hist"][C, 0] == 20 * 24 and GOLD["all_white.hist"][D, 0] == 20 * 24
    assert GOLD["single_valued_non_white.thr"][C] == 110 and not GOLD["single_valued_non_white.mask"].any()
    assert GOLD["two_valued.thr"][C] == 0 and GOLD["two_valued.mask"][C].sum() == 20 * 15        # the lower of the two values
    assert GOLD["otsu_tie_lower_t_wins.thr"][C] == 10 and GOLD["otsu_tie_lower_t_wins.hist"][C, [10, 20, 30]].tolist() == [144] * 3
    assert GOLD["pixels_at_t_and_t_plus_1.given_threshold"] == 40 and GOLD["pixels_at_t_and_t_plus_1.hist"][C, [40, 41]].tolist() == [48, 48]
    assert GOLD["pixels_at_t_and_t_plus_1.mask"][C].sum() == 48
    assert not GOLD["black_stroke_on_white.mask"][C].any() and GOLD["black_stroke_on_white.mask"][D].sum() == 3 * 28     # chroma ignores the pen
    assert GOLD["saturated_primary.hist"][C, 255] == 256 and GOLD["saturated_primary.n_selected"][C, 3] == 4             # full windows only
    assert GOLD["w_equals_1.images"].shape == (41, 1, 3) and GOLD["w_equals_1.size"].tolist() == [8, 1]
    assert GOLD["odd_37x53.images"].size % 4 and GOLD["odd_5x7.images"].size % 4
    assert GOLD["patch_equals_image.tile_rc"].tolist() == [[0, 0]]
    assert GOLD["border_aligned_last_origins.tile_rc"][-1].tolist() == [22, 27]
    assert GOLD["batch_two_thresholds.thr"][C, 0] != GOLD["batch_two_thresholds.thr"][C, 1]
    for name in NAMES:
        T = len(GOLD[f"{name}.tile_rc"])
        ph, pw = np.broadcast_to(GOLD[f"{name}.size"], (2,)).tolist()
        assert GOLD[f"{name}.needs"].tolist() == [0, R.min_pixels(0.01, ph, pw), (ph * pw + 1) // 2, ph * pw, ph * pw + 1]
        assert (GOLD[f"{name}.n_selected"][:, 0] == T).all() and (GOLD[f"{name}.n_selected"][:, 4] == 0).all()   # everything, nothing


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_vectors(name):
    images, size = GOLD[f"{name}.images"], case_size(name)
    ti, rc = GOLD[f"{name}.tile_img"], GOLD[f"{name}.tile_rc"]
    given = int(GOLD[f"{name}.given_threshold"]) if f"{name}.given_threshold" in GOLD.files else None
    for c, ch in enumerate(R.CHANNELS):
        hist = R.histogram(images, ch)
        assert hist.dtype == np.int64 and np.array_equal(hist, GOLD[f"{name}.hist"][c])
        assert hist.sum() == images.size // 3
        thr = R.otsu(hist) if given is None else given
        assert np.array_equal(np.asarray(thr, np.int32), GOLD[f"{name}.thr"][c])
        assert tissue.otsu(hist) == R.otsu(hist)                            # the product's host half against the restatement
        m = R.mask(images, thr, ch)
        assert m.dtype == np.uint8 and np.array_equal(m, GOLD[f"{name}.mask"][c]) and m.max(initial=0) <= 1
        cover = R.coverage(m, ti, rc, size)
        assert cover.dtype == np.int32 and np.array_equal(cover, GOLD[f"{name}.cover"][c])
        ph, pw = np.broadcast_to(GOLD[f"{name}.size"], (2,)).tolist()
        brute = [int(np.count_nonzero(m.reshape((-1,) + m.shape[-2:])[n, r:r + ph, q:q + pw])) for n, (r, q) in zip(ti, rc)]
        assert cover.tolist() == brute                                      # the integral image against plain slices
        for k, need in enumerate(GOLD[f"{name}.needs"]):
            sel, n = R.select(cover, int(need))
            assert np.array_equal(sel, GOLD[f"{name}.selected"][c, k]) and n == GOLD[f"{name}.n_selected"][c, k]
            assert np.all(np.diff(sel[:n]) > 0) and np.all(sel[n:] == -1)


def test_exact_otsu_equals_the_float64_argmax():
    for name in NAMES[:12]:
        for c in (C, D):
            h = GOLD[f"{name}.hist"][c]
            assert R.otsu(h) == R.otsu_float(h) == tissue.otsu(h), name
    for seed in (31, 32):
        slide = R.blob_slide(seed=seed)
        got = {ch: R.otsu(R.histogram(slide, ch)) for ch in R.CHANNELS}
        print(f"blob slide, seed {seed}: thresholds {got}")
        for ch in R.CHANNELS:
            assert got[ch] == R.otsu_float(R.histogram(slide, ch)) == tissue.otsu(R.histogram(slide, ch))
        assert 20 <= got["chroma"] <= 60 and 50 <= got["darkness"] <= 120   # between the ground and the blobs


def test_otsu_edge_cases_and_batches():
    empty = np.zeros(256, np.int64)
    assert tissue.otsu(empty) == 0 and R.otsu(empty) == 0
    one = empty.copy()
    one[77] = 5
    assert tissue.otsu(one) == 77 and tissue.otsu(one.tolist()) == 77 and tissue.otsu(torch.from_numpy(one)) == 77
    two = one.copy()
    two[200] = 1
    assert tissue.otsu(two) == 77 and tissue.otsu(np.stack([one, two, empty])) == [77, 77, 0]
    last = empty.copy()
    last[[254, 255]] = 3
    assert tissue.otsu(last) == 254                                        # t = 254 is the last candidate
    big = empty.copy()
    big[[3, 250]] = 1 << 40                                                # sums far beyond float64's integers
    assert tissue.otsu(big) == 3
    for bad in (np.zeros(255, np.int64), np.zeros((2, 2, 256), np.int64), np.zeros(256, np.float64), -np.ones(256, np.int64)):
        with pytest.raises(ValueError):
            tissue.otsu(bad)


def test_the_slide_of_the_end_to_end_test():
    """the facts tests/test_tissue_gpu.py builds on, from the restatement alone"""
    slide = R.blob_slide(seed=31)
    assert slide.shape == (150, 170, 3) and (slide[10:14, 8:38] == 12).all()
    chroma = R.select_patches(slide, 64, 48, "chroma", need=41)
    assert R.min_pixels(0.01, 64, 64) == 41 and len(chroma["corners"]) == 12
    assert chroma["selected"].tolist() == [5, 6, 7, 9, 10, 11] and not chroma["mask"][:70].any() and not chroma["mask"][:, :60].any()
    dark = R.select_patches(slide, 64, 48, "darkness", need=41)
    assert dark["selected"].tolist() == [0, 5, 6, 7, 9, 10, 11] and dark["coverage"][0] == 120
    assert R.select_patches(np.full((150, 170, 3), 255, np.uint8), 64, 48)["n_selected"] == 0


def test_argument_errors_come_before_the_library_is_loaded(monkeypatch):
    def no_load(*a, **k):
        raise AssertionError("the library or the device was touched")
    monkeypatch.setattr(_lib, "load", no_load)
    monkeypatch.setattr(tissue, "_device", no_load)
    img = np.zeros((8, 9, 3), np.uint8)
    for call in (tissue.histogram, tissue.mask, tissue.select_patches):
        for bad in (img.astype(np.float32), img.astype(np.int32), torch.zeros(8, 9, 3), [[1, 2, 3]], None):
            with pytest.raises(TypeError):
                call(bad)
        for bad in (np.zeros((8, 9), np.uint8), np.zeros((8, 9, 4), np.uint8), np.zeros((0, 9, 3), np.uint8), np.zeros((1, 2, 8, 9, 3), np.uint8)):
            with pytest.raises(ValueError):
                call(bad)
    for call in (tissue.histogram, tissue.mask):
        for bad in ("luma", "Chroma", 0, None):
            with pytest.raises(ValueError):
                call(img, channel=bad)
    for bad in (256, -2, 1.5, True, "3", [1, 2], [300], np.asarray([1.0])):
        with pytest.raises(ValueError):
            tissue.mask(img, bad)
    with pytest.raises(ValueError):
        tissue.mask(np.zeros((2, 8, 9, 3), np.uint8), [1, 2, 3])
    with pytest.raises(ValueError):
        tissue.select_patches(np.zeros((2, 8, 9, 3), np.uint8), 4)          # one slide at a time
    with pytest.raises(ValueError):
        tissue.select_patches(img, 16)                                      # a patch larger than the image
    for bad in (0, -3, (4, 0), "x"):
        with pytest.raises(ValueError):
            tissue.select_patches(img, bad)
    for bad in (object(), "chroma", 5, {"channel": "chroma"}, False):
        with pytest.raises(TypeError):
            tissue.select_patches(img, 4, options=bad)
    m = np.zeros((8, 9), np.uint8)
    for bad in (m.astype(np.float32), m.astype(np.int32), None):
        with pytest.raises(TypeError):
            tissue.coverage(bad, [0], [(0, 0)], 4)
    for bad in (np.zeros((9,), np.uint8), np.zeros((0, 9), np.uint8), np.zeros((1, 1, 8, 9), np.uint8)):
        with pytest.raises(ValueError):
            tissue.coverage(bad, [0], [(0, 0)], 4)
    for ti, rc, size in (([0], [(5, 0)], 4), ([0], [(0, 6)], 4), ([0], [(-1, 0)], 4), ([1], [(0, 0)], 4), ([-1], [(0, 0)], 4), ([0, 0], [(0, 0)], 4),
                         ([0], [(0, 0)], 0), ([0], [(0, 0)], (4, -1)), ([0], [(0, 0)], (9, 4)), ([0], [(1, 0)], (8, 9))):
        with pytest.raises(ValueError):
            tissue.coverage(m, ti, rc, size)
    with pytest.raises(TypeError):
        tissue.coverage(m, [0.0], [(0, 0)], 4)
    with pytest.raises(TypeError):
        tissue.coverage(m, [0], np.zeros((1, 2), np.float32), 4)
    # the raw bindings refuse host tensors of the wrong type or shape before they load anything either
    with pytest.raises(TypeError):
        kernels.tissue_histogram(torch.zeros(1, 8, 9, 3))
    with pytest.raises(TypeError):
        kernels.tissue_mask(torch.zeros(8, 9, 3, dtype=torch.uint8), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError):
        kernels.tissue_mask(torch.zeros(1, 8, 9, 3, dtype=torch.uint8), torch.zeros(2, dtype=torch.int32))
    with pytest.raises(TypeError):
        kernels.tissue_coverage(torch.zeros(8, 9, dtype=torch.uint8), torch.zeros(1, dtype=torch.int32), torch.zeros(1, 2, dtype=torch.int32), 4, 4)
    with pytest.raises(TypeError):
        kernels.tissue_select(torch.zeros(4, dtype=torch.int64), 1)


def test_tissue_options():
    o = tissue.TissueOptions()
    assert (o.channel, o.threshold, o.min_fraction, o.min_pixels, o.min_object_size, o.hole_area_threshold, o.opening_radius) == \
        ("chroma", None, 0.01, None, 0, 0, 0)
    assert o.pixels(64, 64) == 41 and o.pixels(299, 299) == 895 and tissue.TissueOptions(min_fraction=0).pixels(64, 64) == 0
    assert tissue.TissueOptions(min_fraction=1).pixels(7, 9) == 63 and tissue.TissueOptions(min_fraction=0.5).pixels(3, 3) == 5
    assert tissue.TissueOptions(min_pixels=7, min_fraction=0.9).pixels(64, 64) == 7            # min_pixels overrides the fraction
    assert tissue.TissueOptions(min_pixels=0).pixels(64, 64) == 0
    assert tissue.TissueOptions(channel="darkness", threshold=np.int64(30), opening_radius=1.5, min_object_size=10).threshold == 30
    for kw in (dict(channel="luma"), dict(channel=1), dict(threshold=256), dict(threshold=-2), dict(threshold=1.5), dict(threshold=True),
               dict(min_fraction=-0.1), dict(min_fraction=1.01), dict(min_fraction="1"), dict(min_fraction=True), dict(min_fraction=float("nan")),
               dict(min_pixels=-1), dict(min_pixels=1.5), dict(min_pixels=True), dict(min_pixels=1 << 31), dict(min_object_size=-1),
               dict(min_object_size=1.5), dict(hole_area_threshold=-2), dict(opening_radius=-1), dict(opening_radius=float("inf"))):
        with pytest.raises(ValueError):
            tissue.TissueOptions(**kw)
    with pytest.raises(TypeError):
        tissue.TissueOptions(opening_radius="2")
    with pytest.raises(Exception):
        o.channel = "darkness"                                              # frozen, as checked


def test_detect_slide_checks_tissue_before_the_model(monkeypatch):
    def no_load(*a, **k):
        raise AssertionError("the library or the device was touched")
    monkeypatch.setattr(_lib, "load", no_load)
    img = np.zeros((80, 80, 3), np.uint8)

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError(f"the model was touched: {name}")

    for bad in (object(), "chroma", 1, False, {"min_pixels": 3}):
        with pytest.raises(TypeError, match="tissue"):
            inference.detect_slide(img, Untouchable(), patch_size=64, interval=48, tissue=bad)
        with pytest.raises(TypeError, match="tissue"):
            list(inference.detect_slides([img], Untouchable(), patch_size=64, interval=48, tissue=bad))
    # the result record: four positional fields keep working, the new one trails
    r = inference.SlideResult(np.zeros((0, 2), np.int64), [], 0, torch.zeros(2, 2, dtype=torch.uint8))
    assert r.tissue is None and [f for f in r.__dataclass_fields__] == ["points", "discarded", "cell_count", "mask", "tissue"]
    t = tissue.TissueResult(3, torch.zeros(2, 2, dtype=torch.uint8), np.asarray([(0, 0), (0, 4), (4, 0)], np.int32), torch.zeros(3, dtype=torch.int32),
                            torch.tensor([0, 2], dtype=torch.int32), 2)
    assert t.selected_corners.tolist() == [[0, 0], [4, 0]] and t.selected_corners.dtype == np.int32


def test_new_symbols_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "cellseg_hip.h")).read()
    names = ("cs_tissue_histogram", "cs_tissue_mask", "cs_tissue_coverage", "cs_tissue_select")
    for name in names:
        assert re.search(rf"^int {name}\(", header, re.M), name
        assert name in _lib._SIGNATURES and name in _lib.exported_symbols()
    assert re.search(r"^#define CS_TISSUE_CHROMA 0$", header, re.M) and re.search(r"^#define CS_TISSUE_DARKNESS 1$", header, re.M)
    assert (kernels.CS_TISSUE_CHROMA, kernels.CS_TISSUE_DARKNESS) == (0, 1) and tissue.CHANNELS == {"chroma": 0, "darkness": 1}
    assert [len(_lib._SIGNATURES[n][1]) for n in names] == [7, 8, 11, 6]
    assert _lib._SIGNATURES["cs_tissue_coverage"][1][6] is _lib.c_longlong and _lib._SIGNATURES["cs_tissue_select"][1][1] is _lib.c_longlong
    lib = _lib.load()
    for name in names:
        assert hasattr(lib, name)
    src = open(os.path.join(ROOT, "cellsegmentation_amd", "csrc", "tissue.hip")).read()
    code = re.sub(r"//.*", "", src)
    assert "asm" not in code and "float" not in code and "double" not in code, "plain integer C++ only"
    assert "block_reduce<" in code and "block_rank<" in code
    assert "tissue.hip" in open(os.path.join(ROOT, "cellsegmentation_amd", "csrc", "Makefile")).read()


def test_entry_points_refuse_bad_calls_without_a_gpu():
    lib = _lib.load()
    buf = (ctypes.c_int64 * 64)()                                          # host memory: nothing is launched
    base = ctypes.addressof(buf)
    base += -base % 16
    P = ctypes.c_void_p

    def hist(img=base, N=1, H=4, W=4, ch=0, out=base):
        return lib.cs_tissue_histogram(P(img), N, H, W, ch, P(out), None)

    def mask(img=base, N=1, H=4, W=4, ch=0, thr=base, out=base):
        return lib.cs_tissue_mask(P(img), N, H, W, ch, P(thr), P(out), None)

    def cover(m=base, N=1, H=4, W=4, ti=base, rc=base, T=1, ph=2, pw=2, out=base):
        return lib.cs_tissue_coverage(P(m), N, H, W, P(ti), P(rc), T, ph, pw, P(out), None)

    def select(c=base, T=1, need=0, sel=base, n=base):
        return lib.cs_tissue_select(P(c), T, need, P(sel), P(n), None)

    for what, fn, cases in (
        ("tissue_histogram", hist, (dict(N=0), dict(N=65536), dict(H=0), dict(W=-1), dict(H=46341, W=46341), dict(ch=2), dict(ch=-1), dict(img=None),
                                    dict(out=None), dict(out=base + 4))),
        ("tissue_mask", mask, (dict(N=0), dict(N=65536), dict(H=0), dict(W=0), dict(H=65536, W=32768), dict(ch=2), dict(img=None), dict(thr=None),
                               dict(out=None), dict(thr=base + 2))),
        ("tissue_coverage", cover, (dict(N=0), dict(H=0), dict(W=0), dict(H=65536, W=32768), dict(T=-1), dict(T=1 << 31), dict(ph=0), dict(pw=-1),
                                    dict(m=None), dict(ti=None), dict(rc=None), dict(out=None), dict(ti=base + 2), dict(rc=base + 1),
                                    dict(out=base + 3))),
        ("tissue_select", select, (dict(T=-1), dict(T=1 << 31), dict(c=None), dict(sel=None), dict(n=None), dict(n=None, T=0), dict(c=base + 2),
                                   dict(sel=base + 1), dict(n=base + 3))),
    ):
        for kw in cases:
            assert fn(**kw) == -1, (what, kw)
            assert what.encode() in lib.cs_last_error(), (what, kw, lib.cs_last_error())
    assert b"unknown channel" in (hist(ch=7), lib.cs_last_error())[1]
    assert b"NULL" in (mask(thr=None), lib.cs_last_error())[1]
    assert b"misaligned" in (cover(rc=base + 1), lib.cs_last_error())[1]
