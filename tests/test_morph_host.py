"""CPU: the numpy restatement tests/morph_ref.py against the brute-force definition and against the scipy vectors
tests/golden/morph_vectors.npz; the argument errors of cellsegmentation_amd.morph, raised before any device work; the C ABI's own
argument checks."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import morph_ref as MR  # noqa: E402
from cellsegmentation_amd import _lib  # noqa: E402
from cellsegmentation_amd import morph as M  # noqa: E402

GOLD = np.load(os.path.join(ROOT, "tests", "golden", "morph_vectors.npz"), allow_pickle=False)
MASK_NAMES = sorted(k[len("mask/"):-len(".mask")] for k in GOLD.files if k.startswith("mask/") and k.endswith(".mask"))
LABEL_NAMES = sorted(k[len("labels/"):-len(".labels")] for k in GOLD.files if k.endswith(".labels"))
R2S = (0, 1, 2, 4, 5, 13, 25, 56)


def gold_mask(name):
    H, W = GOLD[f"mask/{name}.shape"]
    return np.unpackbits(GOLD[f"mask/{name}.mask"], axis=1)[:, :W].astype(bool)


def gold_bits(key, W):
    return np.unpackbits(GOLD[key], axis=1)[:, :W].astype(bool)


def test_golden_file_holds_what_the_tests_expect():
    assert len(MASK_NAMES) >= 4 and len(LABEL_NAMES) == 4
    assert sorted(int(GOLD[f"labels/{n}.r2"]) for n in LABEL_NAMES) == [6, 9, 25, 64]
    for name in MASK_NAMES:
        for op in ("dilation", "erosion", "opening", "closing"):
            for r2 in R2S:
                for bv in (0, 1):
                    assert f"mask/{name}.{op}.{r2}.{bv}" in GOLD.files


@pytest.mark.parametrize("density", [0.02, 0.1, 0.3, 0.6, 0.95])
def test_separable_scheme_equals_the_definition(density):
    rng = np.random.RandomState(int(density * 100))
    for trial in range(60):
        H, W = rng.randint(1, 15), rng.randint(1, 15)
        sites = rng.rand(H, W) < density
        d2, site = MR.nearest(sites)
        bd2, bsite = MR.nearest_brute(sites)
        assert np.array_equal(d2, bd2) and np.array_equal(site, bsite), (H, W, trial)


def test_single_site_and_no_site_maps():
    for H, W in ((1, 1), (1, 9), (9, 1), (7, 13), (14, 14)):
        none = np.zeros((H, W), bool)
        d2, site = MR.nearest(none)
        assert (d2 == -1).all() and (site == -1).all()
        assert np.array_equal(MR.nearest_brute(none)[0], d2)
        for y0, x0 in ((0, 0), (H - 1, W - 1), (H // 2, W // 3), (0, W - 1)):
            one = none.copy()
            one[y0, x0] = True
            d2, site = MR.nearest(one)
            yy, xx = np.mgrid[0:H, 0:W]
            assert np.array_equal(d2, (yy - y0) ** 2 + (xx - x0) ** 2) and (site == y0 * W + x0).all()
            bd2, bsite = MR.nearest_brute(one)
            assert np.array_equal(d2, bd2) and np.array_equal(site, bsite)


def test_pythagorean_tie_goes_to_the_lowest_row_major_site():
    # from the centre, (0, +5) and (+3, +4) are both at 25: the site on the centre's own row has the lower index, and a search that
    # stops at d * d >= best never reaches it
    sites = np.zeros((21, 21), bool)
    sites[10, 15] = sites[13, 14] = True
    for fn in (MR.nearest, MR.nearest_brute):
        d2, site = fn(sites)
        assert d2[10, 10] == 25 and site[10, 10] == 10 * 21 + 15


def test_offset_search_equals_the_key_matrix(monkeypatch):
    rng = np.random.RandomState(4)
    for density in (0.01, 0.2, 0.7):
        sites = rng.rand(23, 61) < density
        sites[5, 7] = True
        want = MR.nearest(sites)
        monkeypatch.setattr(MR, "KEY_MATRIX_MAX_W", 8)
        got = MR.nearest(sites)
        monkeypatch.undo()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("name", MASK_NAMES)
def test_reference_equals_scipy_masks(name):
    m = gold_mask(name)
    W = m.shape[1]
    assert np.array_equal(MR.nearest(m)[0], GOLD[f"mask/{name}.d2_true"])
    assert np.array_equal(MR.nearest(~m)[0], GOLD[f"mask/{name}.d2_false"])
    for op in ("dilation", "erosion", "opening", "closing"):
        fn = getattr(MR, f"binary_{op}")
        for r2 in R2S:
            for bv in (0, 1):
                assert np.array_equal(fn(m, r2, bv), gold_bits(f"mask/{name}.{op}.{r2}.{bv}", W)), (op, r2, bv)
    for bv in (0, 1):
        assert np.array_equal(MR.binary_dilation(m, 0, bv), m) and np.array_equal(MR.binary_erosion(m, 0, bv), m)


@pytest.mark.parametrize("name", LABEL_NAMES)
def test_reference_equals_scipy_labels(name):
    labels = GOLD[f"labels/{name}.labels"]
    W = labels.shape[1]
    r2 = int(GOLD[f"labels/{name}.r2"])
    filled, ambiguous = gold_bits(f"labels/{name}.filled", W), gold_bits(f"labels/{name}.ambiguous", W)
    assert ambiguous.sum() <= 0.03 * filled.sum() and not (ambiguous & ~filled).any()
    got = MR.expand_labels(labels, r2)
    assert np.array_equal(got[labels != 0], labels[labels != 0])
    assert np.array_equal((got != 0) & (labels == 0), filled)
    sure = filled & ~ambiguous
    assert np.array_equal(got[sure], GOLD[f"labels/{name}.under"][sure])
    # every ambiguous pixel still takes one of the labels in reach
    assert (got[ambiguous] > 0).all()


def test_disk_is_the_structuring_element():
    assert MR.disk(0).shape == (1, 1) and MR.disk(1).sum() == 5 and MR.disk(2).sum() == 9 and MR.disk(2).shape == (3, 3)
    assert MR.disk(13).shape == (7, 7) and MR.disk(56).shape == (15, 15) and MR.disk(25).sum() == 81


# ---- argument errors: no device is touched ------------------------------------------------------------------------------------------
BINARY = (M.binary_dilation, M.binary_erosion, M.binary_opening, M.binary_closing)


def huge(dtype, shape):
    return torch.empty((1,), dtype=dtype).as_strided(shape, (0,) * len(shape))          # one element of storage, any shape


def test_non_boolean_masks_are_refused():
    for fn in BINARY:
        for bad in (np.zeros((4, 4), np.uint8), np.zeros((4, 4), np.int32), torch.zeros((2, 4, 4), dtype=torch.float32)):
            with pytest.raises(TypeError, match="boolean mask"):
                fn(bad, 1)
        with pytest.raises(ValueError):
            fn(np.zeros((4,), bool), 1)
        with pytest.raises(ValueError):
            fn(np.zeros((0, 4), bool), 1)
    with pytest.raises(TypeError, match="boolean mask"):
        M.nearest_sites(np.zeros((4, 4), np.uint8))
    with pytest.raises(TypeError, match="int32 label image"):
        M.expand_labels(np.zeros((4, 4), bool), 2)
    with pytest.raises(TypeError, match="int32 label image"):
        M.expand_labels(np.zeros((4, 4), np.int64), 2)
    with pytest.raises(ValueError, match="background"):
        M.nearest_sites(np.zeros((4, 4), np.int32), background=True)


def test_radius_arguments():
    m = np.zeros((4, 4), bool)
    lab = np.zeros((4, 4), np.int32)
    for fn, x, key in [(fn, m, "radius") for fn in BINARY] + [(M.expand_labels, lab, "distance")]:
        with pytest.raises(ValueError, match="non-negative"):
            fn(x, -1)
        with pytest.raises(ValueError, match="radius_sq"):
            fn(x, radius_sq=-1)
        with pytest.raises(ValueError, match="either"):
            fn(x, 2, radius_sq=4)
        with pytest.raises(ValueError, match="either"):
            fn(x, **{key: 2, "radius_sq": 4})
        with pytest.raises(ValueError, match="either"):
            fn(x)
        for bad in (2.0, True, "2"):
            with pytest.raises(TypeError):
                fn(x, radius_sq=bad)
        with pytest.raises(TypeError):
            fn(x, "2")
        with pytest.raises(ValueError):
            fn(x, float("nan"))
        with pytest.raises(ValueError):
            fn(x, radius_sq=1 << 31)
    assert M._r2("x", 3.7, None) == 13 and M._r2("x", None, 13) == 13 and M._r2("x", 0, None) == 0
    assert M._r2("x", 13 ** 0.5, None) == 12                                 # the float square of sqrt(13) rounds down: radius_sq=13


def test_border_value_is_0_or_1():
    m = np.zeros((4, 4), bool)
    for fn in BINARY:
        for bad in (2, -1, True, None, 0.5):
            with pytest.raises(ValueError, match="border_value"):
                fn(m, 1, border_value=bad)


def test_shape_limits_are_checked_on_the_host():
    for fn in BINARY:
        with pytest.raises(ValueError, match=r"H\^2 \+ W\^2 < 2\^31"):
            fn(huge(torch.bool, (46341, 1)), 1)
        with pytest.raises(ValueError, match=r"H\^2 \+ W\^2 < 2\^31"):
            fn(huge(torch.bool, (2, 32768, 32768)), 1)
    with pytest.raises(ValueError, match=r"H\^2 \+ W\^2 < 2\^31"):
        M.nearest_sites(huge(torch.bool, (1, 46341)))
    with pytest.raises(ValueError, match=r"H\^2 \+ W\^2 < 2\^31"):
        M.expand_labels(huge(torch.int32, (40000, 40000)), 2)
    # the wide-row limit of the calls that carry a site
    assert M.MAX_SITE_WIDTH == 40960 == _lib.load().cs_morph_max_site_width()
    with pytest.raises(ValueError, match="wider than 40960"):
        M.nearest_sites(huge(torch.bool, (3, 40961)))
    with pytest.raises(ValueError, match="wider than 40960"):
        M.expand_labels(huge(torch.int32, (2, 3, 40961)), 2)


def test_pipeline_option_is_checked_before_the_model_runs():
    from cellsegmentation_amd import inference as I
    for bad in (-1, float("nan")):
        with pytest.raises(ValueError, match="opening_radius"):
            I.segment_classes([], None, None, 0.5, opening_radius=bad)
        with pytest.raises(ValueError, match="opening_radius"):
            I.measure_cells([], None, None, 0.5, opening_radius=bad)
        with pytest.raises(ValueError, match="opening_radius"):
            I.measure_slide(np.zeros((4, 4), np.uint8), opening_radius=bad)
    with pytest.raises(TypeError, match="opening_radius"):
        I.segment_classes([], None, None, 0.5, opening_radius="2")


def test_c_abi_argument_checks():
    lib = _lib.load()
    assert lib.cs_morph_workspace(1, 46341, 1) == 0 and lib.cs_morph_workspace(0, 4, 4) == 0 and lib.cs_morph_workspace(65536, 4, 4) == 0
    assert lib.cs_morph_workspace(3, 5, 7) == 16 + 432 and lib.cs_morph_workspace(1, 46340, 1) == 16 + 185360
    assert lib.cs_morph_workspace(1, 32767, 32767) > 0
    assert lib.cs_morph_nearest(None, 0, 0, 1, 4, 4, None, None, None, 0, None) == -1 and b"morph_nearest: NULL" in lib.cs_last_error()
    assert lib.cs_morph_binary(None, 1, 4, 4, 0, 1, 0, None, None, 0, None) == -1 and b"morph_binary: NULL" in lib.cs_last_error()
    assert lib.cs_morph_expand_labels(None, 1, 4, 4, 1, None, None, 0, None) == -1 and b"morph_expand_labels: NULL" in lib.cs_last_error()
    import ctypes
    buf = ctypes.create_string_buffer(4096)
    base = ctypes.addressof(buf)
    base += -base % 16
    p, q, w = ctypes.c_void_p(base), ctypes.c_void_p(base + 1024), ctypes.c_void_p(base + 2048)
    odd = ctypes.c_void_p(base + 2050)
    assert lib.cs_morph_binary(p, 1, 4, 4, 0, -1, 0, q, w, 1024, None) == -1 and b"r2" in lib.cs_last_error()
    assert lib.cs_morph_binary(p, 1, 4, 4, 0, 1, 0, q, w, 16, None) == -1 and b"workspace too small" in lib.cs_last_error()
    assert lib.cs_morph_binary(p, 1, 4, 4, 0, 1, 0, q, odd, 1024, None) == -1 and b"misaligned" in lib.cs_last_error()
    assert lib.cs_morph_binary(p, 1, 46341, 1, 0, 1, 0, q, w, 1024, None) == -1 and b"H^2 + W^2" in lib.cs_last_error()
    assert lib.cs_morph_nearest(p, 1, 1, 1, 4, 4, q, None, w, 1024, None) == -1 and b"background" in lib.cs_last_error()
    assert lib.cs_morph_nearest(p, 0, 0, 1, 1, 40961, q, None, w, 1 << 20, None) == -1 and b"40960" in lib.cs_last_error()
    assert lib.cs_morph_nearest(p, 0, 0, 1, 4, 4, odd, None, w, 1024, None) == -1 and b"misaligned" in lib.cs_last_error()
    assert lib.cs_morph_expand_labels(p, 1, 4, 4, 1, p, w, 1024, None) == -1 and b"must not be the input" in lib.cs_last_error()
    assert lib.cs_morph_expand_labels(p, 1, 1, 40961, 1, q, w, 1 << 20, None) == -1 and b"40960" in lib.cs_last_error()
    assert lib.cs_morph_expand_labels(p, 1, 4, 4, -1, q, w, 1024, None) == -1 and b"r2" in lib.cs_last_error()
