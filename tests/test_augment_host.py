"""CPU: the numpy restatement of the augmented staging (tests/augment_ref.py) against hand-computed known answers,
augment.draw_color_jitter, the argument errors of cellsegmentation_amd.augment (raised before any device work) and the ABI
additions.  Parity of the restatement with torchvision itself is not pinned (torchvision is not a dependency)."""
import itertools
import os
import re

import numpy as np
import pytest
import torch

import augment_ref as R
from cellsegmentation_amd import _lib, augment, kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def px(*rgb):
    return np.asarray(rgb, F).reshape(1, 1, 3)


# ---------------------------------------------------------------- the restatement: known answers
def test_grey_pixels_pass_through_hue_unchanged():
    x = np.asarray([[[0.0] * 3, [0.25] * 3, [1.0] * 3, [100 / 255] * 3]], F)
    for f in (-0.5, -0.05, 0.0, 0.3, 0.5):
        assert R.hue(x, f).tobytes() == x.tobytes()


def test_pure_colours_rotate_by_thirds():
    red, green, blue = px(1, 0, 0), px(0, 1, 0), px(0, 0, 1)
    assert np.array_equal(R.hue(red, 1 / 3), green)                       # h = 0 -> 1/3
    assert np.allclose(R.hue(green, 1 / 3), blue, rtol=0, atol=1e-6)      # 1/3 + fp32(1/3) is not 2/3 exactly
    assert np.array_equal(R.hue(red, 0.0), red) and np.allclose(R.hue(blue, 0.0), blue, rtol=0, atol=1e-6)   # fp32(4 / 6) * 6 > 4
    assert np.array_equal(R.hue(red, 0.5), px(0, 1, 1))                   # the complement
    assert np.array_equal(R.hue(red, -0.5), px(0, 1, 1))
    assert np.array_equal(R.hue(px(0.5, 0, 0), 1 / 3), px(0, 0.5, 0))     # the value is kept


def test_blend_ops_at_their_ends():
    rng = np.random.RandomState(0)
    x = rng.rand(4, 5, 3).astype(F)
    g = R.gray(x)
    assert g.dtype == F and np.allclose(g, 0.2989 * x[..., 0] + 0.587 * x[..., 1] + 0.114 * x[..., 2], atol=1e-6)
    assert R.gray(px(1, 1, 1))[0, 0] == F(F(F(0.2989) + F(0.587)) + F(0.114))
    assert np.array_equal(R.jitter(x, [R.BRIGHTNESS, -1, -1, -1], [0, 0, 0, 0]), np.zeros_like(x))            # brightness 0: black
    assert np.array_equal(R.jitter(x, [R.BRIGHTNESS, -1, -1, -1], [1, 0, 0, 0]), x)
    assert np.array_equal(R.jitter(x, [-1, R.BRIGHTNESS, -1, -1], [0, 2, 0, 0]), np.minimum(F(2) * x, F(1)))  # clamped at 1
    assert np.array_equal(R.jitter(x, [R.SATURATION, -1, -1, -1], [0, 0, 0, 0]), np.repeat(g[..., None], 3, -1))  # saturation 0: gray
    assert np.array_equal(R.jitter(x, [R.SATURATION, -1, -1, -1], [1, 0, 0, 0]), x)
    m = R.tile_mean(x)
    assert m.dtype == F and abs(float(m) - float(g.astype(np.float64).mean())) < 1e-7
    assert np.array_equal(R.jitter(x, [R.CONTRAST, -1, -1, -1], [0, 0, 0, 0]), np.full_like(x, m))            # contrast 0: the mean
    assert np.array_equal(R.jitter(x, [R.CONTRAST, -1, -1, -1], [1, 0, 0, 0]), x)
    # the mean is taken on the tile as the ops in front of the contrast op left it
    dark = R.jitter(x, [R.BRIGHTNESS, R.CONTRAST, -1, -1], [0.5, 0, 0, 0])
    assert np.array_equal(dark, np.full_like(x, R.tile_mean(F(0.5) * x)))
    assert np.array_equal(R.jitter(x, [-1, -1, -1, -1], [9, 9, 9, 9]), x)
    # a hand-computed mean: grey levels 0.25 and 0.75 on two pixels
    two = np.asarray([[[0.25] * 3, [0.75] * 3]], F)
    assert float(R.tile_mean(two)) == pytest.approx(0.5 * (0.2989 + 0.587 + 0.114), abs=1e-7)


def test_the_four_flips_of_a_2x3_tile():
    t = np.arange(6).reshape(2, 3)
    assert R.flip(t, 0).tolist() == [[0, 1, 2], [3, 4, 5]]
    assert R.flip(t, 1).tolist() == [[2, 1, 0], [5, 4, 3]]               # horizontal
    assert R.flip(t, 2).tolist() == [[3, 4, 5], [0, 1, 2]]               # vertical
    assert R.flip(t, 3).tolist() == [[5, 4, 3], [2, 1, 0]]
    assert (augment.FLIP_NONE, augment.FLIP_H, augment.FLIP_V, augment.FLIP_HV) == (0, 1, 2, 3)
    img = np.arange(2 * 4 * 5 * 3, dtype=np.uint8).reshape(2, 4, 5, 3)
    out = R.stage_tiles(img, [1, 1, 1, 1], [(1, 2)] * 4, 2, 3, flips=[0, 1, 2, 3])
    assert out.shape == (4, 2, 3, 8) and out.dtype == F and not out[..., 3:].any()
    want = R.normalise(img[1, 1:3, 2:5].astype(F) / F(255))
    for code in range(4):
        assert np.array_equal(out[code, :, :, :3], R.flip(want, code))
    assert want[0, 0, 0] == (F(img[1, 1, 2, 0]) / F(255) - F(0.485)) / F(0.229)
    whole = R.stage_images(img, idx=[1, 0])
    assert whole.shape == (2, 4, 5, 8) and np.array_equal(whole[0, 1:3, 2:5, :3], want)


def test_bf16_rounding_helper():
    x = np.asarray([1.0, 1.00390625, 1.01171875, -2.5, 0.0, 3.0e-5], F)     # 1 + 2^-8 is a tie: to even (down); 1 + 3 * 2^-8: up
    assert R.to_bf16_bits(x).tolist() == torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16).tolist()


# ---------------------------------------------------------------- draw_color_jitter
def test_draw_color_jitter_orders_and_ranges():
    g = torch.Generator().manual_seed(5)
    order, factors = augment.draw_color_jitter(200, generator=g)
    assert order.dtype == np.int8 and factors.dtype == F and order.shape == factors.shape == (200, 4)
    assert all(sorted(row) == [0, 1, 2, 3] for row in order.tolist())
    assert len({tuple(r) for r in order.tolist()}) > 12                   # the orders do vary
    for op, lo, hi in ((0, 0.9, 1.1), (1, 0.7, 1.3), (2, 0.6, 1.4), (3, -0.05, 0.05)):
        f = factors[order == op]
        assert len(f) == 200 and f.min() >= F(lo) and f.max() <= F(hi) and f.max() - f.min() > 0.5 * (hi - lo)
    # a seeded generator reproduces the result
    again = augment.draw_color_jitter(200, generator=torch.Generator().manual_seed(5))
    assert np.array_equal(order, again[0]) and factors.tobytes() == again[1].tobytes()
    other = augment.draw_color_jitter(200, generator=torch.Generator().manual_seed(6))
    assert factors.tobytes() != other[1].tobytes()
    # large parameters: the lower end stops at 0
    _, f = augment.draw_color_jitter(50, brightness=3.0, contrast=0, saturation=0, hue=0.5, generator=g)
    assert f.min() >= -0.5 and f.max() <= 4.0
    assert augment.draw_color_jitter(0)[0].shape == (0, 4)


def test_disabled_ops_get_minus_one_and_consume_no_draw():
    for off in itertools.chain(itertools.combinations(("brightness", "contrast", "saturation", "hue"), 1),
                               itertools.combinations(("brightness", "contrast", "saturation", "hue"), 2),
                               itertools.combinations(("brightness", "contrast", "saturation", "hue"), 3)):
        names = ("brightness", "contrast", "saturation", "hue")
        kw = {n: (None if i % 2 else 0) for i, n in enumerate(off)}
        g = torch.Generator().manual_seed(11)
        order, factors = augment.draw_color_jitter(7, generator=g, **kw)
        enabled = sorted(i for i, n in enumerate(names) if n not in off)
        for row, frow in zip(order.tolist(), factors.tolist()):
            assert sorted(c for c in row if c >= 0) == enabled and row.count(-1) == len(off)
            assert all(f == 0 for c, f in zip(row, frow) if c < 0)
        # the draws made: per record one randperm(4) and one uniform per ENABLED op, nothing else
        h = torch.Generator().manual_seed(11)
        lo_hi = {0: (0.9, 1.1), 1: (0.7, 1.3), 2: (0.6, 1.4), 3: (-0.05, 0.05)}
        for row, frow in zip(order.tolist(), factors.tolist()):
            perm = torch.randperm(4, generator=h).tolist()
            drawn = {op: float(torch.empty(1).uniform_(*lo_hi[op], generator=h)) for op in enabled}
            assert row == [op if op in drawn else -1 for op in perm]
            assert frow == [float(F(drawn[op])) if op in drawn else 0.0 for op in perm]
        assert torch.equal(g.get_state(), h.get_state())
    for bad in ({"brightness": -0.1}, {"hue": 0.6}, {"contrast": float("nan")}, {"saturation": "1"}):
        with pytest.raises(ValueError):
            augment.draw_color_jitter(1, **bad)
    with pytest.raises(ValueError):
        augment.draw_color_jitter(-1)


# ---------------------------------------------------------------- argument errors, before any device work
def test_argument_errors_come_before_any_device_work(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("device work was started")
    monkeypatch.setattr(_lib, "load", no_device)
    monkeypatch.setattr(kernels, "stage_augmented", no_device)
    img = torch.zeros(2, 8, 10, 3, dtype=torch.uint8)
    ti, rc = [0, 1, 1], [(0, 0), (4, 6), (2, 3)]
    ok_j = (np.asarray([[0, 1, 2, 3]] * 3), np.ones((3, 4), F) * 0.25)
    # dtype and shape of the images
    for bad in (img.float(), img.to(torch.int8), np.zeros((2, 8, 10, 3), np.uint8)):
        with pytest.raises(TypeError):
            augment.stage_tiles(bad, ti, rc, 4)
        with pytest.raises(TypeError):
            augment.stage_images(bad)
    for bad in (img[0], img[..., :2], torch.zeros(2, 3, 8, 10, dtype=torch.uint8), torch.zeros(0, 8, 10, 3, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            augment.stage_tiles(bad, ti, rc, 4)
        with pytest.raises(ValueError):
            augment.stage_images(bad)
    with pytest.raises(TypeError):
        augment.stage_tiles(img, ti, rc, 4, dtype=torch.float16)
    # flip codes outside 0..3, of the wrong type, of the wrong count
    for bad in ([0, 1, 4], [0, -1, 2]):
        with pytest.raises(ValueError, match="flip code"):
            augment.stage_tiles(img, ti, rc, 4, flips=bad)
    with pytest.raises(TypeError):
        augment.stage_tiles(img, ti, rc, 4, flips=[0.0, 1.0, 2.0])
    for bad in ([0, 1], [0, 1, 2, 3], [[0, 1, 2]]):
        with pytest.raises(ValueError):
            augment.stage_tiles(img, ti, rc, 4, flips=bad)
    with pytest.raises(ValueError):
        augment.stage_images(img, flips=[0, 1, 2])
    # op codes: repeated within a record, outside -1..3
    for row in ([0, 0, 1, 2], [3, 1, 2, 3], [-1, 2, 2, -1]):
        with pytest.raises(ValueError, match="repeated"):
            augment.stage_tiles(img, ti, rc, 4, jitter=(np.asarray([[0, 1, 2, 3], row, [0, 1, 2, 3]]), ok_j[1]))
    for code in (4, -2, 100):
        with pytest.raises(ValueError, match="op code"):
            augment.stage_tiles(img, ti, rc, 4, jitter=(np.asarray([[0, 1, 2, code]] * 3), ok_j[1]))
    with pytest.raises(TypeError):
        augment.stage_tiles(img, ti, rc, 4, jitter=(ok_j[0].astype(F), ok_j[1]))
    with pytest.raises(TypeError):
        augment.stage_tiles(img, ti, rc, 4, jitter=(ok_j[0], ok_j[0]))
    with pytest.raises(TypeError):
        augment.stage_tiles(img, ti, rc, 4, jitter=ok_j[0])
    # factors: not finite, negative blend factors, hue outside [-0.5, 0.5]
    for slot, value, what in ((0, float("nan"), "finite"), (1, float("inf"), "finite"), (0, -0.1, "negative"), (1, -1e-3, "negative"),
                              (2, -2.0, "negative"), (3, 0.51, "hue"), (3, -0.75, "hue")):
        f = ok_j[1].copy()
        f[1, slot] = value
        with pytest.raises(ValueError, match=what):
            augment.stage_tiles(img, ti, rc, 4, jitter=(ok_j[0], f))
    f = ok_j[1].copy()
    f[:, 3] = -0.5                                                        # the ends of the ranges are inside: a host image passes
    f[:, 0] = 0.0                                                         # every check and is refused for not being on the GPU
    with pytest.raises(RuntimeError, match="GPU"):
        augment.stage_tiles(img, ti, rc, 4, flips=[0, 1, 2], jitter=(ok_j[0], f))
    # row counts that do not match T
    for bad in ((ok_j[0][:2], ok_j[1][:2]), (ok_j[0], ok_j[1][:2]), (ok_j[0][:, :3], ok_j[1][:, :3]), (ok_j[0].ravel(), ok_j[1].ravel())):
        with pytest.raises(ValueError):
            augment.stage_tiles(img, ti, rc, 4, jitter=bad)
    with pytest.raises(ValueError):
        augment.stage_images(img, jitter=ok_j)                            # 3 records, 2 images
    with pytest.raises(ValueError):
        augment.stage_tiles(img, ti, rc[:2], 4)
    with pytest.raises(ValueError):
        augment.stage_tiles(img, [], np.zeros((0, 2), np.int64), 4)
    # tiles that leave the image, images that do not exist
    for bad in ([(0, 0), (5, 6), (2, 3)], [(0, 0), (4, 7), (2, 3)], [(-1, 0), (4, 6), (2, 3)]):
        with pytest.raises(ValueError, match="leaves"):
            augment.stage_tiles(img, ti, bad, 4)
    for size in (9, 0, -4):
        with pytest.raises(ValueError):
            augment.stage_tiles(img, ti, [(0, 0)] * 3, size)
    for bad in ([0, 1, 2], [0, -1, 1]):
        with pytest.raises(ValueError, match="image index"):
            augment.stage_tiles(img, bad, rc, 4)
    with pytest.raises(ValueError, match="image index"):
        augment.stage_images(img, idx=[0, 2])
    with pytest.raises(TypeError):
        augment.stage_tiles(img, [0.0, 1.0, 1.0], rc, 4)
    # the iterables
    rows = np.asarray([(0, 0, 0, 1), (1, 4, 6, 0)])
    with pytest.raises(ValueError):
        augment.TileTrainBatches(img, rows, [0, 1], 4, 0)
    with pytest.raises(ValueError):
        augment.TileTrainBatches(img, rows, [0, 1, 2], 4, 2)              # one code per image
    with pytest.raises(ValueError):
        augment.TileTrainBatches(img, rows, [0, 5], 4, 2)
    with pytest.raises(ValueError):
        augment.TileTrainBatches(img, np.asarray([(2, 0, 0, 1)]), None, 4, 2)
    with pytest.raises(ValueError):
        augment.MaskTrainBatches(img, torch.zeros(3, 8, 10), torch.zeros(2), 2)
    with pytest.raises(TypeError):
        augment.MaskTrainBatches(img, np.zeros((2, 8, 10)), torch.zeros(2), 2)
    with pytest.raises(TypeError):
        augment.MaskTrainBatches(img, torch.zeros(2, 8, 10), torch.zeros(2), 2, dtype=torch.float64)
    # the raw binding refuses wrong dtypes and shapes before it loads anything
    t32 = torch.zeros(3, dtype=torch.int32)
    monkeypatch.undo()
    monkeypatch.setattr(_lib, "load", no_device)
    for kw in ({"flips": torch.zeros(3, dtype=torch.int32)}, {"ops": torch.zeros(3, 4, dtype=torch.int8)},
               {"ops": torch.zeros(3, 4, dtype=torch.int32), "factors": torch.zeros(3, 4)},
               {"ops": torch.zeros(3, 4, dtype=torch.int8), "factors": torch.zeros(3, 3)}):
        with pytest.raises(TypeError):
            kernels.stage_augmented(img, t32, torch.zeros(3, 2, dtype=torch.int32), 4, 4, **kw)
    with pytest.raises(TypeError):
        kernels.stage_augmented(img, t32.long(), torch.zeros(3, 2, dtype=torch.int32), 4, 4)
    with pytest.raises(ValueError):
        kernels.stage_augmented(img, t32, torch.zeros(3, 2, dtype=torch.int32), 4, 4, has_contrast=True)


# ---------------------------------------------------------------- the ABI additions
def test_new_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "cellseg_hip.h")).read()
    for name in ("cs_stage_augmented_workspace", "cs_stage_augmented"):
        assert re.search(rf"^(size_t|int) {name}\(", header, re.M), name
        assert name in _lib._SIGNATURES and name in _lib.exported_symbols()
    assert len(_lib._SIGNATURES["cs_stage_augmented"][1]) == 20 and _lib._SIGNATURES["cs_stage_augmented_workspace"][0] is _lib.c_size_t
    lib = _lib.load()
    assert hasattr(lib, "cs_stage_augmented") and hasattr(lib, "cs_stage_augmented_workspace")
    assert lib.cs_abi_version() == 10
    assert lib.cs_stage_augmented_workspace(0) == 0 and lib.cs_stage_augmented_workspace(-3) == 0
    assert lib.cs_stage_augmented_workspace(1 << 31) == 0
    assert lib.cs_stage_augmented_workspace(1) == 7 * 8 and lib.cs_stage_augmented_workspace(1000) == 6001 * 8


def test_entry_point_refuses_bad_arguments_without_a_gpu():
    """NULLs, extents, a tile larger than the image, the 2^31 limits, a bad dtype and a missing or small workspace are refused before
    any launch; the pointers are never dereferenced on the host, so dummies do."""
    lib = _lib.load()
    m = (_lib.c_float * 3)(0.485, 0.456, 0.406)
    s = (_lib.c_float * 3)(0.229, 0.224, 0.225)
    P = 4096                                                              # a non-NULL, aligned dummy

    def call(images=P, n=2, H=8, W=10, ti=P, rc=P, flips=None, ops=None, fac=None, contrast=0, T=3, th=4, tw=4, mean=m, std=s, dtype=0,
             out=P, ws=None, ws_bytes=0):
        return lib.cs_stage_augmented(images, n, H, W, ti, rc, flips, ops, fac, contrast, T, th, tw, mean, std, dtype, out, ws, ws_bytes, None)

    bad = [dict(images=None), dict(ti=None), dict(rc=None), dict(out=None), dict(mean=None), dict(std=None),
           dict(n=0), dict(H=0), dict(W=-1), dict(T=0), dict(T=-5), dict(th=0), dict(tw=0),
           dict(th=9), dict(tw=11),                                      # th <= H, tw <= W
           dict(T=1 << 31), dict(H=1 << 16, W=1 << 16, th=1 << 16, tw=1 << 15),
           dict(dtype=2), dict(dtype=-1),
           dict(ops=P), dict(fac=P),                                      # one without the other
           dict(ops=P + 2, fac=P), dict(ops=P, fac=P + 4), dict(out=P + 8),
           dict(contrast=1), dict(contrast=2, ops=P, fac=P, ws=P, ws_bytes=1 << 20),
           dict(contrast=1, ops=P, fac=P), dict(contrast=1, ops=P, fac=P, ws=P, ws_bytes=19 * 8 - 1),
           dict(contrast=1, ops=P, fac=P, ws=P + 4, ws_bytes=1 << 20),
           dict(contrast=1, ops=P, fac=P, ws=P, ws_bytes=1 << 40, T=(1 << 31) - 1, H=1 << 10, W=1 << 10, th=1 << 10, tw=1 << 10)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert lib.cs_last_error().startswith(b"stage_augmented"), kw
    assert b"workspace too small" in (call(contrast=1, ops=P, fac=P, ws=P, ws_bytes=8) and lib.cs_last_error())
    assert b"bad extents" in (call(th=9) and lib.cs_last_error())
    assert b"NULL" in (call(images=None) and lib.cs_last_error())
