"""CPU: the numpy restatement of the rendering rules (tests/render_ref.py) against its pinned vectors
(tests/golden/make_render_golden.py), the two identities the fills rest on (the mask fill is the reference's float expression stored
into uint8; the heat blend is the mean rounded half to even), the colour table, the raster rule of the marks, the argument errors of
cellsegmentation_amd.render, which are raised before the library is loaded, and the ABI additions with their refusals (no GPU
needed)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import render_ref as R
from cellsegmentation_amd import _lib, detect, inference, kernels, render

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "render_vectors.npz"), allow_pickle=False)
COMPOSE = [str(n) for n in GOLD["compose_names"]]
POINTS = [str(n) for n in GOLD["points_names"]]


def test_golden_holds_the_pinned_cases():
    assert len(COMPOSE) == 16 and len(POINTS) == 13
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "render_vectors.npz")) < 256 * 1024
    shapes = {tuple(GOLD[f"{n}.images"].shape[:3]) for n in COMPOSE}
    assert shapes >= {(1, 41, 1), (1, 1, 41), (1, 5, 7), (1, 37, 53), (2, 9, 13)}
    assert {tuple(GOLD[f"{n}.canvas"].shape[:3]) for n in POINTS} == {(1, 16, 20), (2, 33, 29), (3, 9, 11)}
    for v in (0, 1, 254, 255):
        assert (GOLD["heat_u8_37x53_inverted.images"] == v).any()
    assert not GOLD["mask_1x41_all0.mask"].any() and GOLD["mask_5x7_all1.mask"].all()
    assert set(np.unique(GOLD["heat_u8_batch2_5x7_0_and_255.heat"])) == {0, 255}
    p = GOLD["heat_f32_5x7_thr_0.heat"][0, 0]
    assert p[0] == 1 and R.heat_level(p[1], 0.0) == 0 and R.heat_level(p[2], 0.0) == 1 and R.heat_level(p[0], 0.0) == 255
    q = GOLD["heat_f32_batch2_9x13_thr_half.heat"][0, 0]
    assert q[0] == 0.5 and R.heat_level(q[0], 0.5) == 0 and R.heat_level(q[1], 0.5) == 127
    lab = GOLD["outline_37x53.labels"]
    assert lab.min() < 0 and lab.max() == 300 and (lab == 3).sum() == 1 and len(GOLD["outline_37x53_palette_over_heat.palette"]) == 3


@pytest.mark.parametrize("name", COMPOSE)
def test_restatement_reproduces_the_compose_vectors(name):
    kw, want = R.golden_case(GOLD, name, R.COMPOSE_KEYS)
    assert np.array_equal(R.compose(GOLD[f"{name}.images"], **kw), want)


@pytest.mark.parametrize("name", POINTS)
def test_restatement_reproduces_the_points_vectors(name):
    kw, want = R.golden_case(GOLD, name, R.POINTS_KEYS)
    assert np.array_equal(R.draw_points(GOLD[f"{name}.canvas"], GOLD[f"{name}.points"], **kw), want)


def test_mask_fill_is_the_reference_expression_stored_into_uint8():
    """utils/image_processing.py:25: img[:, :, i] = img[:, :, i] * 0.5 + np.uint8(255 * img_bin) * 0.5, for all 256 x 2 inputs"""
    c = np.arange(256, dtype=np.uint8)
    for on in (False, True):
        stored = c.copy()
        stored[:] = c * 0.5 + np.uint8(255 * np.full(256, on)) * 0.5
        assert stored.dtype == np.uint8 and [R.mask_fill(int(v), int(on)) for v in c] == stored.tolist()
        assert stored.tolist() == [(int(v) + 255 * on) >> 1 for v in c]


def test_heat_blend_is_the_mean_rounded_half_to_even():
    """cv2.addWeighted(a, .5, b, .5, 0) saturates rint(a * .5 + b * .5): against np.rint for all 256^2 pairs"""
    a, b = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    want = np.rint(a * .5 + b * .5).astype(np.int64)
    s = a + b
    assert np.array_equal((s >> 1) + ((s & 1) & ((s >> 1) & 1)), want)
    assert all(R.heat_blend(int(x), int(y)) == want[x, y] for x, y in ((0, 1), (1, 0), (1, 2), (254, 255), (255, 255), (0, 0), (255, 0), (2, 3)))
    assert [R.heat_blend(0, 1), R.heat_blend(1, 2), R.heat_blend(254, 255), R.heat_blend(255, 0)] == [0, 2, 254, 128]


def test_jet_is_its_formula():
    t = render.jet()
    assert isinstance(t, np.ndarray) and t.dtype == np.uint8 and t.shape == (256, 3) and np.array_equal(t, R.jet())
    for v in range(256):
        assert t[v].tolist() == [min(max(382 - abs(4 * v - 255 * k), 0), 255) for k in (3, 2, 1)]
    assert t[[0, 64, 128, 191, 255]].tolist() == [[0, 0, 127], [0, 128, 255], [129, 255, 125], [255, 128, 0], [127, 0, 0]]
    assert np.array_equal(t[:, ::-1][:, 0], t[:, 2])                       # the reference's BGR-into-RGB look is a column flip


def test_disc_and_ring_pixels():
    def marks(radius, thickness):
        c = R.draw_points(np.zeros((1, 41, 41, 3), np.uint8), [(20, 20)], radius=radius, thickness=thickness, color=(1, 1, 1))[0, :, :, 0]
        return {(r - 20, q - 20) for r, q in zip(*np.nonzero(c))}
    assert [len(marks(r, -1)) for r in (0, 1, 2, 4)] == [1, 5, 13, 49]
    ring = marks(4, 2)
    assert ring == {(dr, dc) for dr in range(-9, 10) for dc in range(-9, 10) if 9 <= dr * dr + dc * dc <= 25}
    assert marks(4, 8) == {(dr, dc) for dr in range(-9, 10) for dc in range(-9, 10) if dr * dr + dc * dc <= 64}    # t = 2r: out to r + t/2
    assert marks(4, 1) == {(dr, dc) for dr in range(-9, 10) for dc in range(-9, 10) if 49 <= 4 * (dr * dr + dc * dc) <= 81}


def test_argument_errors_come_before_the_library_is_loaded(monkeypatch):
    def no_load(*a, **k):
        raise AssertionError("the library or the device was touched")
    monkeypatch.setattr(_lib, "load", no_load)
    monkeypatch.setattr(render, "_device", no_load)
    img = np.zeros((8, 9, 3), np.uint8)
    m = np.zeros((8, 9), np.uint8)
    # images: dtype and shape, for every entry point that takes some
    calls = (render.compose, lambda x: render.overlap_mask(x, m.astype(bool)), lambda x: render.save_images_with_masks(x, m.astype(np.float32), .5),
             lambda x: render.dotting(x, [(1, 2)]), lambda x: render.locate_cells(x, [(1, 2)]))
    for call in calls:
        for bad in (img.astype(np.float32), img.astype(np.int32), torch.zeros(8, 9, 3), None):
            with pytest.raises(TypeError):
                call(bad)
        for bad in (np.zeros((8, 9), np.uint8), np.zeros((8, 9, 4), np.uint8), np.zeros((0, 9, 3), np.uint8), np.zeros((1, 2, 8, 9, 3), np.uint8)):
            with pytest.raises(ValueError):
                call(bad)
    with pytest.raises(ValueError):
        render.compose(torch.zeros((2, 1 << 15, 1 << 15, 3), dtype=torch.uint8, device="meta"))      # N H W = 2^31
    # the fills
    with pytest.raises(ValueError, match="at most one"):
        render.compose(img, mask=m, heat=m)
    for bad in (m.astype(np.float32), m.astype(np.int32), [[0]], "m"):
        with pytest.raises(TypeError):
            render.compose(img, mask=bad)
    for bad in (m.astype(np.float64), m.astype(bool), m.astype(np.int32)):
        with pytest.raises(TypeError):
            render.compose(img, heat=bad)
    for bad in (np.zeros((9, 8), np.uint8), np.zeros((1, 1, 8, 9), np.uint8), np.zeros((2, 8, 9), np.uint8), np.zeros((8,), np.uint8)):
        with pytest.raises(ValueError):
            render.compose(img, mask=bad)
        with pytest.raises(ValueError):
            render.compose(img, heat=bad)
    with pytest.raises(ValueError):
        render.compose(np.zeros((2, 8, 9, 3), np.uint8), mask=m)           # a batch takes [N, H, W]
    with pytest.raises(ValueError, match="threshold"):
        render.compose(img, heat=m.astype(np.float32))                     # float heat without its threshold
    for bad in ("0.5", True, float("nan"), [0.5]):
        with pytest.raises(ValueError, match="threshold"):
            render.compose(img, heat=m.astype(np.float32), threshold=bad)
    with pytest.raises(ValueError, match="threshold"):
        render.compose(img, heat=m, threshold=0.5)
    with pytest.raises(ValueError, match="threshold"):
        render.compose(img, mask=m, threshold=0.5)
    # the tables
    for bad in (np.zeros((255, 3), np.uint8), np.zeros((256, 4), np.uint8), np.zeros((256,), np.uint8)):
        with pytest.raises(ValueError):
            render.compose(img, heat=m, colormap=bad)
    for bad in (np.zeros((256, 3), np.int32), render.jet().tolist()):
        with pytest.raises(TypeError):
            render.compose(img, heat=m, colormap=bad)
    with pytest.raises(ValueError, match="colormap"):
        render.compose(img, mask=m, colormap=render.jet())
    lab = np.zeros((8, 9), np.int32)
    for rows in (0, 257):
        with pytest.raises(ValueError, match="palette"):
            render.compose(img, outlines=lab, palette=np.zeros((rows, 3), np.uint8))
    with pytest.raises(ValueError, match="palette"):
        render.compose(img, outlines=lab, palette=np.zeros((4, 4), np.uint8))
    with pytest.raises(TypeError):
        render.compose(img, outlines=lab, palette=np.zeros((4, 3), np.int64))
    with pytest.raises(ValueError, match="palette"):
        render.compose(img, palette=np.zeros((4, 3), np.uint8))            # a palette without outlines
    # the outlines
    for bad in (lab.astype(np.int64), lab.astype(np.uint8), lab.astype(np.float32)):
        with pytest.raises(TypeError):
            render.compose(img, outlines=bad)
    with pytest.raises(ValueError):
        render.compose(img, outlines=np.zeros((9, 8), np.int32))
    for bad in (0, 3, "1"):
        with pytest.raises(ValueError, match="connectivity"):
            render.compose(img, outlines=lab.astype(bool), connectivity=bad)
    for bad in ((255, 255), (256, 0, 0), (-1, 0, 0), (1.5, 0, 0), "red", 7):
        with pytest.raises(ValueError, match="outline_color"):
            render.compose(img, outlines=lab, outline_color=bad)
    for bad in (np.zeros((8, 9, 3), np.uint8), torch.zeros(8, 9, 3, dtype=torch.uint8), torch.zeros(1, 8, 9, 3, dtype=torch.uint8, device="meta")):
        with pytest.raises(ValueError, match="out"):
            render.compose(img, out=bad)
    # the marks
    canvas = torch.zeros(16, 20, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="device"):
        render.draw_points(canvas, [(1, 2)])                               # everything else is fine: a host canvas
    for bad in (canvas.numpy(), canvas.float(), None):
        with pytest.raises(TypeError):
            render.draw_points(bad, [(1, 2)])
    for bad in (torch.zeros(16, 20, dtype=torch.uint8), torch.zeros(16, 20, 4, dtype=torch.uint8), torch.zeros(0, 20, 3, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            render.draw_points(bad, [(1, 2)])
    for kw in (dict(radius=65), dict(radius=-1), dict(radius=4, thickness=9), dict(radius=4, thickness=0), dict(radius=0, thickness=1)):
        with pytest.raises(ValueError):
            render.draw_points(canvas, [(1, 2)], **kw)
        with pytest.raises(ValueError):
            render.dotting(img, [(1, 2)], **kw)
    for kw in (dict(radius=2.0), dict(radius=True), dict(thickness=1.0), dict(radius="4")):
        with pytest.raises(TypeError):
            render.draw_points(canvas, [(1, 2)], **kw)
    for bad in ((255, 0), (0, 0, 300), None):
        with pytest.raises(ValueError, match="color"):
            render.draw_points(canvas, [(1, 2)], color=bad)
    with pytest.raises(ValueError):
        render.draw_points(canvas, np.zeros((3, 3), np.int64))
    with pytest.raises(TypeError):
        render.draw_points(canvas, np.zeros((3, 2), np.float32))
    with pytest.raises(ValueError):
        render.draw_points(canvas, np.zeros((3, 2), np.int64), offsets=[0, 2])              # offsets must end at the number of points
    with pytest.raises(ValueError):
        render.draw_points(torch.zeros(2, 16, 20, 3, dtype=torch.uint8), np.zeros((3, 2), np.int64))     # two images need offsets
    with pytest.raises(ValueError):
        render.draw_points(torch.zeros(2, 16, 20, 3, dtype=torch.uint8), [np.zeros((3, 2), np.int64)])
    with pytest.raises(ValueError, match="limits"):
        render.draw_points(canvas, [(1, 2)], limits=[1, 2])
    with pytest.raises(TypeError):
        render.draw_points(canvas, [(1, 2)], limits=1.5)
    with pytest.raises(ValueError, match="tail"):
        render.draw_points(canvas, [(1, 2)], tail=True)
    # the front ends
    with pytest.raises(TypeError):
        render.overlap_mask(img, m)                                        # a boolean mask, as remove_small_regions takes
    with pytest.raises(ValueError):
        render.overlap_mask(img, np.zeros((9, 8), bool))
    with pytest.raises(ValueError):
        render.overlap_mask(img, m.astype(bool), min_object_size=-1)
    with pytest.raises(TypeError):
        render.save_images_with_masks(img, m, 0.5)
    with pytest.raises(ValueError):
        render.save_images_with_masks(img, m.astype(np.float32), None)
    with pytest.raises(ValueError):
        render.save_images_with_masks([img, img], [m.astype(np.float32)], 0.5)
    with pytest.raises(ValueError):
        render.locate_cells(np.zeros((2, 8, 9, 3), np.uint8), [(1, 2)])
    with pytest.raises(ValueError):
        render.locate_cells(img, [(1, 2, 3)])
    res = detect.DetectResult(np.zeros((3, 2), np.int64), np.zeros(3), np.asarray([0, 2, 3]), np.asarray([2, 1]), cell_counts=np.asarray([1, 1]))
    with pytest.raises(ValueError, match="2 maps"):
        res.render(img)
    with pytest.raises(ValueError, match="at most one"):
        res.render(np.zeros((2, 8, 9, 3), np.uint8), mask=np.zeros((2, 8, 9), np.uint8), heat=np.zeros((2, 8, 9), np.uint8))
    slide = inference.SlideResult(np.zeros((0, 2), np.int64), [], 0, torch.zeros(8, 9, dtype=torch.uint8))
    with pytest.raises(TypeError):
        inference.render_slide(img, object())
    for kw in (dict(fill="soft"), dict(fill=1), dict(thr_u8=256), dict(thr_u8=1.5)):
        with pytest.raises(ValueError):
            inference.render_slide(img, slide, **kw)
    for kw in (dict(mask=m), dict(heat=m), dict(threshold=0.5)):
        with pytest.raises(TypeError):
            inference.render_slide(img, slide, **kw)
    with pytest.raises(ValueError):
        inference.render_slide(np.zeros((9, 8, 3), np.uint8), slide)
    with pytest.raises(ValueError):
        inference.render_slide(np.zeros((1, 8, 9, 3), np.uint8), slide)
    with pytest.raises(ValueError, match="palette"):
        inference.render_slide(img, slide, palette=np.zeros((3, 3), np.uint8))
    # the raw bindings refuse host tensors of the wrong type or shape before they load anything either
    t = torch.zeros(1, 8, 9, 3, dtype=torch.uint8)
    with pytest.raises(TypeError):
        kernels.render_compose(torch.zeros(8, 9, 3, dtype=torch.uint8))
    with pytest.raises(TypeError):
        kernels.render_compose(t, kernels.CS_RENDER_FILL_MASK, torch.zeros(1, 8, 9))
    with pytest.raises(ValueError):
        kernels.render_compose(t, kernels.CS_RENDER_FILL_MASK)
    with pytest.raises(ValueError):
        kernels.render_compose(t, 4, torch.zeros(1, 8, 9, dtype=torch.uint8))
    with pytest.raises(TypeError):
        kernels.render_compose(t, kernels.CS_RENDER_FILL_HEAT_U8, torch.zeros(1, 8, 9, dtype=torch.uint8))       # no colour table
    with pytest.raises(ValueError):
        kernels.render_compose(t, labels=torch.zeros(1, 8, 9, dtype=torch.int32), palette=torch.zeros(0, 3, dtype=torch.uint8))
    with pytest.raises(TypeError):
        kernels.render_points(torch.zeros(8, 9, 3, dtype=torch.uint8), None, None)
    with pytest.raises(ValueError):
        kernels.render_points(t, None, None, radius=65)
    with pytest.raises(ValueError):
        kernels.render_points(t, None, None, radius=4, thickness=9)
    with pytest.raises(ValueError):
        kernels.render_points(t, torch.zeros(1, 2, dtype=torch.int64), torch.zeros(2, dtype=torch.int64))        # a host canvas


def test_new_symbols_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "cellseg_hip.h")).read()
    names = ("cs_render_compose", "cs_render_points")
    for name in names:
        assert re.search(rf"^int {name}\(", header, re.M), name
        assert name in _lib._SIGNATURES and name in _lib.exported_symbols() and f" * {name}" in header
    for k, name in enumerate(("NONE", "MASK", "HEAT_U8", "HEAT_F32")):
        assert re.search(rf"^#define CS_RENDER_FILL_{name} {k}$", header, re.M) and getattr(kernels, f"CS_RENDER_FILL_{name}") == k
    assert re.search(r"^#define CS_RENDER_POINTS_XY 1$", header, re.M) and re.search(r"^#define CS_RENDER_POINTS_TAIL 2$", header, re.M)
    assert (kernels.CS_RENDER_POINTS_XY, kernels.CS_RENDER_POINTS_TAIL, kernels.RENDER_MAX_RADIUS, render.MAX_RADIUS) == (1, 2, 64, 64)
    assert [len(_lib._SIGNATURES[n][1]) for n in names] == [15, 13]
    assert _lib._SIGNATURES["cs_render_compose"][1][6] is _lib.c_float and _lib._SIGNATURES["cs_render_points"][1][7] is _lib.c_longlong
    # the argument lists of the header, type by type, against the ctypes table
    kinds = {"int": _lib.c_int, "float": _lib.c_float, "long long": _lib.c_longlong}
    for name in names:
        args = re.search(rf"^int {name}\((.*?)\);", header, re.M | re.S).group(1).split(",")
        want = [_lib._P if "*" in a else kinds[" ".join(a.split()[:-1])] for a in args]
        assert want == _lib._SIGNATURES[name][1], name
    lib = _lib.load()
    for name in names:
        assert hasattr(lib, name)
    assert lib.cs_abi_version() == 10
    src = open(os.path.join(ROOT, "cellsegmentation_amd", "csrc", "render.hip")).read()
    code = re.sub(r"//.*", "", src)
    assert "asm" not in code and "atomic" not in code and "double" not in code, "plain C++ with plain loads and stores only"
    assert code.count("__global__") == 2 and "template <int FILL>" in code and "__shared__" in code     # one body per kernel, tables in LDS
    assert "hipMalloc" not in code and "Synchronize" not in code
    assert "render.hip" in open(os.path.join(ROOT, "cellsegmentation_amd", "csrc", "Makefile")).read()


def test_entry_points_refuse_bad_calls_without_a_gpu():
    lib = _lib.load()
    buf = (ctypes.c_int64 * 64)()                                          # host memory: nothing is launched
    base = ctypes.addressof(buf)
    base += -base % 16
    P = ctypes.c_void_p

    def compose(img=base, N=1, H=4, W=4, fill=0, fmap=None, thr=0.0, invert=1, cmap=None, lab=None, rgb=0xffff, pal=None, rows=0, out=base):
        return lib.cs_render_compose(P(img), N, H, W, fill, P(fmap), thr, invert, P(cmap), P(lab), rgb, P(pal), rows, P(out), None)

    def points(canvas=base, N=1, H=4, W=4, pts=base, off=base, lim=None, n=1, radius=4, t=-1, rgb=255, flags=0):
        return lib.cs_render_points(P(canvas), N, H, W, P(pts), P(off), P(lim), n, radius, t, rgb, flags, None)

    for what, fn, cases in (
        ("render_compose", compose, (dict(N=0), dict(N=65536), dict(H=0), dict(W=-1), dict(N=2, H=32768, W=32768), dict(img=None), dict(out=None),
                                     dict(fill=4), dict(fill=-1), dict(fill=1), dict(fill=0, fmap=base), dict(fill=2, fmap=base),
                                     dict(fill=3, fmap=base + 2, cmap=base), dict(lab=base + 2), dict(rows=3), dict(pal=base), dict(pal=base, rows=257),
                                     dict(pal=base, rows=2), dict(rgb=-1), dict(rgb=1 << 24))),
        ("render_points", points, (dict(N=0), dict(N=65536), dict(H=0), dict(W=0), dict(N=2, H=32768, W=32768), dict(n=-1), dict(n=1 << 31),
                                   dict(radius=-1), dict(radius=65), dict(t=0), dict(t=9), dict(radius=0, t=1), dict(rgb=-1), dict(rgb=1 << 24),
                                   dict(flags=4), dict(flags=-1), dict(flags=2), dict(canvas=None), dict(off=None), dict(pts=None),
                                   dict(pts=base + 4), dict(off=base + 4), dict(lim=base + 2))),
    ):
        for kw in cases:
            assert fn(**kw) == -1, (what, kw)
            assert what.encode() in lib.cs_last_error(), (what, kw, lib.cs_last_error())
    assert b"unknown fill" in (compose(fill=9), lib.cs_last_error())[1]
    assert b"misaligned" in (points(off=base + 4), lib.cs_last_error())[1]
    assert b"tail" in (points(flags=2), lib.cs_last_error())[1]
    assert points(n=0, pts=None) == 0                                      # no points: nothing is launched
