"""Whole-slide streaming, host side: tiles.sample_patches against the reference's own corner lists (tests/golden/slide_vectors.npz,
written by tests/golden/make_slide_golden.py), the argument errors of detect.stitch_logits and inference.detect_slide with host
tensors, and the C ABI of the new entry point.  No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from cellsegmentation_amd import _lib
from cellsegmentation_amd import detect as D
from cellsegmentation_amd import inference as I
from cellsegmentation_amd import tiles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "slide_vectors.npz")


def test_sample_patches_equals_the_reference_on_every_golden_case():
    z = np.load(GOLDEN)
    meta = z["meta"]
    assert len(meta) >= 36 and {int(m[0]) for m in meta} == {0, 1}          # both modes
    assert any(m[3] != m[4] for m in meta) and any(m[5] > m[3] for m in meta)  # non-square patches, an interval larger than the patch
    for i, (_, s0, s1, p0, p1, i0, i1) in enumerate(meta.tolist()):
        got = tiles.sample_patches((s0, s1), (p0, p1), (i0, i1))
        want = z[f"case{i}/corners"]
        assert isinstance(got, list) and np.array_equal(np.asarray(got, dtype=np.int64).reshape(-1, 2), want), (i, s0, s1, p0, p1, i0, i1)
        assert want[-1].tolist() == [s0 - p0, s1 - p1]                       # the last patch is aligned to both borders


def test_sample_patches_known_answers():
    grid = tiles.sample_patches((4096, 4096))                               # 299 / 283: 14 regular origins and a border-aligned one per axis
    assert len(grid) == 225 and grid[0] == (0, 0) and grid[1] == (0, 283) and grid[15] == (283, 0) and grid[-1] == (3797, 3797)
    assert grid == tiles.sample_patches((4096, 4096), 299, 283) == tiles.sample_patches((4096, 4096, 3), (299, 299), np.array([283, 283]))
    assert tiles.sample_patches((150, 170), 64, 48) == [(r, c) for r in (0, 48, 86) for c in (0, 48, 96, 106)]
    assert tiles.sample_patches((299, 299)) == [(0, 0)]
    # each axis has its own size and interval, and the product is x outer, y inner: the get_tiles origins of either axis
    got = tiles.sample_patches((101, 131), (37, 53), (21, 37))
    assert got == [(x, y) for x in tiles._axis_origins(101, 21, 37) for y in tiles._axis_origins(131, 37, 53)]
    assert tiles.sample_patches((97, 89), 16, 16) == tiles.get_tiles((97, 89), 16, 16)


@pytest.mark.parametrize("size,patch,interval", [((298, 400), 299, None), ((400, 298), 299, None), ((10, 10), (4, 11), (2, 2)),
                                                 ((64, 64), 16, 0), ((64, 64), 16, (4, -1)), ((64, 64), 16, None), ((64, 64), 0, 4),
                                                 ((64, 64), (16, 16, 16), 4)])
def test_sample_patches_errors(size, patch, interval):
    with pytest.raises(ValueError):                                         # the reference dies with IndexError on an empty list
        tiles.sample_patches(size, patch, interval)


def test_stitch_logits_argument_errors_before_any_device_work():
    """Host tensors throughout: every check runs before a device is needed; the device check comes last."""
    mask = torch.zeros((40, 50), dtype=torch.uint8)
    logits = torch.zeros((2, 2, 16, 20), dtype=torch.float32)
    ok = [(0, 0), (24, 30)]
    with pytest.raises(TypeError):
        D.stitch_logits(mask, logits.double(), ok)
    with pytest.raises(TypeError):
        D.stitch_logits(mask, logits.numpy(), ok)
    with pytest.raises(ValueError, match=r"\[B, C, ph, pw\]"):
        D.stitch_logits(mask, logits[0], ok)
    with pytest.raises(TypeError):
        D.stitch_logits(mask.float(), logits, ok)
    with pytest.raises(ValueError, match=r"\[H, W\]"):
        D.stitch_logits(mask[None], logits, ok)
    with pytest.raises(ValueError, match="2 patches but 1 corners"):
        D.stitch_logits(mask, logits, ok[:1])
    for bad in ([(0, 0), (25, 30)], [(0, 0), (24, 31)], [(-1, 0), (24, 30)], [(0, -1), (24, 30)]):
        with pytest.raises(ValueError, match="a patch does not lie inside the image"):
            D.stitch_logits(mask, logits, bad)
    for ch in (-1, 2, 0.5):
        with pytest.raises(ValueError, match="channel"):
            D.stitch_logits(mask, logits, ok, ch=ch)
    with pytest.raises(ValueError, match="two channels"):
        D.stitch_logits(mask, logits[:, :1], ok, ch=0)
    with pytest.raises(ValueError, match="device tensor"):                  # everything else is right: only now the device matters
        D.stitch_logits(mask, logits, ok)
    with pytest.raises(ValueError, match="device tensor"):
        D.stitch_logits(mask, logits, torch.tensor(ok), ch=0)
    assert int(mask.sum()) == 0


class _NoModel:
    """detect_slide must refuse its arguments before it touches the model."""

    def __getattr__(self, name):
        raise AssertionError(f"the model was touched ({name}) before the arguments were checked")


def test_detect_slide_argument_errors_before_any_device_work():
    img = np.zeros((150, 170, 3), np.uint8)
    with pytest.raises(ValueError, match="square"):
        I.detect_slide(img, _NoModel(), patch_size=(64, 48))
    with pytest.raises(TypeError, match="unexpected arguments"):
        I.detect_slide(img, _NoModel(), patch_size=64, sigma=3.)
    with pytest.raises(ValueError, match="Smoothing method"):
        I.detect_slide(img, _NoModel(), patch_size=64, method="median")
    with pytest.raises(ValueError):
        I.detect_slide(img, _NoModel(), patch_size=64, ksize=(14, 15))
    with pytest.raises(ValueError):
        I.detect_slide(img, _NoModel(), patch_size=64, batch_size=0)
    with pytest.raises(ValueError):                                         # the patch is larger than the slide
        I.detect_slide(img, _NoModel(), patch_size=299)
    with pytest.raises(TypeError):
        I.detect_slide(img.astype(np.float32), _NoModel(), patch_size=64)
    with pytest.raises(TypeError):
        I.detect_slide(img[..., 0], _NoModel(), patch_size=64)
    with pytest.raises(TypeError):
        I.detect_slide(torch.zeros((3, 150, 170), dtype=torch.uint8), _NoModel(), patch_size=64)
    gen = I.detect_slides([img], _NoModel(), patch_size=(64, 48))           # a generator: nothing runs until it is asked for a slide
    with pytest.raises(ValueError, match="square"):
        next(gen)


def test_header_ctypes_and_library_agree_on_stitch_logits():
    header = open(os.path.join(ROOT, "include", "cellseg_hip.h")).read()
    m = re.search(r"\bint\s+cs_stitch_logits\s*\(([^)]*)\)\s*;", header)
    assert m, "cs_stitch_logits is not declared in include/cellseg_hip.h"
    params = [p.strip() for p in m.group(1).split(",")]
    restype, argtypes = _lib._SIGNATURES["cs_stitch_logits"]
    assert restype is ctypes.c_int and len(argtypes) == len(params) == 11
    for p, t in zip(params, argtypes):                                      # every pointer is a void pointer in the table, every int an int
        assert (t is ctypes.c_void_p) == ("*" in p), p
        assert (t is ctypes.c_int) == (p.startswith("int ")), p
    assert "cs_stitch_logits_workspace" not in header                       # no workspace: ownership needs the corners alone
    lib = _lib.load()
    assert hasattr(lib, "cs_stitch_logits") and lib.cs_abi_version() == 10
    # argument checks come before any launch, so they answer without a GPU
    buf = ctypes.create_string_buffer(64)
    ptr = ctypes.c_void_p(ctypes.addressof(buf))
    call = lib.cs_stitch_logits
    assert call(ptr, 1, 1, 4, 4, 0, ptr, 8, 8, ptr, None) == -1 and b"two channels" in lib.cs_last_error()
    assert call(ptr, 1, 2, 4, 4, 2, ptr, 8, 8, ptr, None) == -1 and b"two channels" in lib.cs_last_error()
    assert call(ptr, 1, 2, 4, 4, 1, ptr, 8, 8, None, None) == -1 and b"bad arguments" in lib.cs_last_error()
    assert call(None, 1, 2, 4, 4, 1, ptr, 8, 8, ptr, None) == -1 and b"NULL" in lib.cs_last_error()
    assert call(ptr, 1, 2, 9, 4, 1, ptr, 8, 8, ptr, None) == -1 and b"fit the mask" in lib.cs_last_error()
    assert call(ptr, 1, 2, 4, 4, 1, ptr, 8, 1 << 29, ptr, None) == -1 and b"2^29" in lib.cs_last_error()
    assert call(None, 0, 2, 4, 4, 1, None, 8, 8, ptr, None) == 0           # an empty batch is no work, not an error
