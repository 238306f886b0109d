"""The pixel-run walker of csrc/cs_pixels.h through every kernel that uses it, at every one of the 16 places the first byte of an image
can have past a 16-byte boundary and on the degenerate spans: one image of 1 x count pixels, count chosen so that the head is the
whole image (no run), there is exactly one run with an empty or a non-empty head and tail, or there are two runs.  The mask, the map
and the outputs lie (5 shift + 3) % 16 bytes past a boundary (4-byte types at the multiple of 4 that gives), so the 16-byte, dword
and byte accesses all occur.  Every view lies inside a padded buffer, outputs are prefilled, and the padding must stay untouched."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import render_ref as RR  # noqa: E402
import stain_ref as SR  # noqa: E402
import tissue_ref as TR  # noqa: E402
from shifted import guards_intact, shifted  # noqa: E402
from cellsegmentation_amd import kernels as K  # noqa: E402
from cellsegmentation_amd import render, stain  # noqa: E402

pytestmark = pytest.mark.gpu

COUNTS = (1, 5, 15, 16, 17, 31, 32, 47)
OPTS = stain.StainOptions()
MAX_OD = np.log(256.0)


def _side(shift, item=1):
    s = (5 * shift + 3) % 16
    return s if item == 1 else 4 * (s % 4)


def _inputs(count):
    """-> images uint8 [1, 1, count, 3], a mask with values other than 0 and 1, a heat map, labels with background and negative ids"""
    rng = np.random.RandomState(100 + count)
    images = rng.randint(0, 256, size=(1, 1, count, 3)).astype(np.uint8)
    mask = (rng.randint(0, 3, size=(1, 1, count)) * 100).astype(np.uint8)
    heat = rng.randint(0, 256, size=(1, 1, count)).astype(np.uint8)
    labels = (rng.randint(0, 4, size=(1, 1, (count + 1) // 2)) - 1).repeat(2, axis=2)[:, :, :count].astype(np.int32)
    return images, mask, heat, np.ascontiguousarray(labels)


def test_the_sizes_and_shifts_cover_every_head_and_access():
    heads = {(11 * (-s % 16)) % 16 for s in range(16)}
    assert heads == set(range(16))                                         # every head length occurs
    assert {_side(s) % 16 == 0 for s in range(16)} == {True, False} and {_side(s) % 4 for s in range(16)} == {0, 1, 2, 3}
    assert {_side(s, 4) for s in range(16)} == {0, 4, 8, 12}
    spans = set()
    for count in COUNTS:
        for head in heads:
            h = min(head, count)
            runs = (count - h) // 16
            spans.add((runs, h > 0, count - h - 16 * runs > 0))
    assert {(0, True, False), (1, False, False), (1, True, False), (1, False, True), (1, True, True), (2, False, True)} <= spans


@pytest.mark.parametrize("count", COUNTS)
def test_tissue_histogram_and_mask(dev, count):
    images, _, _, _ = _inputs(count)
    thr = torch.tensor([100], dtype=torch.int32, device=dev)
    want = [(TR.histogram(images, ch), TR.mask(images, 100, ch)) for ch in TR.CHANNELS]
    for shift in range(16):
        x = shifted(images, shift, dev)[0]
        for c, (hist, m) in enumerate(want):
            assert np.array_equal(K.tissue_histogram(x, c).cpu().numpy(), hist), (shift, c)
            out, flat, span = shifted(m, _side(shift), dev, fill=7)
            assert K.tissue_mask(x, thr, c, out=out) is out
            assert np.array_equal(out.cpu().numpy(), m) and guards_intact(flat, span), (shift, c)


@pytest.mark.parametrize("count", COUNTS)
def test_stain_moments_under_a_mask(dev, count):
    images, mask, _, _ = _inputs(count)
    od = torch.from_numpy(stain.od_table(OPTS.Io)).to(dev)
    want = SR.moments(images, mask)
    for shift in range(16):
        got = K.stain_moments(shifted(images, shift, dev)[0], od, OPTS.beta_q, shifted(mask, _side(shift), dev)[0])
        assert np.array_equal(got.cpu().numpy(), want), shift


@pytest.mark.parametrize("count", COUNTS)
def test_stain_separate_equals_the_aligned_call(dev, count):
    images, _, _, _ = _inputs(count)
    od = torch.from_numpy(stain.od_table(OPTS.Io)).to(dev)
    for residual, Kn in ((False, 2), (True, 3)):
        P = np.linalg.pinv(SR.stain_matrix(SR.HDAB, residual))
        Pd = torch.from_numpy(np.ascontiguousarray(P[None], dtype=np.float32)).to(dev)
        x0 = shifted(images, 0, dev)[0]
        f0 = K.stain_separate(x0, od, Pd, False, out=shifted(np.zeros((1, 1, count, Kn), np.float32), 0, dev)[0]).cpu().numpy()
        b0 = K.stain_separate(x0, od, Pd, True, OPTS.conc_max, out=shifted(np.zeros((1, 1, count, Kn), np.uint8), 0, dev)[0]).cpu().numpy()
        # the aligned call against the restatement, as tests/test_stain_gpu.py holds it: the fp32 rounding bound, one uint8 level
        ref = SR.separate(images, SR.HDAB, residual)[0]
        assert (np.abs(f0 - ref).reshape(-1, Kn).max(axis=0) <= 4 * 2.0 ** -23 * np.abs(P).sum(axis=1) * MAX_OD).all()
        assert np.abs(b0.astype(np.int32) - SR.separate_u8(images, SR.HDAB, residual, conc_max=OPTS.conc_max)).max() <= 1
        for shift in range(16):
            x = shifted(images, shift, dev)[0]
            of, flat_f, span_f = shifted(f0, _side(shift, 4), dev, fill=7)
            ob, flat_b, span_b = shifted(b0, _side(shift), dev, fill=7)
            assert K.stain_separate(x, od, Pd, False, out=of) is of and K.stain_separate(x, od, Pd, True, OPTS.conc_max, out=ob) is ob
            assert np.array_equal(of.cpu().numpy().view(np.uint32), f0.view(np.uint32)) and guards_intact(flat_f, span_f), (Kn, shift)
            assert np.array_equal(ob.cpu().numpy(), b0) and guards_intact(flat_b, span_b), (Kn, shift)


@pytest.mark.parametrize("count", COUNTS)
def test_stain_apply_equals_the_aligned_call(dev, count):
    images, _, _, _ = _inputs(count)
    od = torch.from_numpy(stain.od_table(OPTS.Io)).to(dev)
    A = SR.normalizer(SR.HDAB, (1.5, 0.7))
    Ad = torch.from_numpy(np.ascontiguousarray(A[None], dtype=np.float32)).to(dev)
    first = K.stain_apply(shifted(images, 0, dev)[0], od, Ad, OPTS.Io, out=shifted(images, 0, dev, fill=7)[0]).cpu().numpy()
    diff = np.abs(first.astype(np.int32) - SR.apply(images, A)[0].astype(np.int32))
    print(f"count {count}: {np.count_nonzero(diff)} of {diff.size} bytes differ from the restatement, by at most {diff.max()}")
    assert diff.max() <= 1                                                 # within one level, as test_apply_within_one_level_of_the_reference
    for shift in range(16):
        out, flat, span = shifted(images, _side(shift), dev, fill=7)
        assert K.stain_apply(shifted(images, shift, dev)[0], od, Ad, OPTS.Io, out=out) is out
        assert np.array_equal(out.cpu().numpy(), first) and guards_intact(flat, span), shift


@pytest.mark.parametrize("count", COUNTS)
def test_render_compose(dev, count):
    images, mask, heat, labels = _inputs(count)
    want_mask = RR.compose(images, mask=mask)
    want_heat = RR.compose(images, heat=heat, labels=labels, outline_color=(1, 2, 3))
    assert (labels > 0).any()
    for shift in range(16):
        x = shifted(images, shift, dev)[0]
        out, flat, span = shifted(images, _side(shift), dev, fill=7)
        assert render.compose(x, mask=shifted(mask, _side(shift), dev)[0], out=out) is out
        assert np.array_equal(out.cpu().numpy(), want_mask) and guards_intact(flat, span), shift
        out, flat, span = shifted(images, _side(shift), dev, fill=7)
        lab = shifted(labels, _side(shift, 4), dev)[0]
        assert render.compose(x, heat=shifted(heat, _side(shift), dev)[0], outlines=lab, outline_color=(1, 2, 3), out=out) is out
        assert np.array_equal(out.cpu().numpy(), want_heat) and guards_intact(flat, span), shift
        assert np.array_equal(x.cpu().numpy(), images)                     # the input is read only
