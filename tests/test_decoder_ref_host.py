"""The plain reference of tests/decoder_ref.py is itself checked on the CPU: against ATen (fp64 and fp32), against autograd, and
against the committed golden Dice values.  The GPU tests of the decoder and Dice kernels rest on it."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import decoder_ref as R
from oracle import cellseg_oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "reference_vectors.npz"))

SIZES = [((10, 10), (19, 19)), ((19, 19), (38, 38)), ((38, 38), (75, 75)), ((75, 75), (150, 150)), ((150, 150), (299, 299)),
         ((1, 1), (7, 7)), ((7, 7), (1, 1)), ((5, 5), (5, 5)), ((9, 9), (4, 4)), ((3, 11), (8, 5))]
IDS = [f"{a[0]}x{a[1]}-{b[0]}x{b[1]}" for a, b in SIZES]


def _nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def _x(in_hw, seed, C=3, N=2):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, in_hw[0], in_hw[1], C, generator=g, dtype=torch.float32)


def test_taps_are_fp32_and_sum_to_one():
    for n_in, n_out in [(10, 19), (150, 299), (1, 7), (7, 1), (5, 5), (9, 4), (3, 5)]:
        i0, i1, w0, w1 = R.bilinear_taps(n_in, n_out)
        assert w0.dtype == np.float32 and w1.dtype == np.float32
        assert i0.min() >= 0 and i1.max() <= n_in - 1 and np.all((i1 == i0) | (i1 == i0 + 1))
        assert np.all(w0 >= 0) and np.all(w1 >= 0)
        # 1 - lambda is rounded once in fp32: the pair sums to 1 within half an ulp of 1
        assert np.abs(w0.astype(np.float64) + w1.astype(np.float64) - 1).max() <= R.U32
    i0, i1, w0, w1 = R.bilinear_taps(3, 5)               # scale exactly 0.5
    assert i0.tolist() == [0, 0, 1, 1, 2] and i1.tolist() == [1, 1, 2, 2, 2] and w1.tolist() == [0, .5, 0, .5, 0]
    i0, i1, w0, w1 = R.bilinear_taps(7, 1)               # out == 1: scale 0, the first pixel
    assert i0.tolist() == [0] and w0.tolist() == [1.0]
    i0, i1, w0, w1 = R.bilinear_taps(1, 7)               # in == 1: every output reads pixel 0 with weight 1
    assert i0.tolist() == [0] * 7 and i1.tolist() == [0] * 7 and w0.tolist() == [1.0] * 7


@pytest.mark.parametrize("in_hw,out_hw", SIZES, ids=IDS)
def test_bilinear_fwd_ref_vs_aten_fp64(in_hw, out_hw):
    """ATen on an fp64 tensor uses fp64 taps; the reference uses the fp32 taps.  The interpolant is continuous and piecewise linear in
    the source coordinate with slope <= max|x[i+1] - x[i]| <= 2 max|x| along each axis (a floor that flips between the two tap sets
    moves along the same line), so the two differ by at most 2 max|x| (dy + dx), d = the source coordinate's fp32 error plus the
    rounding of 1 - lambda: scale and scale * dst are each rounded once (relative 2^-24 each, src <= in - 1) -> (in-1) 2^-23, and
    2^-24 for the weight."""
    x = _x(in_hw, 11).double()
    got = R.bilinear_fwd_ref(x, out_hw)
    want = _nhwc(F.interpolate(_nchw(x), size=out_hw, mode="bilinear", align_corners=True))
    d = sum((n - 1) * 2.0 ** -23 + 2.0 ** -24 for n in in_hw)
    bound = 2 * float(x.abs().max()) * d + 1e-14
    err = float((got - want).abs().max())
    print(f"fwd_ref vs ATen fp64 {in_hw}->{out_hw}: err {err:.3e} bound {bound:.3e}")
    assert got.shape == want.shape and err <= bound


@pytest.mark.parametrize("in_hw,out_hw", SIZES, ids=IDS)
def test_bilinear_fwd_ref_vs_aten_fp32(in_hw, out_hw):
    """On an fp32 tensor ATen's taps are the reference's by construction, so only ATen's own fp32 arithmetic separates the two: four
    products and three additions, at most four roundings on the path of any one term, plus one for a 1 - lambda that a vectorised
    path may form differently -> 5 * 2^-24 * sum |w| |x|.  A wrong tap definition would show at the 1e-4 level."""
    x = _x(in_hw, 12)
    got = R.bilinear_fwd_ref(x.double(), out_hw)
    want = _nhwc(F.interpolate(_nchw(x), size=out_hw, mode="bilinear", align_corners=True)).double()
    bound = 5 * R.U32 * R.bilinear_fwd_mag(x.double(), out_hw)
    ratio = float(((got - want).abs() / bound.clamp_min(1e-300)).max())
    print(f"fwd_ref vs ATen fp32 {in_hw}->{out_hw}: worst err/bound {ratio:.3f}")
    assert bool(((got - want).abs() <= bound).all())


@pytest.mark.parametrize("in_hw,out_hw", SIZES, ids=IDS)
def test_bilinear_bwd_ref_is_the_transpose(in_hw, out_hw):
    x = _x(in_hw, 13).double().requires_grad_()
    g = torch.Generator().manual_seed(14)
    dy = torch.randn(2, out_hw[0], out_hw[1], 3, generator=g, dtype=torch.float64)
    y = R.bilinear_fwd_ref(x, out_hw)                      # fp64 autograd through the fp32-tap forward
    (auto,) = torch.autograd.grad(y, x, dy)
    got = R.bilinear_bwd_ref(dy, in_hw)
    scale = float(R.bilinear_bwd_mag(dy, in_hw).max())
    assert float((got - auto).abs().max()) <= 1e-13 * scale
    lhs, rhs = float((y.detach() * dy).sum()), float((x.detach() * got).sum())
    mag = float((R.bilinear_fwd_mag(x.detach(), out_hw) * dy.abs()).sum())
    assert abs(lhs - rhs) <= 1e-12 * mag
    # mask: dx * (mask > 0), negative values and -0.0 mask out
    mask = torch.randn(x.shape, generator=g, dtype=torch.float64)
    mask.view(-1)[0] = -0.0
    gm = R.bilinear_bwd_ref(dy, in_hw, mask)
    assert torch.equal(gm, torch.where(mask > 0, got, torch.zeros_like(got)))


def test_bilinear_bwd_terms():
    assert R.bilinear_bwd_terms((5, 5), (5, 5)) == 1
    assert R.bilinear_bwd_terms((1, 1), (7, 7)) == 49
    assert R.bilinear_bwd_terms((7, 7), (1, 1)) == 1
    assert R.bilinear_bwd_terms((3, 3), (5, 5)) == 9        # the middle pixel: outputs 1, 2, 3 on each axis
    assert R.bilinear_bwd_terms((3, 11), (8, 5)) >= 4


def test_dice_ref_vs_golden_and_autograd():
    a, b = torch.from_numpy(GOLD["loss/dice_in"]), torch.from_numpy(GOLD["loss/dice_tg"])
    ad, bd = a.double(), b.double()
    assert abs(float(R.dice_ref(ad, bd, 1e-6, True)[0]) - float(GOLD["loss/dice_mean"])) < 1e-6
    assert abs(float(R.dice_ref(ad, bd, 1e-6, False)[0]) - float(GOLD["loss/dice_sum"])) < 1e-6
    assert abs(float(R.dice_ref(ad[0], bd[0], 1e-6, True)[0]) - float(GOLD["loss/dice_2d"])) < 1e-6
    for p, t, eps, mean in [(ad, bd, 1e-6, True), (ad, bd, 1.0, False), (ad[0], bd[0], 1e-6, True)]:
        pp = p.clone().requires_grad_()
        want = orc.dice_loss(pp, t, eps, "mean" if mean else "sum")
        want.backward()
        loss, sums, grad = R.dice_ref(p, t, eps, mean)
        assert abs(float(loss) - float(want.detach())) <= 1e-14
        assert grad.shape == p.shape and float((grad - pp.grad).abs().max()) <= 1e-13 * float(pp.grad.abs().max())
        p2 = p.reshape(1, -1) if p.ndim == 2 else p.reshape(p.shape[0], -1)
        t2 = t.reshape(1, -1) if t.ndim == 2 else t.reshape(t.shape[0], -1)
        assert torch.allclose(sums, torch.stack([(p2 * t2).sum(1), (p2 * p2).sum(1), (t2 * t2).sum(1)], 1), rtol=1e-14, atol=0)


@pytest.mark.parametrize("C", [2, 3, 5])
def test_softmax_channel_ref(C):
    g = torch.Generator().manual_seed(20 + C)
    logits = 4 * torch.randn(2, C, 5, 7, generator=g, dtype=torch.float64)
    logits[0, 0, 0, 0] = 300.0                              # the others underflow: p is exactly 1 / 0
    logits[1, :, 1, 1] = 1e4                                # common offset, all equal: 1 / C
    dp = torch.randn(2, 5, 7, generator=g, dtype=torch.float64)
    for ch in range(C):
        want = torch.softmax(logits, 1)[:, ch]
        got = R.softmax_channel_ref(logits, ch)
        assert float((got - want).abs().max()) <= 1e-15
        lg = logits.clone().requires_grad_()
        torch.softmax(lg, 1)[:, ch].backward(dp)
        grad = R.softmax_channel_grad_ref(logits, dp, ch)
        assert float((grad - lg.grad).abs().max()) <= 1e-15 * max(1.0, float(dp.abs().max()))
        assert float(grad.sum(1).abs().max()) <= 1e-15 * float(dp.abs().max())
    assert float(R.softmax_channel_ref(logits, 0)[0, 0, 0]) == 1.0
    assert abs(float(R.softmax_channel_ref(logits, 1)[1, 1, 1]) - 1.0 / C) <= 1e-16
