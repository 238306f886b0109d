"""CPU: the fp64 references of tests/pool_ref.py against torch's own fp64 operators and autograd -- the references are written from the
rules in csrc/pool.hip, csrc/prep.hip and csrc/head.hip, so this is what shows that those rules are the operations of the model
(nn.MaxPool2d(3, 2, 1), AdaptiveAvgPool2d(1) + AdaptiveMaxPool2d(1), the NCHW <-> NHWC boundary, CrossEntropyLoss * gamma, softmax,
the count loss whose weight is ln t from t = 20 on and t below).  Same shape lists and the same designed inputs (ties, -inf, NaN) as tests/test_pool_loss_ref_gpu.py.
Index and selection results are compared exactly; both sides of a floating-point comparison are fp64 and agree to 1e-12 of the
tensor's largest magnitude."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pool_ref as R

RTOL = 1e-12


def _close(got, want):
    assert got.shape == want.shape and got.dtype == torch.float64
    finite = torch.isfinite(want)
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    assert torch.equal(got[~finite & ~torch.isnan(want)], want[~finite & ~torch.isnan(want)])          # infinities, with their sign
    scale = float(want[finite].abs().max()) if bool(finite.any()) else 0.0
    err = float((got[finite] - want[finite]).abs().max()) if bool(finite.any()) else 0.0
    assert err <= RTOL * scale + 1e-300, (err, scale)


def _nchw(x_nhwc):
    return x_nhwc.permute(0, 3, 1, 2).contiguous()


def _sid(s):
    return "x".join(str(v) for v in s)


# ---------------------------------------------------------------------------------------------------------------- max pool
def _taps_of(indices, W):
    """torch's flat input index h * W + w of every window -> the tap kh * 3 + kw inside that window"""
    N, C, P, Q = indices.shape
    iy, ix = indices // W, indices % W
    kh = iy - (2 * torch.arange(P)[:, None] - 1)
    kw = ix - (2 * torch.arange(Q)[None, :] - 1)
    assert bool(((kh >= 0) & (kh < 3) & (kw >= 0) & (kw < 3)).all())
    return kh * 3 + kw


@pytest.mark.parametrize("kind", R.MAXPOOL_KINDS)
@pytest.mark.parametrize("shape", R.MAXPOOL_SHAPES, ids=_sid)
def test_maxpool_matches_max_pool2d_and_autograd(shape, kind):
    N, H, W, C = shape
    x = _nchw(R.maxpool_input(shape, kind))
    xr = x.clone().requires_grad_(True)
    y, ind = F.max_pool2d(xr, 3, 2, 1, return_indices=True)
    got_y, got_tap = R.maxpool_fwd(x)
    _close(got_y, y.detach())
    assert torch.equal(got_tap, _taps_of(ind, W))
    if kind in ("nan1", "nan2"):
        assert bool(torch.isnan(got_y).any())
    dy = R.ints(tuple(y.shape), 7, 1, 8) * (1 - 2 * R.ints(tuple(y.shape), 8, 0, 1))
    y.backward(dy)
    _close(R.maxpool_bwd(dy, got_tap, (H, W)), xr.grad)
    xm = x.clone().requires_grad_(True)
    F.max_pool2d(xm, 3, 2, 1).backward(dy * (y.detach() > 0))
    _close(R.maxpool_bwd(dy, got_tap, (H, W), y_mask=y.detach()), xm.grad)


def test_maxpool_nan_rule_by_hand():
    """one window: 7 first, then NaN at tap 5 and NaN at tap 7 -> y NaN, tap 7 (the last NaN); without NaN the FIRST of two 7s"""
    x = torch.zeros((1, 1, 2, 2), dtype=torch.float64)          # the window of output (0, 0) covers taps 4, 5, 7, 8
    x[0, 0] = torch.tensor([[7.0, float("nan")], [float("nan"), 3.0]])
    y, tap = R.maxpool_fwd(x)
    assert bool(torch.isnan(y).all()) and int(tap) == 7
    x[0, 0] = torch.tensor([[1.0, 7.0], [7.0, 3.0]])
    y, tap = R.maxpool_fwd(x)
    assert float(y) == 7.0 and int(tap) == 5


# ---------------------------------------------------------------------------------------------------------------- global avg + max
@pytest.mark.parametrize("kind", R.GAP_KINDS)
@pytest.mark.parametrize("case", R.GAP_SHAPES, ids=lambda c: "%dx%dx%d" % (c[0] + (c[1],)))
def test_gap_matches_adaptive_pools_and_autograd(case, kind):
    hw, C = case
    x = R.gap_input(hw, C, kind)
    HW = hw[0] * hw[1]
    xr = _nchw(x).requires_grad_(True)
    mx, ind = F.adaptive_max_pool2d(xr, 1, return_indices=True)
    f = (F.adaptive_avg_pool2d(xr, 1) + mx).flatten(1)
    feat, idx = R.gap_fwd(x)
    _close(feat, f.detach())
    assert torch.equal(idx, ind.flatten(1))
    if kind == "ties" and HW > 1:
        want = torch.tensor([R.tie_pair(c, HW)[0] for c in range(C)])
        assert torch.equal(idx, want[None, :].expand_as(idx))
    if kind in ("nan1", "nan2"):
        c = torch.arange(C)
        last = (7 * c + 3) % HW if kind == "nan1" else torch.maximum((7 * c + 3) % HW, (3 * c + 2) % HW)
        assert torch.equal(idx, last[None, :].expand_as(idx)) and bool(torch.isnan(feat).all())
        return
    if kind == "neginf":
        return                                                   # (-inf - -inf in the gradient of nothing: the finite kinds do the backward)
    df = R.ints((R.GAP_N, C), 9, 1, 8) * (1 - 2 * R.ints((R.GAP_N, C), 10, 0, 1))
    f.backward(df)
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()          # noqa: E731
    _close(R.gap_bwd(df, idx, x, False, True), nhwc(xr.grad))
    _close(R.gap_bwd(df, idx, x, True, True), nhwc(xr.grad * (xr.detach() > 0)))
    xa = _nchw(x).requires_grad_(True)
    F.adaptive_avg_pool2d(xa, 1).flatten(1).backward(df)
    _close(R.gap_bwd(df, None, x, False, False), nhwc(xa.grad))
    _close(R.gap_bwd(df, None, x, True, False), nhwc(xa.grad * (xa.detach() > 0)))


def test_gap_nan_rule_is_the_one_reported_for_adaptive_max_pool2d():
    """3 x 3 map, 7 at index 0, NaN at index 5: the NaN's index"""
    x = torch.zeros((1, 3, 3, 8), dtype=torch.float64)
    x[0, 0, 0] = 7.0
    x[0, 1, 2] = float("nan")
    _, idx = R.gap_fwd(x)
    _, ind = F.adaptive_max_pool2d(_nchw(x), 1, return_indices=True)
    assert bool((idx == 5).all()) and bool((ind == 5).all())


# ---------------------------------------------------------------------------------------------------------------- layout
def _same_bits(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    it = torch.int16 if got.dtype == torch.bfloat16 else torch.int32
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan)
    assert torch.equal(got.contiguous().view(it)[~nan], want.contiguous().view(it)[~nan])


def test_bf16_rounding_on_the_bits_is_torch_s():
    x = torch.cat([torch.tensor(R.BF16_SPECIALS, dtype=torch.float32),
                   torch.from_numpy(np.random.RandomState(0).standard_normal(4096).astype(np.float32)) * 37.0,
                   torch.tensor([1e-30, -3e30, 65504.0, 1.0, -2.5], dtype=torch.float32)])
    got = torch.from_numpy(R.round_bf16_bits(x.numpy()).view(np.int16).copy()).view(torch.bfloat16)
    _same_bits(got, x.to(torch.bfloat16))
    assert got[7].item() == 1.0 and got[8].item() == 1.015625 and got[11].item() == 1.0078125 and got[12].item() == 1.0078125
    assert got[5].item() == float("inf") and got[6].item() == -float("inf")


@pytest.mark.parametrize("case", R.TO_NHWC_CASES, ids=_sid)
def test_to_nhwc_matches_pad_permute_cast(case):
    N, C, H, W, Cp, tname = case
    x = R.layout_input(N, C, H, W, 11)
    want = F.pad(x.permute(0, 2, 3, 1), (0, Cp - C)).contiguous().to(R.DTYPES[tname])
    got = R.to_nhwc(x, Cp, R.DTYPES[tname])
    _same_bits(got, want)
    assert not bool(torch.signbit(got[..., C:]).any()) and bool((got[..., C:] == 0).all())


@pytest.mark.parametrize("case", R.TO_NCHW_CASES, ids=_sid)
def test_to_nchw_matches_permute_and_inverts_to_nhwc(case):
    N, C, H, W, Cp = case
    x = R.layout_input(N, C, H, W, 12)
    y = R.to_nhwc(x, Cp, torch.float32)
    y[..., C:] = float("nan")
    back = R.to_nchw(y, C)
    _close(back, y[..., :C].permute(0, 3, 1, 2).double())
    _same_bits(back.float(), x)


# ---------------------------------------------------------------------------------------------------------------- column sums
@pytest.mark.parametrize("shape", R.COLSUM_SHAPES, ids=_sid)
def test_colsum_matches_sum(shape):
    g = torch.from_numpy(np.random.RandomState(5).standard_normal(shape))
    _close(R.colsum(g.view(1, shape[0], 1, shape[1])), g.sum(0))
    gi = R.ints(shape, 6, -8, 8)
    assert torch.equal(R.colsum(gi), gi.sum(0))


# ---------------------------------------------------------------------------------------------------------------- losses
@pytest.mark.parametrize("gamma", R.LOSS_GAMMA)
@pytest.mark.parametrize("kind", R.LOGIT_KINDS)
@pytest.mark.parametrize("C", R.LOSS_C)
@pytest.mark.parametrize("M", R.LOSS_M)
def test_softmax_ce_matches_cross_entropy_and_autograd(M, C, kind, gamma):
    z, lab = R.logits_input(M, C, kind, 100 * C + 7)
    zr = z.double().requires_grad_(True)
    loss = F.cross_entropy(zr, lab) * gamma
    loss.backward()
    got, dl = R.softmax_ce(z, lab, gamma)
    _close(got.reshape(1), loss.detach().reshape(1))
    assert dl.shape == zr.grad.shape
    assert float((dl - zr.grad).abs().max()) <= RTOL * gamma / M
    _close(R.softmax_prob1(z), F.softmax(z.double(), dim=1)[:, 1])
    if kind == "decided":
        top = z.double().max(1).values
        assert torch.equal(R.log_sum_exp(z), top)                # lse is the leading logit exactly, in fp64 as in fp32
        lead = float((top - z.double()[torch.arange(M), lab]).sum())
        assert float(got) == lead * (gamma / M) and (M < 4 or lead > 0)


def _count_weighted_loss(x, t, mean):
    """An oracle of the count loss in this test's own words, from the stated rule alone: a target of 20 or more weighs ln(target), a
    smaller one weighs itself.  The weights are worked out one target at a time with math.log; the squared errors go through autograd."""
    w = torch.tensor([math.log(v) if v >= 20.0 else v for v in t.tolist()], dtype=torch.float64)
    total = (w * (x - t) * (x - t)).sum()
    return total / t.numel() if mean else total


@pytest.mark.parametrize("mean", [True, False])
@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("M", R.LOSS_M)
def test_mse_matches_the_weight_rule_and_autograd(M, weighted, mean):
    x, t = R.mse_input(M, 3 * M + 1)
    xr = x.clone().requires_grad_(True)
    loss = _count_weighted_loss(xr, t, mean) if weighted else F.mse_loss(xr, t, reduction="mean" if mean else "sum")
    loss.backward()
    got, dx = R.mse(x, t, weighted, mean)
    _close(got.reshape(1), loss.detach().reshape(1))
    _close(dx, xr.grad)
    if weighted:
        w = R.mse_weights(torch.tensor(R.MSE_TARGETS, dtype=torch.float64), True)
        assert w.tolist() == [0.0, 19.999, float(np.log(20.0)), float(np.log(1e4))]


def test_mse_gives_the_reference_s_recorded_weighted_losses():
    """tests/golden/reference_vectors.npz holds inputs and the fp32 results of the reference's own weighted loss (mean and sum), and its
    known answer 148.59375 for x = (1, 25, 30), t = (2, 20, 40): fp64 agrees to the rounding of the recorded fp32 value"""
    gold = np.load(os.path.join(os.path.dirname(__file__), "golden", "reference_vectors.npz"), allow_pickle=False)
    x, t = torch.from_numpy(gold["loss/wmse_in"]), torch.from_numpy(gold["loss/wmse_tg"])
    assert bool((t >= 20).any()) and bool((t < 20).any())
    for mean, key in ((True, "loss/wmse_mean"), (False, "loss/wmse_sum")):
        got, _ = R.mse(x, t, True, mean)
        assert abs(float(got) - float(gold[key])) <= 1e-5 * abs(float(gold[key]))
    got, _ = R.mse(torch.tensor([1.0, 25.0, 30.0]), torch.tensor([2.0, 20.0, 40.0]), True, True)
    assert abs(float(got) - 148.59375) <= 1e-5 * 148.59375
