"""CPU: the fp64 references of tests/rows_ref.py against torch's own fp64 BatchNorm, autograd and broadcasting -- the references are
written from the formulas of csrc/bn.hip / include/cellseg_hip.h, so this is what shows that those formulas are the operation
(nn.BatchNorm1d in train() and eval(), followed by nothing / ReLU / SiLU; the squeeze-excite scale with its mean pool; the
StochasticDepth row scale).  Both sides are fp64: they agree to 1e-12 of the tensor's largest magnitude."""
import pytest
import torch
import torch.nn.functional as F

import rows_ref as R
from cellsegmentation_amd import _lib

RTOL = 1e-12
ACTS = {"none": (R.ACT_NONE, lambda u: u, 0), "relu": (R.ACT_RELU, torch.relu, R.OWN_RELU), "silu": (R.ACT_SILU, F.silu, R.ACT_SILU)}


def _close(got, want):
    scale = float(want.abs().max())
    assert got.shape == want.shape and got.dtype == torch.float64
    assert float((got - want).abs().max()) <= RTOL * scale + 1e-300, (float((got - want).abs().max()), scale)


def _rows(M, C, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn((M, C), generator=g, dtype=torch.float64) * 1.3 + 0.2
    dy = torch.randn((M, C), generator=g, dtype=torch.float64)
    gamma = torch.rand((C,), generator=g, dtype=torch.float64) + 0.5
    beta = torch.randn((C,), generator=g, dtype=torch.float64) * 0.3
    return z, dy, gamma, beta, g


def test_constants_are_the_library_s():
    assert (R.ACT_NONE, R.ACT_RELU, R.ACT_SILU) == (_lib.CS_ACT_NONE, _lib.CS_ACT_RELU, _lib.CS_ACT_SILU)
    assert (R.OWN_RELU, R.FROZEN) == (_lib.CS_BN_BWD_OWN_RELU, _lib.CS_BN_BWD_FROZEN)


@pytest.mark.parametrize("act", sorted(ACTS))
@pytest.mark.parametrize("shape", [(2, 8), (37, 24), (64, 16)])
def test_train_mode_matches_batch_norm_and_autograd(shape, act):
    M, C = shape
    code, fn, flags = ACTS[act]
    z, dy, gamma, beta, _ = _rows(M, C, 3 * M + C)
    eps = 1e-3
    zr, gr, br = z.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y = fn(F.batch_norm(zr, None, None, gr, br, training=True, eps=eps))
    y.backward(dy)
    mean, var, rstd = R.bn_moments(z, eps)
    _close(mean, z.mean(0))
    _close(var, z.var(0, unbiased=False))
    _close(R.bn_apply(z, mean, rstd, gamma, beta, None, code), y.detach())
    dz, dgamma, dbeta = R.bn_bwd(dy, z, mean, rstd, gamma, beta, flags)
    _close(dz, zr.grad)
    _close(dgamma, gr.grad)
    _close(dbeta, br.grad)


@pytest.mark.parametrize("act", sorted(ACTS))
@pytest.mark.parametrize("shape", [(1, 8), (37, 24)])
def test_frozen_matches_eval_mode_batch_norm_and_autograd(shape, act):
    M, C = shape
    code, fn, flags = ACTS[act]
    z, dy, gamma, beta, g = _rows(M, C, 5 * M + C)
    eps = 1e-3
    rm = torch.randn((C,), generator=g, dtype=torch.float64)
    rv = torch.rand((C,), generator=g, dtype=torch.float64) + 0.5
    zr, gr, br = z.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y = fn(F.batch_norm(zr, rm, rv, gr, br, training=False, eps=eps))
    y.backward(dy)
    rstd = 1.0 / torch.sqrt(rv + eps)
    _close(R.bn_apply(z, rm, rstd, gamma, beta, None, code), y.detach())
    dz, dgamma, dbeta = R.bn_bwd(dy, z, rm, rstd, gamma, beta, R.FROZEN | flags)
    _close(dz, zr.grad)
    _close(dgamma, gr.grad)
    _close(dbeta, br.grad)


def test_residual_and_absent_affine_parameters():
    z, res, gamma, beta, _ = _rows(19, 16, 11)
    mean, var, rstd = R.bn_moments(z, 1e-5)
    xhat = (z - mean) / torch.sqrt(var + 1e-5)
    _close(R.bn_apply(z, mean, rstd, None, None, None, R.ACT_NONE), xhat)
    _close(R.bn_apply(z, mean, rstd, gamma, None, res, R.ACT_RELU), torch.relu(xhat * gamma + res))
    _close(R.bn_apply(z, mean, rstd, None, beta, res, R.ACT_SILU), F.silu(xhat + beta + res))
    dz, dgamma, dbeta = R.bn_bwd(res, z, mean, rstd, None, None, 0)
    dz1, dgamma1, dbeta1 = R.bn_bwd(res, z, mean, rstd, torch.ones(16), torch.zeros(16), 0)
    assert torch.equal(dz, dz1) and torch.equal(dgamma, dgamma1) and torch.equal(dbeta, dbeta1)


def test_own_relu_mask_is_strict():
    """u == 0 passes no gradient (torch.relu's subgradient at 0 is 0 as well)"""
    z = torch.tensor([[1.0, -2.0], [0.0, 3.0]], dtype=torch.float64)
    dy = torch.ones_like(z)
    zero, one = torch.zeros(2, dtype=torch.float64), torch.ones(2, dtype=torch.float64)
    dz, dgamma, dbeta = R.bn_bwd(dy, z, zero, one, one, zero, R.FROZEN | R.OWN_RELU)
    assert dz.tolist() == [[1.0, 0.0], [0.0, 1.0]] and dbeta.tolist() == [1.0, 1.0] and dgamma.tolist() == [1.0, 3.0]
    with pytest.raises(ValueError):
        R.bn_bwd(dy, z, zero, one, one, zero, R.ACT_RELU)           # ReLU is a flag of the backward, never its activation code


@pytest.mark.parametrize("M", [2, 37])
def test_running_statistics_match_batchnorm1d(M):
    C = 16
    z, _, gamma, beta, g = _rows(M, C, 13 * M)
    bn = torch.nn.BatchNorm1d(C, eps=1e-3, momentum=0.1).double()
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn((C,), generator=g, dtype=torch.float64))
        bn.running_var.copy_(torch.rand((C,), generator=g, dtype=torch.float64) + 0.5)
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    bn.train()
    bn(z)
    mean, var, _ = R.bn_moments(z, bn.eps)
    rm, rv = R.bn_running(rm0, rv0, mean, var, M, bn.momentum)
    _close(rm, bn.running_mean)
    _close(rv, bn.running_var)


def test_running_statistics_of_a_single_row_blend_the_plain_variance():
    z, _, _, _, g = _rows(1, 8, 17)
    rm0, rv0 = torch.randn((8,), generator=g, dtype=torch.float64), torch.rand((8,), generator=g, dtype=torch.float64) + 0.5
    mean, var, rstd = R.bn_moments(z, 1e-3)
    assert torch.equal(var, torch.zeros(8, dtype=torch.float64)) and torch.equal(mean, z[0])
    rm, rv = R.bn_running(rm0, rv0, mean, var, 1, 0.25)
    _close(rm, 0.75 * rm0 + 0.25 * z[0])
    _close(rv, 0.75 * rv0)


def test_se_scale_and_its_input_gradient_match_autograd():
    g = torch.Generator().manual_seed(23)
    N, H, W, C = 3, 4, 5, 16
    x = torch.randn((N, H, W, C), generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn((C, C), generator=g, dtype=torch.float64)
    dy = torch.randn((N, H, W, C), generator=g, dtype=torch.float64)
    # the whole block: s is a function of the mean pool of x
    s = torch.sigmoid(x.mean((1, 2)) @ w)
    y = s[:, None, None, :] * x
    y.backward(dy)
    _close(R.se_scale(x, s), y.detach())
    # the same in the library's steps: ds = sum dy * x, davg = the gradient that ds sends back to the pooled mean
    avg = x.detach().mean((1, 2)).requires_grad_(True)
    s2 = torch.sigmoid(avg @ w)
    s2.backward((dy * x.detach()).sum((1, 2)))
    _close(R.se_scale_bwd_dx(dy, s2, avg.grad), x.grad)
    # davg = None: s held constant
    x2 = x.detach().clone().requires_grad_(True)
    (s.detach()[:, None, None, :] * x2).backward(dy)
    _close(R.se_scale_bwd_dx(dy, s, None), x2.grad)


def test_rowscale_add_matches_broadcasting():
    g = torch.Generator().manual_seed(29)
    a = torch.randn((3, 4, 5, 8), generator=g, dtype=torch.float64)
    b = torch.randn((3, 4, 5, 8), generator=g, dtype=torch.float64)
    rs = torch.tensor([0.0, 1.25, 2.0], dtype=torch.float64)
    _close(R.rowscale_add(a, rs, b), a * rs.view(-1, 1, 1, 1) + b)
    _close(R.rowscale_add(a, None, b), a + b)
    _close(R.rowscale_add(a, rs, None), a * rs.view(-1, 1, 1, 1))
    assert torch.equal(R.rowscale_add(a, rs, b)[0], b[0])
