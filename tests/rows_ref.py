"""Plain fp64 references (CPU, torch) of the row passes: the BatchNorm passes of csrc/bn.hip over rows [M][C] and the squeeze-excite /
StochasticDepth element-wise kernels of csrc/dwse.hip over [N][H][W][C].  Written from the formulas in the header of bn.hip and in
include/cellseg_hip.h, not from autograd: tests/test_rows_ref_host.py holds them to torch's own fp64 BatchNorm and autograd,
tests/test_row_passes_ref_gpu.py holds the kernels to them.

Every function takes tensors of any float dtype, computes in float64 and returns float64.  `None` stands for a nullable argument of
the C ABI (gamma = 1, beta = 0, no residual, davg = 0, row_scale = 1, no b)."""
import torch

ACT_NONE, ACT_RELU, ACT_SILU = 0, 1, 2              # include/cellseg_hip.h: CS_ACT_*
OWN_RELU, FROZEN = 0x100, 0x200                      # CS_BN_BWD_OWN_RELU, CS_BN_BWD_FROZEN


def _d(t):
    return None if t is None else t.detach().to(torch.float64).cpu()


def bn_moments(z, eps):
    """mean, BIASED variance and rstd = 1 / sqrt(var + eps) per channel of rows z[M][C]."""
    z = _d(z)
    mean = z.mean(0)
    var = ((z - mean) ** 2).mean(0)
    return mean, var, 1.0 / torch.sqrt(var + eps)


def bn_running(rm, rv, mean, var, M, momentum):
    """The running statistics after one train-mode step: blended with the batch mean and the UNBIASED batch variance (nn.BatchNorm*d);
    a single row has no unbiased variance and the library blends the plain one (= 0) in."""
    rm, rv, mean, var = _d(rm), _d(rv), _d(mean), _d(var)
    unbiased = var * M / (M - 1) if M > 1 else var
    return (1.0 - momentum) * rm + momentum * mean, (1.0 - momentum) * rv + momentum * unbiased


def bn_preact(z, mean, rstd, gamma, beta):
    """u = gamma * xhat + beta and xhat = (z - mean) * rstd."""
    z, mean, rstd, gamma, beta = _d(z), _d(mean), _d(rstd), _d(gamma), _d(beta)
    xhat = (z - mean) * rstd
    # an absent gamma / beta is 1 / 0 in the same arithmetic (IEEE: -0 + 0 = +0, as in the kernels)
    u = xhat * (1.0 if gamma is None else gamma) + (0.0 if beta is None else beta)
    return u, xhat


def sigmoid(u):
    return 1.0 / (1.0 + torch.exp(-u))


def bn_apply(z, mean, rstd, gamma, beta, residual, act):
    """y = act(gamma * (z - mean) * rstd + beta + residual), act in none / ReLU / SiLU."""
    u, _ = bn_preact(z, mean, rstd, gamma, beta)
    if residual is not None:
        u = u + _d(residual)
    if act == ACT_RELU:
        return torch.where(u > 0, u, torch.zeros_like(u))
    if act == ACT_SILU:
        return u * sigmoid(u)
    if act != ACT_NONE:
        raise ValueError("bn_apply: act %r" % (act,))
    return u


def bn_bwd_g(dy, u, flags):
    """The gradient that reaches the normalisation's own output u: dy, masked by the layer's own ReLU (OWN_RELU: STRICTLY u > 0) and /
    or taken through the SiLU that follows (the low byte of flags = CS_ACT_SILU: d silu(u)/du = sig * (1 + u * (1 - sig)))."""
    g = _d(dy)
    if flags & ~(OWN_RELU | FROZEN | 0xff) or (flags & 0xff) not in (ACT_NONE, ACT_SILU):
        raise ValueError("bn_bwd: flags %#x" % flags)
    if flags & OWN_RELU:
        g = torch.where(u > 0, g, torch.zeros_like(g))
    if (flags & 0xff) == ACT_SILU:
        sg = sigmoid(u)
        g = g * sg * (1.0 + u * (1.0 - sg))
    return g


def bn_bwd(dy, z, mean, rstd, gamma, beta, flags):
    """dz, dgamma, dbeta.  s0 = sum g, s1 = sum g * xhat over the rows; dbeta = s0, dgamma = s1;
    batch statistics: dz = gamma * rstd * (g - s0 / M - xhat * s1 / M);  FROZEN (running statistics): dz = gamma * rstd * g."""
    u, xhat = bn_preact(z, mean, rstd, gamma, beta)
    g = bn_bwd_g(dy, u, flags)
    M = xhat.shape[0]
    s0, s1 = g.sum(0), (g * xhat).sum(0)
    gr = _d(rstd) if gamma is None else _d(gamma) * _d(rstd)
    dz = gr * g if flags & FROZEN else gr * (g - s0 / M - xhat * (s1 / M))
    return dz, s1, s0


def se_scale(x, s):
    """y[n,p,q,c] = x[n,p,q,c] * s[n,c]"""
    return _d(x) * _d(s)[:, None, None, :]


def se_scale_bwd_dx(dy, s, davg):
    """dx[n,p,q,c] = dy[n,p,q,c] * s[n,c] + davg[n,c] / HW: the direct path and the path through the mean pool that made s."""
    dy = _d(dy)
    dx = dy * _d(s)[:, None, None, :]
    return dx + (0.0 if davg is None else _d(davg)[:, None, None, :] / (dy.shape[1] * dy.shape[2]))


def rowscale_add(a, row_scale, b):
    """y[n,...] = a[n,...] * row_scale[n] + b[n,...]"""
    y = _d(a)
    if row_scale is not None:
        y = y * _d(row_scale).view(-1, *([1] * (y.dim() - 1)))
    if b is not None:
        y = y + _d(b)
    return y
