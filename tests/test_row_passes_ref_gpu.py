"""GPU: the BatchNorm row passes of csrc/bn.hip (finalize, apply, apply + finalize in one launch, backward with its flags) and the
squeeze-excite / StochasticDepth element-wise kernels of csrc/dwse.hip against the plain fp64 references of tests/rows_ref.py, which
tests/test_rows_ref_host.py holds to torch's own fp64 BatchNorm and autograd.  tests/test_row_passes_bits_gpu.py pins the bits of these
passes to digests recorded from the library itself; this file says whether those bits are right.

Four kinds of test:
  a. exact     integer-valued inputs and power-of-two constants with mean = 0, rstd = 1: every intermediate is exact in fp32 whatever the
               compiler fuses, so the kernel must give the reference's bits (bf16 outputs that are not representable are the exact value
               rounded once, to nearest even, on both sides);
  b. mask      the ReLU mask of CS_BN_BWD_OWN_RELU against the sign of the forward's own output where gamma * z + beta cancels to
               nothing but the rounding error of the product -- zero if the multiply-add is not fused, a signed residual if it is;
  c. tolerance random inputs with real batch statistics, with bounds derived below from the roundings each pass performs;
  d. SE        cs_se_scale, cs_se_scale_bwd_dx, cs_rowscale_add: exact, with the nullable arguments and the grid-stride wrap.

Notation: u32 = 2^-24, the unit roundoff of fp32; uT = that of the element type (2^-8 for bf16: 8 significant bits, half a unit in the last place; 2^-24 for fp32).  A reduction's sums carry
the bound tests/test_bn_reductions_gpu.py states and derives: 2e-6 of the sum of magnitudes (fp32 partial sums per thread, exact above)."""
import copy

import numpy as np
import pytest
import torch

import rows_ref as R
from cellsegmentation_amd import _lib
from cellsegmentation_amd import functional as HF
from cellsegmentation_amd import kernels as K

pytestmark = pytest.mark.gpu

# (M, C), from ew_split / red_split: a single row; fewer rows than row lanes; a dead lane (CG = 3, rpar = 85); ragged last row blocks with
# odd one-row tails; a last chunk one group wide (CG = 65 for the 32-wide passes, CG = 257 for cs_bn_apply); rpar = 1
SHAPES = [(1, 8), (3, 24), (37, 8), (1000, 40), (8, 512), (300, 520), (300, 2056), (2000, 136), (9001, 288), (5000, 816)]
PARTIAL_SHAPE = (2816, 2304)            # 22 row blocks x 2304 channels x 6 words > the atomics budget: partial rows + fold launch
ALL_SHAPES = SHAPES + [PARTIAL_SHAPE]
EXACT_TRAIN_SHAPES = [(8, 512), (1024, 40), (256, 520)]          # M a power of two: s / M is exact
MASK_SHAPES = [(300, 520), (1000, 40)]
SILU_SHAPES = [(1000, 40), (300, 520), (5000, 816)]
DTYPES = {"bf16": torch.bfloat16, "f32": torch.float32}
BITS = {torch.bfloat16: torch.int16, torch.float32: torch.int32}
U32 = 2.0 ** -24
UT = {torch.bfloat16: 2.0 ** -8, torch.float32: 2.0 ** -24}
SUM_RTOL = 2e-6                         # tests/test_bn_reductions_gpu.py: of the sum of magnitudes
EPS = float(np.float32(1e-3))           # the library takes eps and momentum as C floats
MOMENTUM = float(np.float32(0.1))
NONE, RELU, SILU = K.CS_ACT_NONE, K.CS_ACT_RELU, K.CS_ACT_SILU
OWN_RELU, FROZEN = K.CS_BN_BWD_OWN_RELU, K.CS_BN_BWD_FROZEN
BWD_FLAGS = {"none": 0, "silu": SILU, "own_relu": OWN_RELU, "frozen": FROZEN, "frozen_own_relu": FROZEN | OWN_RELU, "frozen_silu": FROZEN | SILU}

# The SiLU paths use __expf and the hardware reciprocal (cs_common.h: silu_fast, sigmoid_fast; bn.hip: act_grad8).  Their error against
# the fp64 reference was measured with fp32 tensors (no output rounding) on SILU_SHAPES with the inputs of _inputs() below, as the largest
#     forward   |y  - ref| / (u32 * A),  A = |gamma * xhat| + |beta| + |residual|                                  (cs_bn_apply, SiLU)
#     backward  |dz - ref| / (u32 * |gamma * rstd * dy| * (S + A_u)),  S = sig * (1 + |u| * (1 - sig)), A_u = |gamma * xhat| + |beta|
#                                                                                        (cs_bn_bwd_*, CS_BN_BWD_FROZEN | CS_ACT_SILU)
# (A_u is there because the rounding error of u itself reaches the derivative through silu'' <= 1/2.)  The constants are four times the
# largest measured value, rounded up to a power of two: the measurement samples arguments finitely and __expf's error grows with |u|.
# Measured at commit 245fbab on an MI355X (hipcc of ROCm 7.2), forward / backward:
#     (1000, 40)  3.27 / 3.62      (300, 520)  3.97 / 3.93      (5000, 816)  4.50 / 4.47          4 * 4.50 = 18.0 -> 32
SILU_FWD_ULPS = 32.0
SILU_BWD_ULPS = 32.0


def _shape_id(s):
    return "x".join(str(v) for v in s)


def _ratio(err, tol):
    return float((err / tol).max())


def _same_bits(got, want64):
    """`got` holds exactly the bits of the fp64 reference rounded (once, to nearest even) to got's dtype"""
    got = got.detach().cpu().contiguous()
    want = want64.to(got.dtype).contiguous()
    assert got.shape == want.shape
    if got.dtype in BITS:
        same = torch.equal(got.view(BITS[got.dtype]), want.view(BITS[got.dtype]))
    else:
        same = torch.equal(got, want)
    if not same:
        bad = (got.double() != want.double()) | (torch.signbit(got) != torch.signbit(want))
        idx = bad.nonzero()[0].tolist()
        raise AssertionError("%d of %d elements differ, first at %s: got %r want %r"
                             % (int(bad.sum()), bad.numel(), idx, float(got[tuple(idx)]), float(want[tuple(idx)])))


def _within(got, want64, tol, what):
    err = (got.detach().double().cpu() - want64).abs()
    ratio = _ratio(err, tol + 1e-300)
    print("%s: worst error / bound = %.3f" % (what, ratio))
    assert bool((err <= tol).all()), "%s: error up to %.3f x its bound (%d elements over)" % (what, ratio, int((err > tol).sum()))


# ---------------------------------------------------------------------------------------------------------------- launch rule
def test_shape_list_runs_both_reduction_paths(dev):
    """cs_bn_partial_workspace decides between fp64 atomics (0) and partial rows with a fold launch: the list holds both"""
    lib = _lib.load()
    words = [lib.cs_bn_partial_workspace(M, C) for M, C in ALL_SHAPES]
    assert any(w == 0 for w in words) and any(w > 0 for w in words)
    assert lib.cs_bn_partial_workspace(*PARTIAL_SHAPE) > 0
    assert all(M * C <= 7.2e6 for M, C in ALL_SHAPES + EXACT_TRAIN_SHAPES)


# ---------------------------------------------------------------------------------------------------------------- a. exact
def _hash(M, C, seed):
    """uint32 [M, C]: an integer hash of (row, channel, seed), arithmetic mod 2^32 only -- the same on every host"""
    r = np.arange(M, dtype=np.uint32)[:, None]
    c = np.arange(C, dtype=np.uint32)[None, :]
    h = r * np.uint32(2654435761) + c * np.uint32(0x85EBCA6B) + np.uint32((seed * 0x9E3779B1) & 0xFFFFFFFF)
    h ^= h >> np.uint32(15)
    h *= np.uint32(0x2C1B3C6D)
    h ^= h >> np.uint32(13)
    h *= np.uint32(0x297A2D39)
    h ^= h >> np.uint32(16)
    return h


def _ints(M, C, seed, lo, hi):
    return (_hash(M, C, seed) % np.uint32(hi - lo + 1)).astype(np.int64) + lo


_exact_cache = {}


def _exact_inputs(M, C):
    """fp64 CPU tensors: z, res in [-8, 8], dy in +-[1, 8] (never 0), beta in [-4, 4], gamma = +-2^k with k in [-1, 2] -- all integers or
    halves.  u = gamma * z + beta is a multiple of 1/2 below 37, u + res below 45, gamma * dy below 33: all representable in bf16.  Every
    fourth channel has gamma = 1 and z = -beta on its even rows: u is exactly 0 there."""
    if _exact_cache.get("key") != (M, C):
        z = _ints(M, C, 1, -8, 8)
        dy = _ints(M, C, 2, 1, 8) * (1 - 2 * _ints(M, C, 3, 0, 1))
        res = _ints(M, C, 4, -8, 8)
        beta = _ints(1, C, 5, -4, 4)[0]
        gamma = 2.0 ** _ints(1, C, 6, -1, 2)[0] * (1 - 2 * _ints(1, C, 7, 0, 1)[0])
        gamma[::4] = 1.0
        z[::2, ::4] = -beta[::4]
        t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(torch.float64) for k, v in
             (("z", z), ("dy", dy), ("res", res), ("beta", beta), ("gamma", gamma))}
        t["mean"], t["rstd"] = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
        _exact_cache.clear()
        _exact_cache.update(t, key=(M, C))
    return _exact_cache


def _to_dev(d, dtype, dev, names):
    """rows in the element type, per-channel vectors in fp32"""
    return [d[n].to(dtype if d[n].dim() == 2 else torch.float32).to(dev) for n in names]


@pytest.mark.parametrize("tname", sorted(DTYPES))
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=_shape_id)
def test_apply_exact(shape, tname, dev):
    """cs_bn_apply, none / ReLU, with and without residual, gamma and / or beta absent: the reference's bits"""
    M, C = shape
    dtype = DTYPES[tname]
    d = _exact_inputs(M, C)
    z, res, gamma, beta, mean, rstd = _to_dev(d, dtype, dev, ("z", "res", "gamma", "beta", "mean", "rstd"))
    assert bool(((d["z"] * d["gamma"] + d["beta"]) == 0).any())
    for act in (NONE, RELU):
        for r_dev, r_ref in ((None, None), (res, d["res"])):
            for g_dev, g_ref in ((gamma, d["gamma"]), (None, None)):
                for b_dev, b_ref in ((beta, d["beta"]), (None, None)):
                    y = K.bn_apply(z, mean, rstd, g_dev, b_dev, residual=r_dev, act=act)
                    _same_bits(y, R.bn_apply(d["z"], d["mean"], d["rstd"], g_ref, b_ref, r_ref, act))


def _bwd_exact(shape, tname, dev, flag_names):
    M, C = shape
    dtype = DTYPES[tname]
    d = _exact_inputs(M, C)
    z, dy, gamma, beta, mean, rstd = _to_dev(d, dtype, dev, ("z", "dy", "gamma", "beta", "mean", "rstd"))
    zero_u = (d["z"] * d["gamma"] + d["beta"]) == 0
    assert bool(zero_u.any()) and bool((d["dy"] != 0).all())
    for name in flag_names:
        flags = BWD_FLAGS[name]
        dz, dgamma, dbeta = K.bn_bwd(dy, z, mean, rstd, gamma, True, beta=beta, act=flags)
        want = R.bn_bwd(d["dy"], d["z"], d["mean"], d["rstd"], d["gamma"], d["beta"], flags)
        assert float(want[1].abs().max()) < 2 ** 24 and float(want[2].abs().max()) < 2 ** 24
        _same_bits(dz, want[0])
        _same_bits(dgamma, want[1])
        _same_bits(dbeta, want[2])
        if flags == FROZEN | OWN_RELU:                     # the mask is strict: u == 0 passes no gradient
            assert bool((dz.double().cpu()[zero_u] == 0).all())


@pytest.mark.parametrize("tname", sorted(DTYPES))
@pytest.mark.parametrize("shape", EXACT_TRAIN_SHAPES, ids=_shape_id)
def test_bwd_exact_batch_statistics(shape, tname, dev):
    """cs_bn_bwd_reduce + cs_bn_bwd_apply with the batch terms, plain and CS_BN_BWD_OWN_RELU.  |s0| <= 8 M and |s1| <= 64 M are exact
    integers, s / M a multiple of 1 / M (M = 2^k <= 1024), g - s0 / M - z * s1 / M a multiple of 2^-10 below 600: exact in fp32 in either
    association and with or without fused multiply-adds.  A bf16 dz is that value rounded once."""
    _bwd_exact(shape, tname, dev, ("none", "own_relu"))


@pytest.mark.parametrize("tname", sorted(DTYPES))
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=_shape_id)
def test_bwd_exact_frozen(shape, tname, dev):
    """CS_BN_BWD_FROZEN alone and with CS_BN_BWD_OWN_RELU: dz = gamma * g needs no division, so any M is exact"""
    _bwd_exact(shape, tname, dev, ("frozen", "frozen_own_relu"))


# ---------------------------------------------------------------------------------------------------------------- b. mask
@pytest.mark.parametrize("tname", sorted(DTYPES))
@pytest.mark.parametrize("shape", MASK_SHAPES, ids=_shape_id)
def test_own_relu_mask_is_the_sign_of_the_forward_output(shape, tname, dev):
    """include/cellseg_hip.h: the mask of CS_BN_BWD_OWN_RELU is the sign of the layer's own output.  The forward (bn_apply_kernel) and
    the two backward kernels are compiled separately; where u = gamma * z + beta cancels, its sign is the sign of the product's
    rounding error if the multiply-add is fused and u is 0 if it is not, so the three agree only if they fuse alike.
    mean = 0, rstd = 1 (xhat = z exactly), gamma with a full fp32 mantissa, beta[c] = -fl32(z0[c] * gamma[c]), z = z0[c] on the even rows."""
    M, C = shape
    dtype = DTYPES[tname]
    g = torch.Generator().manual_seed(31 * M + C)
    gamma = torch.rand((C,), generator=g) + 0.5
    z0 = (torch.randn((C,), generator=g) * 1.3).to(dtype)
    beta = -(z0.float() * gamma)                                     # one fp32 multiply, rounded once
    z = (torch.randn((M, C), generator=g) * 1.3).to(dtype)
    z[::2] = z0
    zd, gd, bd = z.double(), gamma.double(), beta.double()
    resid = zd[0] * gd + bd                                          # exact in fp64: the rounding error of the fp32 product
    assert bool((resid > 0).any()) and bool((resid < 0).any())
    zero, one, ones = torch.zeros(C, device=dev), torch.ones(C, device=dev), torch.ones((M, C), dtype=dtype, device=dev)
    z_dev, gamma_dev, beta_dev = z.to(dev), gamma.to(dev), beta.to(dev)
    pos = (K.bn_apply(z_dev, zero, one, gamma_dev, beta_dev, act=RELU) > 0).cpu()
    cnt = pos.double().sum(0)
    s1 = (pos.double() * zd).sum(0)
    tol_s1 = SUM_RTOL * (pos.double() * zd.abs()).sum(0) + U32 * s1.abs() + 1e-9
    # running statistics: dz = gamma * [mask] with dy = 1, so dz != 0 IS the mask of cs_bn_bwd_apply; dbeta counts that of cs_bn_bwd_reduce
    dz, dgamma, dbeta = K.bn_bwd(ones, z_dev, zero, one, gamma_dev, True, beta=beta_dev, act=FROZEN | OWN_RELU)
    flips = int(((dz != 0).cpu() != pos).sum())
    assert flips == 0, "%d elements masked unlike the forward's output (frozen)" % flips
    _same_bits(dbeta, cnt)
    _within(dgamma, s1, tol_s1, "dgamma frozen")
    # batch statistics: the sums under the forward's mask, and dz from them
    dz, dgamma, dbeta = K.bn_bwd(ones, z_dev, zero, one, gamma_dev, True, beta=beta_dev, act=OWN_RELU)
    _same_bits(dbeta, cnt)
    _within(dgamma, s1, tol_s1, "dgamma train")
    gm = pos.double()
    k0, k1 = cnt / M, s1 / M
    want = gd * (gm - k0 - zd * k1)
    uT = UT[dtype]
    tol = uT * want.abs() + (1 + uT) * gd * (U32 * (8 * gm + 8 * k0.abs() + 9 * zd.abs() * k1.abs()) + zd.abs() * tol_s1 / M)
    _within(dz, want, tol, "dz train")


# ---------------------------------------------------------------------------------------------------------------- c. tolerance
_input_cache = {}


def _inputs(M, C, tname, dev):
    """tests/test_bn_reductions_gpu.py::_inputs + a residual, with two channels replaced: channel 1 is the constant 100 (var = 0,
    rstd = 1 / sqrt(eps), y = beta) and channel C - 2 has |mean| = 40 >> std = 0.5.  Rows are cast to the element type first: the fp64
    copies are the values the kernels read.  Also the library's own batch moments of z (cs_bn_stats + cs_bn_finalize)."""
    key = (M, C, tname)
    if _input_cache.get("key") != key:
        dtype = DTYPES[tname]
        g = torch.Generator().manual_seed(7 * M + C)
        z = torch.randn((M, C), generator=g) * 1.3 + 0.2
        dy = torch.randn((M, C), generator=g)
        gamma = torch.rand((C,), generator=g) + 0.5
        beta = torch.randn((C,), generator=g) * 0.1
        res = torch.randn((M, C), generator=g)
        z[:, 1] = 100.0
        z[:, C - 2] = 40.0 + 0.5 * torch.randn((M,), generator=g)
        rm = torch.randn((C,), generator=g)
        rv = torch.rand((C,), generator=g) + 0.5
        d = {"z": z.to(dtype), "dy": dy.to(dtype), "res": res.to(dtype), "gamma": gamma, "beta": beta, "rm": rm, "rv": rv}
        _input_cache.clear()
        _input_cache["key"] = key
        _input_cache["cpu"] = {k: v.double() for k, v in d.items()}
        _input_cache["dev"] = {k: v.to(dev) for k, v in d.items()}
        mean, rstd = K.bn_finalize(K.bn_stats(_input_cache["dev"]["z"]), M, EPS, MOMENTUM)
        _input_cache["dev"].update(mean=mean, rstd=rstd)
        _input_cache["cpu"].update(mean=mean.double().cpu(), rstd=rstd.double().cpu())
    return _input_cache["cpu"], _input_cache["dev"]


def _moment_bounds(zd, eps):
    """The fp64 moments of the rows and what the sums' bound leaves of them.  With |dS0| <= e0 = 2e-6 sum|z| and |dS1| <= e1 = 2e-6 sum z^2:
        mean = S0 / M                   |dmean| <= e0 / M
        var  = S1 / M - mean^2 (fp64)   |dvar|  <= e1 / M + 2 |mean| dmean + dmean^2 + 4 * 2^-53 * (S1 / M + mean^2), clamped at 0
        rstd = 1 / sqrt(var + eps)      in [1 / sqrt(var + eps + dvar), 1 / sqrt(max(var + eps - dvar, eps))]   (var >= 0: the clamp)
    the last as an interval because dvar need not be small against var + eps (a constant channel: var = 0 and only eps is left)."""
    M = zd.shape[0]
    mean, var, rstd = R.bn_moments(zd, eps)
    e0 = SUM_RTOL * zd.abs().sum(0) + 1e-9
    e1 = SUM_RTOL * (zd * zd).sum(0) + 1e-9
    dmean = e0 / M
    dvar = e1 / M + 2 * mean.abs() * dmean + dmean ** 2 + 4 * 2.0 ** -53 * ((zd * zd).sum(0) / M + mean ** 2)
    lo = 1.0 / torch.sqrt(var + eps + dvar)
    hi = 1.0 / torch.sqrt(torch.clamp(var + eps - dvar, min=eps))
    return mean, var, rstd, dmean, dvar, lo, hi


@pytest.mark.parametrize("tname", sorted(DTYPES))
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=_shape_id)
def test_finalize_against_fp64_moments(shape, tname, dev):
    """cs_bn_finalize: mean, rstd, and the running statistics blended with the UNBIASED variance (M == 1: the plain one), with and
    without running buffers.  Bounds: _moment_bounds for what the sums carry, + 4 u32 relative for the fp32 steps -- the cast, the
    addition of eps, sqrtf and the division for rstd (each of the first two counts half); (1 - momentum), two products and the sum for a
    blend, each term with the cast of what it blends in."""
    M, C = shape
    cpu, d = _inputs(M, C, tname, dev)
    zd = cpu["z"]
    stats = K.bn_stats(d["z"])
    mean, rstd = K.bn_finalize(stats, M, EPS, MOMENTUM)
    rm, rv = d["rm"].clone(), d["rv"].clone()
    mean_b, rstd_b = K.bn_finalize(stats, M, EPS, MOMENTUM, rm, rv)
    assert torch.equal(mean, mean_b) and torch.equal(rstd, rstd_b)
    assert torch.equal(mean, d["mean"]) and torch.equal(rstd, d["rstd"])
    mean_r, var_r, rstd_r, dmean, dvar, lo, hi = _moment_bounds(zd, EPS)
    _within(mean, mean_r, dmean + 4 * U32 * mean_r.abs(), "mean")
    got = rstd.double().cpu()
    print("rstd: interval width / rstd up to %.3g" % float(((hi - lo) / rstd_r).max()))
    assert bool((got >= lo * (1 - 4 * U32)).all()) and bool((got <= hi * (1 + 4 * U32)).all())
    rm_r, rv_r = R.bn_running(cpu["rm"], cpu["rv"], mean_r, var_r, M, MOMENTUM)
    unb = M / (M - 1.0) if M > 1 else 1.0
    _within(rm, rm_r, MOMENTUM * dmean + 4 * U32 * ((1 - MOMENTUM) * cpu["rm"].abs() + MOMENTUM * mean_r.abs()), "running_mean")
    _within(rv, rv_r, MOMENTUM * unb * dvar + 4 * U32 * ((1 - MOMENTUM) * cpu["rv"].abs() + MOMENTUM * unb * var_r), "running_var")
    # The constant channel.  Its partial sums are exact (100 k and 10000 k are integers below 2^24 for the few rows a thread adds), so
    # only fp64 roundings are left: mean = 100 (1 + d), |d| <= 2^-53, var <= 4 * 2^-53 * 1e4 against eps -- the interval above says
    # nothing there because the GENERAL bound of the sums exceeds eps.
    assert float(var_r[1]) == 0.0 and abs(float(rstd_r[1]) * np.sqrt(EPS) - 1.0) <= 1e-15
    assert abs(float(mean[1]) - 100.0) <= 100.0 * U32
    assert abs(float(rstd[1]) - float(rstd_r[1])) <= (4 * U32 + 0.5 * 4 * 2.0 ** -53 * 1e4 / EPS) * float(rstd_r[1])


def _fwd_bound(cpu, mean, rstd, res, act, uT, dmean=0.0, drstd=0.0):
    """|y - ref| <= uT |ref| + k u32 A,  A = |z - mean| rstd |gamma| + |beta| + |res|.  none / ReLU: k = 6 -- the subtraction, two
    products, the addition of beta (one rounding less if fused) and of the residual: five fp32 roundings, each of a partial result no
    larger than A, + one of slack; ReLU changes none of it.  SiLU: k = SILU_FWD_ULPS (measured, see the constants).
    Derived additions: the final rounding to the element type acts on the COMPUTED value (the factor 1 + uT), and where the moments
    are not the kernel's own (dmean, drstd: what the reference's moments may differ by) their error times the slope of the activation."""
    ref = R.bn_apply(cpu["z"], mean, rstd, cpu["gamma"], cpu["beta"], res, act)
    A = (cpu["z"] - mean).abs() * rstd * cpu["gamma"].abs() + cpu["beta"].abs() + (0.0 if res is None else res.abs())
    k = SILU_FWD_ULPS if act == SILU else 6.0
    slope = 1.1 if act == SILU else 1.0                    # max |silu'| = 1.0998
    stat = cpu["gamma"].abs() * (rstd * dmean + (cpu["z"] - mean).abs() * drstd)
    return ref, A, uT * ref.abs() + (1 + uT) * (k * U32 * A + slope * stat)


@pytest.mark.parametrize("tname", sorted(DTYPES))
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=_shape_id)
def test_apply_against_fp64(shape, tname, dev):
    """cs_bn_apply, none / ReLU / SiLU with and without residual, against the reference fed the kernel's own fp32 mean and rstd, so
    that only the arithmetic of this pass is measured (_fwd_bound).  The constant channel gives y = act(beta + res) up to the rounding
    of its mean."""
    M, C = shape
    dtype = DTYPES[tname]
    cpu, d = _inputs(M, C, tname, dev)
    for aname, act in (("none", NONE), ("relu", RELU), ("silu", SILU)):
        for rname, r_dev, r_ref in (("plain", None, None), ("res", d["res"], cpu["res"])):
            y = K.bn_apply(d["z"], d["mean"], d["rstd"], d["gamma"], d["beta"], residual=r_dev, act=act)
            ref, _, tol = _fwd_bound(cpu, cpu["mean"], cpu["rstd"], r_ref, act, UT[dtype])
            _within(y, ref, tol, "apply/%s/%s" % (aname, rname))
    # y = beta where the channel is constant: |z - mean_f| <= 100 u32 (the rounding of the mean; the subtraction is exact), times
    # rstd * |gamma| with two more roundings, + beta with one, + the rounding to the element type
    y = K.bn_apply(d["z"], d["mean"], d["rstd"], d["gamma"], d["beta"]).double().cpu()[:, 1]
    off = 100.0 * U32 * float(cpu["rstd"][1] * cpu["gamma"][1].abs())
    b = abs(float(cpu["beta"][1]))
    assert float((y - cpu["beta"][1]).abs().max()) <= UT[dtype] * (b + off) + (1 + UT[dtype]) * (off * (1 + 3 * U32) + U32 * (b + off))


@pytest.mark.parametrize("tname", sorted(DTYPES))
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=_shape_id)
def test_apply_stats_has_the_bits_of_finalize_then_apply(shape, tname, dev):
    """cs_bn_apply_stats == cs_bn_finalize + cs_bn_apply bit for bit: y, the saved mean / rstd and the running statistics
    (tests/test_efficientnet_gpu.py holds four bf16 shapes to this; here every decomposition and both element types)"""
    M, C = shape
    dtype = DTYPES[tname]
    _, d = _inputs(M, C, tname, dev)
    stats = K.bn_stats(d["z"])
    for act in (NONE, RELU, SILU):
        for res in (None, d["res"]):
            rm_a, rv_a, rm_b, rv_b = d["rm"].clone(), d["rv"].clone(), d["rm"].clone(), d["rv"].clone()
            mean, rstd = K.bn_finalize(stats, M, EPS, MOMENTUM, rm_a, rv_a)
            y_a = K.bn_apply(d["z"], mean, rstd, d["gamma"], d["beta"], residual=res, act=act)
            y_b, mean_b, rstd_b = K.bn_apply_stats(d["z"], stats, EPS, MOMENTUM, rm_b, rv_b, d["gamma"], d["beta"], residual=res, act=act)
            assert torch.equal(mean.view(torch.int32), mean_b.view(torch.int32)) and torch.equal(rstd.view(torch.int32), rstd_b.view(torch.int32))
            assert torch.equal(rm_a.view(torch.int32), rm_b.view(torch.int32)) and torch.equal(rv_a.view(torch.int32), rv_b.view(torch.int32))
            assert torch.equal(y_a.view(BITS[dtype]), y_b.view(BITS[dtype]))
            assert not torch.equal(rm_a, d["rm"]) and not torch.equal(rv_a, d["rv"])


def _bwd_bounds(cpu, mean, rstd, flags, uT, dmean=0.0, drstd=0.0):
    """Reference dz, dgamma, dbeta of rows_ref.bn_bwd and the bounds of the kernels' results.  xhat = (z - mean) rstd, u = gamma xhat + beta,
    g = dy through the layer's own ReLU / SiLU, s0 = sum g, s1 = sum g xhat, k0 = s0 / M, k1 = s1 / M.

    What the kernel's g may differ by (dg):
      OWN_RELU  the mask is decided in fp32: where |u| <= du = |gamma| dx + 2 u32 (|gamma xhat| + |beta|) (dx: the error of xhat, two
                roundings + the moments'; a product and a sum on top) either decision is right, dg = |dy| there.  (Exact
                cancellation is test_own_relu_mask_is_the_sign_of_the_forward_output's subject.)
      SiLU      SILU_BWD_ULPS u32 |dy| (S + A_u) (measured, see the constants) + |dy| / 2 * |gamma| * (moments' part of dx): silu'' <= 1/2.
    Sums: E0 = 2e-6 sum|g| + sum dg, E1 = 2e-6 sum|g xhat| + sum(dg |xhat| + |g| * moments' part of dx); dbeta and dgamma are the sums cast to
    fp32: + u32 |ref|.
    dz, FROZEN: gamma rstd g -- the product gamma * rstd and the product with g: uT |ref| + 3 u32 |ref| (one of slack) + |gamma rstd| dg
      + |gamma| drstd |g|.
    dz, batch statistics: gamma rstd (g - k0 - xhat k1):
      uT |ref| + u32 |gamma rstd| (8 |g| + 8 |k0| + 9 |xhat k1|)            fp32 roundings, counted below
      + |gamma rstd| (dg + E0 / M + |xhat| E1 / M + dxs |k1|)                what g, the sums and the moments carry
      + |gamma| drstd (|g| + |k0| + |xhat k1|).
      Roundings that reach a term: gamma * rstd and the final product (2) for all; the two subtractions for g (4 in all) and k0; the
      cast of the sum, 1 / M (a cast and a division) and the product with it for k0 (7 in all) and k1; xhat (2) and the product xhat * k1
      (one of the subtractions if fused) for the last: 9, one more than the eight the first two stay under.
    The final rounding to the element type acts on the computed value: the factor 1 + uT on everything but uT |ref|."""
    z, dy, gamma, beta = cpu["z"], cpu["dy"], cpu["gamma"], cpu["beta"]
    M = z.shape[0]
    u, xhat = R.bn_preact(z, mean, rstd, gamma, beta)
    g = R.bn_bwd_g(dy, u, flags)
    dz, dgamma, dbeta = R.bn_bwd(dy, z, mean, rstd, gamma, beta, flags)
    gr = (gamma * rstd).abs()
    A_u = (gamma * xhat).abs() + beta.abs()
    dxs = rstd * dmean + (z - mean).abs() * drstd
    dx = dxs + 2 * U32 * xhat.abs()
    dg = torch.zeros_like(g)
    if flags & OWN_RELU:
        amb = u.abs() <= gamma.abs() * dx + 2 * U32 * A_u
        print("own_relu: %d of %d elements within rounding of u = 0" % (int(amb.sum()), amb.numel()))
        dg = dg + dy.abs() * amb
    if (flags & 0xff) == SILU:
        sg = R.sigmoid(u)
        dg = dg + SILU_BWD_ULPS * U32 * dy.abs() * (sg * (1 + u.abs() * (1 - sg)) + A_u) + 0.5 * dy.abs() * gamma.abs() * dxs
    E0 = SUM_RTOL * g.abs().sum(0) + dg.sum(0) + 1e-9
    E1 = SUM_RTOL * (g * xhat).abs().sum(0) + (dg * xhat.abs() + g.abs() * dxs).sum(0) + 1e-9
    tol_dbeta = E0 + U32 * dbeta.abs()
    tol_dgamma = E1 + U32 * dgamma.abs()
    if flags & FROZEN:
        tol_dz = uT * dz.abs() + (1 + uT) * (3 * U32 * dz.abs() + gr * dg + gamma.abs() * drstd * g.abs())
    else:
        k0, k1 = (dbeta / M).abs(), (dgamma / M).abs()
        tol_dz = uT * dz.abs() + (1 + uT) * (U32 * gr * (8 * g.abs() + 8 * k0 + 9 * xhat.abs() * k1)
                                             + gr * (dg + E0 / M + xhat.abs() * E1 / M + dxs * k1)
                                             + gamma.abs() * drstd * (g.abs() + k0 + xhat.abs() * k1))
    return (dz, dgamma, dbeta), (tol_dz, tol_dgamma, tol_dbeta)


@pytest.mark.parametrize("fname", list(BWD_FLAGS))
@pytest.mark.parametrize("tname", sorted(DTYPES))
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=_shape_id)
def test_bwd_against_fp64(shape, tname, fname, dev):
    """cs_bn_bwd_reduce + cs_bn_bwd_apply under every flag combination functional.py produces (and FROZEN | SiLU, which carries the
    measured constant) against rows_ref.bn_bwd fed the kernel's own mean / rstd: _bwd_bounds."""
    M, C = shape
    dtype = DTYPES[tname]
    flags = BWD_FLAGS[fname]
    cpu, d = _inputs(M, C, tname, dev)
    got = K.bn_bwd(d["dy"], d["z"], d["mean"], d["rstd"], d["gamma"], True, beta=d["beta"], act=flags)
    want, tol = _bwd_bounds(cpu, cpu["mean"], cpu["rstd"], flags, UT[dtype])
    for name, a, b, t in zip(("dz", "dgamma", "dbeta"), got, want, tol):
        _within(a, b, t, "%s/%s" % (fname, name))


def silu_fwd_ulps(shape, dev):
    """the measured quantity behind SILU_FWD_ULPS on one shape, fp32 in and out"""
    cpu, d = _inputs(shape[0], shape[1], "f32", dev)
    worst = 0.0
    for r_dev, r_ref in ((None, None), (d["res"], cpu["res"])):
        y = K.bn_apply(d["z"], d["mean"], d["rstd"], d["gamma"], d["beta"], residual=r_dev, act=SILU)
        ref, A, _ = _fwd_bound(cpu, cpu["mean"], cpu["rstd"], r_ref, SILU, U32)
        worst = max(worst, float(((y.double().cpu() - ref).abs() / (U32 * A)).max()))
    return worst


def silu_bwd_ulps(shape, dev):
    """the measured quantity behind SILU_BWD_ULPS on one shape, fp32 in and out"""
    cpu, d = _inputs(shape[0], shape[1], "f32", dev)
    dz, _, _ = K.bn_bwd(d["dy"], d["z"], d["mean"], d["rstd"], d["gamma"], True, beta=d["beta"], act=FROZEN | SILU)
    u, xhat = R.bn_preact(cpu["z"], cpu["mean"], cpu["rstd"], cpu["gamma"], cpu["beta"])
    ref, _, _ = R.bn_bwd(cpu["dy"], cpu["z"], cpu["mean"], cpu["rstd"], cpu["gamma"], cpu["beta"], FROZEN | SILU)
    sg = R.sigmoid(u)
    scale = (cpu["gamma"] * cpu["rstd"] * cpu["dy"]).abs() * (sg * (1 + u.abs() * (1 - sg)) + (cpu["gamma"] * xhat).abs() + cpu["beta"].abs())
    return float(((dz.double().cpu() - ref).abs() / (U32 * scale + 1e-300)).max())


@pytest.mark.parametrize("shape", SILU_SHAPES, ids=_shape_id)
def test_silu_error_stays_under_the_measured_constants(shape, dev):
    fwd, bwd = silu_fwd_ulps(shape, dev), silu_bwd_ulps(shape, dev)
    print("SiLU error in u32 * scale: forward %.3f, backward %.3f" % (fwd, bwd))
    assert fwd <= SILU_FWD_ULPS and bwd <= SILU_BWD_ULPS


@pytest.mark.parametrize("tname", sorted(DTYPES))
@pytest.mark.parametrize("act", [NONE, RELU], ids=["none", "relu"])
@pytest.mark.parametrize("mode", ["train", "eval"])
def test_batch_norm_rows_against_the_module_in_fp64(mode, act, tname, dev):
    """functional.batch_norm_rows on nn.BatchNorm1d(520), M = 37, against the module itself in fp64 on the CPU: the forward, the input
    gradient, the parameter gradients and the running buffers.  The reference's moments are not the kernels' here, so the bounds of
    _fwd_bound / _bwd_bounds take what the moments may differ by: train() -- _moment_bounds + 4 u32; eval() -- the running mean is read
    as it is and rstd = 1 / sqrtf(var + eps) of cs_bn_fold is within 4 u32."""
    M, C = 37, 520
    dtype = DTYPES[tname]
    g = torch.Generator().manual_seed(41)
    bn = torch.nn.BatchNorm1d(C, eps=float(np.float32(1e-5)), momentum=MOMENTUM)
    with torch.no_grad():
        bn.weight.copy_(torch.rand((C,), generator=g) + 0.5)
        bn.bias.copy_(torch.randn((C,), generator=g) * 0.1)
        bn.running_mean.copy_(torch.randn((C,), generator=g) * 0.3)
        bn.running_var.copy_(torch.rand((C,), generator=g) + 0.5)
    ref = copy.deepcopy(bn).double()
    bn = bn.to(dev)
    bn.train(mode == "train")
    ref.train(mode == "train")
    x = (torch.randn((M, C), generator=g) * 1.3 + 0.2).to(dtype)
    dy = torch.randn((M, C), generator=g).to(dtype)
    cpu = {"z": x.double(), "dy": dy.double(), "gamma": ref.weight.detach().clone(), "beta": ref.bias.detach().clone()}
    rm0, rv0 = ref.running_mean.clone(), ref.running_var.clone()

    xr = x.double().requires_grad_(True)
    yr = ref(xr)
    yr = torch.relu(yr) if act == RELU else yr
    yr.backward(dy.double())
    xg = x.to(dev).requires_grad_(True)
    y = HF.batch_norm_rows(xg, bn, act)
    y.backward(dy.to(dev))
    assert y.dtype == dtype and xg.grad.dtype == dtype

    if mode == "train":
        mean, var, rstd, dmean, dvar, lo, hi = _moment_bounds(cpu["z"], bn.eps)
        drstd = torch.maximum(hi * (1 + 4 * U32) - rstd, rstd - lo * (1 - 4 * U32))
        dmean = dmean + 4 * U32 * mean.abs()
        unb = M / (M - 1.0)
        _within(bn.running_mean, ref.running_mean, MOMENTUM * dmean + 4 * U32 * ((1 - MOMENTUM) * rm0.abs() + MOMENTUM * mean.abs()), "running_mean")
        _within(bn.running_var, ref.running_var, MOMENTUM * unb * dvar + 4 * U32 * ((1 - MOMENTUM) * rv0.abs() + MOMENTUM * unb * var), "running_var")
        assert int(bn.num_batches_tracked) == 1
        flags = OWN_RELU if act == RELU else 0
    else:
        mean, rstd = rm0, 1.0 / torch.sqrt(rv0 + bn.eps)
        dmean, drstd = 0.0, 4 * U32 * rstd
        assert torch.equal(bn.running_mean.cpu().double(), rm0) and torch.equal(bn.running_var.cpu().double(), rv0)
        flags = FROZEN | (OWN_RELU if act == RELU else 0)
    uT = UT[dtype]
    fwd_ref, _, tol = _fwd_bound(cpu, mean, rstd, None, act, uT, dmean, drstd)
    assert float((fwd_ref - yr.detach()).abs().max()) <= 1e-12 * float(fwd_ref.abs().max())
    _within(y, yr.detach(), tol, "forward")
    want, tols = _bwd_bounds(cpu, mean, rstd, flags, uT, dmean, drstd)
    for name, a, b, w, t in zip(("dx", "dweight", "dbias"), (xg.grad, bn.weight.grad, bn.bias.grad), (xr.grad, ref.weight.grad, ref.bias.grad),
                                want, tols):
        assert float((w - b).abs().max()) <= 1e-12 * float(w.abs().max())           # rows_ref is the module (test_rows_ref_host.py)
        _within(a, b, t, name)


def test_batch_norm_rows_refuses_a_single_row_in_train_mode(dev):
    bn = torch.nn.BatchNorm1d(520).to(dev)
    x = torch.randn((1, 520), device=dev)
    with pytest.raises(ValueError):
        HF.batch_norm_rows(x, bn.train())
    assert HF.batch_norm_rows(x, bn.eval()).shape == (1, 520)


# ---------------------------------------------------------------------------------------------------------------- d. SE / StochasticDepth
SE_SHAPES = [(7, 1, 1, 8), (3, 7, 7, 48), (2, 19, 19, 1392), (2, 8, 8, 2136)]
WRAP_SHAPE = (5, 150, 150, 304)         # 4 275 000 eight-channel groups > 16384 workgroups x 256 threads: the grid-stride loop wraps


def _flat_ints(shape, seed, lo, hi):
    """fp32 tensor of integers in [lo, hi]: a hash of the flat index (mod 2^32 arithmetic)"""
    n = int(np.prod(shape))
    h = np.arange(n, dtype=np.uint32) * np.uint32(2654435761) + np.uint32((seed * 0x9E3779B1) & 0xFFFFFFFF)
    h ^= h >> np.uint32(15)
    h *= np.uint32(0x2C1B3C6D)
    h >>= np.uint32(12)
    return torch.from_numpy((h % np.uint32(hi - lo + 1)).astype(np.float32) + np.float32(lo)).view(*shape)


def _pow2(shape, seed):
    """+-2^k, k in [-2, 2]"""
    return torch.exp2(_flat_ints(shape, seed, -2, 2)) * (1 - 2 * _flat_ints(shape, seed + 1, 0, 1))


def _se_cases():
    cases = [(s, t) for s in SE_SHAPES for t in sorted(DTYPES)]
    return cases + [(WRAP_SHAPE, "bf16")]


def _case_id(c):
    return _shape_id(c[0]) + "-" + c[1]


def test_wrap_shape_exceeds_one_launch(dev):
    N, H, W, C = WRAP_SHAPE
    assert N * H * W * (C // 8) > 16384 * 256


@pytest.mark.parametrize("case", _se_cases(), ids=_case_id)
def test_se_scale_exact(case, dev):
    """y = x * s with x in [-8, 8] and s = +-2^k: multiples of 1/4 up to 32, exact in bf16"""
    (N, H, W, C), tname = case
    x = _flat_ints((N, H, W, C), 1, -8, 8).to(DTYPES[tname])
    s = _pow2((N, C), 2)
    _same_bits(K.se_scale(x.to(dev), s.to(dev)), R.se_scale(x, s))


@pytest.mark.parametrize("case", _se_cases(), ids=_case_id)
def test_se_scale_bwd_dx_exact(case, dev):
    """dx = dy * s + davg / HW.  davg = HW * k with k in [-4, 4] where HW is a power of two (the kernel multiplies by 1 / HW, exact only
    then): multiples of 1/4 up to 36; davg = None on every shape."""
    (N, H, W, C), tname = case
    dy = _flat_ints((N, H, W, C), 3, -8, 8).to(DTYPES[tname])
    s = _pow2((N, C), 4)
    dy_dev, s_dev = dy.to(dev), s.to(dev)
    _same_bits(K.se_scale_bwd_dx(dy_dev, s_dev, None), R.se_scale_bwd_dx(dy, s, None))
    HW = H * W
    if HW & (HW - 1) == 0:
        davg = _flat_ints((N, C), 6, -4, 4) * HW
        want = R.se_scale_bwd_dx(dy, s, davg)
        assert HW == 1 or not torch.equal(want, R.se_scale_bwd_dx(dy, s, davg * HW))
        _same_bits(K.se_scale_bwd_dx(dy_dev, s_dev, davg.to(dev)), want)


def test_se_scale_bwd_dx_has_a_power_of_two_case_with_davg():
    assert sum(1 for (N, H, W, C) in SE_SHAPES if (H * W) & (H * W - 1) == 0) >= 2


@pytest.mark.parametrize("case", _se_cases() + [(WRAP_SHAPE, "f32")], ids=_case_id)
def test_rowscale_add_exact(case, dev):
    """y = a * row_scale + b with a, b in [-8, 8] and row_scale in {0, +-2^k}: row_scale = None with b, b = None with row_scale, a 0 in
    row_scale (a dropped sample: y = b exactly)"""
    (N, H, W, C), tname = case
    a = _flat_ints((N, H, W, C), 7, -8, 8).to(DTYPES[tname])
    b = _flat_ints((N, H, W, C), 8, -8, 8).to(DTYPES[tname])
    rs = _pow2((N,), 9)
    rs[N // 2] = 0.0
    a_dev, b_dev, rs_dev = a.to(dev), b.to(dev), rs.to(dev)
    y = K.rowscale_add(a_dev, rs_dev, b_dev)
    _same_bits(y, R.rowscale_add(a, rs, b))
    assert torch.equal(y[N // 2].cpu(), b[N // 2])
    if (N, H, W, C) != WRAP_SHAPE:
        _same_bits(K.rowscale_add(a_dev, None, b_dev), R.rowscale_add(a, None, b))
        _same_bits(K.rowscale_add(a_dev, rs_dev, None), R.rowscale_add(a, rs, None))


@pytest.mark.parametrize("tname", sorted(DTYPES))
def test_se_and_rowscale_random_values(tname, dev):
    """one random-valued case per kernel: uT |ref| + 2 u32 * (sum of the magnitudes of the terms) -- a product and a sum reach each term;
    the davg term of cs_se_scale_bwd_dx carries one rounding more, that of 1 / HW itself (+ u32 |davg / HW|).  The rounding to the
    element type acts on the computed value: the factor 1 + uT."""
    dtype = DTYPES[tname]
    uT = UT[dtype]
    g = torch.Generator().manual_seed(43)
    N, H, W, C = 3, 7, 7, 48
    x = torch.randn((N, H, W, C), generator=g).to(dtype)
    dy = torch.randn((N, H, W, C), generator=g).to(dtype)
    s = torch.rand((N, C), generator=g)
    davg = torch.randn((N, C), generator=g) * H * W
    rs = torch.tensor([0.0, 1.25, 1.0 / 0.7])
    xd, dyd, sd = x.double(), dy.double(), s.double()[:, None, None, :]
    ref = R.se_scale(x, s)
    _within(K.se_scale(x.to(dev), s.to(dev)), ref, uT * ref.abs() + (1 + uT) * 2 * U32 * (xd * sd).abs(), "se_scale")
    ref = R.se_scale_bwd_dx(dy, s, davg)
    pooled = (davg.double()[:, None, None, :] / (H * W)).abs()
    tol = uT * ref.abs() + (1 + uT) * U32 * (2 * ((dyd * sd).abs() + pooled) + pooled)
    _within(K.se_scale_bwd_dx(dy.to(dev), s.to(dev), davg.to(dev)), ref, tol, "se_scale_bwd_dx")
    ref = R.rowscale_add(x, rs, dy)
    terms = (xd * rs.double().view(-1, 1, 1, 1)).abs() + dyd.abs()
    _within(K.rowscale_add(x.to(dev), rs.to(dev), dy.to(dev)), ref, uT * ref.abs() + (1 + uT) * 2 * U32 * terms, "rowscale_add")
