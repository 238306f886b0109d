"""GPU: the oldest kernels of the training path -- the 3x3 / stride 2 max pool and the global average + max pool of csrc/pool.hip, the
NCHW <-> NHWC transposes and the column sums of csrc/prep.hip, cross-entropy, class-1 probability and (weighted) MSE of csrc/head.hip --
against the plain fp64 references of tests/pool_ref.py, which tests/test_pool_ref_host.py holds to torch's own fp64 operators and
autograd.  The looser checks of tests/test_pool_head_topk_gpu.py stay; this file says whether the bits are right, at the edges of every
launch geometry: maps of one and two pixels, a second workgroup along the channels, row partitions and lanes without work, the
16-pixel main loop against its tail, the second and third 256-group chunk of the column sums, both sides of rows_per_block's change,
and every capped grid striding at least once.

Two kinds of test:
  a. exact     inputs chosen so that every intermediate is representable whatever order the kernel adds in and whatever the compiler
               fuses: integer-valued data with |v| <= 8 (bf16 holds it), sums below 2^24, divisors that are powers of two, gamma = 1.
               The kernel must give the reference's bits; a bf16 output is the exact value rounded once, to nearest even.  Index outputs
               (the max pool's tap plane, the global pool's arg max) are always compared exactly, under ATen's rule: strictly greater
               replaces, and so does a NaN -- the first of equal maxima and the LAST NaN of a scan win.  NaN outputs are compared as NaN
               (which NaN pattern a conversion produces is the hardware's decision, not these kernels').
  b. tolerance random data, with the bounds below.

Notation: u32 = 2^-24, the unit roundoff of fp32; uT that of the element type (2^-8 for bf16, u32 for fp32).  k roundings in sequence cost
g(k) = k u32 / (1 - k u32) of the magnitude they act on (Higham's gamma_k).  "then the element type's rounding" means that a bound B on the
fp32 value becomes B + uT (|ref| + B) for the stored bf16 value, and stays B for fp32.

  max pool backward      a sum of at most four dy, the first added to 0 exactly: g(3) * sum |dy taken|, then the element type's rounding.
  global pool forward    integer data: the sum is exact; s / HW and the addition of the maximum round once each; bound g(3) * (|mean| + |max|)
                         (one to spare; bit-equal when HW is a power of two).
  global pool backward   inv = 1 / HW, dfeat * inv, + dfeat: dfeat / HW carries two roundings and the sum one more,
                         |dfeat| (2 u32 / HW + u32 (1 + 1 / HW)) <= 2 u32 |dfeat| (1 + 1 / HW), then the element type's rounding.
  column sums            a sum of k terms in ANY order errs by at most g(k - 1) * sum |terms|.  A thread adds n = ceil(rows_per_block / rpar)
                         rows, the workgroup folds rpar threads, and the B workgroups' partial rows (or atomics, with `out` itself as one
                         more term) are folded last: every element passes through at most n + rpar + B additions, so
                         c = n + rpar + B (+ 1 when accumulating into `out`) and the bound is g(c) * sum |g| per channel, with n, rpar and B
                         worked out per shape by _colsum_depth() from the launch rule (70 for (300, 2048), 769 for (32768, 8)).
  MSE, unweighted        per row: x - t (its rounding counts twice: it is squared), the square, * inv and inv = 1 / M itself: g(5) of the
                         row's term; dx = 2 (x - t) inv: g(3).
  summation of a loss    per-thread chain of ceil(M / 524288) rows, six wave steps, three additions of the waves' sums, then the exact
                         accumulator: g(ceil(M / 524288) + 9) * sum |row terms|.

The bounds of cross-entropy, the class-1 probability and the weighted MSE rest on expf / logf of the device library, whose accuracy nobody
here had measured.  They are MEASURED: the largest error against the fp64 reference over every case of the test that uses the constant
(R.LOSS_M x R.LOSS_C x R.LOSS_GAMMA for the logit kinds, R.LOSS_M x mean / sum for the MSE), in units of
    CE loss      u32 * (gamma / M) * sum_rows (|lse| + |logit_label|)      (the summation term above is added on top in the test)
    CE dlogits   u32 * gamma / M            per element
    prob1        u32 * p1                   per element (+ one fp32 denormal step, 2^-149, as a floor)
    wMSE dx      u32 * |dx|                 per element;  wMSE loss  u32 * sum_rows |term|  (summation term added on top)
and the constant is four times the largest measured value, rounded up to a power of two -- never a value the kernel produced earlier
taken as truth.  Per logit kind, because the magnitude of the logits enters the exponentials' arguments (a row of +-80 logits carries
80 u32 into exp's argument): normal / spread / equal / decided.
Measured on an MI355X with the library of commit 5fcfe92 plus the arg-max merge fix of this change (csrc/head.hip is that commit's;
hipcc of ROCm 7.2, HIP 7.2.26015), the largest value over C in {2, 7} and gamma in {1, 0.7f} (over mean / sum for the MSE) at
M =                          1    255    256    257   1000   4096 524588
    CE loss    normal     0.63   0.24   0.51   0.24   0.24   0.29   0.28    4 * 0.63 = 2.5 -> 4
    CE loss    spread     0.86   0.45   0.46   0.54   0.39   0.22   0.45    4 * 0.86 = 3.5 -> 4
    CE loss    equal      0.57   0.95   0.20   0.16   0.20   0.21   0.53    4 * 0.95 = 3.8 -> 4
    CE loss    decided    0.00   1.27   0.81   1.38   0.66   0.22   0.86    4 * 1.38 = 5.5 -> 8
    CE dlogits normal     0.72   2.71   2.82   2.41   3.41   4.23   5.27    4 * 5.27 = 21.1 -> 32
    CE dlogits spread    20.15  56.20  57.35  59.44  61.05  61.77  64.61    4 * 64.61 = 258.4 -> 512
    CE dlogits equal      0.82   4.48   2.14   4.52   4.34   4.29   4.40    4 * 4.52 = 18.1 -> 32
    CE dlogits decided    0.00   0.99   0.00   0.44   0.80   0.00   0.49    4 * 0.99 = 4.0 -> 4
    prob1      normal     0.87   3.36   3.68   5.53   4.89   5.71   7.76    4 * 7.76 = 31.0 -> 32
    prob1      spread     1.69   2.73   2.31   2.12   2.46   2.57   3.66    4 * 3.66 = 14.6 -> 16
    prob1      equal      0.75   0.75   0.75   0.75   0.75   0.75   0.75    4 * 0.75 = 3.0 -> 4
    prob1      decided    0.00   0.00   0.00   0.00   0.00   0.00   0.00    4 * 0.00 = 0.0 -> 0
    wMSE dx               0.00   3.04   2.97   3.42   3.03   3.16   4.66    4 * 4.66 = 18.6 -> 32
    wMSE loss             0.00   0.97   0.77   0.67   1.26   0.51   0.62    4 * 1.26 = 5.1 -> 8
(decided p1 is exactly 0 or 1 on both sides: nothing to measure, the constant is 0 and only the denormal floor remains.)
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pool_ref as R
from cellsegmentation_amd import _lib
from cellsegmentation_amd import kernels as K

pytestmark = pytest.mark.gpu

DTYPES = R.DTYPES
U32 = 2.0 ** -24
UT = {torch.bfloat16: 2.0 ** -8, torch.float32: 2.0 ** -24}
GAMMAS = [float(np.float32(g)) for g in R.LOSS_GAMMA]          # the library takes gamma as a C float
DENORM = 2.0 ** -149

CE_LOSS_ULPS = {"normal": 4.0, "spread": 4.0, "equal": 4.0, "decided": 8.0}
CE_GRAD_ULPS = {"normal": 32.0, "spread": 512.0, "equal": 32.0, "decided": 4.0}
PROB1_ULPS = {"normal": 32.0, "spread": 16.0, "equal": 4.0, "decided": 0.0}
WMSE_GRAD_ULPS = 32.0
WMSE_LOSS_ULPS = 8.0


def g(k):
    return k * U32 / (1.0 - k * U32)


def _sid(s):
    return "x".join(str(v) for v in s)


def _gid(c):
    return "%dx%dx%d" % (c[0][0], c[0][1], c[1])


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _dev(t64, dtype, dev):
    return t64.to(dtype).contiguous().to(dev)


def _rounded(want64, dtype):
    """the fp64 reference rounded ONCE to `dtype`: fp32 directly; bf16 from the fp32 value, which must then hold the reference exactly"""
    w32 = want64.to(torch.float32)
    if dtype == torch.float32:
        return w32
    ok = (w32.double() == want64) | torch.isnan(want64)
    assert bool(ok.all()), "an exact test's reference is not representable in fp32"
    return torch.from_numpy(R.round_bf16_bits(w32.contiguous().numpy()).view(np.int16).copy()).view(torch.bfloat16)


def _same_bits(got, want64, what=""):
    """`got` holds the bits of the fp64 reference rounded once to its dtype (signed zeros and infinities included); NaN where it is NaN"""
    got = got.detach().cpu().contiguous()
    want = _rounded(want64.contiguous(), got.dtype)
    assert got.shape == want.shape, (got.shape, want.shape)
    it = torch.int16 if got.dtype == torch.bfloat16 else torch.int32
    nan = torch.isnan(want)
    bad = (torch.isnan(got) != nan) | (~nan & (got.view(it) != want.view(it)))
    if bool(bad.any()):
        idx = tuple(bad.nonzero()[0].tolist())
        raise AssertionError("%s: %d of %d elements differ, first at %s: got %r want %r"
                             % (what, int(bad.sum()), bad.numel(), idx, float(got[idx]), float(want[idx])))


def _same_ints(got, want, what=""):
    got, want = got.detach().cpu().to(torch.int64), want.to(torch.int64)
    assert got.shape == want.shape
    bad = got != want
    if bool(bad.any()):
        idx = tuple(bad.nonzero()[0].tolist())
        raise AssertionError("%s: %d of %d indices differ, first at %s: got %d want %d"
                             % (what, int(bad.sum()), bad.numel(), idx, int(got[idx]), int(want[idx])))


def _within(got, want64, tol, what):
    """finite elements within tol; infinities and NaN where the reference has them"""
    got = got.detach().double().cpu()
    fin = torch.isfinite(want64)
    assert torch.equal(got[~fin].nan_to_num(nan=12345.0), want64[~fin].nan_to_num(nan=12345.0)), what + ": non-finite elements differ"
    err = (got - want64).abs()[fin]
    tol = (tol + torch.zeros_like(want64))[fin]
    ratio = float((err / (tol + 1e-300)).max()) if err.numel() else 0.0
    print("%s: worst error / bound = %.3f" % (what, ratio))
    assert bool((err <= tol).all()), "%s: error up to %.3f x its bound (%d elements over)" % (what, ratio, int((err > tol).sum()))


def _stored(bound, ref64, dtype):
    """a bound on the fp32 value -> the bound on the value stored in `dtype`"""
    return bound if dtype == torch.float32 else bound + UT[dtype] * (ref64.abs() + bound)


def _signed_ints(shape, seed):
    """integers in +-[1, 8]"""
    return R.ints(shape, seed, 1, 8) * (1 - 2 * R.ints(shape, seed + 1, 0, 1))


def _normal(shape, seed, dtype):
    """random values already rounded to `dtype`, as fp64"""
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(shape)).to(dtype).double()


# ---------------------------------------------------------------------------------------------------------------- the lists reach the edges
def test_case_lists_reach_every_launch_edge():
    lib = _lib.load()
    assert 1 * 65 * 65 * (8000 // 8) > 16384 * 256 and 1 * 65 * 65 * 1000 > 16384 * 256            # max pool wrap: forward, backward
    assert 4100 * 4 * (2048 // 8) > 16384 * 256                                                     # global pool backward wrap
    assert 1500 * 1500 * 1 > 8192 * 256                                                             # both transposes
    assert max(R.LOSS_M) > 2048 * 256 + 256 and max(R.LOSS_M) < 2 * 2048 * 256                      # every workgroup strides, some twice
    assert lib.cs_colsum_partial_rows(32768) == 512 and lib.cs_colsum_partial_rows(32769) == (32769 + 64) // 65
    assert lib.cs_colsum_partial_rows(1) == 1 and lib.cs_colsum_partial_rows(65) == 2
    assert {C // 8 for _, C in R.COLSUM_SHAPES} >= {1, 3, 8, 65, 256, 257, 513}
    assert {C // 8 for _, C in R.GAP_SHAPES} >= {1, 9, 64, 65, 256}
    assert lib.cs_loss_words() == 16


# ---------------------------------------------------------------------------------------------------------------- max pool
_pool_cache = {}


def _pool_case(shape, kind):
    """x[N,H,W,C] fp64 with the reference's y and tap plane (both NHWC), computed once"""
    key = (shape, kind)
    if key not in _pool_cache:
        x = R.maxpool_input(shape, kind)
        y, tap = R.maxpool_fwd(_nchw(x))
        _pool_cache[key] = (x, _nhwc(y), _nhwc(tap))
    return _pool_cache[key]


@pytest.mark.parametrize("tname", sorted(DTYPES))
@pytest.mark.parametrize("shape", R.MAXPOOL_SHAPES, ids=_sid)
def test_maxpool_forward_bits_and_tap_plane(shape, tname, dev):
    """y bit-equal and the argmax plane byte for byte: post-ReLU ties, all-negative maps, windows of -inf, one and two NaNs per window"""
    dtype = DTYPES[tname]
    for kind in R.MAXPOOL_KINDS:
        x, y_ref, tap_ref = _pool_case(shape, kind)
        xd = _dev(x, dtype, dev)
        y, am = K.maxpool_fwd(xd)
        assert am.dtype == torch.uint8 and am.shape == y.shape
        _same_bits(y, y_ref, kind + " y")
        _same_ints(am, tap_ref, kind + " taps")
        y2, none = K.maxpool_fwd(xd, want_argmax=False)
        assert none is None
        _same_bits(y2, y_ref, kind + " y without the plane")
        if kind in ("nan1", "nan2") and shape[3] >= 3:
            assert bool(torch.isnan(y_ref).any())


@pytest.mark.parametrize("tname", sorted(DTYPES))
@pytest.mark.parametrize("shape", R.MAXPOOL_SHAPES, ids=_sid)
def test_maxpool_backward(shape, tname, dev):
    """integer dy: dx bit-equal in both dtypes, with and without the fused ReLU mask; random dy: within g(3) * sum |dy taken|"""
    N, H, W, C = shape
    dtype = DTYPES[tname]
    for kind in R.MAXPOOL_KINDS:
        x, y_ref, tap_ref = _pool_case(shape, kind)
        tap_nchw = _nchw(tap_ref)
        am = tap_ref.to(torch.uint8).to(dev)
        yd = _dev(y_ref, dtype, dev)
        dy = _signed_ints(tuple(y_ref.shape), 7)
        for mask_dev, mask_ref in ((None, None), (yd, _nchw(y_ref))):
            dx = K.maxpool_bwd(_dev(dy, dtype, dev), am, mask_dev, (H, W))
            _same_bits(dx, _nhwc(R.maxpool_bwd(_nchw(dy), tap_nchw, (H, W), mask_ref)), "%s dx, mask %s" % (kind, mask_dev is not None))
        if kind in ("relu", "negative"):
            dyr = _normal(tuple(y_ref.shape), 8, dtype)
            for mask_dev, mask_ref in ((None, None), (yd, _nchw(y_ref))):
                dx = K.maxpool_bwd(_dev(dyr, dtype, dev), am, mask_dev, (H, W))
                ref = _nhwc(R.maxpool_bwd(_nchw(dyr), tap_nchw, (H, W), mask_ref))
                mag = _nhwc(R.maxpool_bwd(_nchw(dyr.abs()), tap_nchw, (H, W), mask_ref))
                _within(dx, ref, _stored(g(3) * mag, ref, dtype), "%s dx of a random dy, mask %s" % (kind, mask_dev is not None))


def test_maxpool_grid_stride_wrap(dev):
    """(1, 130, 130, 8000) bf16: 65 * 65 * 1000 threads forward and backward, more than the 16384 workgroups of the capped grid hold.
    Integer data generated on the device; the reference of this one case is torch's own max_pool2d and autograd ON THE DEVICE (exact
    operations; tests/test_pool_ref_host.py ties them to pool_ref): y, the tap plane and dx bit-equal."""
    N, H, W, C = 1, 130, 130, 8000
    gen = torch.Generator(device=dev).manual_seed(5)
    x = torch.randint(-8, 9, (N, H, W, C), generator=gen, device=dev).to(torch.bfloat16)
    dy = (torch.randint(1, 9, (N, 65, 65, C), generator=gen, device=dev) * (1 - 2 * torch.randint(0, 2, (N, 65, 65, C), generator=gen, device=dev)))
    dy = dy.to(torch.bfloat16)
    y, am = K.maxpool_fwd(x)
    dx = K.maxpool_bwd(dy, am, None, (H, W))
    xr = x.permute(0, 3, 1, 2).float().requires_grad_(True)
    y_ref, ind = F.max_pool2d(xr, 3, 2, 1, return_indices=True)
    y_ref.backward(dy.permute(0, 3, 1, 2).float())
    kh = ind // W - (2 * torch.arange(65, device=dev)[:, None] - 1)
    kw = ind % W - (2 * torch.arange(65, device=dev)[None, :] - 1)
    assert torch.equal(y.float(), y_ref.detach().permute(0, 2, 3, 1))
    assert torch.equal(am.to(torch.int64), (kh * 3 + kw).permute(0, 2, 3, 1))
    assert torch.equal(dx.float(), xr.grad.permute(0, 2, 3, 1))
    assert float(dx.float().abs().max()) <= 32.0 and int((am > 0).sum()) > 0


# ---------------------------------------------------------------------------------------------------------------- global avg + max
_gap_last = [None, None]                  # the last (case, kind) and its map with the reference's results: one map at a time


def _gap_case(case, kind):
    if _gap_last[0] != (case, kind):
        x = R.gap_input(case[0], case[1], kind)
        _gap_last[:] = [(case, kind), (x,) + R.gap_fwd(x)]
    return _gap_last[1]


@pytest.mark.parametrize("tname", sorted(DTYPES))
@pytest.mark.parametrize("case", R.GAP_SHAPES, ids=_gid)
def test_gap_forward_feat_and_argmax(case, tname, dev):
    """the arg max exactly under the scan rule -- equal maxima in two row partitions in both orders, a constant channel, all-negative,
    -inf, one and two NaNs -- and feat: bit-equal when HW is a power of two, else within g(3) * (|mean| + |max|)"""
    (H, W), C = case
    HW = H * W
    dtype = DTYPES[tname]
    for kind in R.GAP_KINDS:
        x, feat_ref, idx_ref = _gap_case(case, kind)
        feat, am = K.gap_fwd(_dev(x, dtype, dev))
        assert feat.dtype == torch.float32 and am.dtype == torch.int32
        _same_ints(am, idx_ref, kind + " argmax")
        if HW & (HW - 1) == 0:
            _same_bits(feat, feat_ref, kind + " feat")
        else:
            v = x.reshape(R.GAP_N, HW, C)
            mag = v.mean(1).abs() + (feat_ref - v.mean(1)).abs()
            _within(feat, feat_ref, g(3) * mag.nan_to_num(nan=0.0, posinf=0.0, neginf=0.0), kind + " feat")


@pytest.mark.parametrize("tname", sorted(DTYPES))
@pytest.mark.parametrize("case", R.GAP_SHAPES, ids=_gid)
def test_gap_backward(case, tname, dev):
    """relu_mask off and on, with_max True and False; integer dfeat and HW a power of two: bit-equal; otherwise (and for a random dfeat)
    within 2 u32 |dfeat| (1 + 1 / HW), then the element type's rounding"""
    (H, W), C = case
    HW = H * W
    dtype = DTYPES[tname]
    for kind in ("relu", "ties"):
        x, _, idx_ref = _gap_case(case, kind)
        xd = _dev(x, dtype, dev)
        am = idx_ref.to(torch.int32).to(dev)
        for df, exact in ((_signed_ints((R.GAP_N, C), 9), HW & (HW - 1) == 0), (_normal((R.GAP_N, C), 10, torch.float32), False)):
            dfd = _dev(df, torch.float32, dev)
            for relu_mask in (False, True):
                for with_max in (True, False):
                    dx = K.gap_bwd(dfd, am if with_max else None, xd, relu_mask, with_max=with_max)
                    ref = R.gap_bwd(df, idx_ref, x, relu_mask, with_max)
                    what = "%s dx, relu_mask %s, with_max %s" % (kind, relu_mask, with_max)
                    if exact:
                        _same_bits(dx, ref, what)
                    else:
                        bound = 2.0 * U32 * df.abs()[:, None, None, :] * (1.0 + 1.0 / HW) + torch.zeros_like(ref)
                        _within(dx, ref, _stored(bound, ref, dtype), what)


def test_gap_grid_stride_wrap(dev):
    """(4100, 2, 2, 2048) bf16: the backward's 4100 * 4 * 256 threads exceed the capped grid.  Integer data generated on the device; the
    reference is plain torch operations ON THE DEVICE (sum, max, comparison: all exact for integers with HW = 4): feat, the arg max
    (first of equal maxima) and dx with the ReLU mask bit-equal."""
    N, HW, C = 4100, 4, 2048
    gen = torch.Generator(device=dev).manual_seed(6)
    x = torch.randint(-8, 9, (N, 2, 2, C), generator=gen, device=dev).to(torch.bfloat16)
    df = torch.randint(1, 9, (N, C), generator=gen, device=dev).float() * (1 - 2 * torch.randint(0, 2, (N, C), generator=gen, device=dev)).float()
    feat, am = K.gap_fwd(x)
    dx = K.gap_bwd(df, am, x, True)
    v = x.float().view(N, HW, C)
    mx = v.max(1).values
    p = torch.arange(HW, device=dev)[None, :, None]
    first = torch.where(v == mx[:, None, :], p, HW).min(1).values
    assert torch.equal(feat, v.sum(1) / HW + mx)
    assert torch.equal(am.to(torch.int64), first)
    ref = torch.where(v > 0, df[:, None, :] / HW + torch.where(p == first[:, None, :], df[:, None, :], torch.zeros_like(v)), torch.zeros_like(v))
    assert torch.equal(dx.float().view(N, HW, C), ref.to(torch.bfloat16).float())
    assert bool((ref.to(torch.bfloat16).float() == ref).all())             # representable: nothing was rounded on either side


# ---------------------------------------------------------------------------------------------------------------- layout
@pytest.mark.parametrize("case", R.TO_NHWC_CASES, ids=_sid)
def test_to_nhwc_bits_and_zero_padding(case, dev):
    """bit-equal: signed zeros, infinities, NaN, the largest finite fp32 (infinity in bf16), exact halfway cases of both parities; the
    padded channels (a whole group of them in (1, 20, 3, 3, 32)) are +0.0 patterns"""
    N, C, H, W, Cp, tname = case
    dtype = DTYPES[tname]
    x = R.layout_input(N, C, H, W, 11)
    y = K.to_nhwc(x.to(dev), dtype, Cp).cpu()
    want = R.to_nhwc(x, Cp, dtype)
    assert y.dtype == dtype and y.shape == want.shape
    it = torch.int16 if dtype == torch.bfloat16 else torch.int32
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(y), nan)
    assert torch.equal(y.view(it)[~nan], want.view(it)[~nan])
    if Cp > C:
        assert not bool((y[..., C:].contiguous().view(it) != 0).any())            # +0.0: not even a sign bit


@pytest.mark.parametrize("tname", sorted(DTYPES))
@pytest.mark.parametrize("case", R.TO_NCHW_CASES, ids=_sid)
def test_to_nchw_reads_no_padding_and_round_trips(case, tname, dev):
    """the padded input channels hold NaN: any read of them into the output shows; to_nchw(to_nhwc(x)) is x bit for bit in fp32.  (A bf16
    tensor with Cp = 4 is one cs_nchw_to_nhwc refuses to make, but cs_nhwc_to_nchw reads it like any other: the host reference makes it.)"""
    N, C, H, W, Cp = case
    dtype = DTYPES[tname]
    x = R.layout_input(N, C, H, W, 12)
    y = R.to_nhwc(x, Cp, dtype)
    y[..., C:] = float("nan")
    back = K.to_nchw(y.to(dev), C)
    assert back.dtype == torch.float32
    _same_bits(back, R.to_nchw(y, C), "to_nchw")
    if dtype == torch.float32:
        _same_bits(K.to_nchw(K.to_nhwc(x.to(dev), dtype, Cp), C), x.double(), "round trip")


def test_layout_grid_stride_wrap(dev):
    """1500 x 1500 pixels are 8790 workgroups, the grid holds 8192: (1, 3, 1500, 1500) -> Cp = 8 bf16 and (1, 1500, 1500, 8) bf16 -> C = 2,
    both against the host references"""
    x = torch.from_numpy(np.random.RandomState(13).standard_normal((1, 3, 1500, 1500)).astype(np.float32))
    y = K.to_nhwc(x.to(dev), torch.bfloat16, 8).cpu()
    assert torch.equal(y.view(torch.int16), R.to_nhwc(x, 8, torch.bfloat16).view(torch.int16))
    y[..., 2:] = float("nan")
    back = K.to_nchw(y.to(dev), 2).cpu()
    assert torch.equal(back.view(torch.int32), R.to_nchw(y, 2).float().view(torch.int32))


def test_layout_refusals(dev):
    x = torch.zeros((1, 9, 2, 2), device=dev)
    with pytest.raises(RuntimeError, match="bad extents"):
        K.to_nhwc(x, torch.bfloat16, 8)                       # Cp < C
    with pytest.raises(RuntimeError, match="bad extents"):
        K.to_nchw(torch.zeros((1, 2, 2, 8), device=dev), 9)
    with pytest.raises(RuntimeError, match="Cp must be a multiple of 8"):
        K.to_nhwc(x[:, :3].contiguous(), torch.bfloat16, 4)   # bf16 with Cp = 4
    assert K.to_nhwc(x[:, :3].contiguous(), torch.float32, 4).shape == (1, 2, 2, 4)


# ---------------------------------------------------------------------------------------------------------------- column sums
def _colsum_depth(M, C):
    """n + rpar + B of the header, from the launch rule of cs_colsum / cs_colsum_partial (csrc/prep.hip)"""
    rows_per_block = max(64, (M + 511) // 512)
    B = (M + rows_per_block - 1) // rows_per_block
    CG = C // 8
    worst = 0
    for cg0 in range(0, CG, 256):
        rpar = 256 // min(256, CG - cg0)
        worst = max(worst, -(-min(rows_per_block, M) // rpar) + rpar)
    return worst + B


def _colsum_paths(gd, out0, dev):
    """the three paths: partial rows + fold; atomics into a pre-filled `out`; the PartialColsum object"""
    M, C = gd.shape
    lib = _lib.load()
    a = K.colsum(gd)
    out = out0.to(torch.float32).to(dev)
    b = K.colsum(gd, out)
    assert b is out
    pc = K.colsum_partial(gd)
    assert pc.rows == lib.cs_colsum_partial_rows(M) and pc.n_out == C and tuple(pc.buf.shape) == (pc.rows, 2 * C)
    v1 = pc.vector()
    v2 = pc.vector()
    assert v1 is v2 and K.colsum_vector(pc) is v1
    assert a.dtype == torch.float32 and tuple(a.shape) == (C,)
    return a, b, v1


@pytest.mark.parametrize("tname", sorted(DTYPES))
@pytest.mark.parametrize("shape", R.COLSUM_SHAPES, ids=_sid)
def test_colsum_exact(shape, tname, dev):
    """integer data, M * 8 < 2^24: bit-equal on all three paths, `out` accumulated into"""
    M, C = shape
    gi = R.ints(shape, 21, -8, 8)
    out0 = _signed_ints((C,), 22)
    assert M * 8 + 8 < 2 ** 24 and _colsum_depth(M, C) >= 3
    a, b, v = _colsum_paths(_dev(gi, DTYPES[tname], dev), out0, dev)
    ref = R.colsum(gi)
    _same_bits(a, ref, "colsum")
    _same_bits(b, ref + out0, "colsum into out")
    _same_bits(v, ref, "colsum_partial")


@pytest.mark.parametrize("tname", sorted(DTYPES))
@pytest.mark.parametrize("shape", R.COLSUM_SHAPES, ids=_sid)
def test_colsum_tolerance(shape, tname, dev):
    """random data: g(n + rpar + B) * sum |g| per channel (+ 1 and |out| when accumulating)"""
    M, C = shape
    gr = _normal(shape, 23, DTYPES[tname])
    out0 = _normal((C,), 24, torch.float32)
    a, b, v = _colsum_paths(_dev(gr, DTYPES[tname], dev), out0, dev)
    ref, mag, c = R.colsum(gr), R.colsum(gr.abs()), _colsum_depth(M, C)
    _within(a, ref, g(c) * mag, "colsum")
    _within(b, ref + out0, g(c + 1) * (mag + out0.abs()), "colsum into out")
    _within(v, ref, g(c) * mag, "colsum_partial")


# ---------------------------------------------------------------------------------------------------------------- cross-entropy, prob1
def _sum_depth(M):
    return -(-M // 524288) + 9


def _measure(name, kind, shape, value):
    """the figure the constants of the header were taken from, printed before anything is asserted"""
    print("MEASURE %s %s %s %.4f" % (name, kind, _sid(shape), value))


@pytest.mark.parametrize("C", R.LOSS_C)
@pytest.mark.parametrize("M", [m for m in R.LOSS_M if m & (m - 1) == 0])
def test_softmax_ce_decided_rows_exact(M, C, dev):
    """integer logits, one class leading by 105 .. 120: every other exponential is 0 in fp32, lse is the leading logit exactly, the
    row's loss an integer (0 where the label leads) -- with M a power of two and gamma = 1 the loss and the gradient are bit-equal, and
    the exact accumulator behind the loss has summed M / 256 workgroups' contributions"""
    z, lab = R.logits_input(M, C, "decided", 100 * C + 7)
    loss_ref, dl_ref = R.softmax_ce(z, lab, 1.0)
    assert float(loss_ref) * M == round(float(loss_ref) * M) and (M < 4 or float(loss_ref) > 0)
    loss, dl = K.softmax_ce(z.to(dev), lab.to(dev), 1.0)
    _same_bits(loss, loss_ref.reshape(1), "loss")
    _same_bits(dl, dl_ref, "dlogits")
    loss2, none = K.softmax_ce(z.to(dev), lab.to(dev), 1.0, want_grad=False)
    assert none is None
    _same_bits(loss2, loss_ref.reshape(1), "loss without the gradient")
    p1 = K.softmax_prob1(z.to(dev))
    _same_bits(p1, R.softmax_prob1(z), "p1")


@pytest.mark.parametrize("C", R.LOSS_C)
@pytest.mark.parametrize("M", R.LOSS_M)
def test_softmax_ce_and_prob1_tolerance(M, C, dev):
    """every logit kind and gamma: the loss, dlogits and p1 within the measured constants of the header; want_grad=False returns None and
    the same loss bits"""
    for kind in R.LOGIT_KINDS:
        z, lab = R.logits_input(M, C, kind, 100 * C + 7)
        zd, labd = z.to(dev), lab.to(dev)
        lse = R.log_sum_exp(z)
        picked = z.double()[torch.arange(M), lab]
        for gamma in GAMMAS:
            loss_ref, dl_ref = R.softmax_ce(z, lab, gamma)
            loss, dl = K.softmax_ce(zd, labd, gamma)
            loss2, none = K.softmax_ce(zd, labd, gamma, want_grad=False)
            assert none is None and torch.equal(loss.view(torch.int32), loss2.view(torch.int32))
            unit = U32 * (gamma / M) * float((lse.abs() + picked.abs()).sum())
            summ = g(_sum_depth(M)) * (gamma / M) * float((lse - picked).abs().sum())
            err = abs(float(loss.double().cpu()) - float(loss_ref))
            _measure("ce_loss", kind, (M, C), err / (unit + 1e-300))
            gerr = (dl.double().cpu() - dl_ref).abs()
            _measure("ce_grad", kind, (M, C), float(gerr.max()) / (U32 * gamma / M))
            assert err <= CE_LOSS_ULPS[kind] * unit + summ, "%s gamma %g: loss off by %.3g, bound %.3g" % (kind, gamma, err, CE_LOSS_ULPS[kind] * unit + summ)
            _within(dl, dl_ref, torch.full_like(dl_ref, CE_GRAD_ULPS[kind] * U32 * gamma / M), "%s gamma %g dlogits" % (kind, gamma))
        p1_ref = R.softmax_prob1(z)
        p1 = K.softmax_prob1(zd)
        perr = (p1.double().cpu() - p1_ref).abs()
        _measure("prob1", kind, (M, C), float(((perr - DENORM).clamp(min=0) / (U32 * p1_ref + 1e-300)).max()))
        _within(p1, p1_ref, PROB1_ULPS[kind] * U32 * p1_ref + DENORM, kind + " p1")


# ---------------------------------------------------------------------------------------------------------------- MSE
@pytest.mark.parametrize("M", R.LOSS_M)
def test_mse_unweighted_exact(M, dev):
    """integer x and t: the sum for any M (every workgroup of the capped grid strides at 524588), the mean for M a power of two --
    loss and dx bit-equal; want_grad=False: None and the same bits"""
    x, t = R.ints((M,), 31, -8, 8), R.ints((M,), 32, -8, 8)
    xd, td = _dev(x, torch.float32, dev), _dev(t, torch.float32, dev)
    for mean in ([False, True] if M & (M - 1) == 0 else [False]):
        loss_ref, dx_ref = R.mse(x, t, False, mean)
        loss, dx = K.mse(xd, td, weighted=False, mean=mean)
        _same_bits(loss, loss_ref.reshape(1), "loss, mean %s" % mean)
        _same_bits(dx, dx_ref, "dx, mean %s" % mean)
        loss2, none = K.mse(xd, td, weighted=False, mean=mean, want_grad=False)
        assert none is None
        _same_bits(loss2, loss_ref.reshape(1), "loss without the gradient")


@pytest.mark.parametrize("M", R.LOSS_M)
def test_mse_tolerance(M, dev):
    """counts with targets 0, 19.999, 20 and 1e4 among them, weighted on / off, mean on / off"""
    x64, t64 = R.mse_input(M, 3 * M + 1)
    x, t = x64.float(), t64.float()
    assert M < 4 or {0.0, 20.0, 1e4} <= set(t.tolist()[:11])
    xd, td = x.to(dev), t.to(dev)
    for weighted in (False, True):
        for mean in (True, False):
            loss_ref, dx_ref = R.mse(x, t, weighted, mean)
            loss, dx = K.mse(xd, td, weighted=weighted, mean=mean)
            terms = float((R.mse_weights(t, weighted) * (x.double() - t.double()) ** 2).sum()) * (1.0 / M if mean else 1.0)
            err = abs(float(loss.double().cpu()) - float(loss_ref))
            what = "weighted %s mean %s" % (weighted, mean)
            if weighted:
                gerr = (dx.double().cpu() - dx_ref).abs()
                _measure("wmse_grad", "all", (M,), float((gerr / (U32 * dx_ref.abs() + 1e-300)).max()))
                _measure("wmse_loss", "all", (M,), err / (U32 * terms + 1e-300))
                _within(dx, dx_ref, WMSE_GRAD_ULPS * U32 * dx_ref.abs(), what + " dx")
                bound = (WMSE_LOSS_ULPS * U32 + g(_sum_depth(M))) * terms
            else:
                _within(dx, dx_ref, g(3) * dx_ref.abs(), what + " dx")
                bound = (g(5) + g(_sum_depth(M))) * terms
            assert err <= bound, "%s: loss off by %.3g, bound %.3g" % (what, err, bound)


def test_weight_rule_boundary_at_twenty(dev):
    """w = ln t from t = 20 on, w = t below: with x = t + 1 the row's loss IS its weight and dx is twice it.  Bound: x = fl(t + 1) is
    off by at most half a unit in the last place of [16, 32), D = 2^-20, and x - t is then exact, so d = 1 + e with |e| <= D: d^2 is
    within 2 D (1 + D) of 1 and d within D, relative to the weight; logf and the products add the measured WMSE_LOSS_ULPS / WMSE_GRAD_ULPS
    u32 of the header (one row: nothing is summed)."""
    D = 2.0 ** -20
    t = torch.tensor([19.0, 19.999, 20.0, 20.000002, 21.0], dtype=torch.float32)
    for i in range(len(t)):
        loss, dx = K.mse((t[i:i + 1] + 1.0).to(dev), t[i:i + 1].to(dev), weighted=True, mean=False)
        w = float(t[i]) if float(t[i]) < 20.0 else math.log(float(t[i]))
        assert abs(float(loss.cpu()) - w) <= (2.0 * D * (1.0 + D) + WMSE_LOSS_ULPS * U32) * w, (float(t[i]), float(loss.cpu()), w)
        assert abs(float(dx.cpu()) - 2.0 * w) <= (D + WMSE_GRAD_ULPS * U32) * 2.0 * w, (float(t[i]), float(dx.cpu()), w)


# ---------------------------------------------------------------------------------------------------------------- the accumulator's flag and range
def test_non_finite_inputs_give_a_nan_loss_and_the_next_call_is_clean(dev):
    """one NaN logit / one NaN in x sets the sticky flag of the exact accumulator: the loss reads NaN.  The accumulator is cleared by
    every call: the same clean data gives the same clean bits afterwards."""
    M = 1000
    z, lab = R.logits_input(M, 7, "normal", 41)
    zd, labd = z.to(dev), lab.to(dev)
    clean, _ = K.softmax_ce(zd, labd, 1.0)
    clean = clean.clone()
    bad = z.clone()
    bad[777, 3] = float("nan")
    loss, _ = K.softmax_ce(bad.to(dev), labd, 1.0)
    assert math.isnan(float(loss.cpu()))
    again, _ = K.softmax_ce(zd, labd, 1.0)
    assert torch.equal(again.view(torch.int32), clean.view(torch.int32)) and math.isfinite(float(again.cpu()))
    x64, t64 = R.mse_input(M, 42)
    xd, td = x64.float().to(dev), t64.float().to(dev)
    clean, _ = K.mse(xd, td, weighted=True)
    clean = clean.clone()
    bad = x64.float().clone()
    bad[300] = float("nan")
    loss, _ = K.mse(bad.to(dev), td, weighted=True)
    assert math.isnan(float(loss.cpu()))
    again, _ = K.mse(xd, td, weighted=True)
    assert torch.equal(again.view(torch.int32), clean.view(torch.int32)) and math.isfinite(float(again.cpu()))


def test_large_finite_loss_inside_the_accumulator_s_range(dev):
    """x = 2^15, t = 0, 1000 rows summed: 2^30 per row, 2^38 per workgroup -- below the 2^40 a contribution may reach (cs_common.h) --
    and 1000 * 2^30 in all, exactly"""
    M = 1000
    x = torch.full((M,), 32768.0)
    loss, dx = K.mse(x.to(dev), torch.zeros(M, device=dev), weighted=False, mean=False)
    assert float(loss.cpu()) == 1000.0 * 2.0 ** 30
    assert bool((dx.cpu() == 65536.0).all())
