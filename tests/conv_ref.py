"""Host restatement (torch, fp64, CPU) of the convolution family the implicit-GEMM kernels serve, and the integer operand
generators of the exact tests.  Written from the operation's definition, one filter tap at a time:

    y[n][k][p][q]   = sum_{c,r,s} x[n][c][p*stride - pad + r][q*stride - pad + s] * w[k][c][r][s]
    dx[n][c][h][w]  = sum_{k,r,s} dy[n][k][p][q] * w[k][c][r][s]      over the (p, q) with p*stride - pad + r == h (same for w)
    dw[k][c][r][s]  = sum_{n,p,q} dy[n][k][p][q] * x[n][c][p*stride - pad + r][q*stride - pad + s]

Tensors are NCHW / KCRS like torch's; nothing here touches the GPU or the HIP library.

THE EXACT DOMAIN.  With small-integer operands a bf16 or fp32 MFMA product is exact, every fp32 partial sum is an integer, and while
all of them stay below 2^24 any accumulation order gives the same bits; an integer of magnitude <= 256 is stored exactly in bf16
(8 significand bits).  Inside that domain a kernel owes BIT EQUALITY with the fp64 result, and one mis-indexed tap, chunk, pixel or
tile tail changes an output integer.  `assert_exact_domain` checks, from the fp64 reference, that a case is inside it, so that a case
which leaves the domain fails loudly instead of passing (or failing) for the wrong reason."""
import torch
import torch.nn.functional as F

F64 = torch.float64
LIMIT = float(2 ** 24)        # integers of magnitude below this are exact in fp32, and so is their sum in any order
BF16_INT = 256.0              # integers (and half-integers) of magnitude up to this are exact in bf16
TILE_ROWS = 128               # most rows one workgroup folds into an fp32 partial sum of statistics / column sums


# ------------------------------------------------------------------------------------------------ operand generators
def ints(shape, lo, hi, g):
    """fp64 tensor of integers drawn uniformly from [lo, hi]"""
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).to(F64)


def activations(shape, g):
    return ints(shape, -4, 4, g)


def gradients(shape, g, for_wgrad=False):
    return ints(shape, -3, 3, g) if for_wgrad else ints(shape, -4, 4, g)


def sparse_pm1(shape, per_row, g):
    """[rows, ...] tensor with `per_row` entries of +-1 / +-2 per leading index, zeros elsewhere."""
    rows = shape[0]
    flat = int(torch.tensor(shape[1:]).prod())
    w = torch.zeros((rows, flat))
    for r in range(rows):
        idx = torch.randperm(flat, generator=g)[:per_row]
        w[r, idx] = torch.randint(1, 3, (per_row,), generator=g).float() * (torch.randint(0, 2, (per_row,), generator=g).float() * 2 - 1)
    return w.view(shape)


def fwd_filters(K, Cg, R, S, per_row, g):
    """[K][Cg][R][S]: `per_row` non-zeros per OUTPUT channel (the forward contracts over (c, r, s))"""
    return sparse_pm1((K, Cg, R, S), min(per_row, Cg * R * S), g).to(F64)


def dgrad_filters(K, C, R, S, per_row, g):
    """[K][C][R][S]: `per_row` non-zeros per INPUT channel (the data gradient contracts over (k, r, s))"""
    return sparse_pm1((C, K, R, S), min(per_row, K * R * S), g).permute(1, 0, 2, 3).contiguous().to(F64)


def dgrad_filters_grouped(C, Cg, R, S, per_row, g):
    """Conv2d(groups = C / Cg).weight layout [C][Cg][R][S], `per_row` non-zeros per INPUT channel: input channel grp*Cg + j is fed by
    the filters of output channels grp*Cg .. grp*Cg + Cg - 1 at their column j."""
    G = C // Cg
    t = sparse_pm1((C, Cg, R, S), min(per_row, Cg * R * S), g).to(F64)          # [input channel][output channel inside the group][r][s]
    return t.view(G, Cg, Cg, R, S).permute(0, 2, 1, 3, 4).reshape(C, Cg, R, S).contiguous()


# ------------------------------------------------------------------------------------------------ fp64 references
def out_extent(n, r, stride, pad):
    return (n + 2 * pad - r) // stride + 1


def _fwd1(x, w, stride, pad):
    N, C, H, W = x.shape
    K, _, R, S = w.shape
    P, Q = out_extent(H, R, stride, pad), out_extent(W, S, stride, pad)
    xp = F.pad(x, (pad, pad, pad, pad))
    y = torch.zeros((N, K, P, Q), dtype=F64)
    for r in range(R):
        for s in range(S):
            win = xp[:, :, r:r + stride * (P - 1) + 1:stride, s:s + stride * (Q - 1) + 1:stride]
            y += torch.einsum("ncpq,kc->nkpq", win, w[:, :, r, s])
    return y


def _dgrad1(dy, w, in_hw, stride, pad):
    N, K, P, Q = dy.shape
    _, C, R, S = w.shape
    H, W = in_hw
    dxp = torch.zeros((N, C, H + 2 * pad, W + 2 * pad), dtype=F64)
    for r in range(R):
        for s in range(S):
            dxp[:, :, r:r + stride * (P - 1) + 1:stride, s:s + stride * (Q - 1) + 1:stride] += torch.einsum("nkpq,kc->ncpq", dy, w[:, :, r, s])
    return dxp[:, :, pad:pad + H, pad:pad + W].contiguous()


def _wgrad1(x, dy, R, S, stride, pad):
    N, C, H, W = x.shape
    _, K, P, Q = dy.shape
    xp = F.pad(x, (pad, pad, pad, pad))
    dw = torch.zeros((K, C, R, S), dtype=F64)
    for r in range(R):
        for s in range(S):
            win = xp[:, :, r:r + stride * (P - 1) + 1:stride, s:s + stride * (Q - 1) + 1:stride]
            dw[:, :, r, s] = torch.einsum("nkpq,ncpq->kc", dy, win)
    return dw


def conv_fwd(x, w, stride, pad, groups=1, scale=None, shift=None, residual=None, relu=False):
    """relu(scale[k] * conv(x, w) + shift[k] + residual); w is [K][C / groups][R][S]"""
    x, w = x.to(F64), w.to(F64)
    if groups == 1:
        y = _fwd1(x, w, stride, pad)
    else:
        y = torch.cat([_fwd1(xg, wg, stride, pad) for xg, wg in zip(x.chunk(groups, 1), w.chunk(groups, 0))], dim=1)
    if scale is not None:
        y = y * scale.to(F64).view(1, -1, 1, 1)
    if shift is not None:
        y = y + shift.to(F64).view(1, -1, 1, 1)
    if residual is not None:
        y = y + residual.to(F64)
    return torch.relu(y) if relu else y


def conv_dgrad(dy, w, in_hw, stride, pad, groups=1, add=None, mask=None):
    """(conv_transpose(dy, w) + add) where mask else 0; `mask` is a bool tensor of dx's shape"""
    dy, w = dy.to(F64), w.to(F64)
    if groups == 1:
        dx = _dgrad1(dy, w, in_hw, stride, pad)
    else:
        dx = torch.cat([_dgrad1(dg, wg, in_hw, stride, pad) for dg, wg in zip(dy.chunk(groups, 1), w.chunk(groups, 0))], dim=1)
    if add is not None:
        dx = dx + add.to(F64)
    if mask is not None:
        dx = torch.where(mask, dx, torch.zeros_like(dx))
    return dx


def conv_wgrad(x, dy, R, S, stride, pad, groups=1):
    """[K][C / groups][R][S]"""
    x, dy = x.to(F64), dy.to(F64)
    if groups == 1:
        return _wgrad1(x, dy, R, S, stride, pad)
    return torch.cat([_wgrad1(xg, dg, R, S, stride, pad) for xg, dg in zip(x.chunk(groups, 1), dy.chunk(groups, 1))], dim=0)


def channel_stats(y):
    """per-channel sum and sum of squares of an NCHW tensor: fp64 [2][C]"""
    y = y.to(F64)
    return torch.stack([y.sum(dim=(0, 2, 3)), (y * y).sum(dim=(0, 2, 3))])


def column_sums(dx):
    return dx.to(F64).sum(dim=(0, 2, 3))


# ------------------------------------------------------------------------------------------------ the exact domain
def _is_multiple_of(t, unit):
    return bool((torch.round(t / unit) * unit == t).all())


def assert_exact_domain(stored=(), abs_sums=(), stats_of=None, colsum_of=None, half_integers=False):
    """The conditions under which a kernel owes bit equality with the fp64 reference (AssertionError otherwise):

    stored     fp64 tensors a kernel stores in the activation dtype: integers (multiples of 1/2 with `half_integers`, for a
               power-of-two scale below 1) of magnitude <= 256;
    abs_sums   fp64 tensors of sum |a| |b| over the contraction of every output (conv_fwd / conv_dgrad / conv_wgrad of the absolute
               values, plus |shift|, |residual|, |add| where fused): below 2^24, so that no partial sum in any order can round;
    stats_of   the stored tensor whose per-channel sum / sum of squares a launch accumulates: a workgroup folds up to 128 rows in
               fp32 (128 * max y^2 < 2^24); the totals are kept in exact fp64 accumulators;
    colsum_of  the stored data gradient whose column sums a launch accumulates: 128 * max |dx| < 2^24 per workgroup, and the total
               sum |dx| per channel < 2^24 because the folded result is an fp32 vector."""
    unit = 0.5 if half_integers else 1.0
    for t in stored:
        t = t.to(F64)
        assert _is_multiple_of(t, unit), "exact domain: a stored value is not an integer" + (" or half-integer" if half_integers else "")
        assert float(t.abs().max()) <= BF16_INT, f"exact domain: stored magnitude {float(t.abs().max())} > 256 is not exact in bf16"
    for t in abs_sums:
        assert float(t.to(F64).abs().max()) < LIMIT, f"exact domain: sum |a||b| = {float(t.abs().max())} reaches 2^24"
    if stats_of is not None:
        y = stats_of.to(F64)
        assert _is_multiple_of(y, unit), "exact domain: statistics of non-integers"
        assert TILE_ROWS * float((y * y).max()) < LIMIT, f"exact domain: 128 * max y^2 = {TILE_ROWS * float((y * y).max())} reaches 2^24"
    if colsum_of is not None:
        d = colsum_of.to(F64)
        assert _is_multiple_of(d, unit), "exact domain: column sums of non-integers"
        assert TILE_ROWS * float(d.abs().max()) < LIMIT, f"exact domain: 128 * max |dx| = {TILE_ROWS * float(d.abs().max())} reaches 2^24"
        assert float(d.abs().sum(dim=(0, 2, 3)).max()) < LIMIT, "exact domain: a column sum reaches 2^24 (fp32 result vector)"


# ------------------------------------------------------------------------------------------------ staged weight operands
def staged_operands(w, scale, dtype, Cp, Kp):
    """The plain staged operands of w[K][C][R][S] (fp32) from their definition, in torch on w's device: every element is the fp32
    product w * scale[k] (scale None: w itself) rounded once to `dtype`, laid out as w_khwc [Kp][R][S][Cp] and w_chwk [Cp][R][S][Kp]
    with exact zeros in the padding.  One IEEE multiplication and one round-to-nearest-even: a kernel owes the same bits."""
    K, C = w.shape[:2]
    v = (w if scale is None else w * scale[:, None, None, None]).to(dtype)
    v = F.pad(v, (0, 0, 0, 0, 0, Cp - C, 0, Kp - K))
    return v.permute(0, 2, 3, 1).contiguous(), v.permute(1, 2, 3, 0).contiguous()


def same_bits(a, b):
    """bit equality of two tensors of one dtype and element count (0.0 and -0.0 differ, equal NaN patterns agree)"""
    it = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return a.dtype == b.dtype and a.numel() == b.numel() and torch.equal(a.reshape(-1).view(it), b.reshape(-1).view(it))
