"""Plain fp64 references (CPU, torch) of the oldest kernels of the training path: the 3x3 / stride 2 / pad 1 max pool and the global
average + max pool of csrc/pool.hip, the boundary transposes and the column sums of csrc/prep.hip, and the cross-entropy, class-1
probability and (weighted) MSE of csrc/head.hip.  Written from the rules stated in those files, not from torch's operators:
tests/test_pool_ref_host.py holds them to torch's own fp64 operators and autograd, tests/test_pool_loss_ref_gpu.py holds the kernels to
them.

Every function takes tensors of any float dtype, computes in float64 and returns float64 (indices as int64); only to_nhwc returns the
element type it was asked for, since its rounding is what it specifies.  The pooling scan rule is ATen's: the first element seeds the
maximum, a later one replaces it when it is STRICTLY greater or when it is NaN -- so the first of equal maxima wins and the LAST NaN in
scan order wins."""
import numpy as np
import torch


def _d(t):
    return None if t is None else t.detach().to(torch.float64).cpu()


# ---------------------------------------------------------------------------------------------------------------- max pool 3x3 / 2 / 1
def pool_out(n):
    return (n + 2 - 3) // 2 + 1


def _tap_rows(n_in, n_out, k):
    """input coordinate 2 * o - 1 + k of every output coordinate o, and whether it lies inside the map"""
    i = 2 * torch.arange(n_out) - 1 + k
    return i.clamp(0, n_in - 1), (i >= 0) & (i < n_in)


def maxpool_fwd(x_nchw):
    """y[N,C,P,Q] and the tap kh * 3 + kw (0..8) that supplied it: the nine taps in row-major order, taps outside the map skipped."""
    x = _d(x_nchw)
    N, C, H, W = x.shape
    P, Q = pool_out(H), pool_out(W)
    y = torch.zeros((N, C, P, Q), dtype=torch.float64)
    tap = torch.zeros((N, C, P, Q), dtype=torch.int64)
    seeded = torch.zeros((P, Q), dtype=torch.bool)
    for kh in range(3):
        iy, vy = _tap_rows(H, P, kh)
        for kw in range(3):
            ix, vx = _tap_rows(W, Q, kw)
            v = x[:, :, iy][:, :, :, ix]
            valid = vy[:, None] & vx[None, :]
            take = valid & (~seeded | (v > y) | torch.isnan(v))
            y = torch.where(take, v, y)
            tap = torch.where(take, torch.full_like(tap, kh * 3 + kw), tap)
            seeded = seeded | valid
    assert bool(seeded.all())                  # the centre tap of every window is inside the map
    return y, tap


def maxpool_bwd(dy, tap, in_hw, y_mask=None):
    """dx[N,C,H,W]: every window adds its dy to the pixel its tap names.  y_mask: dy is first zeroed where y_mask <= 0 (the ReLU that
    precedes the pool, commuted past it)."""
    g = _d(dy)
    if y_mask is not None:
        g = torch.where(_d(y_mask) > 0, g, torch.zeros_like(g))
    N, C, P, Q = g.shape
    H, W = in_hw
    dx = torch.zeros((N, C, H, W), dtype=torch.float64)
    for kh in range(3):
        for kw in range(3):
            sel = torch.where(tap == kh * 3 + kw, g, torch.zeros_like(g))
            for p in range(P):
                iy = 2 * p - 1 + kh
                if iy < 0 or iy >= H:
                    continue
                for q in range(Q):
                    ix = 2 * q - 1 + kw
                    if ix < 0 or ix >= W:
                        continue
                    dx[:, :, iy, ix] += sel[:, :, p, q]
    return dx


# ---------------------------------------------------------------------------------------------------------------- global avg + max
def gap_fwd(x):
    """x[N,H,W,C] -> feat[N,C] = mean + max over the H * W pixels, and the flat pixel index h * W + w of the maximum under one
    sequential scan p = 0 .. HW - 1 with the rule above."""
    x = _d(x)
    N, H, W, C = x.shape
    HW = H * W
    v = x.reshape(N, HW, C)
    s = torch.zeros((N, C), dtype=torch.float64)
    best = v[:, 0].clone()
    idx = torch.zeros((N, C), dtype=torch.int64)
    for p in range(HW):
        s = s + v[:, p]
        if p:
            take = (v[:, p] > best) | torch.isnan(v[:, p])
            best = torch.where(take, v[:, p], best)
            idx = torch.where(take, torch.full_like(idx, p), idx)
    return s / HW + best, idx


def gap_bwd(dfeat, argmax, x, relu_mask, with_max):
    """dx[N,H,W,C] = dfeat / HW at every pixel, + dfeat at the pixel argmax names (with_max); relu_mask: zero where x <= 0 (or NaN)."""
    g, x = _d(dfeat), _d(x)
    N, H, W, C = x.shape
    HW = H * W
    dx = (g / HW)[:, None, :].expand(N, HW, C).clone()
    if with_max:
        hit = torch.arange(HW)[None, :, None] == argmax.cpu().to(torch.int64)[:, None, :]
        dx = dx + torch.where(hit, g[:, None, :].expand(N, HW, C), torch.zeros_like(dx))
    dx = dx.reshape(N, H, W, C)
    if relu_mask:
        dx = torch.where(x > 0, dx, torch.zeros_like(dx))
    return dx


# ---------------------------------------------------------------------------------------------------------------- layout
def round_bf16_bits(x32):
    """uint16 patterns of fp32 values rounded to bfloat16, to nearest, ties to even, on the bits (numpy): add 0x7fff + the lowest kept
    bit, keep the upper half.  A NaN becomes the quiet NaN 0x7fc0 with its sign."""
    u = np.ascontiguousarray(x32, dtype=np.float32).view(np.uint32)
    r = ((u.astype(np.uint64) + 0x7FFF + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint64(16)).astype(np.uint16)
    nan = np.isnan(x32)
    return np.where(nan, ((u >> np.uint32(16)) & np.uint32(0x8000)).astype(np.uint16) | np.uint16(0x7FC0), r)


def to_nhwc(x, Cp, dtype):
    """x[N,C,H,W] fp32 -> [N,H,W,Cp] of `dtype`: channels C .. Cp - 1 are +0.0, bf16 values are rounded once (round_bf16_bits)."""
    x = x.detach().cpu()
    assert x.dtype == torch.float32 and Cp >= x.shape[1]
    N, C, H, W = x.shape
    y = torch.zeros((N, H, W, Cp), dtype=torch.float32)
    y[..., :C] = x.permute(0, 2, 3, 1)
    if dtype == torch.float32:
        return y
    assert dtype == torch.bfloat16
    bits = round_bf16_bits(y.numpy())
    return torch.from_numpy(bits.view(np.int16).copy()).view(torch.bfloat16)


def to_nchw(y, C):
    """y[N,H,W,Cp] -> [N,C,H,W]: the first C channels; nothing of the padding is read."""
    return _d(y[..., :C]).permute(0, 3, 1, 2).contiguous()


# ---------------------------------------------------------------------------------------------------------------- column sums
def colsum(g):
    """out[c] = sum over every leading index of g[..., c]"""
    g = _d(g)
    return g.reshape(-1, g.shape[-1]).sum(0)


# ---------------------------------------------------------------------------------------------------------------- losses
def log_sum_exp(logits):
    z = _d(logits)
    mx = z.max(dim=1, keepdim=True).values
    return (mx + torch.log(torch.exp(z - mx).sum(dim=1, keepdim=True))).squeeze(1)


def softmax_ce(logits, labels, gamma):
    """loss = gamma / M * sum_m (lse_m - logit[m, label_m]) and dlogits = gamma / M * (exp(logit - lse) - onehot)."""
    z = _d(logits)
    M, C = z.shape
    lab = labels.detach().cpu().to(torch.int64)
    lse = log_sum_exp(z)
    picked = z[torch.arange(M), lab]
    loss = (lse - picked).sum() * (gamma / M)
    onehot = torch.zeros_like(z)
    onehot[torch.arange(M), lab] = 1.0
    return loss, (torch.exp(z - lse[:, None]) - onehot) * (gamma / M)


def softmax_prob1(logits):
    """the probability of class 1"""
    z = _d(logits)
    return torch.exp(z[:, 1] - log_sum_exp(z))


def mse_weights(t, weighted):
    """w = ln t where t >= 20, else w = t (the rule of the reference's weighted count loss); unweighted: 1"""
    t = _d(t)
    if not weighted:
        return torch.ones_like(t)
    return torch.where(t >= 20, torch.log(t.clamp(min=1.0)), t)


def mse(x, t, weighted, mean):
    """loss = sum w (x - t)^2 (/ M with mean) and dx = 2 w (x - t) (/ M)."""
    x, t = _d(x), _d(t)
    w = mse_weights(t, weighted)
    inv = 1.0 / x.numel() if mean else 1.0
    d = x - t
    return (w * d * d).sum() * inv, 2.0 * w * d * inv


# ---------------------------------------------------------------------------------------------------------------- shared cases
# The shape lists and the designed inputs of tests/test_pool_ref_host.py (references against torch, CPU) and
# tests/test_pool_loss_ref_gpu.py (kernels against the references): one definition, so both files see the same maps.
MAXPOOL_SHAPES = [(1, 1, 1, 8), (1, 1, 2, 8), (2, 2, 1, 8), (1, 2, 2, 16), (2, 3, 3, 8), (1, 4, 5, 24), (2, 7, 9, 16), (3, 15, 14, 40),
                  (1, 10, 10, 64)]                                                     # (N, H, W, C)
MAXPOOL_KINDS = ["relu", "negative", "neginf", "nan1", "nan2"]
GAP_N = 2
GAP_SHAPES = [((1, 1), 8), ((1, 2), 72), ((1, 3), 8), ((2, 2), 512), ((1, 5), 520), ((3, 4), 72), ((1, 13), 8), ((4, 4), 2048),
              ((1, 17), 520), ((1, 29), 72), ((7, 7), 2048), ((10, 10), 520)]         # ((H, W), C)
GAP_KINDS = ["relu", "negative", "neginf", "const", "ties", "nan1", "nan2"]
TO_NHWC_CASES = [(1, 3, 5, 7, 8, "bf16"), (1, 3, 4, 4, 8, "f32"), (2, 3, 4, 4, 4, "f32"), (2, 1, 1, 1, 8, "bf16"), (1, 8, 3, 3, 8, "bf16"),
                 (2, 13, 6, 5, 16, "bf16"), (1, 20, 3, 3, 32, "bf16"), (1, 64, 9, 9, 64, "f32")]       # (N, C, H, W, Cp, dtype)
TO_NCHW_CASES = [(1, 2, 6, 5, 8), (2, 3, 4, 4, 4), (1, 8, 3, 3, 8), (1, 9, 3, 3, 16), (2, 13, 6, 5, 16)]   # (N, C, H, W, Cp)
COLSUM_SHAPES = [(1, 8), (63, 24), (64, 64), (65, 24), (1000, 520), (300, 2048), (300, 2056), (130, 4104), (32768, 8), (32769, 64),
                 (40000, 24)]                                                          # (M, C)
LOSS_M = [1, 255, 256, 257, 1000, 4096, 524588]
LOSS_C = [2, 7]
LOSS_GAMMA = [1.0, 0.7]
LOGIT_KINDS = ["normal", "spread", "equal", "decided"]
MSE_TARGETS = [0.0, 19.999, 20.0, 1e4]
DTYPES = {"bf16": torch.bfloat16, "f32": torch.float32}


def ints(shape, seed, lo, hi):
    """fp64 tensor of integers in [lo, hi], the same on every host (numpy's MT19937)"""
    return torch.from_numpy(np.random.RandomState(seed).randint(lo, hi + 1, size=shape).astype(np.float64))


def maxpool_input(shape, kind):
    """x[N,H,W,C], integer-valued with |v| <= 8 (bf16 holds it), -inf and NaN apart.
    relu: half the map is exactly 0 (ties everywhere);  negative: no tap beats the seed by being >= 0;  neginf: three pixels in four are
    -inf and channel 0 is -inf throughout (whole windows of -inf: the seed tap stands);  nan1 / nan2: one / two NaNs inside the window
    of output (0, 0), at other pixels in every third channel, none in channels 2, 5, 8, ..."""
    N, H, W, C = shape
    seed = 1000 * H + 10 * W + C
    if kind == "relu":
        return ints(shape, seed, -8, 8).clamp(min=0)
    if kind == "negative":
        return ints(shape, seed + 1, -8, -1)
    x = ints(shape, seed + 2, -8, 8)
    if kind == "neginf":
        x[ints(shape, seed + 3, 0, 3) > 0] = -np.inf
        x[..., 0] = -np.inf
        return x
    h1, w1 = min(1, H - 1), min(1, W - 1)
    nan = float("nan")
    if kind == "nan1":
        x[:, 0, 0, 0::3] = nan
        x[:, h1, w1, 1::3] = nan
    elif kind == "nan2":
        x[:, 0, 0, 0::3] = nan
        x[:, h1, w1, 0::3] = nan
        x[:, 0, w1, 1::3] = nan
        x[:, h1, 0, 1::3] = nan
    else:
        raise ValueError(kind)
    return x


def tie_pair(c, HW):
    """indices i < j of channel c's two equal maxima, i and j in different row partitions (i != j mod 4); over the channels both orders
    of partition occur (e.g. 1, 2 and 3, 4).  None for a single pixel."""
    if HW < 2:
        return None
    i = c % HW
    j = i + 1 + c % 3
    if j >= HW:
        j = HW - 1
        if i == j:
            i = j - 1
    assert 0 <= i < j < HW and (j - i) % 4
    return i, j


def gap_input(hw, C, kind):
    """x[GAP_N,H,W,C], integer-valued with |v| <= 8.  const: every third channel is one value throughout;  ties: the maximum 8 twice per
    channel, at tie_pair(c, HW), everything else <= 7;  nan1: one NaN per channel at pixel (7 c + 3) % HW;  nan2: a second one at
    (3 c + 2) % HW -- whichever comes later in the scan is the arg max."""
    H, W = hw
    HW = H * W
    shape = (GAP_N, H, W, C)
    seed = 1000 * H + 10 * W + C
    if kind == "relu":
        return ints(shape, seed, -8, 8).clamp(min=0)
    if kind == "negative":
        return ints(shape, seed + 1, -8, -1)
    x = ints(shape, seed + 2, -8, 7).reshape(GAP_N, HW, C)
    c = torch.arange(C)
    if kind == "neginf":
        x[ints(x.shape, seed + 3, 0, 3) > 0] = -np.inf
        x[:, :, 0::5] = -np.inf
    elif kind == "const":
        x[:, :, 0::3] = ints((GAP_N, 1, len(c[0::3])), seed + 4, -8, 8)
    elif kind == "ties":
        for ch in range(C):
            pair = tie_pair(ch, HW)
            if pair:
                x[:, pair[0], ch] = 8.0
                x[:, pair[1], ch] = 8.0
    elif kind in ("nan1", "nan2"):
        x[:, (7 * c + 3) % HW, c] = float("nan")
        if kind == "nan2":
            x[:, (3 * c + 2) % HW, c] = float("nan")
    else:
        raise ValueError(kind)
    return x.reshape(shape)


BF16_SPECIALS = [0.0, -0.0, float("inf"), -float("inf"), float("nan"), 3.4028234663852886e38, -3.4028234663852886e38,
                 1.00390625,           # 1 + 2^-8: halfway between bf16 1.0 (even) and 1.0078125 -> down
                 1.01171875,           # 1 + 3 * 2^-8: halfway between 1.0078125 (odd) and 1.015625 -> up
                 -1.00390625, -1.01171875,
                 1.0039063692092896,   # the fp32 just above the first halfway point -> up
                 1.0117186307907104]   # the fp32 just below the second -> down


def layout_input(N, C, H, W, seed):
    """fp32 x[N,C,H,W]: normal values that need rounding in bf16, with BF16_SPECIALS (signed zeros, infinities, NaN, the largest finite
    fp32 -- it rounds to infinity -- and exact halfway cases of both parities) written over the last elements, as many as fit"""
    x = torch.from_numpy(np.random.RandomState(seed).standard_normal((N, C, H, W)).astype(np.float32))
    flat = x.view(-1)
    k = min(len(BF16_SPECIALS), flat.numel())
    flat[flat.numel() - k:] = torch.tensor(BF16_SPECIALS[:k], dtype=torch.float32)
    return x


def logits_input(M, C, kind, seed):
    """fp32 logits [M, C] and int64 labels [M].  spread: +-80, probabilities that are exactly 0 or 1 in fp32;  equal: every row one
    value;  decided: integer logits, one class of each row leads every other by 105 .. 120 (each other exponential underflows to 0 in
    fp32, so lse is that logit exactly) and is never 0; it is the row's label in three rows of four, else the label is another class and
    the row's loss is that integer lead."""
    rs = np.random.RandomState(seed)
    lab = rs.randint(0, C, size=M)
    if kind == "normal":
        z = rs.standard_normal((M, C))
    elif kind == "spread":
        z = rs.choice([-80.0, 80.0], size=(M, C)) + rs.standard_normal((M, C))
    elif kind == "equal":
        z = np.repeat(rs.standard_normal((M, 1)) * 3.0, C, axis=1)
    elif kind == "decided":
        lead = rs.randint(0, C, size=M)
        top = rs.randint(1, 9, size=M) * rs.choice([-1, 1], size=M)
        z = top[:, None] - rs.randint(105, 121, size=(M, C))
        z[np.arange(M), lead] = top
        other = (lead + 1 + rs.randint(0, C - 1, size=M)) % C
        lab = np.where(np.arange(M) % 4 == 3, other, lead)
    else:
        raise ValueError(kind)
    return torch.from_numpy(z.astype(np.float32)), torch.from_numpy(lab.astype(np.int64))


def mse_input(M, seed):
    """x, t fp64 [M]: counts 0 .. 59 with MSE_TARGETS (0, just below 20, 20, 1e4: both sides of the weight rule's boundary) at every
    eleventh place, x = t + noise"""
    rs = np.random.RandomState(seed)
    t = rs.randint(0, 60, size=M).astype(np.float64)
    for i, v in enumerate(MSE_TARGETS):
        t[i::11] = v
    x = t + rs.standard_normal(M) * 3.0
    return torch.from_numpy(x), torch.from_numpy(t)
