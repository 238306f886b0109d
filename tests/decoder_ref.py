"""Host restatement (numpy / torch, fp64) of the segmentation decoder's data movement and of the Dice path:
align-corners bilinear resize and its transpose, softmax over channels for one channel, Dice loss with its sums and gradient.
Written from the operation definitions (ATen's align_corners source-index rule for an fp32 tensor, the softmax Jacobian, the Dice
formula of cellsegmentation_amd/train/losses.py); nothing here touches the GPU or the HIP library.

The interpolation WEIGHTS are part of the operation's definition for an fp32 tensor, so `bilinear_taps` computes them in fp32 exactly
as ATen does; everything after the weights is fp64."""
import numpy as np
import torch

U32 = 2.0 ** -24          # unit roundoff of fp32 (half an ulp of 1)
U16 = 2.0 ** -8           # half a bf16 ulp relative to the bottom of its binade (8 significand bits)


# ------------------------------------------------------------------------------------------------ bilinear, align_corners=True
def bilinear_taps(n_in, n_out):
    """i0, i1 (int64), w0, w1 (float32) per output index: scale = (in-1)/(out-1) in fp32 (0 when out == 1), src = scale * dst in
    fp32, i0 = floor(src) clamped to in-1, i1 = i0 + (i0 < in-1), lambda = src - i0 in fp32 clamped to [0, 1], w1 = lambda,
    w0 = 1 - lambda in fp32."""
    scale = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0)
    src = (scale * np.arange(n_out, dtype=np.float32)).astype(np.float32)
    i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    lam = np.clip((src - i0.astype(np.float32)).astype(np.float32), np.float32(0), np.float32(1))
    w0 = (np.float32(1) - lam).astype(np.float32)
    return i0, i1, w0, lam


def _taps_t(n_in, n_out):
    i0, i1, w0, w1 = bilinear_taps(n_in, n_out)
    return (torch.from_numpy(i0), torch.from_numpy(i1), torch.from_numpy(w0.astype(np.float64)), torch.from_numpy(w1.astype(np.float64)))


def _resize_axis(x, axis, n_out):
    """fp64 gather along one axis: y[o] = w0[o] x[i0[o]] + w1[o] x[i1[o]]"""
    i0, i1, w0, w1 = _taps_t(x.shape[axis], n_out)
    shape = [1] * x.ndim
    shape[axis] = n_out
    return x.index_select(axis, i0) * w0.view(shape) + x.index_select(axis, i1) * w1.view(shape)


def _scatter_axis(dy, axis, n_in):
    """the transpose of _resize_axis: dx[i0[o]] += w0[o] dy[o]; dx[i1[o]] += w1[o] dy[o]"""
    n_out = dy.shape[axis]
    i0, i1, w0, w1 = _taps_t(n_in, n_out)
    shape = [1] * dy.ndim
    shape[axis] = n_out
    out_shape = list(dy.shape)
    out_shape[axis] = n_in
    dx = torch.zeros(out_shape, dtype=torch.float64)
    dx.index_add_(axis, i0, dy * w0.view(shape))
    dx.index_add_(axis, i1, dy * w1.view(shape))
    return dx


def bilinear_fwd_ref(x, out_hw):
    """x [N, H, W, C] fp64 -> [N, P, Q, C] fp64 (rows first, then columns, like the definition; the order is immaterial in fp64)"""
    assert x.dtype == torch.float64 and x.ndim == 4
    return _resize_axis(_resize_axis(x, 1, out_hw[0]), 2, out_hw[1])


def bilinear_fwd_mag(x, out_hw):
    """the same operator applied to |x|: the weights are non-negative, so this is sum |w| |x|, the scale of the rounding error"""
    return bilinear_fwd_ref(x.abs(), out_hw)


def bilinear_bwd_ref(dy, in_hw, mask=None):
    """dy [N, P, Q, C] fp64 -> dx [N, H, W, C] fp64, the exact transpose of bilinear_fwd_ref as a scatter over its taps;
    mask (same shape as dx): dx * (mask > 0)"""
    assert dy.dtype == torch.float64 and dy.ndim == 4
    dx = _scatter_axis(_scatter_axis(dy, 2, in_hw[1]), 1, in_hw[0])
    if mask is not None:
        dx = dx * (mask > 0).to(torch.float64)
    return dx


def bilinear_bwd_mag(dy, in_hw, mask=None):
    return bilinear_bwd_ref(dy.abs(), in_hw, mask)


def _fan_in(n_in, n_out):
    """per input index: how many output indices reach it with a non-zero weight"""
    i0, i1, w0, w1 = bilinear_taps(n_in, n_out)
    hit = np.zeros((n_out, n_in), dtype=bool)
    hit[np.arange(n_out)[w0 != 0], i0[w0 != 0]] = True
    hit[np.arange(n_out)[w1 != 0], i1[w1 != 0]] = True
    return hit.sum(0)


def bilinear_bwd_terms(in_hw, out_hw):
    """the largest number of output pixels that feed one input pixel (the length of the longest backward sum)"""
    return int(_fan_in(in_hw[0], out_hw[0]).max()) * int(_fan_in(in_hw[1], out_hw[1]).max())


# ------------------------------------------------------------------------------------------------ softmax over channels, one channel
def _softmax_all(logits):
    assert logits.dtype == torch.float64 and logits.ndim == 4
    e = torch.exp(logits - logits.max(dim=1, keepdim=True).values)
    return e / e.sum(dim=1, keepdim=True)


def softmax_channel_ref(logits, ch):
    """logits [N, C, H, W] fp64 -> softmax over C, channel ch: [N, H, W]"""
    return _softmax_all(logits)[:, ch]


def softmax_channel_grad_ref(logits, g, ch):
    """d sum(g * softmax(logits)[:, ch]) / d logits, [N, C, H, W]: g p_ch (delta(c, ch) - p_c)"""
    p = _softmax_all(logits)
    delta = torch.zeros(logits.shape[1], dtype=torch.float64)
    delta[ch] = 1.0
    return (g * p[:, ch]).unsqueeze(1) * (delta.view(1, -1, 1, 1) - p)


# ------------------------------------------------------------------------------------------------ Dice
def dice_ref(p, t, eps=1e-6, mean=True):
    """loss, sums [N, 3] = per-sample (sum p t, sum p^2, sum t^2), dloss/dp (shape of p); all fp64.
    loss = mean | sum over samples of 1 - (2a + eps) / (b + c + eps); 2-D inputs are ONE global sample."""
    assert p.dtype == torch.float64 and t.dtype == torch.float64 and p.shape == t.shape
    if p.ndim == 2:
        p2, t2 = p.reshape(1, -1), t.reshape(1, -1)
    else:
        p2, t2 = p.reshape(p.shape[0], -1), t.reshape(t.shape[0], -1)
    N = p2.shape[0]
    a, b, c = (p2 * t2).sum(1), (p2 * p2).sum(1), (t2 * t2).sum(1)
    num, den = 2 * a + eps, b + c + eps
    per = 1 - num / den
    scale = 1.0 / N if mean else 1.0
    loss = per.sum() * scale
    grad = -scale * (2 * t2 * den.unsqueeze(1) - 2 * p2 * num.unsqueeze(1)) / (den * den).unsqueeze(1)
    return loss, torch.stack([a, b, c], dim=1), grad.reshape(p.shape)
