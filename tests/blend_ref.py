"""The blended stitch of detect.StitchBlend restated in numpy, int64 throughout (the sums of the tests stay far below 2^63):

  level   q = uint32(256 * clamp(255 p, 0, 255)) in float32, a NaN giving 0
  weight  w = tr[i] * tc[j] for the pixel at (i, j) of its patch ON THE SLIDE (a flipped patch is flipped back first)
  sums    num += w q, den += w per slide pixel
  mask    num // (256 den), 0 where den == 0
"""
import numpy as np


def levels(p):
    """float32 probabilities -> int64 levels 0..65280; fmax / fmin drop the NaN as the device's fmaxf / fminf do"""
    v = np.fmin(np.fmax(np.float32(255) * np.asarray(p, dtype=np.float32), np.float32(0)), np.float32(255))
    q = (np.float32(256) * v).astype(np.int64)
    assert q.min(initial=0) >= 0 and q.max(initial=0) <= 65280
    return q


def taps(n, window="linear", ramp=None):
    if window == "uniform":
        return np.ones(n, np.int64)
    assert window == "linear"
    ramp = 255 if ramp is None else ramp
    return np.array([min(i + 1, n - i, ramp) for i in range(n)], np.int64)


def unflip(a, code):
    """the last two axes of a flipped patch put back as they lie on the slide"""
    if code & 2:
        a = a[..., ::-1, :]
    if code & 1:
        a = a[..., ::-1]
    return a


def accumulate(probs, grid, hw, flips, tr, tc):
    """(num, den) int64 [H, W]"""
    tr, tc = np.asarray(tr, dtype=np.int64), np.asarray(tc, dtype=np.int64)
    w = tr[:, None] * tc[None, :]
    num, den = np.zeros(hw, np.int64), np.zeros(hw, np.int64)
    ph, pw = w.shape
    flips = [0] * len(grid) if flips is None else flips
    for p, (r, c), code in zip(probs, grid, flips):
        assert p.shape == (ph, pw)
        num[r:r + ph, c:c + pw] += w * unflip(levels(p), int(code))
        den[r:r + ph, c:c + pw] += w
    assert den.max(initial=0) < 2 ** 31                            # the device's den is int32
    return num, den


def finish(num, den):
    return np.where(den > 0, num // (256 * np.maximum(den, 1)), 0).astype(np.uint8)


def blend(probs, grid, hw, flips, tr, tc):
    """probs float32 [M, ph, pw] (patch m as the model saw it: flipped when flips[m] says so), grid M (row, col) corners -> uint8 [H, W]"""
    return finish(*accumulate(probs, grid, hw, flips, tr, tc))
