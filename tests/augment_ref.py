"""numpy fp32 restatement of the augmented input staging (csrc/augment.hip, cellsegmentation_amd/augment.py): per tile
crop -> /255 -> colour ops on the un-flipped crop -> flip -> (v - mean) / std, every step one rounded fp32 operation in the order the
kernel performs it.

The colour ops restate the float-image arithmetic of torchvision 0.11.2 ``functional_tensor`` (``_blend``, ``rgb_to_grayscale``,
``_rgb2hsv``, ``_hsv2rgb``) from its published source; torchvision is not a dependency of this project, so parity with torchvision
itself is NOT pinned by any test here -- as cellsegmentation_amd/regions.py says of scikit-image.  What is pinned: hand-computed
known answers (tests/test_augment_host.py) and the kernels against this file (tests/test_augment_gpu.py).

The contrast mean is ``np.float32(math.fsum(gray) / n)``: the exactly rounded sum of the fp32 grey values, divided in float64.
"""
import math

import numpy as np

F = np.float32
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3


def gray(x):
    """x float32 [..., 3] -> float32 [...]"""
    return (F(0.2989) * x[..., 0] + F(0.587) * x[..., 1]) + F(0.114) * x[..., 2]


def blend(a, b, f):
    f = F(f)
    return np.clip(f * a + (F(1) - f) * b, F(0), F(1)).astype(F)


def hue(x, f):
    f = F(f)
    r, g, b = x[..., 0], x[..., 1], x[..., 2]
    maxc = np.maximum(np.maximum(r, g), b)
    minc = np.minimum(np.minimum(r, g), b)
    eq = maxc == minc
    cr = maxc - minc
    one = np.ones_like(maxc)
    s = cr / np.where(eq, one, maxc)
    d = np.where(eq, one, cr)
    rc, gc, bc = (maxc - r) / d, (maxc - g) / d, (maxc - b) / d
    h = np.where(maxc == r, bc - gc, np.where(maxc == g, (F(2) + rc) - bc, (F(4) + gc) - rc))
    h = np.fmod(h / F(6) + F(1), F(1))
    hf = h + f
    h = hf - np.floor(hf)
    h6 = h * F(6)
    fl = np.floor(h6)
    fr = h6 - fl
    i = fl.astype(np.int32) % 6
    v = maxc
    p = np.clip(v * (F(1) - s), F(0), F(1))
    q = np.clip(v * (F(1) - s * fr), F(0), F(1))
    t = np.clip(v * (F(1) - s * (F(1) - fr)), F(0), F(1))
    tab = np.stack([np.stack(c, axis=-1) for c in ((v, q, p, p, t, v), (t, v, v, q, p, p), (p, p, t, v, v, q))], axis=-2)   # [..., 3, 6]
    out = np.take_along_axis(tab, np.broadcast_to(i[..., None, None], tab.shape[:-1] + (1,)), axis=-1)[..., 0]
    assert out.dtype == F
    return out


def tile_mean(x):
    g = gray(x).ravel()
    return F(math.fsum(float(v) for v in g) / g.size)


def jitter(x, order, factors):
    """x float32 [h, w, 3] in [0, 1]; order: 4 op codes in application order (-1 = unused); factors: 4 floats"""
    x = x.astype(F)
    for code, f in zip(order, factors):
        code = int(code)
        if code == BRIGHTNESS:
            x = blend(x, np.zeros_like(x), f)
        elif code == CONTRAST:
            x = blend(x, tile_mean(x), f)
        elif code == SATURATION:
            x = blend(x, gray(x)[..., None], f)
        elif code == HUE:
            x = hue(x, f)
        else:
            assert code == -1, code
    assert x.dtype == F
    return x


def flip(x, code):
    """the reference's transformIDX: 1 horizontal, 2 vertical, 3 both; x [h, w, ...]"""
    if code & 2:
        x = x[::-1]
    if code & 1:
        x = x[:, ::-1]
    return x


def normalise(x, mean=MEAN, std=STD):
    m = np.asarray(mean, F)
    s = np.asarray(std, F)
    return ((x - m) / s).astype(F)


def stage_tiles(images_u8, tile_img, tile_rc, th, tw, flips=None, jitters=None, mean=MEAN, std=STD):
    """images_u8 uint8 [n, H, W, 3] -> float32 [T, th, tw, 8] (channels 3..7 zero); jitters = (order [T, 4], factors [T, 4]) or None"""
    T = len(tile_img)
    out = np.zeros((T, th, tw, 8), F)
    for t in range(T):
        r, c = (int(v) for v in tile_rc[t])
        x = images_u8[int(tile_img[t]), r:r + th, c:c + tw].astype(F) / F(255)
        if jitters is not None:
            x = jitter(x, jitters[0][t], jitters[1][t])
        if flips is not None:
            x = flip(x, int(flips[t]))
        out[t, :, :, :3] = normalise(x, mean, std)
    return out


def stage_images(images_u8, flips=None, jitters=None, idx=None):
    n, H, W, _ = images_u8.shape
    idx = np.arange(n) if idx is None else np.asarray(idx)
    return stage_tiles(images_u8, idx, np.zeros((len(idx), 2), np.int64), H, W, flips, jitters)


def to_bf16_bits(x):
    """float32 array -> uint16 bf16 bit patterns, round to nearest even (finite inputs)"""
    u = np.ascontiguousarray(x, F).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def make_images():
    """the inputs of tests/test_augment_gpu.py: 3 random 20x24 images, one of them with grey, all-0 and all-255 rows, and one 67x61"""
    rng = np.random.RandomState(20)
    small = rng.randint(0, 256, (3, 20, 24, 3)).astype(np.uint8)
    small[1, 2:5] = small[1, 2:5, :, :1]                                  # r = g = b
    small[1, 7:9] = 0
    small[1, 11:13] = 255
    big = rng.randint(0, 256, (1, 67, 61, 3)).astype(np.uint8)
    return small, big
