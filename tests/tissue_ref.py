"""A plain numpy restatement of cellsegmentation_amd.tissue (csrc/tissue.hip): the two pixel features, the 256-bin histogram,
exact Otsu, the mask, the per-window coverage by integral image, and the selection.  Test infrastructure only."""
import math

import numpy as np

CHANNELS = ("chroma", "darkness")


def feature(images_u8, channel="chroma"):
    """uint8 [..., 3] -> int64 [...] in [0, 255]"""
    a = np.asarray(images_u8)
    assert a.dtype == np.uint8 and a.shape[-1] == 3
    r, g, b = (a[..., k].astype(np.int64) for k in range(3))
    if channel == "chroma":
        return np.maximum(np.maximum(r, g), b) - np.minimum(np.minimum(r, g), b)
    if channel == "darkness":
        return 255 - ((77 * r + 150 * g + 29 * b + 128) >> 8)
    raise ValueError(channel)


def histogram(images_u8, channel="chroma"):
    """[H, W, 3] -> int64 [256]; [N, H, W, 3] -> int64 [N, 256]"""
    f = feature(images_u8, channel)
    if f.ndim == 2:
        return np.bincount(f.reshape(-1), minlength=256).astype(np.int64)
    return np.stack([np.bincount(x.reshape(-1), minlength=256) for x in f]).astype(np.int64)


def otsu(hist):
    """exact: the fractions (S0 Wt - S w0)^2 / (w0 (Wt - w0)) compared by cross-multiplication, the lowest t winning a tie; a
    histogram with one occupied bin gives that bin, an empty one 0"""
    h = np.asarray(hist)
    if h.ndim == 2:
        return [otsu(row) for row in h]
    h = [int(c) for c in h]
    assert len(h) == 256
    Wt, S = sum(h), sum(v * c for v, c in enumerate(h))
    best = None
    for t in range(255):
        w0 = sum(h[:t + 1])
        S0 = sum(v * h[v] for v in range(t + 1))
        if w0 == 0 or Wt - w0 == 0:
            continue
        num, den = (S0 * Wt - S * w0) ** 2, w0 * (Wt - w0)
        if best is None or num * best[2] > best[1] * den:
            best = (t, num, den)
    if best is None:
        occupied = [v for v, c in enumerate(h) if c]
        return occupied[0] if occupied else 0
    return best[0]


def otsu_float(hist):
    """the textbook float64 form: argmax over t of w0 w1 (mu0 - mu1)^2 with class 0 = values <= t (the first maximum)"""
    h = np.asarray(hist, np.float64)
    v = np.arange(256, dtype=np.float64)
    w0 = np.cumsum(h)[:255]
    w1 = h.sum() - w0
    s0 = np.cumsum(v * h)[:255]
    s1 = (v * h).sum() - s0
    ok = (w0 > 0) & (w1 > 0)
    var = np.where(ok, w0 * w1 * (s0 / np.where(ok, w0, 1) - s1 / np.where(ok, w1, 1)) ** 2, -1.0)
    return int(np.argmax(var))


def mask(images_u8, threshold=None, channel="chroma"):
    """[H, W, 3] or [N, H, W, 3] -> uint8 0 / 1 of the same leading shape; threshold None (Otsu per image), an int or one per image"""
    f = feature(images_u8, channel)
    if f.ndim == 2:
        t = otsu(histogram(images_u8, channel)) if threshold is None else int(threshold)
        return (f > t).astype(np.uint8)
    if threshold is None:
        thr = otsu(histogram(images_u8, channel))
    else:
        thr = [int(threshold)] * len(f) if np.ndim(threshold) == 0 else [int(t) for t in threshold]
    return np.stack([(x > t).astype(np.uint8) for x, t in zip(f, thr)])


def coverage(mask_u8, tile_img, tile_rc, size):
    """the non-zero pixels under every window, by integral image; windows are clamped to the image -> int32 [T]"""
    m = np.asarray(mask_u8)
    if m.ndim == 2:
        m = m[None]
    ph, pw = (size, size) if np.ndim(size) == 0 else size
    N, H, W = m.shape
    ii = np.zeros((N, H + 1, W + 1), np.int64)
    ii[:, 1:, 1:] = np.cumsum(np.cumsum(m != 0, axis=1), axis=2)
    out = []
    for n, (r, c) in zip(np.asarray(tile_img).reshape(-1), np.asarray(tile_rc).reshape(-1, 2)):
        r0, r1 = min(max(int(r), 0), H), min(max(int(r) + ph, 0), H)
        c0, c1 = min(max(int(c), 0), W), min(max(int(c) + pw, 0), W)
        if not 0 <= n < N or r1 <= r0 or c1 <= c0:
            out.append(0)
            continue
        out.append(int(ii[n, r1, c1] - ii[n, r0, c1] - ii[n, r1, c0] + ii[n, r0, c0]))
    return np.asarray(out, np.int32).reshape(-1)


def select(cover, min_pixels):
    """-> (int32 [T]: the kept indices in rising order, then -1; their number)"""
    cover = np.asarray(cover).reshape(-1)
    keep = np.flatnonzero(cover >= min_pixels).astype(np.int32)
    out = np.full(len(cover), -1, np.int32)
    out[:len(keep)] = keep
    return out, len(keep)


def axis_origins(length, interval, size):
    o = list(range(0, length - size + 1, interval))
    assert o, "patch larger than the image"
    if o[-1] + size != length:
        o.append(length - size)
    return o


def sample_patches(hw, patch, interval):
    """tiles.sample_patches restated: rows outer, columns inner, the last origin of an axis aligned to the border"""
    return [(x, y) for x in axis_origins(hw[0], interval, patch) for y in axis_origins(hw[1], interval, patch)]


def min_pixels(min_fraction, ph, pw):
    return int(math.ceil(float(min_fraction) * (ph * pw)))


def blob_slide(H=150, W=170, seed=31, stroke=True, blobs=14):
    """uint8 [H, W, 3]: a light ground with +-6 noise, dark Gaussian blobs (a little different per channel) whose centres lie in
    rows >= 70 + 16 and columns >= 60 + 20 only -- no blob reaches above row 70 or left of column 60 -- and, with ``stroke``, a grey
    pen stroke of value 12, 4 rows x 30 columns, near the top-left corner"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    p = np.zeros((H, W), np.float32)
    for cy, cx in zip(rng.randint(86, H, blobs), rng.randint(80, W, blobs)):
        r = rng.uniform(3, 5)
        p = np.maximum(p, np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * r * r)).astype(np.float32))
    p[:70] = 0
    p[:, :60] = 0
    img = np.stack([235 - 150 * p, 225 - 170 * p, 230 - 90 * p], -1) + rng.randint(-6, 7, size=(H, W, 3))
    img = np.clip(img, 0, 255).astype(np.uint8)
    if stroke:
        img[10:14, 8:38] = 12
    return img


def select_patches(image_u8, patch, interval, channel="chroma", threshold=None, need=None, min_fraction=0.01):
    """one slide -> dict(threshold, mask, corners int32 [T, 2], coverage, selected int32 [n], n_selected, selected_corners)"""
    t = otsu(histogram(image_u8, channel)) if threshold is None else int(threshold)
    m = mask(image_u8, t, channel)
    corners = np.asarray(sample_patches(image_u8.shape[:2], patch, interval), np.int32).reshape(-1, 2)
    cover = coverage(m, np.zeros(len(corners), np.int32), corners, patch)
    need = min_pixels(min_fraction, patch, patch) if need is None else need
    sel, n = select(cover, need)
    return dict(threshold=t, mask=m, corners=corners, coverage=cover, selected=sel[:n], n_selected=n, selected_corners=corners[sel[:n]])
