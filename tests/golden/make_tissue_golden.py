"""Writes tests/golden/tissue_vectors.npz: small RGB images and what the numpy restatement tests/tissue_ref.py returns for them --
per feature channel the 256-bin histogram, the threshold (Otsu's unless the case gives one), the tissue mask, the tissue pixels
under every window of the case's table and the selections for the case's list of min_pixels (``needs``).  Axis 0 of every result is
the channel (chroma, darkness); axis 1 of ``selected`` / ``n_selected`` the entry of ``needs``.  Inputs and recorded results only.

    python tests/golden/make_tissue_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import tissue_ref as R  # noqa: E402


def const(h, w, rgb):
    return np.broadcast_to(np.asarray(rgb, np.uint8), (h, w, 3)).copy()


def grid(hw, patch, interval, n=1):
    """(tile_img, tile_rc) of sample_patches for n equally sized images"""
    rc = np.asarray(R.sample_patches(hw, patch, interval), np.int32).reshape(-1, 2)
    return np.repeat(np.arange(n, dtype=np.int32), len(rc)), np.tile(rc, (n, 1))


def blobs(rng, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    p = np.zeros((h, w), np.float32)
    for _ in range(3):
        cy, cx, r = rng.randint(0, h), rng.randint(0, w), rng.uniform(2, 6)
        p = np.maximum(p, np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * r * r)).astype(np.float32))
    img = np.stack([235 - 150 * p, 225 - 170 * p, 230 - 90 * p], -1) + rng.randint(-6, 7, size=(h, w, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def hand_written():
    """[(name, images, threshold or None, size, tile_img, tile_rc)]"""
    out = []
    white = const(20, 24, (255, 255, 255))
    out.append(("all_white", white, None, 8, *grid((20, 24), 8, 6)))
    out.append(("single_valued_non_white", const(20, 24, (200, 120, 90)), None, 8, *grid((20, 24), 8, 6)))
    two = const(20, 24, (200, 200, 200))
    two[:, 9:] = (200, 150, 200)                                           # chroma 0 and 50: the threshold is the lower value
    out.append(("two_valued", two, None, 8, *grid((20, 24), 8, 6)))
    tie = const(18, 24, (110, 100, 100))                                   # chroma 10, 20, 30, a third of the pixels each
    tie[6:12] = (120, 100, 100)
    tie[12:] = (130, 100, 100)
    out.append(("otsu_tie_lower_t_wins", tie, None, 6, *grid((18, 24), 6, 6)))
    edge = const(16, 16, (100, 100, 100))
    edge[4:12, 2:8] = (140, 100, 100)                                      # chroma 40 = t: not tissue
    edge[4:12, 8:14] = (141, 100, 100)                                     # chroma 41 = t + 1: tissue
    out.append(("pixels_at_t_and_t_plus_1", edge, 40, 8, *grid((16, 16), 8, 4)))
    stroke = const(24, 40, (255, 255, 255))
    stroke[3:6, 2:30] = 0                                                  # a pure black pen stroke
    out.append(("black_stroke_on_white", stroke, None, 8, *grid((24, 40), 8, 8)))
    red = const(24, 24, (255, 255, 255))
    red[8:, 8:] = (255, 0, 0)
    out.append(("saturated_primary", red, None, 8, *grid((24, 24), 8, 8)))
    rng = np.random.RandomState(7)
    col = rng.randint(0, 256, size=(41, 1, 3)).astype(np.uint8)
    rows = np.arange(0, 41 - 8 + 1, 8).tolist() + [41 - 8]
    out.append(("w_equals_1", col, None, (8, 1), np.zeros(len(rows), np.int32), np.asarray([(r, 0) for r in rows], np.int32)))
    out.append(("odd_37x53", blobs(rng, 37, 53), None, 16, *grid((37, 53), 16, 12)))        # 5883 bytes: no multiple of 4
    out.append(("odd_5x7", rng.randint(0, 256, size=(5, 7, 3)).astype(np.uint8), None, 3, *grid((5, 7), 3, 2)))
    out.append(("patch_equals_image", blobs(rng, 16, 16), None, 16, *grid((16, 16), 16, 16)))
    out.append(("border_aligned_last_origins", blobs(rng, 30, 35), None, 8, *grid((30, 35), 8, 8)))   # origins 0, 8, 16, then 22 / 27
    pair = np.stack([blobs(rng, 21, 27), np.clip(blobs(rng, 21, 27).astype(np.int32) // 2 + 20, 0, 255).astype(np.uint8)])
    out.append(("batch_two_thresholds", pair, None, 8, *grid((21, 27), 8, 5, n=2)))
    return out


def cases():
    rng = np.random.RandomState(2026)
    out = []
    for i in range(12):
        h, w = int(rng.randint(8, 29)), int(rng.randint(8, 29))
        img = blobs(rng, h, w) if i % 2 else rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
        patch = int(rng.randint(3, min(h, w) + 1))
        interval = int(rng.randint((patch + 1) // 2, patch + 1))
        out.append((f"random_{i:02d}", img, None, patch, *grid((h, w), patch, interval)))
    return out + hand_written()


def needs(size):
    ph, pw = (size, size) if np.ndim(size) == 0 else size
    return np.asarray([0, R.min_pixels(0.01, ph, pw), (ph * pw + 1) // 2, ph * pw, ph * pw + 1], np.int32)


def record(images, threshold, size, tile_img, tile_rc):
    """name -> array for one case"""
    v = {"images": images, "size": np.asarray(size, np.int32).reshape(-1), "tile_img": tile_img, "tile_rc": tile_rc, "needs": needs(size)}
    if threshold is not None:
        v["given_threshold"] = np.asarray(threshold, np.int32)
    per = {k: [] for k in ("hist", "thr", "mask", "cover", "selected", "n_selected")}
    for ch in R.CHANNELS:                                                  # axis 0 of every result: the channel
        hist = R.histogram(images, ch)
        thr = R.otsu(hist) if threshold is None else ([threshold] * len(images) if images.ndim == 4 else threshold)
        m = R.mask(images, thr, ch)
        cover = R.coverage(m, tile_img, tile_rc, size if np.ndim(size) == 0 else tuple(size))
        picks = [R.select(cover, int(need)) for need in v["needs"]]        # axis 1 of the selections: the entry of `needs`
        for k, a in zip(per, (hist, np.asarray(thr, np.int32), m, cover, np.stack([p[0] for p in picks]), np.asarray([p[1] for p in picks], np.int32))):
            per[k].append(a)
    v.update({k: np.stack(a) for k, a in per.items()})
    return v


def main():
    vec, names = {}, []
    for name, images, threshold, size, tile_img, tile_rc in cases():
        names.append(name)
        for key, a in record(images, threshold, size, tile_img, tile_rc).items():
            vec[f"{name}.{key}"] = a
    vec["names"] = np.asarray(names)
    g = lambda k: vec[k]  # noqa: E731
    C, D = 0, 1                                                            # chroma, darkness
    assert g("all_white.thr").tolist() == [0, 0] and not g("all_white.mask").any()
    assert g("single_valued_non_white.thr")[C] == 110 and not g("single_valued_non_white.mask").any()
    assert g("two_valued.thr")[C] == 0 and g("two_valued.mask")[C].sum() == 20 * 15
    assert g("otsu_tie_lower_t_wins.thr")[C] == 10 and g("otsu_tie_lower_t_wins.mask")[C].sum() == 12 * 24
    assert g("pixels_at_t_and_t_plus_1.mask")[C].sum() == 8 * 6
    assert not g("black_stroke_on_white.mask")[C].any() and g("black_stroke_on_white.mask")[D].sum() == 3 * 28
    assert g("black_stroke_on_white.n_selected")[:, 1].tolist() == [0, 4]
    assert g("saturated_primary.hist")[C, 255] == 16 * 16 and g("saturated_primary.n_selected")[C, 3] == 4           # full windows only
    assert g("patch_equals_image.tile_rc").tolist() == [[0, 0]]
    assert g("border_aligned_last_origins.tile_rc")[-1].tolist() == [22, 27]
    assert g("batch_two_thresholds.thr")[C, 0] != g("batch_two_thresholds.thr")[C, 1]
    for n in names:
        assert (g(f"{n}.n_selected")[:, 0] == len(g(f"{n}.tile_rc"))).all() and (g(f"{n}.n_selected")[:, 4] == 0).all()
    np.savez_compressed(os.path.join(HERE, "tissue_vectors.npz"), **vec)
    print(f"{len(names)} cases written, {os.path.getsize(os.path.join(HERE, 'tissue_vectors.npz'))} bytes")


if __name__ == "__main__":
    main()
