"""Writes tests/golden/render_vectors.npz: small images, maps, label images and point lists, and what the numpy restatement
tests/render_ref.py draws for them.  ``compose_names`` / ``points_names`` list the cases; ``<name>.images`` (compose) or
``<name>.canvas`` and ``<name>.points`` (points) are the inputs, ``<name>.<keyword>`` the arguments that differ from the defaults
and ``<name>.expected`` the result.  Inputs and recorded results only.

    python tests/golden/make_render_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import render_ref as R  # noqa: E402

EXTREMES = np.asarray([0, 1, 254, 255], np.uint8)        # sums with the table odd and even, half-even rounding both ways


def image(rng, *shape):
    """random bytes, every other pixel one of the extremes"""
    img = rng.randint(0, 256, size=shape + (3,)).astype(np.uint8)
    pick = EXTREMES[rng.randint(0, 4, size=shape + (3,))]
    return np.where((np.arange(img.size).reshape(img.shape) // 3) % 2 == 0, pick, img).astype(np.uint8)


def labels_37x53():
    lab = np.zeros((1, 37, 53), np.int32)
    lab[0, 0:6, 0:8] = 1                                  # on the image's corner, with an interior
    lab[0, 0:6, 8:15] = 2                                 # adjacent to 1: both sides of the contact are edges
    lab[0, 10, 10] = 3                                    # a one-pixel object
    lab[0, 12:16, 12:16] = 4
    lab[0, 16:20, 16:20] = 5                              # diagonal contact with 4 at (15, 15) / (16, 16)
    lab[0, 22:30, 20:30] = 6
    lab[0, 25:27, 24:26] = 0                              # a hole: its rim is edge
    lab[0, 20:24, 0:5] = -7                               # negative: background
    lab[0, 25:37, 40:53] = 300                            # on the bottom right corner, an id above the palette size
    return lab


def compose_cases():
    rng = np.random.RandomState(20261)
    out = []
    out.append(("copy_5x7", dict(images=image(rng, 1, 5, 7))))
    out.append(("mask_41x1", dict(images=image(rng, 1, 41, 1), mask=rng.randint(0, 2, size=(1, 41, 1)).astype(np.uint8))))
    out.append(("mask_1x41_all0", dict(images=image(rng, 1, 1, 41), mask=np.zeros((1, 1, 41), np.uint8))))
    out.append(("mask_5x7_all1", dict(images=image(rng, 1, 5, 7), mask=np.ones((1, 5, 7), np.uint8))))
    out.append(("mask_37x53_any_nonzero", dict(images=image(rng, 1, 37, 53), mask=(rng.randint(0, 3, size=(1, 37, 53)) * 127).astype(np.uint8))))
    out.append(("mask_batch2_9x13", dict(images=image(rng, 2, 9, 13), mask=rng.randint(0, 2, size=(2, 9, 13)).astype(np.uint8))))
    heat = rng.randint(0, 256, size=(1, 37, 53)).astype(np.uint8)
    heat[0, :, ::3] = 0
    heat[0, :, 1::3] = 255
    img = image(rng, 1, 37, 53)
    out.append(("heat_u8_37x53_inverted", dict(images=img, heat=heat)))
    out.append(("heat_u8_37x53_direct", dict(images=img, heat=heat, invert=False)))
    out.append(("heat_u8_41x1_own_table", dict(images=image(rng, 1, 41, 1), heat=rng.randint(0, 256, size=(1, 41, 1)).astype(np.uint8),
                                               colormap=rng.randint(0, 256, size=(256, 3)).astype(np.uint8))))
    out.append(("heat_u8_batch2_5x7_0_and_255", dict(images=image(rng, 2, 5, 7), heat=(rng.randint(0, 2, size=(2, 5, 7)) * 255).astype(np.uint8))))
    u = np.float32(1.0) / np.float32(255.0)
    p = rng.uniform(0, 1, size=(1, 5, 7)).astype(np.float32)
    p[0, 0, :4] = (np.float32(1.0), np.nextafter(u, np.float32(0)), np.nextafter(u, np.float32(1)), np.float32(0.0))
    out.append(("heat_f32_5x7_thr_0", dict(images=image(rng, 1, 5, 7), heat=p, threshold=0.0)))
    p = rng.uniform(0, 1, size=(2, 9, 13)).astype(np.float32)
    p[:, 0, :3] = (np.float32(0.5), np.nextafter(np.float32(0.5), np.float32(1)), np.float32(1.0))      # at the threshold: 0
    out.append(("heat_f32_batch2_9x13_thr_half", dict(images=image(rng, 2, 9, 13), heat=p, threshold=0.5, invert=False)))
    lab = labels_37x53()
    img = image(rng, 1, 37, 53)
    out.append(("outline_37x53", dict(images=img, labels=lab)))
    out.append(("outline_37x53_over_mask", dict(images=img, labels=lab, mask=(lab > 0).astype(np.uint8), outline_color=np.asarray((0, 255, 17)))))
    out.append(("outline_37x53_palette_over_heat", dict(images=img, labels=lab, heat=heat,
                                                        palette=np.asarray([(255, 0, 0), (0, 255, 0), (1, 2, 254)], np.uint8))))
    two = np.zeros((2, 12, 13), np.int32)
    two[0, 8:12, 2:9] = 1                                 # the last rows of image 0 and the first of image 1 carry one id:
    two[1, 0:5, 2:9] = 1                                  # outside an image is id 0, so both rows are edges
    two[1, 7:11, 10:13] = 2
    out.append(("outline_batch2_12x13", dict(images=image(rng, 2, 12, 13), labels=two)))
    return out


def points_cases():
    rng = np.random.RandomState(20262)
    out = []
    c1 = rng.randint(0, 256, size=(1, 16, 20, 3)).astype(np.uint8)
    pts = np.asarray([(0, 0), (0, 19), (15, 0), (15, 19),                 # the four corners
                      (-3, 10), (18, 4), (8, -2), (7, 23),                # outside, the mark reaches in
                      (-5, 5), (25, 25), (8, -40), (1 << 40, 3),          # wholly outside
                      (8, 9), (9, 11), (8, 9)], np.int64)                 # overlapping, one twice
    for r in (0, 1, 4):
        out.append((f"dots_16x20_r{r}", dict(canvas=c1, points=pts, radius=r)))
    for t in (1, 2, 8):
        out.append((f"rings_16x20_r4_t{t}", dict(canvas=c1, points=pts, radius=4, thickness=t, color=np.asarray((0, 200, 255)))))
    out.append(("rings_16x20_r1_t2", dict(canvas=c1, points=pts, radius=1, thickness=2)))
    out.append(("no_points_16x20", dict(canvas=c1, points=np.zeros((0, 2), np.int64))))
    c2 = rng.randint(0, 256, size=(2, 33, 29, 3)).astype(np.uint8)
    pts2 = np.stack([rng.randint(-4, 37, size=11), rng.randint(-4, 33, size=11)], 1).astype(np.int64)
    off2 = np.asarray([0, 6, 11], np.int64)
    out.append(("batch_2x33x29", dict(canvas=c2, points=pts2, offsets=off2, radius=2, color=np.asarray((9, 8, 7)))))
    out.append(("batch_2x33x29_limits", dict(canvas=c2, points=pts2, offsets=off2, limits=np.asarray([4, 0], np.int32))))
    out.append(("batch_2x33x29_tail", dict(canvas=c2, points=pts2, offsets=off2, limits=np.asarray([4, 2], np.int32), tail=True,
                                           color=np.asarray((0, 0, 255)))))
    out.append(("batch_2x33x29_xy", dict(canvas=c2, points=pts2[:, ::-1].copy(), offsets=off2, xy=True, radius=3, thickness=2)))
    c3 = rng.randint(0, 256, size=(3, 9, 11, 3)).astype(np.uint8)
    out.append(("empty_image_between_3x9x11", dict(canvas=c3, points=np.asarray([(2, 2), (8, 10), (4, 5)], np.int64),
                                                   offsets=np.asarray([0, 2, 2, 3], np.int64), radius=1)))
    return out


def main():
    vec = {}
    names = {"compose": [], "points": []}
    for name, kw in compose_cases():
        names["compose"].append(name)
        vec[f"{name}.expected"] = R.compose(**kw)
        vec.update({f"{name}.{k}": np.asarray(v) for k, v in kw.items()})
    for name, kw in points_cases():
        names["points"].append(name)
        vec[f"{name}.expected"] = R.draw_points(**kw)
        vec.update({f"{name}.{k}": np.asarray(v) for k, v in kw.items()})
    vec["compose_names"], vec["points_names"] = np.asarray(names["compose"]), np.asarray(names["points"])
    g = lambda k: vec[k]  # noqa: E731
    assert np.array_equal(g("copy_5x7.expected"), g("copy_5x7.images"))
    assert np.array_equal(g("mask_1x41_all0.expected"), g("mask_1x41_all0.images") >> 1)
    assert g("mask_5x7_all1.expected").min() >= 127
    assert g("heat_f32_5x7_thr_0.heat")[0, 0, 1] * np.float32(255) < 1 <= g("heat_f32_5x7_thr_0.heat")[0, 0, 2] * np.float32(255)
    edges = R.boundaries(labels_37x53())[0]
    assert edges[10, 10] and edges[0, 0] and not edges[2, 3] and edges[3, 7] and edges[3, 8] and edges[15, 15] and edges[16, 16]
    assert edges[36, 52] and not edges[30, 45] and edges[25, 23] and not edges[21, 2]
    assert (g("outline_37x53.expected")[0][edges] == (255, 255, 0)).all()
    assert (g("outline_37x53_palette_over_heat.expected")[0, 36, 52] == (1, 2, 254)).all()          # (300 - 1) % 3 = 2
    assert R.boundaries(g("outline_batch2_12x13.labels"))[0, 11, 2:9].all() and R.boundaries(g("outline_batch2_12x13.labels"))[1, 0, 2:9].all()
    assert np.array_equal(g("no_points_16x20.expected"), g("no_points_16x20.canvas"))
    assert np.array_equal(g("empty_image_between_3x9x11.expected")[1], g("empty_image_between_3x9x11.canvas")[1])
    path = os.path.join(HERE, "render_vectors.npz")
    np.savez_compressed(path, **vec)
    assert os.path.getsize(path) < 256 << 10
    print(f"{len(names['compose'])} + {len(names['points'])} cases written, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
