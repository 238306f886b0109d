"""Plain-loop restatement of polygons to pixels (cellsegmentation_amd.polygons.rasterize), the reference of
tests/test_polygon_gpu.py, in Python integers.  It does not import the package.  The rule, as ``rasterize``'s docstring states it:

* vertices are (row, col) integers in units of 1/S pixel, S = 2**sub; pixel (i, j) is the closed unit square with corners (i, j)
  and (i+1, j+1) and its centre decides: in units of 1/(2S) the centre is Y = (2i+1)S, X = (2j+1)S and a vertex (R, C) is y = 2R,
  x = 2C;
* for every edge a -> b of every ring of a shape, the closing edge last -> first included, d = yb - ya and
  cross = (xb - xa)(Y - ya) - (X - xa) d; the edge counts for the pixel when (ya <= Y) != (yb <= Y) and (d > 0 and cross <= 0, or
  d < 0 and cross >= 0); it weighs +1 if d > 0, else -1; the winding number is the sum over all rings of the shape;
* "evenodd" takes the pixel when the winding number is odd, "nonzero" when it is not 0;
* shape s of an image (counted from 0) paints label s + 1, the highest label wins; the mask is 1 where any shape takes the pixel.
"""
import numpy as np


def winding(rings, shape, sub=0):
    """rings: a list of rings, each a sequence of (R, C) integers in units of 1/2**sub pixel -> int64 [H, W] winding numbers"""
    H, W = shape
    S = 1 << sub
    wind = np.zeros((H, W), np.int64)
    for ring in rings:
        ring = [(int(r), int(c)) for r, c in ring]
        n = len(ring)
        for k in range(n):
            (ra, ca), (rb, cb) = ring[k], ring[(k + 1) % n]
            ya, xa, yb, xb = 2 * ra, 2 * ca, 2 * rb, 2 * cb
            d = yb - ya
            for i in range(H):
                Y = (2 * i + 1) * S
                if (ya <= Y) == (yb <= Y):
                    continue
                for j in range(W):
                    X = (2 * j + 1) * S
                    cross = (xb - xa) * (Y - ya) - (X - xa) * d
                    if (d > 0 and cross <= 0) or (d < 0 and cross >= 0):
                        wind[i, j] += 1 if d > 0 else -1
    return wind


def taken(wind, rule="evenodd"):
    assert rule in ("evenodd", "nonzero")
    return (wind % 2 != 0) if rule == "evenodd" else (wind != 0)


def rasterize(per_image, shape, sub=0, rule="evenodd", mode="labels", values=None, base=None):
    """per_image: a list over images of lists of shapes, a shape a list of rings -> int32 labels or uint8 mask [N, H, W].
    ``values``: per image a list with one value per shape, written in place of the label (the highest shape still wins);
    ``base``: what the buffer held before (labels: the larger stays; mask: or)."""
    assert mode in ("labels", "mask")
    N = len(per_image)
    out = np.zeros((N,) + tuple(shape), np.int32 if mode == "labels" else np.uint8) if base is None else np.array(base)
    for n, shapes in enumerate(per_image):
        top = np.zeros(shape, np.int64)
        for s, rings in enumerate(shapes):
            top[taken(winding(rings, shape, sub), rule)] = s + 1
        if mode == "mask":
            out[n][top > 0] = 1
        elif values is None:
            out[n] = np.maximum(out[n], top)
        else:
            v = np.asarray([0] + list(values[n]), np.int64)[top]
            out[n] = np.where(top > 0, np.maximum(out[n], v) if base is not None else v, out[n])
    return out
