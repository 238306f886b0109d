"""A plain numpy restatement of the rendering rules (cellsegmentation_amd/render.py, csrc/render.hip): loops and the formulas as they
are written down, sharing no code with the package.  Images are uint8 [N, H, W, 3]; maps and labels are [N, H, W]."""
import numpy as np


def jet():
    t = np.zeros((256, 3), np.uint8)
    for v in range(256):
        for ch, k in enumerate((3, 2, 1)):
            t[v, ch] = min(max(382 - abs(4 * v - 255 * k), 0), 255)
    return t


def mask_fill(c, m):
    return (c + 255 * (1 if m != 0 else 0)) >> 1


def heat_blend(c, k):
    s = c + k
    return (s >> 1) + ((s & 1) & ((s >> 1) & 1))


def heat_level(p, threshold):
    """h = p > threshold ? (uint8)(255.0f * p) : 0 in float32"""
    p = np.float32(p)
    if not p > np.float32(threshold):
        return 0
    return int(np.float32(255.0) * p) & 255


def boundaries(labels):
    """an edge pixel has a positive id = max(label, 0) and a 4-neighbour of another id; outside the image counts as id 0"""
    N, H, W = labels.shape
    out = np.zeros((N, H, W), bool)
    for n in range(N):
        for r in range(H):
            for c in range(W):
                l = max(int(labels[n, r, c]), 0)
                if l == 0:
                    continue
                for rr, cc in ((r - 1, c), (r + 1, c), (r, c - 1), (r, c + 1)):
                    other = max(int(labels[n, rr, cc]), 0) if 0 <= rr < H and 0 <= cc < W else 0
                    if other != l:
                        out[n, r, c] = True
    return out


def compose(images, mask=None, heat=None, threshold=None, colormap=None, invert=True, labels=None, outline_color=(255, 255, 0),
            palette=None):
    assert mask is None or heat is None
    N, H, W, _ = images.shape
    out = np.array(images, dtype=np.uint8, copy=True)
    table = jet() if colormap is None else colormap
    edges = None if labels is None else boundaries(labels)
    for n in range(N):
        for r in range(H):
            for c in range(W):
                for ch in range(3):
                    v = int(out[n, r, c, ch])
                    if mask is not None:
                        v = mask_fill(v, int(mask[n, r, c]))
                    if heat is not None:
                        h = heat_level(heat[n, r, c], threshold) if heat.dtype == np.float32 else int(heat[n, r, c])
                        v = heat_blend(v, int(table[255 - h if invert else h][ch]))
                    if edges is not None and edges[n, r, c]:
                        l = int(labels[n, r, c])
                        v = int(outline_color[ch]) if palette is None else int(palette[(l - 1) % len(palette)][ch])
                    out[n, r, c, ch] = v
    return out


COMPOSE_KEYS = ("mask", "heat", "threshold", "colormap", "invert", "labels", "outline_color", "palette")
POINTS_KEYS = ("offsets", "limits", "radius", "color", "thickness", "xy", "tail")


def golden_case(gold, name, keys):
    """the arrays ``<name>.<key>`` of tests/golden/render_vectors.npz -> (keyword arguments, expected); 0-d entries become scalars"""
    kw = {}
    for k in keys:
        if f"{name}.{k}" in gold.files:
            v = gold[f"{name}.{k}"]
            kw[k] = v.item() if v.ndim == 0 else v
    return kw, gold[f"{name}.expected"]


def in_mark(dr, dc, radius, thickness):
    d2 = dr * dr + dc * dc
    if thickness < 0:
        return d2 <= radius * radius
    return (2 * radius - thickness) ** 2 <= 4 * d2 <= (2 * radius + thickness) ** 2


def draw_points(canvas, points, offsets=None, limits=None, radius=4, color=(255, 0, 0), thickness=-1, xy=False, tail=False):
    """-> a drawn copy of canvas uint8 [N, H, W, 3]; image n owns points[offsets[n]:offsets[n + 1]], of which limits[n] keeps [:c]
    and ``tail`` draws [c:] instead"""
    out = np.array(canvas, dtype=np.uint8, copy=True)
    N, H, W, _ = out.shape
    points = np.asarray(points, np.int64).reshape(-1, 2)
    if offsets is None:
        assert N == 1
        offsets = [0, len(points)]
    reach = radius + max(thickness, 0)
    for n in range(N):
        mine = points[int(offsets[n]):int(offsets[n + 1])]
        if limits is not None:
            mine = mine[int(limits[n]):] if tail else mine[:int(limits[n])]
        else:
            assert not tail
        for a, b in mine:
            pr, pc = (int(b), int(a)) if xy else (int(a), int(b))
            for dr in range(-reach, reach + 1):
                for dc in range(-reach, reach + 1):
                    r, c = pr + dr, pc + dc
                    if in_mark(dr, dc, radius, thickness) and 0 <= r < H and 0 <= c < W:
                        out[n, r, c] = color
    return out
