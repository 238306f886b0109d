"""A float64 numpy restatement of cellsegmentation_amd.stain (csrc/stain.hip): the optical-density table, the kept pixels and their
integer moments, Macenko's estimate with TRUE order statistics from a sort (the product uses histograms), the normalising matrix,
``apply`` and ``separate``; and a synthetic H-DAB generator with known stain vectors."""
import math

import numpy as np

OD_UNIT = 4096
H_VEC = np.asarray((0.650, 0.704, 0.286)) / np.linalg.norm((0.650, 0.704, 0.286))
DAB_VEC = np.asarray((0.268, 0.570, 0.776)) / np.linalg.norm((0.268, 0.570, 0.776))
HDAB = np.stack([H_VEC, DAB_VEC], axis=1)                                  # [3, 2]: Ruifrok's vectors as columns
DENSE_TILE = 22                                                            # synth_hdab(96, 96, 0, tile=DENSE_TILE): the dense fixture


def od_table(Io=240):
    v = np.arange(256, dtype=np.float64)
    return np.maximum(0.0, np.rint(OD_UNIT * np.log(Io / (v + 1.0)))).astype(np.int32)


def od_q(images_u8, Io=240):
    """uint8 [..., 3] -> int64 [..., 3]"""
    return od_table(Io)[np.asarray(images_u8)].astype(np.int64)


def od(images_u8, Io=240):
    return od_q(images_u8, Io) / float(OD_UNIT)


def kept(images_u8, mask=None, Io=240, beta=0.15):
    """bool [...]: no channel below rint(4096 beta), and the mask non-zero where one is given"""
    k = od_q(images_u8, Io).min(axis=-1) >= int(np.rint(OD_UNIT * beta))
    return k if mask is None else k & (np.asarray(mask).reshape(k.shape) != 0)


def moments(images_u8, mask=None, Io=240, beta=0.15):
    """[H, W, 3] -> int64 [10]; [N, H, W, 3] -> int64 [N, 10]: count, r, g, b, rr, rg, rb, gg, gb, bb of od_q over the kept pixels"""
    images_u8 = np.asarray(images_u8)
    if images_u8.ndim == 4:
        return np.stack([moments(im, None if mask is None else np.asarray(mask).reshape(images_u8.shape[:3])[i], Io, beta)
                         for i, im in enumerate(images_u8)])
    q = od_q(images_u8, Io)[kept(images_u8, mask, Io, beta)]               # [n, 3]
    r, g, b = q[:, 0], q[:, 1], q[:, 2]
    return np.asarray([len(q), r.sum(), g.sum(), b.sum(), (r * r).sum(), (r * g).sum(), (r * b).sum(), (g * g).sum(), (g * b).sum(),
                       (b * b).sum()], np.int64)


def plane(m):
    """the two leading eigenvectors of the covariance behind the moments, [3, 2], or None"""
    m = [int(v) for v in m]
    n = m[0]
    if n < 2:
        return None
    S = np.asarray([[m[4], m[5], m[6]], [m[5], m[7], m[8]], [m[6], m[8], m[9]]], object)
    s = np.asarray(m[1:4], object)
    C = ((n * S - np.outer(s, s)) / 1).astype(np.float64) / (float(n) * (n - 1) * OD_UNIT ** 2)
    w, E = np.linalg.eigh(C)
    if not w[1] > 0:
        return None
    V = E[:, [2, 1]]
    return V * np.where(V.sum(axis=0) < 0, -1.0, 1.0)


def ranks(n, alpha=1.0):
    return int(math.floor(alpha / 100.0 * (n - 1))), int(math.ceil((100.0 - alpha) / 100.0 * (n - 1)))


def stain_vectors(V, phi_lo, phi_hi):
    a = V @ np.asarray([math.cos(phi_lo), math.sin(phi_lo)])
    b = V @ np.asarray([math.cos(phi_hi), math.sin(phi_hi)])
    return np.stack([a, b] if a[0] >= b[0] else [b, a], axis=1)


def estimate(image_u8, mask=None, Io=240, beta=0.15, alpha=1.0):
    """one image -> dict: vectors [3, 2], max_conc [2], n_kept, ok, and the intermediate V, P, the sorted angles ``phi`` with the ranks
    ``k_lo`` / ``k_hi`` taken from them, the sorted concentrations ``conc`` [2, n] with the rank ``k_conc``"""
    x = od(image_u8, Io)[kept(image_u8, mask, Io, beta)]                   # [n, 3]
    n = len(x)
    V = plane(moments(image_u8, mask, Io, beta))
    if V is None:
        return dict(vectors=HDAB.copy(), max_conc=np.ones(2), n_kept=n, ok=False)
    p = x @ V
    phi = np.sort(np.arctan2(p[:, 1], p[:, 0]))
    k_lo, k_hi = ranks(n, alpha)
    S = stain_vectors(V, phi[k_lo], phi[k_hi])
    P = np.linalg.pinv(S)
    conc = np.sort(x @ P.T, axis=0).T                                      # [2, n]
    k_conc = int(math.ceil(0.99 * (n - 1)))
    return dict(vectors=S, max_conc=conc[:, k_conc].copy(), n_kept=n, ok=True, V=V, P=P, phi=phi, k_lo=k_lo, k_hi=k_hi, conc=conc,
                k_conc=k_conc)


def normalizer(src_vectors, src_max, tgt_vectors=HDAB, tgt_max=(1.0, 1.0)):
    return np.asarray(tgt_vectors) @ np.diag(np.asarray(tgt_max, np.float64) / np.asarray(src_max, np.float64)) @ np.linalg.pinv(src_vectors)


def apply(images_u8, A, Io=240):
    """uint8 [..., 3], A [3, 3] -> (uint8 [..., 3], the float64 values before rounding)"""
    v = Io * np.exp(-(od(images_u8, Io) @ np.asarray(A, np.float64).T))
    return np.clip(np.rint(v), 0, 255).astype(np.uint8), v


def normalize(image_u8, mask=None, Io=240, beta=0.15, alpha=1.0):
    e = estimate(image_u8, mask, Io, beta, alpha)
    return apply(image_u8, normalizer(e["vectors"], e["max_conc"]), Io)[0]


def stain_matrix(S, residual=False):
    S = np.asarray(S, np.float64)
    if residual:
        c = np.cross(S[:, 0], S[:, 1])
        S = np.concatenate([S, (c / np.linalg.norm(c))[:, None]], axis=1)
    return S


def separate(images_u8, S=HDAB, residual=False, Io=240):
    """-> (float64 [..., K] concentrations, P [K, 3])"""
    P = np.linalg.pinv(stain_matrix(S, residual))
    return od(images_u8, Io) @ P.T, P


def separate_u8(images_u8, S=HDAB, residual=False, Io=240, conc_max=8.0):
    c, _ = separate(images_u8, S, residual, Io)
    return np.clip(np.rint(255.0 * c / conc_max), 0, 255).astype(np.uint8)


def angle_between(a, b):
    """radians between two vectors"""
    c = float(np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b)))
    return math.acos(max(-1.0, min(1.0, c)))


def synth_hdab(h, w, seed=0, n_h=None, n_dab=None, Io=240, S=HDAB, sigma=1.5, floor=0.05, tile=1):
    """uint8 [h tile, w tile, 3]: Gaussian blobs of two stains with the unit vectors S [3, 2] (nuclei of haematoxylin, cells of DAB),
    each concentration on a floor drawn uniformly from [0, floor], the image Io exp(-c S^T) plus N(0, sigma) noise, rounded and
    clipped.  ``tile`` repeats the h x w field of blobs that many times along both axes; floor and noise are drawn for every pixel
    of the whole image, so that a large image has the small one's distribution of stains with that many times its pixels."""
    rng = np.random.RandomState(seed)
    area = h * w
    n_h = max(1, area // 150) if n_h is None else n_h
    n_dab = max(1, area // 300) if n_dab is None else n_dab
    yy, xx = np.mgrid[0:h, 0:w]
    c = rng.uniform(0, floor, size=(h * tile, w * tile, 2))
    blobs = np.zeros((h, w, 2))
    for k, count in enumerate((n_h, n_dab)):
        for _ in range(count):
            cy, cx, r, amp = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(2.5, 5.0), rng.uniform(1.0, 2.0)
            blobs[..., k] += amp * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * r * r))
    c += np.tile(blobs, (tile, tile, 1))
    img = Io * np.exp(-(c @ np.asarray(S).T)) + rng.normal(0, sigma, size=c.shape[:2] + (3,))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)
