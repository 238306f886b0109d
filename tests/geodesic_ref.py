"""Plain-loop statement of the geodesic seeded split (cellsegmentation_amd.regions.split_geodesic), the reference of
tests/test_geodesic_gpu.py, tests/golden/geodesic_vectors.npz and tools/regions_microbench.py --split --geodesic.  Components come
from ``scipy.ndimage.label``; seeds, limits, ``live`` and the numbering of the seedless components are those of tests/split_ref.py;
the core is a heap Dijkstra on the key (dist, k).

The rule (regions.split_geodesic's docstring): a step goes from a foreground pixel to a foreground pixel of its 8-neighbourhood, an
axial step costs 5 and a diagonal one 7; with connectivity 1 a diagonal step (r, c) -> (r + dr, c + dc) is allowed only if
(r + dr, c) or (r, c + dc) is foreground.  dist(p, k) = the cheapest path from live seed k to p, and p gets 1 + the k that minimises
(dist(p, k), k).  ``jacobi_rounds`` models the tiled relaxation of csrc/regions.hip with every tile reading the previous round's halo.
"""
import heapq

import numpy as np
from scipy import ndimage as ndi

import split_ref as S

AXIAL, DIAGONAL = 5, 7
STEPS = [(dr, dc, DIAGONAL if dr and dc else AXIAL) for dr in (-1, 0, 1) for dc in (-1, 0, 1) if dr or dc]
UNREACHED = (1 << 64) - 1


def _allowed(m, r, c, dr, dc, connectivity):
    """the step (r, c) -> (r + dr, c + dc) between two foreground pixels of m"""
    return connectivity == 2 or dr == 0 or dc == 0 or bool(m[r + dr, c]) or bool(m[r, c + dc])


def _dijkstra(m, sources, connectivity, window=None):
    """sources: {(r, c): (dist, k)} -> {(r, c): (dist, k)}, the lexicographic minimum over all paths from a source.  window
    (r0, r1, c0, c1): only pixels inside it are relaxed; sources outside it still push into it (a tile and its halo)."""
    H, W = m.shape
    r0, r1, c0, c1 = (0, H, 0, W) if window is None else window
    best = dict(sources)
    heap = [(d, k, r, c) for (r, c), (d, k) in sources.items()]
    heapq.heapify(heap)
    while heap:
        d, k, r, c = heapq.heappop(heap)
        if best[(r, c)] != (d, k):
            continue
        for dr, dc, w in STEPS:
            rr, cc = r + dr, c + dc
            if not (r0 <= rr < r1 and c0 <= cc < c1 and m[rr, cc]) or not _allowed(m, r, c, dr, dc, connectivity):
                continue
            if (d + w, k) < best.get((rr, cc), (UNREACHED, 0)):
                best[(rr, cc)] = (d + w, k)
                heapq.heappush(heap, (d + w, k, rr, cc))
    return best


def _live_sources(m, seeds):
    """{(r, c): (0, k)} of the live seeds, the lowest k of a pixel that holds several; live bool [S']"""
    H, W = m.shape
    sources, live = {}, np.zeros(len(seeds), bool)
    for k, (r, c) in enumerate(seeds):
        if 0 <= r < H and 0 <= c < W and m[r, c]:
            live[k] = True
            sources.setdefault((int(r), int(c)), (0, k))
    return sources, live


def split_one(m, seeds, connectivity=1):
    """m bool [H, W]; seeds int [S', 2], already cut to the limit -> (labels int32, count, live bool [S'], distance int32: the
    chamfer cost to the owner, 0 on the background, -1 on a component without a live seed)"""
    m = np.asarray(m, bool)
    seeds = np.asarray(seeds, np.int64).reshape(-1, 2)
    comp, n_comp = ndi.label(m, structure=S.STRUCTURE[connectivity])
    sources, live = _live_sources(m, seeds)
    labels, dist = np.zeros(m.shape, np.int32), np.zeros(m.shape, np.int32)
    for (r, c), (d, k) in _dijkstra(m, sources, connectivity).items():
        labels[r, c], dist[r, c] = k + 1, d
    seeded = np.zeros(n_comp + 1, bool)
    for r, c in sources:
        seeded[comp[r, c]] = True
    seedless = ~seeded
    seedless[0] = False
    number = np.where(seedless, len(seeds) + np.cumsum(seedless), 0).astype(np.int32)      # in scipy's order, after the seeds
    labels, dist = np.where(seedless[comp], number[comp], labels), np.where(seedless[comp], -1, dist).astype(np.int32)
    assert np.array_equal(labels > 0, m)                    # every pixel of a seeded component was reached
    return labels, len(seeds) + int(seedless.sum()), live, dist


def split(m, points, offsets=None, limits=None, connectivity=1):
    """split_ref.split's arguments -> its dict plus ``distance`` int32 of m's shape"""
    m = np.asarray(m, bool)
    ms = m[None] if m.ndim == 2 else m
    points = np.asarray(points, np.int64).reshape(-1, 2)
    off = np.asarray([0, len(points)] if offsets is None else offsets, np.int64)
    assert len(off) == len(ms) + 1
    lim = [None] * len(ms) if limits is None else np.broadcast_to(np.asarray(limits), (len(ms),))
    labels, dist = np.zeros(ms.shape, np.int32), np.zeros(ms.shape, np.int32)
    counts, seeds_n, live = np.zeros(len(ms), np.int32), np.zeros(len(ms), np.int32), np.zeros(len(points), bool)
    for n, x in enumerate(ms):
        s = S.n_seeds(off[n + 1] - off[n], lim[n])
        labels[n], counts[n], live[off[n]:off[n] + s], dist[n] = split_one(x, points[off[n]:off[n] + s], connectivity)
        seeds_n[n] = s
    two_d = m.ndim == 2
    return {"labels": labels[0] if two_d else labels, "counts": counts, "n_seeds": seeds_n, "live": live,
            "distance": dist[0] if two_d else dist}


def jacobi_rounds(m, seeds, connectivity=1, tile=64, want_state=False):
    """The rounds of the tiled relaxation when every tile sees its neighbours' keys as the previous round left them: in a round
    every tile takes its own keys and a one-pixel halo from the state before the round and relaxes to its fixpoint.  -> the number
    of rounds, the first one in which nothing changes included (with ``want_state``: and the final {pixel: (dist, k)})."""
    m = np.asarray(m, bool)
    H, W = m.shape
    state, _ = _live_sources(m, np.asarray(seeds, np.int64).reshape(-1, 2))
    rounds = 0
    while True:
        rounds += 1
        new = {}
        for r0 in range(0, H, tile):
            for c0 in range(0, W, tile):
                r1, c1 = min(r0 + tile, H), min(c0 + tile, W)
                near = {p: v for p, v in state.items() if r0 - 1 <= p[0] <= r1 and c0 - 1 <= p[1] <= c1}
                for p, v in _dijkstra(m, near, connectivity, (r0, r1, c0, c1)).items():
                    if r0 <= p[0] < r1 and c0 <= p[1] < c1:
                        new[p] = v
        if new == state:
            return (rounds, state) if want_state else rounds
        state = new


def disconnected_labels(labels):
    """the positive labels whose pixel set is not one 8-connected piece"""
    labels = np.asarray(labels)
    return [int(k) for k in np.unique(labels[labels > 0]) if ndi.label(labels == k, structure=np.ones((3, 3), bool))[1] != 1]


# ---- shapes shared by the golden vectors and the tests ----------------------------------------------------------------------------
two_discs, foreign_seed = S.two_discs, S.foreign_seed


def horseshoe():
    """70 x 90: a U whose right arm straddles the tile edge at column 64 and whose base ends 2 rows short of the edge at row 64;
    one seed at the top of the left arm, one in the middle of the base -> (mask, points)"""
    m = np.zeros((70, 90), bool)
    m[8:62, 10:80] = True
    m[8:50, 22:68] = False
    return m, np.asarray([[12, 15], [56, 45]], np.int64)


def serpentine():
    """37 x 130: a one-pixel path of 17 horizontal runs over columns 60 .. 68 on rows 2, 4, ..., 34, joined alternately at either
    end, its seed at (2, 60): 169 pixels that cross the tile edge between columns 63 and 64 seventeen times -> (mask, points)"""
    m = np.zeros((37, 130), bool)
    for i, r in enumerate(range(2, 35, 2)):
        m[r, 60:69] = True
        if r < 34:
            m[r + 1, 68 if i % 2 == 0 else 60] = True
    return m, np.asarray([[2, 60]], np.int64)


def noise_masks(n, H, W, seed, density=0.7):
    """n random masks: uniform noise of the given density, opened by a 3 x 3 square -- clumps with necks, bays and holes"""
    rng = np.random.RandomState(seed)
    return np.stack([ndi.binary_opening(rng.rand(H, W) < density, structure=np.ones((3, 3), bool)) for _ in range(n)])
