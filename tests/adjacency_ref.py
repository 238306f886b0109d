"""The numpy statement of ``regions.adjacency_labels``: per image the dense (cap + 1) x (cap + 1) tables of sides and corners, every
rule applied to them in Python integers.  It shares nothing with the device's hash table or its runs; only for small label counts.

Input: int32 label images [H, W] or [N, H, W].  All rules are exact integers, per image:

  id           a pixel's id is its label when 1 <= label <= cap, else 0 (a label above the capacity is background; counts still
               reports the largest label)
  sides        every unordered pair of 4-adjacent pixels of the image is one interior side; a pixel side on the image edge is an
               exterior side of that pixel
  sides(a, b)  a < b both positive: the interior sides whose two ids are {a, b}
  corners(a, b) connectivity 2 only, else 0: the unordered diagonal pixel pairs {(r, c), (r + 1, c + 1)} and {(r, c + 1), (r + 1, c)}
               whose ids are {a, b}, whether or not the two labels also share a side
  listed       sides > 0 (connectivity 1), sides + corners > 0 (connectivity 2)
  per label a  n_neighbors = the listed pairs that contain a; contact = the sum of sides over them; background = the interior
               sides with ids {a, 0}; outside = the exterior sides of a's pixels; partner / partner_sides = the listed neighbour of
               largest sides, ties to the lower label, and that count; partner 0 without a neighbour; all zero without pixels
  identity     contact + background + outside = 4 area - 2 (interior sides with both ids a)

By hand:   1 1 2     sides (1,2)=1 (1,3)=2 (2,3)=2; corners at connectivity 2 (1,2)=1 (1,3)=2 (2,3)=2; background [1, 0, 1];
           1 3 2     outside [4, 3, 3]; contact [3, 3, 4]; n_neighbors [2, 2, 2]; partner [3, 3, 1] (label 3's neighbours tie at 2
           0 3 3     sides: the lower label)
"""
import numpy as np

TABLES = ("counts", "n_pairs", "n_neighbors", "contact", "background", "outside", "partner", "partner_sides")
PAIRS = ("image", "a", "b", "sides", "corners")


def _pair_table(x, y, cap):
    """ids x against ids y, elementwise -> int64 [cap + 1, cap + 1], symmetric: tab[a, b] = the positions with ids {a, b}, a != b;
    tab[a, a] = the positions with both ids a"""
    tab = np.zeros((cap + 1, cap + 1), np.int64)
    np.add.at(tab, (x.ravel(), y.ravel()), 1)
    return tab + tab.T - np.diag(np.diag(tab))


def adjacency(labels, cap=None, connectivity=1):
    """-> dict: the TABLES (int32; counts and n_pairs [N], the others [N, cap]), cap (None: the largest label of the batch, at least
    1), connectivity, area and same_sides int64 [N, cap] (for the identity), and pairs = (image, a, b, sides, corners) int64, sorted"""
    labels = np.asarray(labels)
    assert labels.ndim in (2, 3) and connectivity in (1, 2)
    if labels.ndim == 2:
        labels = labels[None]
    labels = labels.astype(np.int64)
    N, H, W = labels.shape
    counts = np.maximum(labels.reshape(N, -1).max(axis=1), 0)
    cap = max(1, int(counts.max())) if cap is None else int(cap)
    out = {"counts": counts.astype(np.int32), "cap": cap, "connectivity": connectivity, "n_pairs": np.zeros((N,), np.int32),
           "area": np.zeros((N, cap), np.int64), "same_sides": np.zeros((N, cap), np.int64)}
    for k in TABLES[2:]:
        out[k] = np.zeros((N, cap), np.int32)
    listed = []
    for n in range(N):
        ids = np.where((labels[n] >= 1) & (labels[n] <= cap), labels[n], 0)
        sides = _pair_table(ids[:, :-1], ids[:, 1:], cap) + _pair_table(ids[:-1, :], ids[1:, :], cap)
        corners = np.zeros_like(sides)
        if connectivity == 2:
            corners = _pair_table(ids[:-1, :-1], ids[1:, 1:], cap) + _pair_table(ids[:-1, 1:], ids[1:, :-1], cap)
        edge = np.zeros((H, W), np.int64)                                  # the exterior sides of every pixel
        edge[0, :] += 1
        edge[-1, :] += 1
        edge[:, 0] += 1
        edge[:, -1] += 1
        for a in range(1, cap + 1):
            out["area"][n, a - 1] = int((ids == a).sum())
            out["same_sides"][n, a - 1] = int(sides[a, a])
            out["background"][n, a - 1] = int(sides[a, 0])
            out["outside"][n, a - 1] = int(edge[ids == a].sum())
            best = (0, 0)                                                  # (sides, partner)
            for b in range(1, cap + 1):                                    # ascending: only a strictly larger count replaces
                s, k = int(sides[a, b]), int(corners[a, b])
                if b == a or s + k == 0:
                    continue
                out["n_neighbors"][n, a - 1] += 1
                out["contact"][n, a - 1] += s
                if best[1] == 0 or s > best[0]:
                    best = (s, b)
                if a < b:
                    listed.append((n, a, b, s, k))
                    out["n_pairs"][n] += 1
            out["partner_sides"][n, a - 1], out["partner"][n, a - 1] = best
    out["pairs"] = tuple(np.asarray([row[k] for row in listed], np.int64) for k in range(5))
    return out


def boundary(t):
    return t["contact"] + t["background"] + t["outside"]


def hand_cases():
    """name -> (labels int32 [H, W], cap or None): worked by hand (tests/test_adjacency_host.py has the answers)"""
    a = lambda rows: np.asarray(rows, np.int32)  # noqa: E731
    return {
        "three": (a([[1, 1, 2], [1, 3, 2], [0, 3, 3]]), None),
        "one_row": (a([[1, 1, 2, 0, 2, 3]]), None),
        "one_column": (a([[1], [2], [2], [0], [1]]), None),
        "empty": (a([[0, 0, 0], [0, 0, 0]]), None),
        "single_pixel": (a([[1]]), None),
        "corner_only": (a([[1, 0], [0, 2]]), None),
        "disconnected": (a([[1, 2, 1], [0, 2, 0], [1, 2, 3]]), None),
        "non_positive": (a([[1, -3, 2], [1, 0, 2], [-1, -1, 2]]), None),
        "above_capacity": (a([[1, 1, 5], [2, 4, 5], [2, 3, 3]]), 3),
    }


def stacked(cases=None):
    """the hand cases that take their own capacity, each padded with background to the largest, as one batch ->
    (names, labels int32 [N, H, W])"""
    cases = hand_cases() if cases is None else cases
    cases = {k: lab for k, (lab, cap) in cases.items() if cap is None}
    H, W = max(x.shape[0] for x in cases.values()), max(x.shape[1] for x in cases.values())
    return list(cases), np.stack([np.pad(x, ((0, H - x.shape[0]), (0, W - x.shape[1]))) for x in cases.values()])
