"""Writes tests/golden/spatial_vectors.npz: small integer point sets and what the brute-force restatement tests/spatial_ref.py
returns for them -- the k = 8 nearest neighbours, the counts within radii (0, 4.99, 5, 16) and the 7-pixel bin counts, among the
points themselves and, where the case has a second set, against it.  Inputs and recorded results only.

    python tests/golden/make_spatial_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import spatial_ref as R  # noqa: E402

HW = (61, 45)
K = 8
RADII = (0, 4.99, 5, 16)
BIN = 7


def hand_written():
    """[(name, points, other or None)], (row, col) on a 61 x 45 image"""
    lattice = np.stack(np.meshgrid(np.arange(8), np.arange(8), indexing="ij"), axis=-1).reshape(-1, 2)
    return [
        ("empty", [], None),
        ("one_point", [(5, 5)], None),
        ("two_points", [(5, 5), (5, 9)], None),
        ("tie_goes_to_the_lower_index", [(10, 10), (10, 15), (15, 10), (10, 5), (5, 10)], None),
        ("radius_5_edge_3_4_and_0_5", [(20, 20), (23, 24), (20, 25), (25, 25), (20, 26)], None),
        ("duplicates_are_neighbours_at_0", [(7, 7), (7, 7), (7, 7), (30, 30)], None),
        ("corners_and_borders", [(0, 0), (60, 44), (0, 44), (60, 0), (30, 0), (0, 22)], None),
        ("outside_points_are_not_live", [(5, 5), (-1, 5), (5, 45), (61, 0), (6, 6), (5, -1)], None),
        ("lattice_8x8", lattice, None),
        ("cross_same_coordinates", [(5, 5), (40, 40)], [(40, 40), (5, 5), (5, 6)]),
        ("cross_empty_targets", [(5, 5), (6, 6)], []),
        ("cross_empty_queries", [], [(5, 5)]),
    ]


def cases():
    rng = np.random.RandomState(2025)
    out = []
    for i in range(12):
        n, m = rng.randint(0, 60), rng.randint(0, 60)
        pts = np.stack([rng.randint(-2, HW[0] + 2, n), rng.randint(-2, HW[1] + 2, n)], axis=1)
        other = np.stack([rng.randint(0, HW[0], m), rng.randint(0, HW[1], m)], axis=1) if i % 2 else None
        out.append((f"random_{i:02d}", pts, other))
    return out + hand_written()


def record(pts, other):
    """name -> array for one case"""
    pts = np.asarray(pts, np.int64).reshape(-1, 2)
    v = {"pts": pts}
    v["index"], v["d2"] = R.nearest(pts, HW, K)
    v["counts"], v["pairs"] = R.count_within(pts, HW, RADII)
    v["bins"] = R.bin_counts(pts, HW, BIN)
    if other is not None:
        other = np.asarray(other, np.int64).reshape(-1, 2)
        v["other"] = other
        v["x_index"], v["x_d2"] = R.nearest(pts, HW, K, other=other)
        v["x_counts"], v["x_pairs"] = R.count_within(pts, HW, RADII, other=other)
    return v


def main():
    vec, names = {}, []
    for name, pts, other in cases():
        names.append(name)
        for key, a in record(pts, other).items():
            vec[f"{name}.{key}"] = a
    vec["names"] = np.asarray(names)
    assert vec["tie_goes_to_the_lower_index.index"][0, :4].tolist() == [1, 2, 3, 4]
    assert vec["radius_5_edge_3_4_and_0_5.counts"][0].tolist() == [0, 0, 2, 4]
    assert vec["duplicates_are_neighbours_at_0.d2"][0, :3].tolist() == [0, 0, 1058]
    assert vec["cross_same_coordinates.x_index"][0, :2].tolist() == [1, 2] and vec["cross_same_coordinates.x_d2"][0, 0] == 0
    np.savez_compressed(os.path.join(HERE, "spatial_vectors.npz"), **vec)
    print(f"{len(names)} cases written")


if __name__ == "__main__":
    main()
