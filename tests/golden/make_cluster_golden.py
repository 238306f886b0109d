"""Writes tests/golden/cluster_vectors.npz: small integer point sets on a 61 x 45 image with eps, min_samples and what
scikit-learn's ``DBSCAN(eps, min_samples, algorithm="brute")`` returns for them on float64 points -- labels and core flags, and the
per-cluster tables formed from those two -- and asserts that the restatement tests/cluster_ref.py agrees.  The radii are integers
or x.5, so that floor(eps^2) and scikit-learn's float eps * eps admit the same integer d2.  Inputs and recorded results only.

    python tests/golden/make_cluster_golden.py
"""
import os
import sys

import numpy as np
from sklearn.cluster import DBSCAN

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import cluster_ref as C  # noqa: E402

HW = (61, 45)
COLUMNS = ("labels", "core", "n_clusters", "size", "n_core", "sums", "bbox")


def clump(rng, centre, n, spread):
    p = np.asarray(centre) + rng.randint(-spread, spread + 1, size=(n, 2))
    return np.clip(p, 0, np.asarray(HW) - 1)


def cases():
    """[(name, points (row, col), eps, min_samples)]"""
    rng = np.random.RandomState(77)
    uniform = lambda n: np.stack([rng.randint(0, HW[0], n), rng.randint(0, HW[1], n)], axis=1)  # noqa: E731
    lattice = np.stack(np.meshgrid(np.arange(8), np.arange(8), indexing="ij"), axis=-1).reshape(-1, 2) * 3 + 2
    left = np.asarray([(20, 18), (19, 18), (21, 18), (20, 17), (19, 17), (21, 17), (20, 16)])
    two = np.concatenate([[(20, 22)], left, left * (1, -1) + (0, 44)])    # row 0 is 4 from (20, 18) and from its mirror image (20, 26)
    return [
        ("empty", np.zeros((0, 2), np.int64), 3, 2),
        ("all_noise", [(2, 2), (2, 10), (30, 30), (50, 5), (58, 40)], 5, 2),
        ("duplicates", [(7, 7), (7, 7), (7, 7), (30, 30), (7, 8), (30, 30), (40, 40)], 0.5, 2),     # d2 == 0 only; scikit-learn refuses eps = 0
        ("d2_equals_r2", [(20, 20), (23, 24), (20, 30), (40, 10), (40, 15), (45, 15), (45, 21)], 5, 2),
        ("border_between_two_clusters", two, 4, 5),
        ("lattice_ties_and_duplicates", np.concatenate([lattice, lattice[[0, 9, 9, 27, 63]]]), 3, 5),
        ("random_min_samples_1", uniform(70), 4.5, 1),
        ("random_min_samples_2", uniform(90), 3.5, 2),
        ("random_min_samples_5", uniform(150), 5, 5),
        ("clumps_min_samples_5", np.concatenate([clump(rng, (15, 12), 30, 4), clump(rng, (40, 30), 40, 5), uniform(30)]), 2.5, 5),
    ]


def tables(pts, labels, core):
    """the columns of spatial.ClusterTable for one image from scikit-learn's labels and core flags"""
    P, C_ = len(pts), int(labels.max()) + 1 if len(labels) else 0
    v = {"labels": labels.astype(np.int32), "core": core.astype(np.uint8), "n_clusters": np.asarray([C_], np.int32),
         "size": np.zeros(P, np.int32), "n_core": np.zeros(P, np.int32), "sums": np.zeros((P, 2), np.int64),
         "bbox": np.zeros((P, 4), np.int32)}
    for c in range(C_):
        mine = pts[labels == c]
        v["size"][c], v["n_core"][c], v["sums"][c] = len(mine), int(core[labels == c].sum()), mine.sum(axis=0)
        v["bbox"][c] = (*mine.min(axis=0), *(mine.max(axis=0) + 1))
    return v


def record(pts, eps, min_samples):
    pts = np.asarray(pts, np.int64).reshape(-1, 2)
    labels, core = np.zeros(0, np.int64), np.zeros(0, bool)
    if len(pts):
        fit = DBSCAN(eps=float(eps), min_samples=min_samples, algorithm="brute").fit(pts.astype(np.float64))
        labels = fit.labels_
        core = np.zeros(len(pts), bool)
        core[fit.core_sample_indices_] = True
    v = tables(pts, labels, core)
    ours = C.cluster(pts, HW, eps, min_samples)
    for k in COLUMNS:
        assert v[k].dtype == ours[k].dtype and np.array_equal(v[k], ours[k]), k
    return {"pts": pts, "eps": np.float64(eps), "min_samples": np.int64(min_samples), **v}


def main():
    vec, names = {}, []
    for name, pts, eps, min_samples in cases():
        names.append(name)
        for key, a in record(pts, eps, min_samples).items():
            vec[f"{name}.{key}"] = a
    vec["names"] = np.asarray(names)
    assert vec["all_noise.labels"].tolist() == [-1] * 5 and vec["all_noise.n_clusters"][0] == 0
    assert vec["duplicates.labels"].tolist() == [0, 0, 0, 1, -1, 1, -1]
    assert vec["d2_equals_r2.labels"].tolist() == [0, 0, -1, 1, 1, 1, -1]
    b = "border_between_two_clusters"
    assert vec[f"{b}.n_clusters"][0] == 2 and vec[f"{b}.core"][0] == 0 and vec[f"{b}.labels"][0] == 0
    assert sorted(set(vec[f"{b}.labels"][1:8])) == [0] and sorted(set(vec[f"{b}.labels"][8:])) == [1]
    assert vec["random_min_samples_1.core"].all() and (vec["random_min_samples_5.labels"] == -1).any()
    np.savez_compressed(os.path.join(HERE, "cluster_vectors.npz"), **vec)
    print(f"{len(names)} cases written")


if __name__ == "__main__":
    main()
