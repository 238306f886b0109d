"""Writes tests/golden/detect_vectors.npz: scikit-learn DBSCAN(eps, min_samples=1) labels of designed point sets (duplicates,
pairs exactly eps apart, chains, single points), so the clustering contract is pinned where scikit-learn is not installed.

    python tests/golden/make_detect_golden.py
"""
import os

import numpy as np
from sklearn.cluster import DBSCAN

HERE = os.path.dirname(os.path.abspath(__file__))


def designed_sets():
    rng = np.random.RandomState(11)
    sets = [
        (np.array([[5, 5]]), 11.0),                                                  # one point
        (np.array([[5, 5], [5, 5], [5, 5], [40, 40], [40, 40]]), 11.0),              # duplicates
        (np.array([[0, 0], [0, 11], [11, 0], [30, 30], [30, 42]]), 11.0),            # exactly eps apart (joined), eps + 1 (not)
        (np.array([[10, 10], [13, 14], [50, 50], [53, 54]]), 5.0),                   # 3-4-5: diagonal exactly eps
        (np.array([[0, 10 * i] for i in range(12)] + [[100, 100]]), 10.0),           # chain of 12, then a loner
        (np.array([[0, 10 * i] for i in range(12)][::-1]), 10.0),                    # the chain in reverse index order
        (np.array([[60, 60], [0, 0], [60, 71], [0, 12], [60, 82], [0, 24]]), 11.0),  # interleaved chains, gap 12 > eps in one
        (np.array([[0, 0], [7, 8], [14, 16], [3, 200]]), 10.63014581273465),         # eps = sqrt(113) rounded: 7^2 + 8^2 = 113
        (rng.randint(0, 120, size=(200, 2)), 11.0),                                  # random, dense
        (rng.randint(0, 2000, size=(300, 2)), 15.0),                                 # random, sparse
    ]
    return sets


def main():
    pts, off, eps, labels = [], [0], [], []
    for p, e in designed_sets():
        lab = DBSCAN(eps=e, min_samples=1).fit_predict(p.astype(np.float64))
        pts.append(p.astype(np.int64))
        labels.append(lab.astype(np.int64))
        off.append(off[-1] + len(p))
        eps.append(e)
    np.savez_compressed(os.path.join(HERE, "detect_vectors.npz"), points=np.concatenate(pts), offsets=np.asarray(off, dtype=np.int64),
                        eps=np.asarray(eps, dtype=np.float64), labels=np.concatenate(labels))


if __name__ == "__main__":
    main()
