"""Writes tests/golden/texture_vectors.npz: small uint8 planes with label images and what the numpy restatement
tests/texture_ref.py tabulates for them -- the co-occurrence tables of every label in the four directions.  Inputs and recorded
results only.

    python tests/golden/make_texture_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import texture_ref as T  # noqa: E402

TABLES = ("pairs", "diff", "sum", "marg", "sq", "cross", "matrix")


def cases():
    """[(name, dict)]: plane uint8 [N, H, W], labels int32 [N, H, W], levels, distance, capacity, want_matrix"""
    rng = np.random.RandomState(31)
    noise = lambda n, h, w: rng.randint(0, 256, size=(n, h, w)).astype(np.uint8)  # noqa: E731
    smooth = lambda n, h, w: (np.add.outer(np.arange(h) * 5, np.arange(w) * 3)[None] + rng.randint(0, 24, size=(n, h, w))).astype(np.uint8)  # noqa: E731
    wide = T.blocks(40, 130, seed=5, n_labels=9)[None]
    strip = T.blocks(5, 129, seed=6, n_labels=4, gaps=False)[None]
    batch = np.stack([T.blocks(17, 65, seed=s, n_labels=3 + s) for s in range(3)])
    return [
        ("hand_3x4", dict(plane=T.HAND_PLANE, labels=T.HAND_LABELS, levels=8, distance=1, capacity=2, want_matrix=True)),
        ("strip_5x129", dict(plane=noise(1, 5, 129), labels=strip, levels=16, distance=2, capacity=4, want_matrix=True)),
        ("batch3_17x65", dict(plane=smooth(3, 17, 65), labels=batch, levels=32, distance=1, capacity=5, want_matrix=False)),
        ("wide_40x130_short", dict(plane=noise(1, 40, 130), labels=wide, levels=16, distance=3, capacity=6, want_matrix=False)),
    ]


def record(case):
    out = T.texture(case["plane"], case["labels"], case["capacity"], case["levels"], case["distance"], case["want_matrix"])
    rec = {"plane": case["plane"], "labels": case["labels"], "levels": np.asarray(case["levels"]), "distance": np.asarray(case["distance"]),
           "capacity": np.asarray(case["capacity"]), "want_matrix": np.asarray(case["want_matrix"])}
    rec.update(out)
    return rec


def build():
    vec, names = {}, []
    for name, case in cases():
        names.append(name)
        for key, a in record(case).items():
            vec[f"{name}.{key}"] = a
    vec["names"] = np.asarray(names)
    return vec


def main():
    vec = build()
    assert int(vec["wide_40x130_short.labels"].max()) > 6, "the short table leaves labels above its capacity"
    assert (vec["batch3_17x65.pairs"] > 0).any() and vec["strip_5x129.matrix"].shape == (1, 4, 4, 16, 16)
    path = os.path.join(HERE, "texture_vectors.npz")
    np.savez_compressed(path, **vec)
    print(f"{len(vec['names'])} cases written, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
