"""Writes tests/golden/quantify_vectors.npz: small RGB images with label images and what the numpy restatement
tests/quantify_ref.py tabulates for them -- the quantised stain matrices and the per-(label, compartment) tables of integer stain
levels.  Inputs and recorded results only.

    python tests/golden/make_quantify_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import quantify_ref as Q  # noqa: E402

TABLES = ("counts", "n", "sum", "sumsq", "max", "pos", "hist")
OTHER = np.stack([Q.DAB_VEC, Q.H_VEC[[2, 0, 1]]], axis=1)                  # stains of its own for one member of the batch


def cases():
    """[(name, dict)]: images uint8 [N, H, W, 3], labels int32 [N, H, W], optionally expanded; stains (a list of N [3, 2]
    matrices), residual, conc_max, pixel_threshold (or None), bins, capacity"""
    rng = np.random.RandomState(23)
    noise = lambda n, h, w: rng.randint(0, 256, size=(n, h, w, 3)).astype(np.uint8)  # noqa: E731
    hand = np.asarray([[1, 1, 2], [1, 2, 2], [0, -1, 2]], np.int32)[None]
    wide = Q.blocks(64, 130, seed=5, n_labels=9)[None]
    strip = Q.blocks(5, 129, seed=6, n_labels=4, gaps=False)[None]
    batch = np.stack([Q.blocks(17, 65, seed=s, n_labels=3 + s) for s in range(3)])
    return [
        ("hand_3x3", dict(images=noise(1, 3, 3), labels=hand, stains=[Q.HDAB], residual=False, conc_max=8.0, pixel_threshold=(1.0, 1.0),
                          bins=16, capacity=2)),
        ("strip_5x129_ring", dict(images=noise(1, 5, 129), labels=strip, expanded=np.stack([Q.grow(strip[0], 3)]), stains=[Q.HDAB],
                                  residual=False, conc_max=2.5, pixel_threshold=(0.5, 0.25), bins=16, capacity=4)),
        ("batch3_17x65_k3", dict(images=noise(3, 17, 65), labels=batch, stains=[Q.HDAB, OTHER, Q.HDAB[:, ::-1]], residual=True, conc_max=8.0,
                                 pixel_threshold=(2.0, 1.5, 0.1), bins=256, capacity=5)),
        ("wide_64x130_short", dict(images=noise(1, 64, 130), labels=wide, expanded=np.stack([Q.grow(wide[0], 2)]), stains=[OTHER],
                                   residual=False, conc_max=0.7, pixel_threshold=None, bins=0, capacity=6)),
    ]


def record(case):
    Mq = np.stack([Q.quantised_matrix(S, case["residual"], case["conc_max"]) for S in case["stains"]])
    levels = None if case["pixel_threshold"] is None else Q.positive_levels(case["pixel_threshold"], case["conc_max"])
    out = Q.quantify(case["images"], case["labels"], Mq, case["capacity"], case.get("expanded"), levels, case["bins"])
    rec = {"images": case["images"], "labels": case["labels"], "stains": np.stack(case["stains"]), "residual": np.asarray(case["residual"]),
           "conc_max": np.asarray(case["conc_max"]), "bins": np.asarray(case["bins"]), "capacity": np.asarray(case["capacity"]),
           "Mq": Mq.astype(np.int32)}
    if "expanded" in case:
        rec["expanded"] = case["expanded"]
    if levels is not None:
        rec["pixel_threshold"], rec["pos_levels"] = np.asarray(case["pixel_threshold"], np.float64), np.asarray(levels, np.int64)
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
    assert int(vec["wide_64x130_short.counts"][0]) > 6, "the short table leaves labels above its capacity"
    assert (vec["strip_5x129_ring.n"][0, :, 1] > 0).any() and vec["batch3_17x65_k3.sum"].shape == (3, 5, 1, 3)
    path = os.path.join(HERE, "quantify_vectors.npz")
    np.savez_compressed(path, **vec)
    print(f"{len(names_of(vec))} cases written, {os.path.getsize(path)} bytes")


def names_of(vec):
    return [str(n) for n in vec["names"]]


if __name__ == "__main__":
    main()
