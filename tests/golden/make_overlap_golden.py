"""Writes tests/golden/overlap_vectors.npz: small pairs of label images and what tests/overlap_ref.py (a dense contingency table,
every rule in Python integers) makes of them -- the tables and the pair list of ``regions.overlap_labels`` and the AJI / object-level
Dice of ``OverlapTable.score``.  The host test checks the reference against these bytes, so a change of the reference's behaviour
shows; the GPU test checks the kernels against the same bytes.

    python tests/golden/make_overlap_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import match_ref as M  # noqa: E402
import overlap_ref as O  # noqa: E402
import regions_ref as R  # noqa: E402


def cases():
    """name -> (pred, truth int32 [N, H, W], cap_pred or None, cap_truth or None)"""
    _, pred, truth = O.stacked()
    yield "hand", (pred, truth, None, None)
    b = M.blocks(16, 16)
    yield "blocks_rolled", (np.roll(b, (1, 1), axis=(0, 1))[None], b[None], None, None)
    masks = R.blobs(3, 63, 65, seed=11, density=1 / 150.0)
    pred, truth = M.noisy_pair(masks, 12, lambda m: R.label(m)[0])
    yield "blobs", (pred, truth, None, None)
    yield "blobs_capped", (pred, truth, 3, 5)


def main():
    out = {}
    for name, (pred, truth, cp, ct) in cases():
        t = O.overlap(pred, truth, cp, ct)
        out[f"{name}.pred"], out[f"{name}.truth"] = pred, truth
        out[f"{name}.caps"] = np.asarray([t["cap_pred"], t["cap_truth"]], np.int32)
        for key in O.TABLES:
            out[f"{name}.{key}"] = t[key]
        for key, col in zip(O.PAIRS, t["pairs"]):
            out[f"{name}.pair_{key}"] = col
        s = O.score(t)
        for key in O.SCORES:
            out[f"{name}.score.{key}"] = s[key]
    path = os.path.join(HERE, "overlap_vectors.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
