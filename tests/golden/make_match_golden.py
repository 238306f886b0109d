"""Writes tests/golden/match_vectors.npz: small pairs of label images and what tests/match_ref.py (a dense contingency table, every
pair tried) makes of them -- the tables of ``regions.match_labels`` and the scores at IoU thresholds 0.5, 0.75 and 1.  The host
test checks the reference against these bytes, so a change of the reference's behaviour shows; the GPU test checks the kernels
against the same bytes.

    python tests/golden/make_match_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import match_ref as M  # noqa: E402
import regions_ref as R  # noqa: E402

THRESHOLDS = (0.5, 0.75, 1.0)


def cases():
    """name -> (pred, truth int32 [N, H, W], cap_pred or None, cap_truth or None)"""
    for name, (pred, truth, cp, ct) in M.hand_cases().items():
        yield name, (pred[None], truth[None], cp, ct)
    b = M.blocks(16, 16)
    cleared = b.copy()
    cleared[1::2, 1::2] = 0
    yield "blocks_cleared", (b[None], cleared[None], None, None)
    yield "blocks_rolled", (b[None], np.roll(b, 1, axis=1)[None], None, None)
    masks = R.blobs(3, 63, 65, seed=11, density=1 / 150.0)
    pred, truth = M.noisy_pair(masks, 12, lambda m: R.label(m)[0])
    yield "blobs", (pred, truth, None, None)
    yield "blobs_capped", (pred, truth, 3, 5)


def main():
    out = {}
    for name, (pred, truth, cp, ct) in cases():
        t = M.match(pred, truth, cp, ct)
        out[f"{name}.pred"], out[f"{name}.truth"] = pred, truth
        out[f"{name}.caps"] = np.asarray([t["cap_pred"], t["cap_truth"]], np.int32)
        for key in M.TABLES:
            out[f"{name}.{key}"] = t[key]
        for thr in THRESHOLDS:
            s = M.score(t, thr)
            for key in M.SCORES:
                out[f"{name}.score{thr}.{key}"] = s[key]
    path = os.path.join(HERE, "match_vectors.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
