"""Writes tests/golden/score_vectors.npz: point lists and what the reference's own ``get_prf1`` (test_seg.py:120-141) with
``euclid_dist`` and ``precision_recall`` (metrics/metrics.py:56-66) returns for them.  The three functions are taken out of the
reference sources with ``ast`` and compiled alone into a namespace (test_seg.py itself parses a command line and loads a model
on import); nothing of their text is written anywhere, the file holds inputs and recorded results only.  numpy 2 has no
``np.Inf``, which get_prf1 names, so this process supplies it.  Before anything is written the restatement tests/score_ref.py
is asserted equal to the reference on every case and on 300 random ones.

    python tests/golden/make_score_golden.py [path/to/test_seg.py path/to/metrics/metrics.py]     (run on numpy 2.2.6)
"""
import ast
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import score_ref as S  # noqa: E402

REF = "/root/reference"
WANTED = {"get_prf1", "euclid_dist", "precision_recall"}


def reference_functions(paths):
    if not hasattr(np, "Inf"):
        np.Inf = np.inf
    ns = {"np": np}
    for path in paths:
        tree = ast.parse(open(path).read(), path)
        tree.body = [node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name in WANTED]
        exec(compile(tree, path, "exec"), ns)
    missing = WANTED - set(ns)
    assert not missing, f"not found in {paths}: {sorted(missing)}"
    return ns["get_prf1"]


def hand_written():
    """[(name, detections, annotations)], both (row, col)"""
    chain = np.stack([np.zeros(30, np.int64), 16 * np.arange(30)], axis=1)
    return [
        ("both_empty", [], []),
        ("no_detections_one_annotation", [], [(5, 5)]),
        ("one_detection_no_annotations", [(5, 5)], []),
        ("tie_goes_to_index_0", [(0, 0)], [(0, 16), (16, 0)]),
        ("d2_257_is_outside", [(0, 0)], [(1, 16)]),
        ("d2_244_is_inside", [(0, 0)], [(10, 12)]),
        ("duplicate_annotations", [(5, 5), (5, 5), (5, 5)], [(5, 5), (5, 5)]),
        ("duplicate_detections", [(5, 5), (5, 5)], [(5, 5)]),
        ("stolen_neighbour_next_inside", [(0, 1), (0, 2)], [(0, 0), (0, 10)]),
        ("stolen_neighbour_next_outside", [(0, 1), (0, 2)], [(0, 0), (0, 30)]),
        ("order_a_tp1", [(0, 10), (0, -10)], [(0, 0), (0, 20)]),
        ("order_b_tp2", [(0, -10), (0, 10)], [(0, 0), (0, 20)]),
        ("chain_30_shifted_by_8", chain + (0, 8), chain),
    ]


def cases():
    rng = np.random.RandomState(2024)
    out = [(f"random_{k:02d}", S.random_points(rng, rng.randint(0, 41), 64), S.random_points(rng, rng.randint(0, 41), 64)) for k in range(28)]
    return out + [(name, np.asarray(h, np.int64).reshape(-1, 2), np.asarray(g, np.int64).reshape(-1, 2)) for name, h, g in hand_written()]


def check(get_prf1, hat, gt):
    """the reference's answer, asserted equal to the restatement's -> (counts int64 [3], ratios float64 [3])"""
    p, r, f1, tp, fp, fn = get_prf1(hat if len(hat) else np.asarray([]), gt if len(gt) else np.asarray([]))
    mine = S.score(hat, gt)
    assert (int(tp), int(fp), int(fn)) == mine[:3], (hat, gt)
    ratios = np.asarray([p, r, f1], np.float64)
    assert ratios.tobytes() == S.prf(tp, fp, fn).tobytes()
    return np.asarray([tp, fp, fn], np.int64), ratios


def main():
    paths = sys.argv[1:] or [os.path.join(REF, "test_seg.py"), os.path.join(REF, "metrics", "metrics.py")]
    get_prf1 = reference_functions(paths)
    rng = np.random.RandomState(7)
    for _ in range(300):
        check(get_prf1, S.random_points(rng, rng.randint(0, 41), 64), S.random_points(rng, rng.randint(0, 41), 64))
    vec, names = {}, []
    for name, hat, gt in cases():
        counts, ratios = check(get_prf1, hat, gt)
        names.append(name)
        vec[f"{name}.hat"], vec[f"{name}.gt"], vec[f"{name}.counts"], vec[f"{name}.prf"] = hat, gt, counts, ratios
    vec["names"] = np.asarray(names)
    got = {n: tuple(vec[f"{n}.counts"]) for n in names}
    assert got["tie_goes_to_index_0"] == (1, 0, 1) and got["d2_257_is_outside"] == (0, 1, 1) and got["d2_244_is_inside"] == (1, 0, 0)
    assert got["stolen_neighbour_next_inside"] == (2, 0, 0) and got["stolen_neighbour_next_outside"] == (1, 1, 1)
    assert got["order_a_tp1"] == (1, 1, 1) and got["order_b_tp2"] == (2, 0, 0) and got["chain_30_shifted_by_8"] == (30, 0, 0)
    np.savez_compressed(os.path.join(HERE, "score_vectors.npz"), **vec)
    print(f"{len(names)} cases written")


if __name__ == "__main__":
    main()
