"""Times the neighbourhood queries of cellsegmentation_amd.spatial (csrc/spatial.hip) on an MI355X: device events around the whole
call -- uploads excluded, the points are device tensors -- median of 7 after a warm-up.

    python tools/spatial_microbench.py [--json PATH] [--quick]
    python tools/spatial_microbench.py --cluster [--json PATH]

Workloads: 128 images of 299^2 with about 80 points each (the workload of the ``regions.split`` table), one 4096^2 image with 10^4
and 10^5 uniformly placed points, and the same 10^5 points in 100 tight clumps.  Each runs ``nearest`` (k = 1 and 8) and
``count_within`` (radius 16 and 64) three ways:

    grid     the bucket side of ``spatial.choose_bucket``
    single   ``_bucket=max(H, W)``: one bucket per image, i.e. all pairs through the same inner loop -- what the grid buys
             (3 repetitions on the 10^5-point rows, where one workgroup does 10^10 pair tests)
    kdtree   ``scipy.spatial.cKDTree`` on the host, the copy of the points to the host included

Every row reports the bucket side, the buckets per image and the largest bucket occupancy, and whether grid and single agree bit
for bit (and, for the distances and counts, with the tree).  ``--quick`` leaves out the single-bucket runs of the 10^5-point rows.

``--cluster`` times ``spatial.cluster`` (DBSCAN, min_samples 5, eps 16 and 64) on the same point sets instead, next to two
yardsticks: ``spatial.count_within`` at the same radius on the same points -- the cost of one box walk, of which the cluster call
makes three plus the grid build, the numbering and the table pass -- and the host library on the same box, the copy of the points
to the host included: ``sklearn.cluster.DBSCAN`` image by image, or, where scikit-learn is absent, ``scipy.spatial.cKDTree`` pairs
and ``scipy.sparse.csgraph.connected_components`` over the core points (the clusters without their border points).  The host run
is left out where the pairs within eps, which ``count_within`` has just counted, pass 5 x 10^7: its neighbour lists would not fit.
Every row says whether the labels equal the host library's."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cellsegmentation_amd import spatial as S  # noqa: E402


def time_dev(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def time_host(fn, reps=3):
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts)), out


def workloads():
    """[(name, points [P, 2], offsets [N + 1], (H, W))]"""
    rng = np.random.RandomState(0)
    n = rng.randint(60, 101, size=128)
    off = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    out = [("128 x 299^2, ~80 points each", rng.randint(0, 299, size=(int(off[-1]), 2)), off, (299, 299))]
    for P in (10 ** 4, 10 ** 5):
        out.append((f"4096^2, {P} uniform", rng.randint(0, 4096, size=(P, 2)), np.asarray([0, P], np.int64), (4096, 4096)))
    centres = rng.randint(64, 4096 - 64, size=(100, 2))
    clumps = np.clip(centres[rng.randint(0, 100, size=10 ** 5)] + np.rint(rng.normal(0, 12, size=(10 ** 5, 2))).astype(np.int64), 0, 4095)
    out.append(("4096^2, 100000 in 100 clumps", clumps, np.asarray([0, 10 ** 5], np.int64), (4096, 4096)))
    return out


def kdtree(dev_pts, off, k=None, radius=None):
    """the host yardstick: copy, one tree per image, the query -> (d2 int64 [P, k] | None, counts int64 [P] | None)"""
    from scipy.spatial import cKDTree
    pts = dev_pts.cpu().numpy().astype(np.float64)
    d2s, cnts = [], []
    for n in range(len(off) - 1):
        p = pts[off[n]:off[n + 1]]
        tree = cKDTree(p)
        if k is not None:
            d, _ = tree.query(p, k=k + 1)
            d2s.append(np.rint(d[:, 1:] ** 2).astype(np.int64))
        else:
            cnts.append(np.asarray(tree.query_ball_point(p, np.sqrt(radius * radius + 0.5), return_length=True), np.int64) - 1)
    return (np.concatenate(d2s), None) if k is not None else (None, np.concatenate(cnts))


MAX_HOST_PAIRS = 5 * 10 ** 7


def host_dbscan(dev_pts, off, eps, min_samples):
    """the host yardstick: copy, then image by image -> (labels int64 [P] | None, core bool [P], library name).  Without
    scikit-learn the labels are None: the components of the core points are timed, border points are not assigned."""
    pts = dev_pts.cpu().numpy().astype(np.float64)
    labels, core = np.full(len(pts), -1, np.int64), np.zeros(len(pts), bool)
    try:
        from sklearn.cluster import DBSCAN
    except ImportError:
        DBSCAN = None
    for n in range(len(off) - 1):
        p = pts[off[n]:off[n + 1]]
        if not len(p):
            continue
        if DBSCAN is not None:
            fit = DBSCAN(eps=np.sqrt(eps * eps + 0.5), min_samples=min_samples).fit(p)
            labels[off[n]:off[n + 1]] = fit.labels_
            core[off[n] + fit.core_sample_indices_] = True
            continue
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        from scipy.spatial import cKDTree
        pairs = cKDTree(p).query_pairs(np.sqrt(eps * eps + 0.5), output_type="ndarray")
        c = np.bincount(pairs.ravel(), minlength=len(p)) + 1 >= min_samples
        keep = pairs[c[pairs[:, 0]] & c[pairs[:, 1]]]
        connected_components(coo_matrix((np.ones(len(keep), bool), (keep[:, 0], keep[:, 1])), shape=(len(p), len(p))), directed=False)
        core[off[n]:off[n + 1]] = c
    return (labels if DBSCAN is not None else None), core, "sklearn.cluster.DBSCAN" if DBSCAN is not None else "scipy cKDTree + connected_components"


def cluster_rows(dev, min_samples=5):
    rows = []
    for name, pts, off, (H, W) in workloads():
        d_pts, d_off = torch.from_numpy(pts.astype(np.int64)).to(dev), torch.from_numpy(off).to(dev)
        N, P = len(off) - 1, len(pts)
        for eps in (16, 64):
            b = S.choose_bucket(H, W, N, P, eps)
            row = {"workload": name, "eps": eps, "min_samples": min_samples, "bucket": b, "buckets_per_image": S.n_buckets(H, W, b),
                   "max_occupancy": int(S.bin_counts(d_pts, (H, W), b, offsets=d_off).max())}
            row["cluster_ms"] = time_dev(lambda: S.cluster(d_pts, (H, W), eps, min_samples, offsets=d_off), 7)
            row["count_within_ms"] = time_dev(lambda: S.count_within(d_pts, (H, W), eps, offsets=d_off), 7)
            row["walks"] = row["cluster_ms"] / row["count_within_ms"]
            got = S.cluster(d_pts, (H, W), eps, min_samples, offsets=d_off)
            row["pairs_within_eps"] = int(S.count_within(d_pts, (H, W), eps, offsets=d_off).pair_counts.sum())
            row.update(clusters=int(got.n_clusters.sum()), core=int(got.core.sum()), noise=int(got.n_noise.sum()))
            if row["pairs_within_eps"] <= MAX_HOST_PAIRS:
                row["host_ms"], (labels, core, row["host"]) = time_host(lambda: host_dbscan(d_pts, off, eps, min_samples), 3 if P < 10 ** 5 else 1)
                row["host_agrees"] = bool(np.array_equal(got.core.cpu().numpy().astype(bool), core) and
                                          (labels is None or np.array_equal(got.labels.cpu().numpy(), labels)))
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--cluster", action="store_true", help="time spatial.cluster against count_within and the host library instead")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    if args.cluster:
        rows = cluster_rows(dev)
        ok = all(r.get("host_agrees", True) for r in rows)
        out = {"device": torch.cuda.get_device_name(0), "threads": S.THREADS, "chunk": S.CHUNK, "occupancy_target": S.OCCUPANCY, "rows": rows,
               "all_agree": ok}
        if args.json:
            with open(args.json, "w") as f:
                json.dump(out, f, indent=1)
        print(json.dumps({"all_agree": ok, "rows": len(rows)}))
        return 0 if ok else 1
    rows = []
    for name, pts, off, (H, W) in workloads():
        d_pts, d_off = torch.from_numpy(pts.astype(np.int64)).to(dev), torch.from_numpy(off).to(dev)
        N, P = len(off) - 1, len(pts)
        heavy = P >= 10 ** 5
        queries = [("nearest", {"k": 1}), ("nearest", {"k": 8}), ("count_within", {"radii": 16}), ("count_within", {"radii": 64})]
        for what, kw in queries:
            reach = kw.get("radii", 0)
            b = S.choose_bucket(H, W, N, P, reach)
            fn = getattr(S, what)
            call = lambda bucket: fn(d_pts, (H, W), offsets=d_off, _bucket=bucket, **kw)  # noqa: E731
            row = {"workload": name, "query": what, **kw, "bucket": b, "buckets_per_image": S.n_buckets(H, W, b),
                   "max_occupancy": int(S.bin_counts(d_pts, (H, W), b, offsets=d_off).max())}
            row["grid_ms"] = time_dev(lambda: call(b), 7)
            got = call(b)
            fields = ("index", "d2") if what == "nearest" else ("counts", "pair_counts")
            if not (heavy and args.quick):
                row["single_ms"] = time_dev(lambda: call(max(H, W)), 3 if heavy else 7)
                one = call(max(H, W))
                row["single_equals_grid"] = all(torch.equal(getattr(got, f), getattr(one, f)) for f in fields)
            row["kdtree_ms"], (d2, cnt) = time_host(lambda: kdtree(d_pts, off, kw.get("k"), kw.get("radii")))
            row["kdtree_agrees"] = bool(np.array_equal(got.d2.cpu().numpy(), d2) if d2 is not None else
                                        np.array_equal(got.counts.cpu().numpy()[:, 0], cnt))
            rows.append(row)
            print(json.dumps(row), flush=True)
    ok = all(r.get("single_equals_grid", True) and r["kdtree_agrees"] for r in rows)
    out = {"device": torch.cuda.get_device_name(0), "threads": S.THREADS, "chunk": S.CHUNK, "occupancy_target": S.OCCUPANCY, "rows": rows,
           "all_agree": ok}
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps({"all_agree": ok, "rows": len(rows)}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
