"""Small-region clean-up timing: remove_small_regions(., 300, 100) of 128 thresholded maps of 299^2 (one batch) and of one 4096^2
whole-image mask, device-event timed after warm-up, next to the numpy restatement (tests/regions_ref.py) on the host for the
same work.  Checks that the GPU outputs equal the restatement.

    python tools/regions_microbench.py [--reps 5] [--host-maps 128] [--json PATH]

--measure times ``regions.measure`` (uint8 intensity, a fixed ``max_regions``: no synchronisation) next to ``regions.label`` on the
same two mask sets, checks the tables against tests/props_ref.py, and reports the masks' component statistics.

    python tools/regions_microbench.py --measure [--reps 5] [--host-maps 8] [--json PATH]

--split times ``regions.split`` + ``regions.measure_labels`` next to ``regions.label`` + ``regions.measure`` on the same two mask
sets, with about 1 and about 10 seeds in every component, and on all-foreground masks of the same shapes (one component, 40 seeds
per 299^2 of area: the worst case of the seed walk).  It reports the distance evaluations of every case -- (foreground pixels) x
(live seeds of their component), the cost bound of the assign pass -- and checks the first ``--host-maps`` maps against
tests/split_ref.py (scipy).

    python tools/regions_microbench.py --split [--reps 5] [--host-maps 2] [--json PATH]

--split --geodesic times ``regions.split_geodesic`` next to ``regions.split`` on the same masks and seeds (about 1 and about 10 per
component): with ``max_rounds`` fixed to the rounds the case needs (found once, a round at a time: the first round in which nothing
changes included), with one round only -- the start, the finish and the round that does nearly all of the in-tile sweeps -- and in
the exact mode, which reads the convergence flags back.  The first ``--host-maps`` maps are checked against tests/geodesic_ref.py.

    python tools/regions_microbench.py --split --geodesic [--reps 5] [--host-maps 2] [--json PATH]

--shape times ``regions.shape_labels`` with the table given (the boundary map, the second moments and the perimeter tallies: three
launches) next to ``regions.measure_labels`` on the same label images: ``regions.split`` of the same two mask sets at about 1 and
about 10 seeds per component.  Both are captured into a graph once and the replays are timed, so the figures hold no launch
overhead of the host.  The first ``--host-maps`` maps are checked against tests/shape_ref.py.

    python tools/regions_microbench.py --shape [--reps 5] [--host-maps 2] [--json PATH]

--hull times ``regions.hull_labels`` with the table given (one launch, one workgroup per label) next to ``regions.measure_labels``
and ``regions.shape_labels`` on the label images of ``--shape``, graph replays again.  It reports the two terms of the cost model --
the sum of the bounding-box areas and the sum of the squared vertex counts -- and checks the first ``--host-maps`` maps against
tests/hull_ref.py.

    python tools/regions_microbench.py --hull [--reps 5] [--host-maps 2] [--json PATH]

--contours times ``regions.contour_labels`` with the table and an int ``max_vertices`` given (one launch, one workgroup per label,
the ring walked by one thread in an LDS bitmap) and its counting-only form, next to ``regions.measure_labels`` and
``regions.shape_labels`` on the label images of ``--shape``, graph replays again, and next to the copy of the int32 label image into
pinned host memory: the floor of any route that traces the outlines on the host.  It reports the terms of the cost model -- the sum
of the bounding-box areas (staging and counting) and the sum of the ring lengths (the walk), with the longest ring, which bounds the
launch from below -- and checks the first ``--host-maps`` maps against tests/contour_ref.py, both connectivities, the first 512
labels of every map (the restatement is plain Python loops).

    python tools/regions_microbench.py --contours [--reps 5] [--host-maps 2] [--json PATH]

--adjacency times ``regions.adjacency_labels`` with ``max_regions``, ``max_pairs`` and ``counts`` given (four launches, nothing
synchronises) at both connectivities, next to ``regions.measure_labels`` and ``regions.shape_labels`` on the label images of
``--shape``, graph replays again.  It reports the pairs found and the table size, and checks the pair list and the contact column of
the first ``--host-maps`` maps against numpy's ``unique`` over the id pairs of adjacent pixels.

    python tools/regions_microbench.py --adjacency [--reps 5] [--host-maps 2] [--json PATH]

--morph times ``morph.binary_opening`` at radii 1, 2 and 5, ``morph.expand_labels`` at 4 (of ``regions.label`` of the masks) and
``morph.nearest_sites`` (towards the background) next to ``detect.distance_transform_sq`` on the same two mask sets, graph replays
again, and checks the first ``--host-maps`` maps against scipy: ``binary_opening`` by the disk, the squared
``distance_transform_edt``, and for the expansion the filled set from scipy's distances and the labels from tests/morph_ref.py
(scipy fixes no tie rule).

    python tools/regions_microbench.py --morph [--reps 5] [--host-maps 2] [--json PATH]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import regions_ref as R  # noqa: E402
from cellsegmentation_amd import regions as G  # noqa: E402

MIN_OBJECT, MAX_HOLE = 300, 100


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
    return float(np.median(ts)), ts


def time_graph(fn, reps):
    """fn captured into one graph after a warm-up on a side stream; the median replay time in ms, and all of them"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return time_dev(graph.replay, reps)


def case(name, masks, reps, host_maps, dev):
    d = torch.from_numpy(masks).to(dev)
    out = torch.empty_like(d)
    ms, ts = time_dev(lambda: G.remove_small_regions(d, MIN_OBJECT, MAX_HOLE, out=out), reps)
    got = out.cpu().numpy()
    t0 = time.perf_counter()
    ok = True
    for i in range(host_maps):
        ok &= bool(np.array_equal(got[i], R.remove_small_regions(masks[i], MIN_OBJECT, MAX_HOLE)))
    host_ms = (time.perf_counter() - t0) * 1e3
    res = {"device_ms": ms, "device_ms_all": ts, "host_ms": host_ms, "host_maps": host_maps, "pixels_changed": int((got != masks).sum()),
           "equal_to_host": ok}
    print(json.dumps({name: res}), flush=True)
    return res


def mask_sets():
    yield "batch128_299", R.blobs(128, 299, 299, seed=1)
    # one whole-image mask: 299^2 blob patches tiled into 4096^2 (objects and holes cross the patch seams)
    patches = R.blobs(14 * 14, 299, 299, seed=2)
    whole = patches.reshape(14, 14, 299, 299).transpose(0, 2, 1, 3).reshape(14 * 299, 14 * 299)[:4096, :4096]
    yield "whole_4096", np.ascontiguousarray(whole)[None]


MAX_REGIONS = {"batch128_299": 256, "whole_4096": 16384}


def measure_case(name, masks, reps, host_maps, dev):
    import props_ref as P
    d = torch.from_numpy(masks).to(dev)
    v = np.random.RandomState(3).randint(0, 256, size=masks.shape).astype(np.uint8)
    dv = torch.from_numpy(v).to(dev)
    cap = MAX_REGIONS[name]
    label_ms, _ = time_dev(lambda: G.label(d), reps)
    measure_ms, ts = time_dev(lambda: G.measure(d, intensity=dv, max_regions=cap), reps)
    res = {"label_ms": label_ms, "measure_ms": measure_ms, "measure_ms_all": ts, "max_regions": cap}
    t = G.measure(d, intensity=dv, max_regions=cap)
    counts, area = t.counts.cpu().numpy(), t.area.cpu().numpy()
    used = area[area > 0]
    runs = int((np.diff(np.pad(masks, ((0, 0), (0, 0), (1, 0))).astype(np.int8), axis=2) == 1).sum())
    res.update(components_per_image_mean=float(counts.mean()), components_per_image_max=int(counts.max()),
               overflowed=int(t.overflowed().sum()), area_median=float(np.median(used)), area_mean=float(used.mean()),
               area_max=int(used.max()), foreground_fraction=float(masks.mean()), foreground_pixels=int(masks.sum()), row_runs=runs)
    ok = True
    for i in range(min(host_maps, len(masks))):
        ref = P.measure(masks[i], v[i], 1, cap)
        ok &= int(counts[i]) == int(ref["counts"][0])
        for key in ("area", "bbox", "sum_rc", "intensity_sum", "intensity_max"):
            ok &= bool(np.array_equal(getattr(t, key)[i].cpu().numpy(), ref[key][0]))
    res.update(equal_to_host=ok, host_maps=min(host_maps, len(masks)))
    print(json.dumps({name: res}), flush=True)
    return res


def measure_main(args):
    dev = torch.device("cuda:0")
    return {name: measure_case(name, masks, args.reps, args.host_maps, dev) for name, masks in mask_sets()}


def seeds_in_components(lab, per_component, seed):
    """lab int32 [N, H, W] -> (points int64 [P, 2], offsets [N + 1]): per_component random pixels of every component"""
    rng = np.random.RandomState(seed)
    pts, off = [], [0]
    W = lab.shape[2]
    for x in lab:
        flat = np.flatnonzero(x)
        order = flat[np.argsort(x.ravel()[flat], kind="stable")]           # the pixels of component 1, then of 2, ...
        size = np.bincount(x.ravel()[flat])[1:]
        start = np.concatenate([[0], np.cumsum(size)[:-1]])
        pick = (start[:, None] + (rng.rand(len(size), per_component) * size[:, None]).astype(np.int64)).ravel()
        pts.append(np.stack([order[pick] // W, order[pick] % W], axis=1))
        off.append(off[-1] + len(pick))
    return np.concatenate(pts).astype(np.int64).reshape(-1, 2), np.asarray(off, np.int64)


def split_case(name, masks, pts, off, reps, host_maps, dev):
    import split_ref as S
    d, dp, doff = torch.from_numpy(masks).to(dev), torch.from_numpy(pts).to(dev), torch.from_numpy(off).to(dev)
    v = np.random.RandomState(3).randint(0, 256, size=masks.shape).astype(np.uint8)
    dv = torch.from_numpy(v).to(dev)
    parts = G.split(d, dp, doff)
    cap = max(1, int(parts.counts.max()))                                  # sized once, outside the timed region
    components = G.measure(d, max_regions=cap)
    cap_mask = max(1, int(components.counts.max()))
    label_ms, _ = time_dev(lambda: G.label(d), reps)
    measure_ms, _ = time_dev(lambda: G.measure(d, intensity=dv, max_regions=cap_mask), reps)
    split_ms, _ = time_dev(lambda: G.split(d, dp, doff), reps)
    tables_ms, _ = time_dev(lambda: G.measure_labels(parts.labels, intensity=dv, max_regions=cap, counts=parts.counts), reps)

    def both():
        p = G.split(d, dp, doff)
        return G.measure_labels(p.labels, intensity=dv, max_regions=cap, counts=p.counts)

    both_ms, ts = time_dev(both, reps)
    # the cost bound: every foreground pixel looks at every live seed of its component
    root = G.label(d).to(torch.int64) + torch.arange(len(masks), device=dev)[:, None, None] * (int(components.counts.max()) + 1)
    live = parts.live.nonzero()[:, 0]
    image = torch.bucketize(live, doff[1:], right=True)
    seeds_of = torch.bincount(root[image, dp[live, 0], dp[live, 1]], minlength=int(root.max()) + 1)
    evaluations = int(seeds_of[root[d]].sum())
    res = {"label_ms": label_ms, "measure_ms": measure_ms, "label_plus_measure_ms": label_ms + measure_ms, "split_ms": split_ms,
           "measure_labels_ms": tables_ms, "split_plus_measure_labels_ms": both_ms, "split_plus_measure_labels_ms_all": ts,
           "points": int(len(pts)), "live_seeds": int(parts.live.sum()), "rows_max": cap, "components_max": cap_mask,
           "foreground_pixels": int(masks.sum()), "distance_evaluations": evaluations}
    t = both()
    ok = True
    if evaluations / len(masks) > 2e8:                                     # the brute-force reference would take hours
        host_maps = 0
    for i in range(min(host_maps, len(masks))):
        ref = S.split(masks[i], pts[off[i]:off[i + 1]])
        ok &= bool(np.array_equal(parts.labels[i].cpu().numpy(), ref["labels"])) and int(parts.counts[i]) == int(ref["counts"][0])
        tab = S.tables(ref["labels"], v[i], cap, ref["counts"])
        for key in ("area", "bbox", "sum_rc", "intensity_sum", "intensity_max"):
            ok &= bool(np.array_equal(getattr(t, key)[i].cpu().numpy(), tab[key][0]))
    res.update(equal_to_host=ok, host_maps=min(host_maps, len(masks)))
    print(json.dumps({name: res}), flush=True)
    return res


def split_main(args):
    dev = torch.device("cuda:0")
    res = {}
    for name, masks in mask_sets():
        lab = G.label(torch.from_numpy(masks).to(dev)).cpu().numpy()
        for per in (1, 10):
            pts, off = seeds_in_components(lab, per, seed=per)
            res[f"{name}.seeds{per}"] = split_case(f"{name}.seeds{per}", masks, pts, off, args.reps, args.host_maps, dev)
        full = np.ones_like(masks)
        n = max(1, int(round(40 * masks.shape[1] * masks.shape[2] / 299.0 ** 2)))
        pts, off = seeds_in_components(full.astype(np.int32), n, seed=40)
        res[f"{name}.all_foreground"] = split_case(f"{name}.all_foreground", full, pts, off, args.reps, min(args.host_maps, 1), dev)
    return res


def geodesic_case(name, masks, pts, off, reps, host_maps, dev):
    import geodesic_ref as GR
    from cellsegmentation_amd import kernels as K
    d, dp, doff = torch.from_numpy(masks).to(dev), torch.from_numpy(pts).to(dev), torch.from_numpy(off).to(dev)
    exact = G.split_geodesic(d, dp, doff, want_distance=True)
    # the rounds this case needs: one round per call, resumed until the flags say that nothing changed
    out = K.regions_split_geodesic(d.view(torch.uint8), dp, doff, rounds=1)
    rounds = 1
    while not bool(out[4].all()) and rounds < 4096:
        K.regions_split_geodesic(d.view(torch.uint8), dp, doff, rounds=1, resume=True, labels=out[0], counts=out[1], live=out[2],
                                 converged=out[4], ws=out[5])
        rounds += 1
    fixed = G.split_geodesic(d, dp, doff, max_rounds=rounds, want_distance=True)
    ok = bool(fixed.converged.all()) and torch.equal(fixed.labels, exact.labels) and torch.equal(fixed.distance, exact.distance)
    ok &= torch.equal(out[0], exact.labels)
    split_ms, _ = time_dev(lambda: G.split(d, dp, doff), reps)
    fixed_ms, ts = time_dev(lambda: G.split_geodesic(d, dp, doff, max_rounds=rounds), reps)
    one_ms, _ = time_dev(lambda: G.split_geodesic(d, dp, doff, max_rounds=1), reps)
    exact_ms, _ = time_dev(lambda: G.split_geodesic(d, dp, doff), reps)
    euclid = G.split(d, dp, doff)
    res = {"split_ms": split_ms, "geodesic_fixed_ms": fixed_ms, "geodesic_fixed_ms_all": ts, "geodesic_one_round_ms": one_ms,
           "geodesic_exact_ms": exact_ms, "rounds": rounds, "points": int(len(pts)), "live_seeds": int(exact.live.sum()),
           "foreground_pixels": int(masks.sum()), "distance_max": int(exact.distance.max()),
           "pixels_unlike_split": int((euclid.labels != exact.labels).sum())}
    if masks.shape[1] * masks.shape[2] > 1 << 20:                          # the plain-loop reference would take too long
        host_maps = 0
    for i in range(min(host_maps, len(masks))):
        ref = GR.split(masks[i], pts[off[i]:off[i + 1]])
        ok &= bool(np.array_equal(exact.labels[i].cpu().numpy(), ref["labels"])) and int(exact.counts[i]) == int(ref["counts"][0])
        ok &= bool(np.array_equal(exact.distance[i].cpu().numpy(), ref["distance"]))
    res.update(equal_to_host=bool(ok), host_maps=min(host_maps, len(masks)))
    print(json.dumps({name: res}), flush=True)
    return res


def shape_case(name, masks, pts, off, reps, host_maps, dev):
    import shape_ref as SR
    d, dp, doff = torch.from_numpy(masks).to(dev), torch.from_numpy(pts).to(dev), torch.from_numpy(off).to(dev)
    parts = G.split(d, dp, doff)
    cap = max(1, int(parts.counts.max()))                                  # sized once, outside the timed region
    table = G.measure_labels(parts.labels, max_regions=cap, counts=parts.counts)
    measure_ms, _ = time_graph(lambda: G.measure_labels(parts.labels, max_regions=cap, counts=parts.counts), reps)
    edges_ms, _ = time_graph(lambda: G.boundaries(parts.labels), reps)
    shape_ms, ts = time_graph(lambda: G.shape_labels(parts.labels, table=table), reps)
    st = G.shape_labels(parts.labels, table=table)
    res = {"measure_labels_ms": measure_ms, "boundaries_ms": edges_ms, "shape_labels_ms": shape_ms, "shape_labels_ms_all": ts,
           "shape_over_measure_labels": shape_ms / measure_ms, "rows_max": cap, "foreground_pixels": int(masks.sum()),
           "edge_pixels": int(st.edges.sum())}
    ok = True
    labels = parts.labels.cpu().numpy()
    for i in range(min(host_maps, len(masks))):
        ref = SR.shape_labels(labels[i], cap)
        ok &= bool(np.array_equal(st.edges[i].cpu().numpy(), ref["edges"]))
        for key in ("moments", "tallies"):
            ok &= bool(np.array_equal(getattr(st, key)[i].cpu().numpy(), ref[key][0]))
    res.update(equal_to_host=ok, host_maps=min(host_maps, len(masks)))
    print(json.dumps({name: res}), flush=True)
    return res


def hull_case(name, masks, pts, off, reps, host_maps, dev):
    import hull_ref as HR
    d, dp, doff = torch.from_numpy(masks).to(dev), torch.from_numpy(pts).to(dev), torch.from_numpy(off).to(dev)
    parts = G.split(d, dp, doff)
    cap = max(1, int(parts.counts.max()))                                  # sized once, outside the timed region
    table = G.measure_labels(parts.labels, max_regions=cap, counts=parts.counts)
    measure_ms, _ = time_graph(lambda: G.measure_labels(parts.labels, max_regions=cap, counts=parts.counts), reps)
    shape_ms, _ = time_graph(lambda: G.shape_labels(parts.labels, table=table), reps)
    hull_ms, ts = time_graph(lambda: G.hull_labels(parts.labels, table=table), reps)
    ht = G.hull_labels(parts.labels, table=table)
    box = table.bbox.to(torch.int64)
    vertices = ht.hull[..., 0].clamp(min=0).to(torch.int64)
    res = {"measure_labels_ms": measure_ms, "shape_labels_ms": shape_ms, "hull_labels_ms": hull_ms, "hull_labels_ms_all": ts,
           "hull_over_measure_plus_shape": hull_ms / (measure_ms + shape_ms), "rows_max": cap, "objects": int((table.area > 0).sum()),
           "too_large": int(ht.too_large().sum()), "foreground_pixels": int(masks.sum()),
           "box_area_sum": int(((box[..., 2] - box[..., 0]) * (box[..., 3] - box[..., 1])).sum()),
           "vertices_max": int(vertices.max()), "vertices_squared_sum": int((vertices * vertices).sum())}
    ok = True
    labels = parts.labels.cpu().numpy()
    for i in range(min(host_maps, len(masks))):
        ok &= bool(np.array_equal(ht.hull[i].cpu().numpy(), HR.hull_labels(labels[i], cap)["hull"][0]))
    res.update(equal_to_host=ok, host_maps=min(host_maps, len(masks)))
    print(json.dumps({name: res}), flush=True)
    return res


def contour_case(name, masks, pts, off, reps, host_maps, dev):
    import contour_ref as CR
    d, dp, doff = torch.from_numpy(masks).to(dev), torch.from_numpy(pts).to(dev), torch.from_numpy(off).to(dev)
    parts = G.split(d, dp, doff)
    cap = max(1, int(parts.counts.max()))                                  # sized once, outside the timed region
    table = G.measure_labels(parts.labels, max_regions=cap, counts=parts.counts)
    both = {conn: G.contour_labels(parts.labels, table=table, connectivity=conn) for conn in (1, 2)}   # max_vertices sized here
    ct = both[1]
    maxv = ct.max_vertices
    measure_ms, _ = time_graph(lambda: G.measure_labels(parts.labels, max_regions=cap, counts=parts.counts), reps)
    shape_ms, _ = time_graph(lambda: G.shape_labels(parts.labels, table=table), reps)
    contour_ms, ts = time_graph(lambda: G.contour_labels(parts.labels, table=table, max_vertices=maxv), reps)
    count_ms, _ = time_graph(lambda: G.contour_labels(parts.labels, table=table, max_vertices=0), reps)
    host = torch.empty(parts.labels.shape, dtype=torch.int32, pin_memory=True)
    copy_ms, _ = time_dev(lambda: host.copy_(parts.labels, non_blocking=True), reps)
    box = table.bbox.to(torch.int64)
    cracks = ct.contour[..., 1].clamp(min=0).to(torch.int64)
    res = {"measure_labels_ms": measure_ms, "shape_labels_ms": shape_ms, "contour_labels_ms": contour_ms, "contour_labels_ms_all": ts,
           "contour_count_only_ms": count_ms, "labels_to_pinned_host_ms": copy_ms, "label_image_bytes": parts.labels.numel() * 4,
           "contour_over_measure_plus_shape": contour_ms / (measure_ms + shape_ms), "rows_max": cap, "max_vertices": maxv,
           "objects": int((table.area > 0).sum()), "too_large": int(ct.too_large().sum()), "simple": int(ct.is_simple().sum()),
           "foreground_pixels": int(masks.sum()), "box_area_sum": int(((box[..., 2] - box[..., 0]) * (box[..., 3] - box[..., 1])).sum()),
           "ring_cracks_sum": int(cracks.sum()), "ring_cracks_max": int(cracks.max()), "vertices_sum": int(ct.contour[..., 0].clamp(min=0).sum())}
    ok = True
    labels = parts.labels.cpu().numpy()
    rows = min(cap, 512)
    for i in range(min(host_maps, len(masks))):
        for conn, got in both.items():
            ref = CR.contour_labels(labels[i], rows, conn, got.max_vertices)
            ok &= bool(np.array_equal(got.contour[i, :rows].cpu().numpy(), ref["contour"][0]))
            ok &= bool(np.array_equal(got.vertices[i, :rows].cpu().numpy(), ref["vertices"][0]))
    res.update(equal_to_host=ok, host_maps=min(host_maps, len(masks)), host_rows=rows)
    print(json.dumps({name: res}), flush=True)
    return res


def host_pairs(lab, conn):
    """lab int [H, W] -> int64 [n, 4] rows (a, b, sides, corners), a < b both positive, sorted: numpy's unique over the id pairs of
    the adjacent pixels (no dense table: a whole-image mask has thousands of labels)"""
    lab = np.maximum(lab.astype(np.int64), 0)

    def counted(x, y):
        x, y = x.ravel(), y.ravel()
        keep = (x > 0) & (y > 0) & (x != y)
        keys, n = np.unique(np.minimum(x, y)[keep] << 32 | np.maximum(x, y)[keep], return_counts=True)
        return dict(zip(keys.tolist(), n.tolist()))

    sides = counted(np.concatenate([lab[:, :-1].ravel(), lab[:-1, :].ravel()]), np.concatenate([lab[:, 1:].ravel(), lab[1:, :].ravel()]))
    corners = {}
    if conn == 2:
        corners = counted(np.concatenate([lab[:-1, :-1].ravel(), lab[:-1, 1:].ravel()]),
                          np.concatenate([lab[1:, 1:].ravel(), lab[1:, :-1].ravel()]))
    keys = sorted(set(sides) | set(corners))
    return np.asarray([(k >> 32, k & 0xFFFFFFFF, sides.get(k, 0), corners.get(k, 0)) for k in keys], np.int64).reshape(-1, 4)


def adjacency_case(name, masks, pts, off, reps, host_maps, dev):
    d, dp, doff = torch.from_numpy(masks).to(dev), torch.from_numpy(pts).to(dev), torch.from_numpy(off).to(dev)
    parts = G.split(d, dp, doff)
    cap = max(1, int(parts.counts.max()))                                  # sized once, outside the timed region
    table = G.measure_labels(parts.labels, max_regions=cap, counts=parts.counts)
    sized = {conn: G.adjacency_labels(parts.labels, conn, max_regions=cap, counts=parts.counts) for conn in (1, 2)}   # max_pairs sized here
    max_pairs = {conn: t.slot_keys.shape[1] // 2 for conn, t in sized.items()}
    measure_ms, _ = time_graph(lambda: G.measure_labels(parts.labels, max_regions=cap, counts=parts.counts), reps)
    shape_ms, _ = time_graph(lambda: G.shape_labels(parts.labels, table=table), reps)
    res = {"measure_labels_ms": measure_ms, "shape_labels_ms": shape_ms, "rows_max": cap, "objects": int((table.area > 0).sum()),
           "foreground_pixels": int(masks.sum())}
    ok = True
    labels = parts.labels.cpu().numpy()
    for conn in (1, 2):
        ms, ts = time_graph(lambda: G.adjacency_labels(parts.labels, conn, max_regions=cap, max_pairs=max_pairs[conn],
                                                       counts=parts.counts), reps)
        t = sized[conn]
        res.update({f"adjacency_c{conn}_ms": ms, f"adjacency_c{conn}_ms_all": ts,
                    f"adjacency_c{conn}_over_measure_plus_shape": ms / (measure_ms + shape_ms), f"max_pairs_c{conn}": max_pairs[conn],
                    f"pairs_c{conn}": int(t.n_pairs.sum()), f"pairs_per_image_max_c{conn}": int(t.n_pairs.max())})
        image, a, b, sides, corners = t.pairs()
        contact = t.contact.cpu().numpy()
        for i in range(min(host_maps, len(masks))):
            ref = host_pairs(labels[i], conn)
            ok &= bool(np.array_equal(np.stack([a, b, sides, corners], axis=1)[image == i], ref))
            want = np.zeros(cap, np.int64)
            np.add.at(want, ref[:, 0] - 1, ref[:, 2])
            np.add.at(want, ref[:, 1] - 1, ref[:, 2])
            ok &= bool(np.array_equal(contact[i], want))
    res["contact_sides"] = int(sized[1].contact.sum())
    res["background_sides"] = int(sized[1].background.sum())
    res.update(equal_to_host=ok, host_maps=min(host_maps, len(masks)))
    print(json.dumps({name: res}), flush=True)
    return res


def morph_case(name, masks, reps, host_maps, dev):
    from scipy import ndimage
    import morph_ref as MR
    from cellsegmentation_amd import detect as D
    from cellsegmentation_amd import morph as M
    d = torch.from_numpy(masks).to(dev)
    u8 = d.to(torch.uint8) * 255                                          # the same maps as the EDT reads them: foreground = u8 > 10
    lab = G.label(d)
    res = {"foreground_fraction": float(masks.mean())}
    for r in (1, 2, 5):
        res[f"opening_r{r}_ms"], _ = time_graph(lambda: M.binary_opening(d, r), reps)
    res["expand_labels_r4_ms"], _ = time_graph(lambda: M.expand_labels(lab, 4), reps)
    res["nearest_sites_ms"], res["nearest_sites_ms_all"] = time_graph(lambda: M.nearest_sites(d, background=True), reps)
    res["distance_transform_sq_ms"], _ = time_graph(lambda: D.distance_transform_sq(u8), reps)
    opened = {r: M.binary_opening(d, r).cpu().numpy() for r in (1, 2, 5)}
    grown = M.expand_labels(lab, 4).cpu().numpy()
    d2 = M.nearest_sites(d, background=True)[0].cpu().numpy()
    ok = bool(np.array_equal(np.where(d2 < 0, -1, d2), D.distance_transform_sq(u8).cpu().numpy()))
    labels = lab.cpu().numpy()
    t0 = time.perf_counter()
    for i in range(min(host_maps, len(masks))):
        for r in (1, 2, 5):
            ok &= bool(np.array_equal(opened[r][i], ndimage.binary_opening(masks[i], structure=MR.disk(r * r))))
        if not masks[i].all():
            ok &= bool(np.array_equal(d2[i], np.rint(ndimage.distance_transform_edt(masks[i]) ** 2).astype(np.int32)))
        if masks[i].any():
            to_label = np.rint(ndimage.distance_transform_edt(~masks[i]) ** 2)
            ok &= bool(np.array_equal(grown[i] != 0, to_label <= 16))
        ok &= bool(np.array_equal(grown[i], MR.expand_labels(labels[i], 16)))
    res.update(host_ms=(time.perf_counter() - t0) * 1e3, equal_to_host=ok, host_maps=min(host_maps, len(masks)))
    print(json.dumps({name: res}), flush=True)
    return res


def morph_main(args):
    dev = torch.device("cuda:0")
    return {name: morph_case(name, masks, args.reps, args.host_maps, dev) for name, masks in mask_sets()}


def seeded_main(case_fn, args):
    """case_fn on ``regions.split`` of both mask sets at about 1 and about 10 seeds per component"""
    dev = torch.device("cuda:0")
    res = {}
    for name, masks in mask_sets():
        lab = G.label(torch.from_numpy(masks).to(dev)).cpu().numpy()
        for per in (1, 10):
            pts, off = seeds_in_components(lab, per, seed=per)
            res[f"{name}.seeds{per}"] = case_fn(f"{name}.seeds{per}", masks, pts, off, args.reps, args.host_maps, dev)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-maps", type=int, default=128, help="maps of the batch also run (and checked) on the host")
    ap.add_argument("--json", default=None, help="also write the results to this file")
    ap.add_argument("--measure", action="store_true", help="time regions.measure next to regions.label instead")
    ap.add_argument("--split", action="store_true", help="time regions.split + measure_labels next to label + measure instead")
    ap.add_argument("--geodesic", action="store_true", help="with --split: time regions.split_geodesic next to regions.split instead")
    ap.add_argument("--shape", action="store_true", help="time regions.shape_labels next to regions.measure_labels instead")
    ap.add_argument("--hull", action="store_true", help="time regions.hull_labels next to measure_labels + shape_labels instead")
    ap.add_argument("--contours", action="store_true", help="time regions.contour_labels next to measure_labels + shape_labels instead")
    ap.add_argument("--adjacency", action="store_true", help="time regions.adjacency_labels next to measure_labels + shape_labels instead")
    ap.add_argument("--morph", action="store_true", help="time morph.binary_opening / expand_labels / nearest_sites next to the EDT instead")
    args = ap.parse_args()
    if args.morph:
        res = morph_main(args)
    elif args.adjacency:
        res = seeded_main(adjacency_case, args)
    elif args.contours:
        res = seeded_main(contour_case, args)
    elif args.hull:
        res = seeded_main(hull_case, args)
    elif args.shape:
        res = seeded_main(shape_case, args)
    elif args.split:
        res = seeded_main(geodesic_case, args) if args.geodesic else split_main(args)
    elif args.measure:
        res = measure_main(args)
    else:
        dev = torch.device("cuda:0")
        res = {name: case(name, masks, args.reps, min(args.host_maps, len(masks)), dev) for name, masks in mask_sets()}
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    if not all(v.get("equal_to_host", True) for v in res.values()):
        sys.exit(1)


if __name__ == "__main__":
    main()
