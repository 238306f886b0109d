"""Per-component measurements on the GPU (csrc/regions.hip through cellsegmentation_amd.regions.measure), exact against the numpy
restatement tests/props_ref.py and the scipy.ndimage vectors of tests/golden/props_vectors.npz: degenerate and ragged sizes, row
ends, runs across the 64-column segments of a wave and across 64 x 64 tiles, many and few destinations, sums beyond 32 bits,
capacity below the count, batches and chunks, repeatability, graph replay and the inference layer.  Every comparison is exact:
integers by value, the float64 centroid and mean bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import props_ref as P  # noqa: E402
import regions_ref as R  # noqa: E402
from cellsegmentation_amd import detect  # noqa: E402
from cellsegmentation_amd import kernels as K  # noqa: E402
from cellsegmentation_amd import regions as G  # noqa: E402

pytestmark = pytest.mark.gpu
MASKS = np.load(os.path.join(ROOT, "tests", "golden", "regions_vectors.npz"), allow_pickle=False)
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "props_vectors.npz"), allow_pickle=False)
NAMES = sorted(k[:-len(".intensity")] for k in GOLD.files if k.endswith(".intensity"))
TABLES = ("area", "bbox", "sum_rc", "intensity_sum", "intensity_max")


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _intensity(shape, seed):
    return np.random.RandomState(seed).randint(0, 256, size=shape).astype(np.uint8)


def assert_table(t, ref):
    """a RegionTable against the restatement's dict: every table by value, centroid and mean bit for bit in the used rows and NaN
    in the others, per_image trimmed"""
    assert isinstance(t, G.RegionTable) and t.capacity == ref["capacity"]
    assert t.counts.dtype == torch.int32 and t.counts.is_cuda and np.array_equal(_np(t.counts), ref["counts"])
    dtypes = {"area": torch.int32, "bbox": torch.int32, "sum_rc": torch.int64, "intensity_sum": torch.int64, "intensity_max": torch.int32}
    for name in TABLES:
        got = getattr(t, name)
        if name not in ref:
            assert got is None
            continue
        assert got.dtype == dtypes[name] and got.is_cuda and tuple(got.shape) == ref[name].shape, name
        assert np.array_equal(_np(got), ref[name]), name
    used = np.arange(t.capacity)[None, :] < np.minimum(ref["counts"], t.capacity)[:, None]
    floats = [(t.centroid(), P.centroid(ref))]
    if "intensity_sum" in ref:
        floats.append((t.mean_intensity(), P.mean_intensity(ref)))
    for got, want in floats:
        assert got.dtype == torch.float64 and got.is_cuda
        got = _np(got)
        assert got.shape == want.shape and np.array_equal(_bits(got[used]), _bits(want[used])) and np.isnan(got[~used]).all()
    assert np.array_equal(_np(t.overflowed()), ref["counts"] > t.capacity)
    per, want = t.per_image(), P.per_image(ref)
    assert len(per) == len(want)
    for g, w in zip(per, want):
        assert sorted(g) == sorted(w)
        for k in w:
            assert g[k].shape == w[k].shape and g[k].dtype == w[k].dtype
            assert np.array_equal(_bits(g[k]), _bits(w[k])) if w[k].dtype == np.float64 else np.array_equal(g[k], w[k])


def check(m, v=None, connectivity=1, max_regions=None):
    t = G.measure(m, intensity=v, connectivity=connectivity, max_regions=max_regions)
    assert_table(t, P.measure(m, v, connectivity, max_regions))
    return t


@pytest.mark.parametrize("connectivity", [1, 2])
@pytest.mark.parametrize("hw", [(1, 1), (1, 37), (41, 1), (5, 3), (64, 64), (65, 65), (130, 97)])
def test_degenerate_and_ragged_sizes(dev, hw, connectivity):
    rng = np.random.RandomState(hw[0] * 131 + hw[1])
    v = _intensity(hw, hw[0] + 7 * hw[1])
    for m in (rng.rand(*hw) > 0.45, rng.rand(*hw) > 0.8, np.zeros(hw, bool), np.ones(hw, bool)):
        check(m, None, connectivity)
        check(m, v, connectivity)


@pytest.mark.parametrize("W", [37, 97])
def test_row_ends_do_not_join_runs(dev, W):
    """the last column of row r and the first column of row r + 1 are consecutive in memory and no neighbours"""
    m = np.zeros((9, W), bool)
    m[2, W - 3:] = True
    m[3, :4] = True
    m[6, W - 1] = True
    m[7, 0] = True
    v = _intensity(m.shape, W)
    t = check(m, v, 1)
    assert _np(t.counts).tolist() == [4]
    assert _np(t.bbox)[0].tolist() == [[2, W - 3, 3, W], [3, 0, 4, 4], [6, W - 1, 7, W], [7, 0, 8, 1]]
    assert _np(t.area)[0].tolist() == [3, 4, 1, 1]
    check(m, v, 2)
    d = m.copy()
    d[3, :] = False
    d[3, W - 4] = True                         # diagonal neighbour of (2, W - 3): one component with connectivity 2 only
    d[7, 0] = False
    d[7, W - 2] = True                         # diagonal neighbour of (6, W - 1)
    assert _np(check(d, v, 1).counts).tolist() == [4]
    t = check(d, v, 2)
    assert _np(t.counts).tolist() == [2] and _np(t.bbox)[0].tolist() == [[2, W - 4, 4, W], [6, W - 2, 8, W]]


def test_runs_across_segments_and_tiles(dev):
    m = np.zeros((130, 200), bool)
    m[10, 50:141] = True                       # one row run over three 64-column segments and three tiles
    m[20, 5:30] = True
    m[20, 30] = False
    m[20, 31:60] = True                        # two components in one segment, one background pixel apart
    m[20, 29] = True
    m[30, 0] = m[30, 63] = True                # runs of length 1 at lanes 0 and 63
    m[31, 64] = m[31, 127] = m[31, 128] = True
    m[60:70, 100] = True                       # a column across the tile edge at row 64
    v = _intensity(m.shape, 11)
    for conn in (1, 2):
        t = check(m, v, conn)
        assert _np(t.area)[0, 0] == 91 and _np(t.bbox)[0, 0].tolist() == [10, 50, 11, 141]
        assert _np(t.sum_rc)[0, 0].tolist() == [910, sum(range(50, 141))]
        assert _np(t.intensity_sum)[0, 0] == int(v[10, 50:141].sum()) and _np(t.intensity_max)[0, 0] == int(v[10, 50:141].max())
    assert _np(check(m, v, 1).area)[0, 1:3].tolist() == [25, 29]
    check(~m, v, 1)
    check(m.T.copy(), np.ascontiguousarray(v.T), 2)


def test_many_destinations_checkerboard(dev):
    m = (np.indices((64, 64)).sum(0) % 2).astype(bool)
    v = _intensity(m.shape, 5)
    t = check(m, v, 1)
    assert t.capacity == 2048 and bool((t.area == 1).all()) and np.array_equal(_np(t.intensity_sum)[0], v[m])
    assert check(m, v, 2).capacity == 1


def test_few_destinations(dev):
    s = R.serpentine(33, 70)
    v = _intensity(s.shape, 9)
    for conn in (1, 2):
        t = check(s, v, conn)
        assert _np(t.counts).tolist() == [1] and _np(t.area).tolist() == [[17 * 70 + 16]]
    full = np.ones((299, 299), bool)
    v = _intensity(full.shape, 10)
    t = check(full, v, 1)                      # every run of every wave adds to one row: maximal contention
    assert _np(t.area).tolist() == [[299 * 299]] and _np(t.intensity_sum).tolist() == [[int(v.sum(dtype=np.int64))]]


def test_sums_need_64_bits(dev):
    """2100 is the smallest square whose row / column sum (2100^2 * 1049.5 = 4 628 295 000) passes 2^32: a 32-bit accumulator,
    signed or unsigned, wraps.  Expected values in closed form."""
    S = 2100
    m = torch.ones((S, S), dtype=torch.bool, device=dev)
    v = torch.full((S, S), 255, dtype=torch.uint8, device=dev)
    want = S * S * (S - 1) // 2
    assert want > 2 ** 32
    for cap in (None, 3):
        t = G.measure(m, intensity=v, max_regions=cap)
        k = 1 if cap is None else cap
        assert t.capacity == k and _np(t.counts).tolist() == [1]
        assert _np(t.area).tolist() == [[S * S] + [0] * (k - 1)]
        assert _np(t.sum_rc)[0].tolist() == [[want, want]] + [[0, 0]] * (k - 1)
        assert _np(t.bbox)[0].tolist() == [[0, 0, S, S]] + [[0, 0, 0, 0]] * (k - 1)
        assert _np(t.intensity_sum).tolist() == [[255 * S * S] + [0] * (k - 1)] and _np(t.intensity_max).tolist() == [[255] + [0] * (k - 1)]
        c = _np(t.centroid())[0, 0]
        assert np.array_equal(_bits(c), _bits(np.array([want / (S * S)] * 2))) and c[0] == (S - 1) / 2


@pytest.mark.parametrize("connectivity", [1, 2])
def test_capacity_below_the_count(dev, connectivity):
    m = R.blobs(2, 70, 90, seed=4, density=1 / 150.0)
    m[1, ::2, ::3] = True                      # many more components in the second image
    v = _intensity(m.shape, 12)
    full = P.measure(m, v, connectivity)
    counts = full["counts"]
    assert counts.min() >= 3
    for cap in (1, int(counts.min()) - 1, int(counts.min()), int(counts.max()) + 5):
        t = check(m, v, connectivity, max_regions=cap)
        assert np.array_equal(_np(t.counts), counts) and np.array_equal(_np(t.overflowed()), counts > cap)
        k = min(cap, full["capacity"])
        for name in TABLES:
            assert np.array_equal(_np(getattr(t, name))[:, :k], full[name][:, :k])


def test_tables_are_written_inside_their_views_only(dev):
    m = R.blobs(2, 70, 90, seed=4, density=1 / 150.0)
    d = torch.from_numpy(m.view(np.uint8)).to(dev)
    v = _intensity(m.shape, 13)
    dv = torch.from_numpy(v).to(dev)
    N, cap, pad = 2, 5, 16
    ref = P.measure(m, v, 1, max_regions=cap)
    assert (ref["counts"] > cap).all()
    shapes = {"counts": ((N,), torch.int32), "area": ((N, cap), torch.int32), "bbox": ((N, cap, 4), torch.int32),
              "sums": ((N, cap, 2), torch.int64), "isum": ((N, cap), torch.int64), "imax": ((N, cap), torch.int32)}
    bufs, views = {}, {}
    for name, (shape, dtype) in shapes.items():
        n = int(np.prod(shape))
        bufs[name] = torch.full((n + 2 * pad,), -77, dtype=dtype, device=dev)
        views[name] = bufs[name][pad:pad + n].view(shape)
    ws = K.regions_workspace(N, 70, 90, dev)
    ws.fill_(0xAB)                                                      # stale contents must not matter
    for numbered in (False, True):
        for b in bufs.values():
            b.fill_(-77)
        if numbered:
            K.regions_number(d, 1, counts=views["counts"], ws=ws)
        out = K.regions_measure(d, cap, dv, 1, numbered, ws=ws, **views)
        assert all(o is views[k] for o, k in zip(out, ("counts", "area", "bbox", "sums", "isum", "imax")))
        for name, b in bufs.items():
            n = int(np.prod(shapes[name][0]))
            assert bool((b[:pad] == -77).all()) and bool((b[pad + n:] == -77).all()), name
        for name, key in (("counts", "counts"), ("area", "area"), ("bbox", "bbox"), ("sums", "sum_rc"), ("isum", "intensity_sum"),
                          ("imax", "intensity_max")):
            assert np.array_equal(_np(views[name]), ref[key]), name
    # without an intensity image the intensity tables are not touched
    for b in bufs.values():
        b.fill_(-77)
    K.regions_measure(d, cap, None, 1, False, ws=ws, **{k: views[k] for k in ("counts", "area", "bbox", "sums")})
    assert bool((bufs["isum"] == -77).all()) and bool((bufs["imax"] == -77).all())
    assert np.array_equal(_np(views["area"]), ref["area"])
    with pytest.raises(RuntimeError):
        K.regions_measure(d, 0, None, ws=ws)                            # capacity < 1: refused, nothing launched
    with pytest.raises(RuntimeError):
        K.regions_measure(d, 70 * 90 + 1, None, ws=ws)
    with pytest.raises(RuntimeError):
        K.regions_measure(d, cap, None, ws=ws[:-16].clone())
    with pytest.raises(RuntimeError):
        K.regions_number(d, 3, ws=ws)


def test_batches_and_chunks(dev, monkeypatch):
    m = R.blobs(5, 70, 90, seed=3, density=1 / 150.0)
    m[1] = False                                                        # an image without components inside the batch
    v = _intensity(m.shape, 14)
    ref = P.measure(m, v, 1)
    whole = check(m, v, 1)
    for i in range(5):
        one = G.measure(m[i], intensity=v[i], max_regions=whole.capacity)
        for name in TABLES:
            assert torch.equal(getattr(one, name)[0], getattr(whole, name)[i]), name
        assert int(one.counts[0]) == int(whole.counts[i])
    monkeypatch.setattr(G, "_MAX_PIXELS", 2 * 70 * 90 + 5)             # two images per call: 2 + 2 + 1
    assert [b - a for a, b in G._chunks(torch.empty(5, 70, 90))] == [2, 2, 1]
    assert_table(G.measure(m, intensity=v), ref)
    assert_table(G.measure(m, intensity=v, connectivity=2, max_regions=7), P.measure(m, v, 2, 7))
    assert_table(G.measure(m), P.measure(m))


def test_two_runs_identical_and_graph_replay(dev):
    m = R.blobs(3, 130, 97, seed=7, density=1 / 200.0)
    other = R.blobs(3, 130, 97, seed=8, density=1 / 200.0)
    v, w = _intensity(m.shape, 15), _intensity(m.shape, 16)
    cap = 18                                                            # below the count of the first image, above the others'
    d, dv = torch.from_numpy(m).to(dev), torch.from_numpy(v).to(dev)
    a, b = G.measure(d, intensity=dv, max_regions=cap), G.measure(d, intensity=dv, max_regions=cap)
    for name in ("counts",) + TABLES:
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    static_m, static_v = torch.zeros_like(d), torch.zeros_like(dv)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        G.measure(static_m, intensity=static_v, max_regions=cap)        # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        t = G.measure(static_m, intensity=static_v, max_regions=cap)
    static_m.copy_(d)
    static_v.copy_(dv)
    graph.replay()
    assert_table(t, P.measure(m, v, 1, cap))
    static_m.copy_(torch.from_numpy(other).to(dev))
    static_v.copy_(torch.from_numpy(w).to(dev))
    graph.replay()
    assert_table(t, P.measure(other, w, 1, cap))


@pytest.mark.parametrize("connectivity", [1, 2])
@pytest.mark.parametrize("name", NAMES)
def test_golden_scipy_vectors(dev, name, connectivity):
    H, W = MASKS[f"{name}.shape"]
    m = np.unpackbits(MASKS[f"{name}.mask"], axis=1)[:, :W].astype(bool)
    v = GOLD[f"{name}.intensity"]
    f64, i32 = GOLD[f"{name}.f64_{connectivity}"], GOLD[f"{name}.i32_{connectivity}"]
    n = len(i32)
    t = G.measure(m, intensity=v, connectivity=connectivity)
    assert _np(t.counts).tolist() == [n] == [int(GOLD[f"{name}.counts"][connectivity - 1])] and t.capacity == max(n, 1)
    assert np.array_equal(_np(t.area)[0, :n], i32[:, 0]) and np.array_equal(_np(t.intensity_sum)[0, :n], i32[:, 1])
    assert np.array_equal(_np(t.intensity_max)[0, :n], i32[:, 2]) and np.array_equal(_np(t.bbox)[0, :n], i32[:, 3:])
    assert np.array_equal(_bits(_np(t.centroid())[0, :n]), _bits(f64[:, :2]))
    assert np.array_equal(_bits(_np(t.mean_intensity())[0, :n]), _bits(f64[:, 2]))
    d = t.per_image()[0]
    assert np.array_equal(_bits(d["centroid"]), _bits(f64[:, :2])) and np.array_equal(_bits(d["intensity_mean"]), _bits(f64[:, 2]))


def test_measure_cells_end_to_end_resnet18(dev):
    from cellsegmentation_amd import inference, synth
    from cellsegmentation_amd.model import resnet as RN
    m = RN.MILresnet18()
    sd = m.state_dict()
    synth.fill_state_dict(sd)
    m.load_state_dict(sd)
    m = m.to(dev).set_compute_dtype(torch.float32)
    m.setmode("segment")
    x = synth.normalise(synth.ihc_tiles(4, 299, seed=23))
    loader = [x[:3], x[3:]]
    probs = inference.inference_seg(loader, m, dev, mode="test")
    thr = float(np.median(probs))                                      # a threshold that splits this model's output
    classes = _np(inference.segment_classes(loader, m, dev, thr, 40, 15))
    q = _np(detect.quantize(probs))
    want = P.per_image(P.measure(classes, q, 1))
    assert sum(len(w["area"]) for w in want) >= 1
    for kw in ({}, {"max_regions": 3}):
        ref = want if not kw else P.per_image(P.measure(classes, q, 1, 3))
        got = inference.measure_cells(loader, m, dev, thr, 40, 15, **kw)
        assert len(got) == 4
        for g, w in zip(got, ref):
            assert sorted(g) == sorted(w)
            for k in w:
                assert g[k].shape == w[k].shape and np.array_equal(_bits(g[k]) if w[k].dtype == np.float64 else g[k],
                                                                   _bits(w[k]) if w[k].dtype == np.float64 else w[k]), k
    assert m.mode == "segment"


def test_measure_slide(dev):
    from cellsegmentation_amd import inference
    H, W = 300, 420
    blobs = R.blobs(1, H, W, seed=21)[0]
    u8 = np.where(blobs, _intensity((H, W), 17) // 2 + 128, _intensity((H, W), 18) // 2).astype(np.uint8)
    assert np.array_equal(u8 > 127, blobs)
    for kw in ({}, {"connectivity": 2, "max_regions": 6, "min_object_size": 50, "hole_area_threshold": 20, "thr_u8": 140}):
        t = inference.measure_slide(u8, **kw)
        conn, thr = kw.get("connectivity", 1), kw.get("thr_u8", 127)
        clean = R.remove_small_regions(u8 > thr, kw.get("min_object_size", 300), kw.get("hole_area_threshold", 100), conn)
        ref = P.measure(clean, u8, conn, kw.get("max_regions"))
        assert ref["counts"][0] >= 2
        assert_table(t, ref)
        assert_table(inference.measure_slide(torch.from_numpy(u8).to(dev), **kw), ref)
