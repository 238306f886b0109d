"""CPU: the numpy restatement of the per-component measurements (tests/props_ref.py) against vectors made with scipy.ndimage
(tests/golden/make_props_golden.py), bit for bit; the argument errors of cellsegmentation_amd.regions.measure, which are raised
before any device work; the new entry points in the header and the ctypes table; RegionTable on host tensors."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import props_ref as P
from cellsegmentation_amd import _lib, inference, kernels, regions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASKS = np.load(os.path.join(ROOT, "tests", "golden", "regions_vectors.npz"), allow_pickle=False)
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "props_vectors.npz"), allow_pickle=False)
NAMES = sorted(k[:-len(".intensity")] for k in GOLD.files if k.endswith(".intensity"))


def _mask(name):
    H, W = MASKS[f"{name}.shape"]
    return np.unpackbits(MASKS[f"{name}.mask"], axis=1)[:, :W].astype(bool)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def golden(name, connectivity):
    """(count, scipy's per-label results by name) of one mask of props_vectors.npz"""
    f64, i32 = GOLD[f"{name}.f64_{connectivity}"], GOLD[f"{name}.i32_{connectivity}"]
    return len(i32), {"com": f64[:, :2], "mean": f64[:, 2], "area": i32[:, 0], "sum": i32[:, 1], "max": i32[:, 2], "bounds": i32[:, 3:]}


def test_golden_covers_the_pinned_masks():
    assert NAMES == ["blobs70x90", "checker6x7", "rand5x3", "rand64x80", "serpentine9x6"]
    for name in NAMES:
        v = GOLD[f"{name}.intensity"]
        assert v.dtype == np.uint8 and v.shape == _mask(name).shape
        for conn in (1, 2):
            f64, i32 = GOLD[f"{name}.f64_{conn}"], GOLD[f"{name}.i32_{conn}"]
            assert f64.dtype == np.float64 and i32.dtype == np.int32 and f64.shape[1:] == (3,) and i32.shape[1:] == (7,)
            assert len(f64) == len(i32) == int(MASKS[f"{name}.count{conn}"]) == int(GOLD[f"{name}.counts"][conn - 1])
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "props_vectors.npz")) < 64 * 1024


@pytest.mark.parametrize("connectivity", [1, 2])
@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_scipy_vectors(name, connectivity):
    m, v = _mask(name), GOLD[f"{name}.intensity"]
    t = P.measure(m, v, connectivity)
    n, want = golden(name, connectivity)
    assert t["counts"].dtype == np.int32 and t["counts"].tolist() == [n] and t["capacity"] == max(n, 1)
    assert t["area"].dtype == np.int32 and t["bbox"].dtype == np.int32 and t["sum_rc"].dtype == np.int64
    assert t["intensity_sum"].dtype == np.int64 and t["intensity_max"].dtype == np.int32
    key = want.__getitem__
    assert np.array_equal(t["area"][0, :n], key("area")) and np.array_equal(t["bbox"][0, :n], key("bounds"))
    assert np.array_equal(t["intensity_sum"][0, :n], key("sum")) and np.array_equal(t["intensity_max"][0, :n], key("max"))
    assert _same_bits(P.centroid(t)[0, :n], key("com"))
    assert _same_bits(P.mean_intensity(t)[0, :n], key("mean"))
    d = P.per_image(t)[0]
    assert len(d["area"]) == n and _same_bits(d["centroid"], key("com")) and _same_bits(d["intensity_mean"], key("mean"))
    # a capacity below the count keeps the first rows; one above it leaves zero rows
    for cap in (1, max(1, n // 2), n + 3):
        c = P.measure(m, v, connectivity, max_regions=cap)
        k = min(n, cap)
        assert c["counts"].tolist() == [n] and c["area"].shape == (1, cap)
        for name_ in ("area", "bbox", "sum_rc", "intensity_sum", "intensity_max"):
            assert np.array_equal(c[name_][0, :k], t[name_][0, :k]) and not c[name_][0, k:].any()


def test_restatement_without_components_and_batches():
    t = P.measure(np.zeros((2, 3, 4), bool))
    assert t["counts"].tolist() == [0, 0] and t["capacity"] == 1 and not t["area"].any() and not t["bbox"].any()
    assert "intensity_sum" not in t and np.isnan(P.centroid(t)).all()
    m = np.stack([_mask("checker6x7"), ~_mask("checker6x7")])
    t = P.measure(m, connectivity=1)
    assert t["counts"].tolist() == [21, 21] and (t["area"] == 1).all()
    assert np.array_equal(t["bbox"][0, 0], [0, 1, 1, 2]) and np.array_equal(t["sum_rc"][1, 0], [0, 0])


def test_argument_errors_come_before_device_work():
    m = np.zeros((4, 5), bool)
    v = np.zeros((4, 5), np.uint8)
    for bad in (m.astype(np.uint8), m.astype(np.int32), m.astype(np.float32), torch.zeros(4, 5, dtype=torch.int64)):
        with pytest.raises(TypeError):
            regions.measure(bad)
    with pytest.raises(TypeError):
        regions.measure([[True, False]])
    for bad in (np.zeros(5, bool), np.zeros((1, 2, 3, 4), bool), np.zeros((0, 5), bool)):
        with pytest.raises(ValueError):
            regions.measure(bad)
    for bad in (v.astype(np.int32), v.astype(np.float32), m, torch.zeros(4, 5, dtype=torch.int8), [[1, 2]]):
        with pytest.raises(TypeError):
            regions.measure(m, intensity=bad)
    for bad in (np.zeros((5, 4), np.uint8), np.zeros((1, 4, 5), np.uint8), np.zeros((4,), np.uint8)):
        with pytest.raises(ValueError):
            regions.measure(m, intensity=bad)
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError):
            regions.measure(m, max_regions=bad)
    for conn in (0, 3, 1.5, None):
        with pytest.raises(ValueError):
            regions.measure(m, connectivity=conn)
    with pytest.raises(TypeError):
        inference.measure_slide(np.zeros((4, 5), np.float32))
    with pytest.raises(TypeError):
        inference.measure_slide(np.zeros((1, 4, 5), np.uint8))
    with pytest.raises(ValueError):
        inference.measure_slide(v, thr_u8=256)


def test_entry_points_in_header_table_and_library():
    header = open(os.path.join(ROOT, "include", "cellseg_hip.h")).read()
    lib = _lib.load()
    assert lib.cs_abi_version() == 10
    for name, n_args in (("cs_regions_number", 9), ("cs_regions_measure", 17)):
        decl = re.search(rf"\bint {name}\((.*?)\);", header, flags=re.S)
        assert decl is not None and len(decl.group(1).split(",")) == n_args
        restype, argtypes = _lib._SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == n_args and hasattr(lib, name)
        assert argtypes[-1] is ctypes.c_void_p and argtypes[-2] is ctypes.c_size_t
        assert f" * {name}" in header                                   # described in the section's comment
    assert callable(kernels.regions_number) and callable(kernels.regions_measure)


def test_region_table_on_host_tensors():
    """RegionTable's methods are plain tensor arithmetic: per_image trims to min(count, capacity) and agrees with the restatement."""
    m = np.stack([_mask("rand5x3"), np.zeros((5, 3), bool), np.ones((5, 3), bool)])
    v = np.random.RandomState(3).randint(0, 256, size=m.shape).astype(np.uint8)
    for cap in (None, 2):
        ref = P.measure(m, v, 1, max_regions=cap)
        t = regions.RegionTable(torch.from_numpy(ref["counts"]), ref["capacity"], torch.from_numpy(ref["area"]), torch.from_numpy(ref["bbox"]),
                                torch.from_numpy(ref["sum_rc"]), torch.from_numpy(ref["intensity_sum"]), torch.from_numpy(ref["intensity_max"]))
        assert t.centroid().dtype == torch.float64 and _same_bits(t.centroid().numpy(), P.centroid(ref))
        assert _same_bits(t.mean_intensity().numpy(), P.mean_intensity(ref))
        assert t.overflowed().tolist() == [int(c) > ref["capacity"] for c in ref["counts"]]
        got, want = t.per_image(), P.per_image(ref)
        assert len(got) == 3 and [len(d["area"]) for d in got] == [min(int(c), ref["capacity"]) for c in ref["counts"]]
        for g, w in zip(got, want):
            assert sorted(g) == ["area", "bbox", "centroid", "intensity_max", "intensity_mean", "intensity_sum"]
            for k in w:
                assert g[k].dtype == w[k].dtype and g[k].shape == w[k].shape
                assert _same_bits(g[k], w[k]) if g[k].dtype == np.float64 else np.array_equal(g[k], w[k])
    bare = regions.RegionTable(torch.zeros(1, dtype=torch.int32), 1, torch.zeros(1, 1, dtype=torch.int32),
                               torch.zeros(1, 1, 4, dtype=torch.int32), torch.zeros(1, 1, 2, dtype=torch.int64))
    assert sorted(bare.per_image()[0]) == ["area", "bbox", "centroid"] and bare.per_image()[0]["area"].shape == (0,)
    with pytest.raises(ValueError):
        bare.mean_intensity()
