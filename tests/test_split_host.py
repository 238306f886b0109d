"""CPU: the brute-force statement of the seeded split (tests/split_ref.py) against hand-written arrays for the cases a plausible wrong
implementation gets wrong (tie, duplicate seed, foreign seed) and against tests/golden/split_vectors.npz; the label-image tables
of the reference; the argument errors of regions.split / regions.measure_labels, which are raised before any device work; the new
entry points in the header and the ctypes table."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import props_ref as P
import regions_ref as R
import split_ref as S
from cellsegmentation_amd import _lib, detect, inference, kernels, regions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "split_vectors.npz"), allow_pickle=False)
NAMES = sorted(k[:-len(".labels")] for k in GOLD.files if k.endswith(".labels"))


def _grid(text):
    return np.asarray([[int(ch) for ch in row] for row in text.split()], np.int32)


def test_tie_goes_to_the_lower_index_and_follows_a_swap():
    m = np.ones((2, 7), bool)
    pts = np.asarray([[0, 1], [0, 5]])                     # column 3 is equidistant
    got = S.split(m, pts)
    assert np.array_equal(got["labels"], _grid("1111222 1111222")) and got["counts"].tolist() == [2] and got["live"].tolist() == [True, True]
    assert np.array_equal(S.split(m, pts[::-1])["labels"], _grid("2221111 2221111"))
    m2, p2 = S.two_discs()
    lab = S.split(m2, p2)["labels"]
    assert (lab[:, :69][m2[:, :69]] == 1).all() and (lab[:, 69:][m2[:, 69:]] == 2).all() and m2[:, 68].any()
    lab = S.split(m2, p2[::-1])["labels"]
    assert (lab[:, :68][m2[:, :68]] == 2).all() and (lab[:, 68:][m2[:, 68:]] == 1).all()


def test_duplicate_dead_and_limited_seeds():
    m = _grid("1111100 0000000 0110111").astype(bool)
    pts = np.asarray([[0, 2], [0, 2], [1, 1], [2, 6], [0, 0]])       # a duplicate, one on the background, one beyond the limit
    got = S.split(m, pts, limits=4)
    assert got["n_seeds"].tolist() == [4] and got["live"].tolist() == [True, True, False, True, False]
    assert np.array_equal(got["labels"], _grid("1111100 0000000 0550444")) and got["counts"].tolist() == [5]
    t = S.tables(got["labels"], counts=got["counts"])
    assert t["area"].tolist() == [[5, 0, 0, 3, 2]] and t["bbox"][0].tolist() == [[0, 0, 1, 5], [0, 0, 0, 0], [0, 0, 0, 0], [2, 4, 3, 7], [2, 1, 3, 3]]
    assert np.isnan(t["centroid"][0, 1]).all() and t["centroid"][0, 3].tolist() == [2.0, 5.0]
    # without the limit the last point is a seed of the first component too, and negative limits cut from the end
    assert np.array_equal(S.split(m, pts)["labels"], _grid("5111100 0000000 0660444"))
    assert S.split(m, pts, limits=-1)["n_seeds"].tolist() == [4] and S.split(m, pts, limits=-9)["n_seeds"].tolist() == [0]
    assert np.array_equal(S.split(m, pts, limits=0)["labels"], R.label(m)[0])


def test_a_nearer_seed_of_another_component_does_not_win():
    m = _grid("1110111111 1110111111").astype(bool)
    pts = np.asarray([[0, 2], [0, 9]])                     # (0, 4) is 2 from the first seed and 5 from its own
    assert np.array_equal(S.split(m, pts)["labels"], _grid("1110222222 1110222222"))
    assert np.array_equal(S.split(m, pts[:1])["labels"], _grid("1110222222 1110222222"))      # seedless: numbered after the seed
    joined = m.copy()
    joined[1, 3] = True                                    # one component: now the plain Voronoi cut
    assert np.array_equal(S.split(joined, pts)["labels"], _grid("1110112222 1111112222"))
    big, bp = S.foreign_seed()
    lab = S.split(big, bp)["labels"]
    assert (lab[8:28, 42:100] == 2).all() and (lab[5:30, 10:40] == 1).all()
    assert ((np.arange(42, 60) - 39) ** 2 < (np.arange(42, 60) - 97) ** 2).all()       # a Voronoi cut would give these to seed 0


def test_seedless_components_are_numbered_after_the_seeds_in_scipy_order():
    m = _grid("1010001 0000000 1110101").astype(bool)
    pts = np.asarray([[2, 1], [0, 2]])
    got = S.split(m, pts)
    assert np.array_equal(got["labels"], _grid("3020004 0000000 1110506")) and got["counts"].tolist() == [6]
    # diagonal contact merges only with connectivity 2
    d = _grid("100 010 001").astype(bool)
    assert np.array_equal(S.split(d, [[1, 1]], connectivity=1)["labels"], _grid("200 010 003"))
    assert np.array_equal(S.split(d, [[1, 1]], connectivity=2)["labels"], _grid("100 010 001"))


@pytest.mark.parametrize("name", NAMES)
def test_reference_equals_the_golden_vectors(name):
    shape = tuple(GOLD[f"{name}.shape"])
    m = np.unpackbits(GOLD[f"{name}.mask"], axis=1)[:, :shape[2]].astype(bool).reshape(shape)
    lim = GOLD[f"{name}.limits"]
    got = S.split(m, GOLD[f"{name}.points"], GOLD[f"{name}.offsets"], lim if len(lim) else None, int(GOLD[f"{name}.connectivity"]))
    for key in ("labels", "counts", "n_seeds", "live"):
        assert got[key].dtype == GOLD[f"{name}.{key}"].dtype and np.array_equal(got[key], GOLD[f"{name}.{key}"]), key
    assert np.array_equal(got["labels"] > 0, m)
    t = S.tables(got["labels"], GOLD[f"{name}.intensity"], counts=got["counts"])
    for key in ("area", "bbox", "sum_rc", "intensity_sum", "intensity_max"):
        assert np.array_equal(t[key], GOLD[f"{name}.{key}"]), key
    assert t["area"].sum() == m.sum()


def test_golden_file_holds_the_named_cases():
    assert NAMES == ["batch1", "batch2", "foreign", "tie", "tie_swapped"]
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "split_vectors.npz")) < 256 * 1024
    assert (GOLD["batch1.area"] == 0).any(axis=1).all() and not GOLD["batch1.live"].all()


def test_label_tables_of_a_plain_labelling_equal_the_mask_tables():
    m = R.blobs(2, 40, 50, seed=2, density=1 / 150.0)
    v = np.random.RandomState(1).randint(0, 256, size=m.shape).astype(np.uint8)
    lab = np.stack([R.label(x)[0] for x in m])
    t, ref = S.tables(lab, v), P.measure(m, v)
    for key in ("counts", "area", "bbox", "sum_rc", "intensity_sum", "intensity_max"):
        assert np.array_equal(t[key], ref[key]), key
    used = t["area"] > 0
    assert np.array_equal(t["centroid"][used].view(np.uint64), P.centroid(ref)[used].view(np.uint64))
    assert np.array_equal(t["intensity_mean"][used].view(np.uint64), P.mean_intensity(ref)[used].view(np.uint64))
    c = S.tables(lab, v, capacity=3)
    assert np.array_equal(c["counts"], ref["counts"]) and np.array_equal(c["area"], ref["area"][:, :3])


def test_split_argument_errors_come_before_device_work():
    m = np.zeros((4, 5), bool)
    pts = np.asarray([[1, 1], [2, 3]])
    for bad in (m.astype(np.uint8), m.astype(np.int32), torch.zeros(4, 5, dtype=torch.float32)):
        with pytest.raises(TypeError):
            regions.split(bad, pts)
    for bad in (np.zeros(5, bool), np.zeros((1, 2, 3, 4), bool), np.zeros((0, 5), bool)):
        with pytest.raises(ValueError):
            regions.split(bad, pts)
    for conn in (0, 3, None):
        with pytest.raises(ValueError):
            regions.split(m, pts, connectivity=conn)
    for bad in ([[-1, 0]], [[4, 0]], [[0, 5]], [[0, -1]]):              # host points outside the image
        with pytest.raises(ValueError, match="outside"):
            regions.split(m, np.asarray(bad))
        with pytest.raises(ValueError, match="outside"):
            regions.split(m, torch.tensor(bad))
    with pytest.raises(TypeError):
        regions.split(m, pts.astype(np.float32))
    with pytest.raises(ValueError):
        regions.split(m, np.zeros((3, 3), np.int64))
    with pytest.raises(ValueError):
        regions.split(np.zeros((2, 4, 5), bool), pts)                     # two images: a list or offsets
    with pytest.raises(ValueError):
        regions.split(np.zeros((2, 4, 5), bool), [pts])                   # one array for two images
    with pytest.raises(ValueError):
        regions.split(np.zeros((2, 4, 5), bool), pts, offsets=[0, 1, 3])  # offsets do not end at the points
    with pytest.raises(ValueError):
        regions.split(np.zeros((2, 4, 5), bool), pts, offsets=[0, 2])
    with pytest.raises(ValueError):
        regions.split(m, pts, limits=[1, 2])
    with pytest.raises(TypeError):
        regions.split(m, pts, limits=1.5)
    with pytest.raises(ValueError, match="2\\^31"):
        regions.split(torch.zeros((1, 40000, 40000), dtype=torch.bool, device="meta"), pts)    # as the distance transform's limit
    with pytest.raises(ValueError, match="2\\^31"):
        detect._check_dt_shape((40000, 40000))


def test_measure_labels_argument_errors_come_before_device_work():
    lab = np.zeros((4, 5), np.int32)
    for bad in (lab.astype(bool), lab.astype(np.int64), lab.astype(np.uint8), lab.astype(np.float32), torch.zeros(4, 5, dtype=torch.int16)):
        with pytest.raises(TypeError):
            regions.measure_labels(bad)
    with pytest.raises(TypeError):
        regions.measure_labels([[1, 2]])
    for bad in (np.zeros(5, np.int32), np.zeros((1, 2, 3, 4), np.int32), np.zeros((0, 5), np.int32)):
        with pytest.raises(ValueError):
            regions.measure_labels(bad)
    with pytest.raises(TypeError):
        regions.measure_labels(lab, intensity=np.zeros((4, 5), np.int32))
    with pytest.raises(ValueError):
        regions.measure_labels(lab, intensity=np.zeros((5, 4), np.uint8))
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError):
            regions.measure_labels(lab, max_regions=bad)
    for bad in (np.zeros(1, np.int32), torch.zeros(1, dtype=torch.int64), torch.zeros(2, dtype=torch.int32)):
        with pytest.raises(TypeError):
            regions.measure_labels(lab, counts=bad)
    with pytest.raises(TypeError):
        regions.measure(lab)                                              # integer input stays refused there
    with pytest.raises(TypeError):
        inference.measure_slide_cells(np.zeros((4, 5), np.uint8))
    res = inference.SlideResult(np.zeros((0, 2), np.int64), [], 0, torch.zeros(4, 5, dtype=torch.float32))
    with pytest.raises(TypeError):
        inference.measure_slide_cells(res)
    res.mask = torch.zeros(4, 5, dtype=torch.uint8)
    with pytest.raises(ValueError):
        inference.measure_slide_cells(res, thr_u8=300)


def test_entry_points_in_header_table_and_library():
    header = open(os.path.join(ROOT, "include", "cellseg_hip.h")).read()
    lib = _lib.load()
    for name, n_args, restype in (("cs_regions_split_workspace", 4, ctypes.c_size_t), ("cs_regions_split", 15, ctypes.c_int),
                                  ("cs_regions_measure_labels", 13, ctypes.c_int)):
        decl = re.search(rf"\b(?:int|size_t) {name}\((.*?)\);", header, flags=re.S)
        assert decl is not None and len(decl.group(1).split(",")) == n_args
        got_restype, argtypes = _lib._SIGNATURES[name]
        assert got_restype is restype and len(argtypes) == n_args and hasattr(lib, name)
        assert f" * {name}" in header or name.endswith("_workspace")     # described in the section's comment
    assert _lib._SIGNATURES["cs_regions_split"][1][-1] is ctypes.c_void_p and _lib._SIGNATURES["cs_regions_split"][1][-2] is ctypes.c_size_t
    assert callable(kernels.regions_split) and callable(kernels.regions_measure_labels) and callable(kernels.regions_split_workspace)
    # sizes a call would refuse have no workspace; the seed records come on top of the labelling's
    assert lib.cs_regions_split_workspace(0, 4, 5, 1) == 0 and lib.cs_regions_split_workspace(1, 4, 5, -1) == 0
    assert lib.cs_regions_split_workspace(2, 70, 90, 5) == lib.cs_regions_workspace(2, 70, 90) + 5 * 16
    assert lib.cs_regions_split_workspace(2, 70, 90, 0) == lib.cs_regions_workspace(2, 70, 90)
    # argument checks of the library itself: refused with a message, nothing launched
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    assert lib.cs_regions_split(p, 1, 4, 5, 3, p, p, None, 1, p, p, p, p, 4096, None) == -1 and b"connectivity" in lib.cs_last_error()
    assert lib.cs_regions_split(p, 1, 4, 5, 1, None, p, None, 1, p, p, p, p, 4096, None) == -1 and b"points" in lib.cs_last_error()
    assert lib.cs_regions_split(p, 1, 4, 5, 1, p, p, None, 100, p, p, p, p, 1024, None) == -1 and b"workspace" in lib.cs_last_error()
    assert lib.cs_regions_split(p, 1, 40000, 40000, 1, p, p, None, 1, p, p, p, p, 1 << 40, None) == -1 and b"2^31" in lib.cs_last_error()
    assert lib.cs_regions_measure_labels(p, None, 1, 4, 5, 0, p, p, p, p, None, None, None) == -1 and b"capacity" in lib.cs_last_error()
    assert lib.cs_regions_measure_labels(p, p, 1, 4, 5, 2, p, p, p, p, None, None, None) == -1 and b"intensity" in lib.cs_last_error()
    assert lib.cs_regions_measure_labels(None, None, 1, 4, 5, 2, p, p, p, p, None, None, None) == -1 and b"NULL" in lib.cs_last_error()
