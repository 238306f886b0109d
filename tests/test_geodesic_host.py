"""CPU: the plain-loop statement of the geodesic seeded split (tests/geodesic_ref.py) against its own guarantees -- connected cells
that hold their seed, the tiled model's fixpoint equal to Dijkstra's, no label across a 4-component -- and against
tests/golden/geodesic_vectors.npz; the precondition of the headline GPU test (the Euclidean split tears the horseshoe, the geodesic
one does not); the new entry points in the header and the ctypes table, and the argument errors of the library and of
regions.split_geodesic, which come before any device work."""
import ctypes
import dataclasses
import os
import re
import sys

import numpy as np
import pytest
import torch
from scipy import ndimage as ndi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import geodesic_ref as G  # noqa: E402
import make_geodesic_golden as MK  # noqa: E402
import split_ref as S  # noqa: E402
from cellsegmentation_amd import _lib, detect, inference, kernels, regions  # noqa: E402

GOLD_PATH = os.path.join(ROOT, "tests", "golden", "geodesic_vectors.npz")
GOLD = np.load(GOLD_PATH, allow_pickle=False)
NAMES = sorted(k[:-len(".labels")] for k in GOLD.files if k.endswith(".labels"))
SHAPES = [(70, 90), (37, 130), (130, 67)]
FULL = np.ones((3, 3), bool)


def _random_case(hw, connectivity):
    m = G.noise_masks(1, *hw, seed=hw[1] + connectivity, density=0.8)[0]
    return m, S.random_seeds([m], 14, seed=hw[0])[0]


@pytest.mark.parametrize("connectivity", [1, 2])
@pytest.mark.parametrize("hw", SHAPES)
def test_every_seeded_cell_is_connected_and_the_tiled_model_agrees(hw, connectivity):
    m, pts = _random_case(hw, connectivity)
    labels, count, live, dist = G.split_one(m, pts, connectivity)
    assert live.sum() >= 5 and np.array_equal(labels > 0, m) and count == labels.max()
    first = {}
    for k, (r, c) in enumerate(pts):
        if live[k]:
            first.setdefault((r, c), k)                                 # of two seeds on one pixel the lower index owns it
    for (r, c), k in first.items():
        cell = labels == k + 1
        assert cell[r, c] and dist[r, c] == 0 and ndi.label(cell, structure=FULL)[1] == 1, k
    for k in np.nonzero(~live)[0]:
        assert not (labels == k + 1).any()
    assert G.disconnected_labels(np.where(labels <= len(pts), labels, 0)) == []
    assert ((dist == -1) == (labels > len(pts))).all() and (dist[~m] == 0).all()
    rounds, state = G.jacobi_rounds(m, pts, connectivity, want_state=True)
    assert 2 <= rounds <= 8
    tiled = np.zeros_like(labels)
    tiled_d = np.full_like(dist, -1)
    for (r, c), (d, k) in state.items():
        tiled[r, c], tiled_d[r, c] = k + 1, d
    seeded = (labels > 0) & (labels <= len(pts))
    assert np.array_equal(tiled[seeded], labels[seeded]) and np.array_equal(tiled_d[seeded], dist[seeded]) and not tiled[~seeded].any()
    if connectivity == 1:                                               # no label crosses a 4-component
        comp = ndi.label(m)[0]
        for k in np.unique(labels[seeded]):
            assert len(np.unique(comp[labels == k])) == 1


def test_the_euclidean_split_tears_the_horseshoe_and_the_geodesic_one_does_not():
    m, pts = G.horseshoe()
    assert m.shape == (70, 90) and m[8:62, 64].any() and m[8:62, 63].any() and m[61].any() and not m[62:].any()
    euclid = S.split_one(m, pts)[0]
    assert G.disconnected_labels(euclid) == [1]
    labels, count, live, dist = G.split_one(m, pts)
    assert G.disconnected_labels(labels) == [] and count == 2 and live.all()
    # the far arm is the base's, though its top corner is nearer to the other seed as the crow flies
    assert (labels[8:50, 68:80] == 2).all() and euclid[8, 68] == 1
    assert G.jacobi_rounds(m, pts) <= 4


def test_the_serpentine_needs_nineteen_rounds_of_the_model():
    m, pts = G.serpentine()
    assert m.shape == (37, 130) and m.sum() == 169 and ndi.label(m)[1] == 1
    assert (m[:, 63] & m[:, 64]).sum() == 17
    assert G.jacobi_rounds(m, pts) == 19
    labels, count, live, dist = G.split_one(m, pts)
    assert dist.max() == 744 and (labels[m] == 1).all() and count == 1


def test_ties_and_foreign_seeds():
    m, pts = G.two_discs()
    mid = int(pts[:, 1].sum()) // 2
    lab = G.split_one(m, pts)[0]
    assert (lab[:, :mid + 1][m[:, :mid + 1]] == 1).all() and (lab[:, mid + 1:][m[:, mid + 1:]] == 2).all()
    lab = G.split_one(m, pts[::-1])[0]
    assert (lab[:, :mid][m[:, :mid]] == 2).all() and (lab[:, mid:][m[:, mid:]] == 1).all()
    m, pts = G.foreign_seed()
    for conn in (1, 2):
        lab = G.split_one(m, pts, conn)[0]
        assert (lab[8:28, 42:100] == 2).all() and (lab[5:30, 10:40] == 1).all()


@pytest.mark.parametrize("name", NAMES)
def test_reference_equals_the_golden_vectors(name):
    shape = tuple(GOLD[f"{name}.shape"])
    m = np.unpackbits(GOLD[f"{name}.mask"], axis=1)[:, :shape[2]].astype(bool).reshape(shape)
    lim = GOLD[f"{name}.limits"]
    got = G.split(m, GOLD[f"{name}.points"], GOLD[f"{name}.offsets"], lim if len(lim) else None, int(GOLD[f"{name}.connectivity"]))
    for key in MK.KEYS:
        assert got[key].dtype == GOLD[f"{name}.{key}"].dtype and np.array_equal(got[key], GOLD[f"{name}.{key}"]), key
    assert np.array_equal(got["labels"] > 0, m)


def test_golden_file_regenerates_bit_for_bit():
    assert NAMES == ["batch1", "batch2", "horseshoe", "noise_70x90", "serpentine", "tie"]
    assert os.path.getsize(GOLD_PATH) < 96 * 1024
    fresh = MK.build()
    assert sorted(fresh) == sorted(GOLD.files)
    for key, want in fresh.items():
        assert GOLD[key].dtype == np.asarray(want).dtype and np.array_equal(GOLD[key], want), key
    assert {int(GOLD[f"{n}.connectivity"]) for n in NAMES} == {1, 2}
    assert GOLD["batch1.shape"].tolist() == [3, 130, 67] and GOLD["batch1.offsets"].tolist() == [0, 14, 14, 37]
    assert GOLD["batch1.n_seeds"].tolist() == [14, 0, 9] and not GOLD["batch1.live"].all()


def test_entry_points_in_header_table_and_library():
    header = open(os.path.join(ROOT, "include", "cellseg_hip.h")).read()
    lib = _lib.load()
    for name, n_args, restype in (("cs_regions_geodesic_workspace", 4, ctypes.c_size_t), ("cs_regions_split_geodesic", 19, ctypes.c_int)):
        decl = re.search(rf"\b(?:int|size_t) {name}\((.*?)\);", header, flags=re.S)
        assert decl is not None and len(decl.group(1).split(",")) == n_args
        got_restype, argtypes = _lib._SIGNATURES[name]
        assert got_restype is restype and len(argtypes) == n_args and hasattr(lib, name) and name in _lib.exported_symbols()
    assert " * cs_regions_split_geodesic" in header
    assert _lib._SIGNATURES["cs_regions_split_geodesic"][1][-1] is ctypes.c_void_p
    assert _lib._SIGNATURES["cs_regions_split_geodesic"][1][-2] is ctypes.c_size_t
    assert callable(kernels.regions_split_geodesic) and callable(kernels.regions_geodesic_workspace)
    assert lib.cs_abi_version() == 10
    # the Euclidean split's entry points stand as they were
    assert len(_lib._SIGNATURES["cs_regions_split"][1]) == 15
    assert lib.cs_regions_split_workspace(2, 70, 90, 5) == lib.cs_regions_workspace(2, 70, 90) + 5 * 16


def test_workspace_sizes():
    lib = _lib.load()
    ws = lib.cs_regions_geodesic_workspace
    assert ws(0, 4, 5, 1) == 0 and ws(1, 4, 5, -1) == 0 and ws(1, 0, 5, 1) == 0 and ws(65536, 4, 5, 1) == 0
    assert ws(1, 20000, 20000, 1) == 0                                  # 7 H W >= 2^31
    assert ws(1, 17000, 18000, 1) > 0                                   # 7 H W just below it
    # the split's arrays, a 64-bit key per pixel and two bytes per 64 x 64 tile, each array padded to 16 bytes
    assert ws(2, 70, 90, 5) == lib.cs_regions_split_workspace(2, 70, 90, 5) + 8 * 2 * 70 * 90 + 16
    assert ws(2, 70, 90, 6) - ws(2, 70, 90, 5) == 16 and ws(2, 70, 90, 0) < ws(2, 70, 90, 1)


def test_library_argument_checks_without_a_gpu():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(8192)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    call = lib.cs_regions_split_geodesic

    def refused(why, *, conn=1, points=p, P=1, rounds=4, converged=p, H=4, W=5, bytes_=8000):
        assert call(p, 1, H, W, conn, points, p, None, P, rounds, 0, p, p, p, None, converged, p, bytes_, None) == -1
        assert why in lib.cs_last_error(), lib.cs_last_error()

    assert lib.cs_regions_geodesic_workspace(1, 4, 5, 1) <= 8000
    refused(b"connectivity", conn=3)
    refused(b"converged", converged=None)
    refused(b"rounds", rounds=0)
    refused(b"rounds", rounds=-2)
    refused(b"points", points=None)
    refused(b"workspace", bytes_=lib.cs_regions_geodesic_workspace(1, 4, 5, 1) - 1)
    refused(b"workspace", bytes_=lib.cs_regions_split_workspace(1, 4, 5, 1))          # the Euclidean split's is too small
    refused(b"7 H W < 2^31", H=20000, W=20000, bytes_=1 << 40)


def test_split_geodesic_argument_errors_come_before_device_work():
    m = np.zeros((4, 5), bool)
    pts = np.asarray([[1, 1], [2, 3]])
    for bad in (m.astype(np.uint8), m.astype(np.int32), torch.zeros(4, 5, dtype=torch.float32)):
        with pytest.raises(TypeError):
            regions.split_geodesic(bad, pts)
    for bad in (np.zeros(5, bool), np.zeros((1, 2, 3, 4), bool), np.zeros((0, 5), bool)):
        with pytest.raises(ValueError):
            regions.split_geodesic(bad, pts)
    for conn in (0, 3, None):
        with pytest.raises(ValueError):
            regions.split_geodesic(m, pts, connectivity=conn)
    for bad in ([[-1, 0]], [[4, 0]], [[0, 5]], [[0, -1]]):
        with pytest.raises(ValueError, match="outside"):
            regions.split_geodesic(m, np.asarray(bad))
        with pytest.raises(ValueError, match="outside"):
            regions.split_geodesic(m, torch.tensor(bad))
    with pytest.raises(TypeError):
        regions.split_geodesic(m, pts.astype(np.float32))
    with pytest.raises(ValueError):
        regions.split_geodesic(m, np.zeros((3, 3), np.int64))
    with pytest.raises(ValueError):
        regions.split_geodesic(np.zeros((2, 4, 5), bool), pts)
    with pytest.raises(ValueError):
        regions.split_geodesic(np.zeros((2, 4, 5), bool), [pts])
    with pytest.raises(ValueError):
        regions.split_geodesic(np.zeros((2, 4, 5), bool), pts, offsets=[0, 1, 3])
    with pytest.raises(ValueError):
        regions.split_geodesic(m, pts, limits=[1, 2])
    with pytest.raises(TypeError):
        regions.split_geodesic(m, pts, limits=1.5)
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="max_rounds"):
            regions.split_geodesic(m, pts, max_rounds=bad)
    with pytest.raises(ValueError, match="2\\^31"):
        regions.split_geodesic(torch.zeros((1, 40000, 40000), dtype=torch.bool, device="meta"), pts)
    with pytest.raises(ValueError, match="7 H W"):
        regions.split_geodesic(torch.zeros((1, 20000, 20000), dtype=torch.bool, device="meta"), pts)    # split itself takes this one


def test_result_type_and_opt_in_wiring():
    assert issubclass(regions.GeodesicSplitResult, regions.SplitResult)
    names = [f.name for f in dataclasses.fields(regions.GeodesicSplitResult)]
    assert names == ["labels", "counts", "n_seeds", "live", "converged", "distance"]
    import inspect
    assert inspect.signature(detect.DetectResult.split).parameters["geodesic"].default is False
    assert inspect.signature(inference.measure_slide_cells).parameters["geodesic"].default is False
    assert inspect.signature(inference.evaluate_instances).parameters["geodesic"].default is False
    sig = inspect.signature(regions.split_geodesic).parameters
    assert list(sig) == ["m", "points", "offsets", "limits", "connectivity", "max_rounds", "want_distance"]
    assert sig["max_rounds"].default is None and sig["connectivity"].default == 1 and sig["want_distance"].default is False
