"""cellsegmentation_amd/_points.py and csrc/cs_points.h without a GPU: every input form of ``PointSet`` gives the arrays of a plain
numpy restatement (tests/spatial_ref.py), limits mean Python's ``[:c]`` literally, the argument errors of the five front ends are
still raised, and the header's two functions agree with a slice on every small offsets array (tests/host/points_window.cpp, a
stand-alone program built with the address and undefined-behaviour sanitizers)."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import spatial_ref as SR  # noqa: E402
from cellsegmentation_amd import _points as P  # noqa: E402
from cellsegmentation_amd import detect, regions, render, score, spatial  # noqa: E402

PER_IMAGE = [[(1, 2), (3, 4), (5, 6)], [], [(7, 8)], [(9, 10), (-1, 40), (11, 12), (13, 14)]]
PTS, OFF = SR.ragged(PER_IMAGE)


def _same(ps, pts, off, lim=None):
    assert not ps.on_device and ps.pts.dtype == np.int64 and ps.off.dtype == np.int64
    assert np.array_equal(ps.pts, pts) and np.array_equal(ps.off, off) and ps.n_images == len(off) - 1 and ps.rows == len(pts)
    assert (ps.lim is None) if lim is None else (ps.lim.dtype == np.int32 and np.array_equal(ps.lim, lim))


def test_every_input_form_gives_the_same_arrays():
    one = np.asarray(PER_IMAGE[0])
    for form in (one, one.tolist(), [tuple(r) for r in one], torch.from_numpy(one), one.astype(np.int16), one.astype(np.uint64),
                 torch.from_numpy(one).to(torch.int32)):
        _same(P.PointSet(form), one, [0, 3])
        _same(P.PointSet(form, n_images=1), one, [0, 3])
    for empty in ([], np.asarray([]), np.zeros((0, 2), np.int32), torch.zeros((0, 2), dtype=torch.int64)):
        _same(P.PointSet(empty), np.zeros((0, 2), np.int64), [0, 0])
    lists = [np.asarray(a, np.int64).reshape(-1, 2) for a in PER_IMAGE]
    for form in (PER_IMAGE, tuple(lists), [torch.from_numpy(a) for a in lists], [a.astype(np.int32) for a in lists]):
        _same(P.PointSet(form, n_images=4, per_image=True), PTS, OFF)
        pts, off = P.ragged(form)
        assert np.array_equal(pts, PTS) and np.array_equal(off, OFF) and pts.dtype == off.dtype == np.int64
    assert score.ragged is P.ragged                                        # the tools import it from score
    for off in (OFF, OFF.tolist(), OFF.astype(np.int32), torch.from_numpy(OFF), torch.from_numpy(OFF).to(torch.int32)):
        _same(P.PointSet(PTS, off), PTS, OFF)
        _same(P.PointSet(torch.from_numpy(PTS), off, n_images=4), PTS, OFF)
        _same(P.PointSet(PTS.tolist(), off, [1, 2, 3, 4]), PTS, OFF, [1, 2, 3, 4])


@pytest.mark.parametrize("limits", [None, 0, 2, -1, -9, 50, [50, 0, -2, 1], [-4, -3, 3, 4], np.asarray([1, 1, 1, 1], np.int64),
                                    torch.tensor([2, -1, 0, -5]), [1 << 40, -(1 << 40), 2, 2]])
def test_limits_are_python_slices(limits):
    ps = P.PointSet(PTS, OFF, limits)
    lim = None if limits is None else np.broadcast_to(np.asarray(limits), (4,))
    kept = np.zeros(len(PTS), bool)
    for n, rows in enumerate(PER_IMAGE):
        idx = list(range(OFF[n], OFF[n + 1]))
        c = len(rows) if ps.lim is None else int(ps.lim[n])
        # the count the kernels form from the uploaded limit (point_window) against the literal slice of the list
        k = min(c, len(rows)) if c >= 0 else max(len(rows) + c, 0)
        want = idx if lim is None else idx[:int(lim[n])]
        assert idx[:k] == want
        kept[want] = True
    inside = (PTS[:, 0] >= 0) & (PTS[:, 0] < 20) & (PTS[:, 1] >= 0) & (PTS[:, 1] < 30)
    assert np.array_equal(SR.live_mask(PTS, OFF, None if limits is None else np.asarray(lim), (20, 30)), kept & inside)
    assert P.limits(limits, 4) is None if limits is None else np.array_equal(P.limits(limits, 4), ps.lim)


def test_point_set_argument_errors():
    good = np.asarray(PER_IMAGE[0])
    for bad in (good.astype(np.float64), good.astype(bool), torch.zeros(2, 2), torch.zeros(2, 2, dtype=torch.bool)):
        with pytest.raises(TypeError, match="integer coordinates"):
            P.PointSet(bad)
    for bad in (np.zeros((2, 3), np.int64), np.zeros(4, np.int64), np.zeros((1, 2, 2), np.int64), torch.zeros(2, 3, dtype=torch.int64)):
        with pytest.raises(ValueError, match=r"\[n, 2\]"):
            P.PointSet(bad)
    with pytest.raises(ValueError, match="int64"):
        P.PointSet(np.asarray([[1 << 63, 0]], np.uint64))
    for bad in ([0, 1], [0, 4], [1, 3], [0, 2, 1, 3], [0], np.asarray([0.0, 3.0])):
        with pytest.raises(ValueError, match="offsets"):
            P.PointSet(good, bad)
    with pytest.raises(TypeError, match="offsets"):
        P.PointSet(good, torch.zeros(2))
    with pytest.raises(ValueError, match="5 offsets"):
        P.PointSet(good, [0, 3], n_images=4)
    with pytest.raises(ValueError, match="one point array per image, or offsets"):
        P.PointSet(good, n_images=2)
    with pytest.raises(ValueError, match="2 images but 1 point arrays"):
        P.PointSet([good], n_images=2, per_image=True)
    with pytest.raises(ValueError, match="65535"):
        P.PointSet(good, np.r_[np.zeros(65536, np.int64), 3])
    P.PointSet(good, np.r_[np.zeros(65536, np.int64), 3], max_images=65536)
    with pytest.raises(TypeError, match="limits"):
        P.PointSet(good, limits_=1.5)
    for bad in ([1, 2], np.zeros((1, 1), np.int64), np.zeros(0, np.int32)):
        with pytest.raises(ValueError, match="limits"):
            P.PointSet(good, limits_=bad)


def test_the_front_ends_still_refuse_what_they_refused():
    good, m = np.asarray([[1, 1], [2, 3]]), np.zeros((4, 5), bool)
    canvas = torch.zeros(16, 20, 3, dtype=torch.uint8)
    calls = {
        "score": lambda p, **kw: score.score_points(p, good, **{"hat_offsets" if k == "offsets" else k: v for k, v in kw.items()}),
        "nearest": lambda p, **kw: spatial.nearest(p, (16, 16), **kw),
        "cluster": lambda p, **kw: spatial.cluster(p, (16, 16), 3, **kw),
        "bin_counts": lambda p, **kw: spatial.bin_counts(p, (16, 16), 4, **kw),
        "split": lambda p, **kw: regions.split(m, p, **kw),
        "split_geodesic": lambda p, **kw: regions.split_geodesic(m, p, **kw),
        "draw_points": lambda p, **kw: render.draw_points(canvas, p, **kw),
    }
    for name, call in calls.items():
        with pytest.raises(TypeError, match="integer"):
            call(good.astype(np.float32))
        with pytest.raises(ValueError, match="shape"):
            call(np.zeros((3, 3), np.int64))
        with pytest.raises(ValueError, match="offsets"):
            call(good, offsets=[0, 1])
        with pytest.raises(TypeError, match="limits"):
            call(good, limits=1.5)
        with pytest.raises(ValueError, match="limits"):
            call(good, limits=[1, 2])
    with pytest.raises(ValueError, match="65535"):
        score.score_points(good, good[:1], hat_offsets=np.r_[np.zeros(65536, np.int64), 2], offsets=np.r_[np.zeros(65536, np.int64), 1])
    with pytest.raises(ValueError, match="int32"):
        score.score_points(good, np.asarray([(0, 1 << 31)]))
    with pytest.raises(ValueError):
        score.score_points(good, good, hat_offsets=[0, 1, 2], offsets=[0, 2])
    with pytest.raises(ValueError):
        spatial.nearest(good, (16, 16), offsets=[0, 1, 2], other=good, other_offsets=[0, 2])
    for fn in (regions.split, regions.split_geodesic):
        for bad in ([[-1, 0]], [[4, 0]], [[0, 5]], [[0, -1]]):
            with pytest.raises(ValueError, match="outside"):
                fn(m, np.asarray(bad))
            with pytest.raises(ValueError, match="outside"):
                fn(m, torch.tensor(bad))
        with pytest.raises(ValueError, match="per image, or offsets"):
            fn(np.zeros((2, 4, 5), bool), good)
        with pytest.raises(ValueError, match="point arrays"):
            fn(np.zeros((2, 4, 5), bool), [good])
    two = torch.zeros(2, 16, 20, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="per image, or offsets"):
        render.draw_points(two, good)
    with pytest.raises(ValueError, match="point arrays"):
        render.draw_points(two, [good])
    with pytest.raises(ValueError, match="tail"):
        render.draw_points(canvas, [(1, 2)], tail=True)
    with pytest.raises(ValueError, match="device"):                        # a list of pairs is one image's points: all is well but the canvas
        render.draw_points(canvas, [(1, 2), (3, 4)], limits=1, tail=True)
    res = detect.DetectResult(good, np.zeros(2, np.int64), np.asarray([0, 1, 2]), np.asarray([1, 1]))
    for bad in (good, [good], np.zeros((3, 1, 2), np.int64)):
        with pytest.raises(ValueError):
            res.score(bad)


def test_the_header_agrees_with_a_slice_on_every_small_offsets_array(tmp_path):
    rocm_clang = os.path.join(os.path.dirname(os.path.realpath(shutil.which("hipcc") or "/opt/rocm/bin/hipcc")), "..", "lib", "llvm", "bin",
                              "clang++")
    cxx = shutil.which("g++") or (rocm_clang if os.path.exists(rocm_clang) else None)
    if cxx is None:
        pytest.skip("no g++ and no hipcc")
    exe = str(tmp_path / "points_window")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "cellsegmentation_amd", "csrc"), os.path.join(ROOT, "tests", "host", "points_window.cpp"), "-o", exe],
                   check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok "), run.stdout + run.stderr
    assert int(run.stdout.split()[1]) > 100000                             # every case was visited
