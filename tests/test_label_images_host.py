"""CPU: the argument errors of the nine ``regions`` calls that take a label image (``measure_labels``, ``match_labels``,
``overlap_labels``, ``hausdorff_labels``, ``adjacency_labels``, ``shape_labels``, ``hull_labels``, ``contour_labels``, ``boundaries``),
which the shared front end (``regions._LabelImage`` / ``_LabelPair``) raises before anything is copied to a device; the reader of a
raw pair table on a table made by hand; the growth of a pair table with a run that drops pairs up to a given size; the gathering of
the chunks' tables; the host cache and the workspace memo."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cellsegmentation_amd import _args  # noqa: E402
from cellsegmentation_amd import regions as G  # noqa: E402

ONE = ("measure_labels", "adjacency_labels", "shape_labels", "hull_labels", "contour_labels", "boundaries")
TWO = ("match_labels", "overlap_labels", "hausdorff_labels")
LAB = np.zeros((2, 4, 5), np.int32)


@pytest.fixture(autouse=True)
def no_device(monkeypatch):
    """whoever asks for a device fails the test"""
    def touched(*_):
        raise AssertionError("a device was asked for before the arguments were checked")
    monkeypatch.setattr(G, "_device", touched)
    monkeypatch.setattr(_args, "_device", touched)


def _call(name, x, other=LAB, **kw):
    """``name`` with ``x`` as its label image; a pair call takes ``other`` as the second one"""
    return getattr(G, name)(x, other, **kw) if name in TWO else getattr(G, name)(x, **kw)


@pytest.mark.parametrize("name", ONE + TWO)
def test_label_image_errors_name_the_call_and_touch_no_device(name):
    with pytest.raises(TypeError, match=f"{name}: expected an int32 label image, got torch.float32"):
        _call(name, LAB.astype(np.float32))
    with pytest.raises(TypeError, match=f"{name}: expected an int32 label image, got torch.int64"):
        _call(name, torch.zeros((4, 5), dtype=torch.int64))
    with pytest.raises(TypeError, match=f"{name}: expected a numpy array or a torch tensor"):
        _call(name, [[1, 2]])
    if name != "boundaries":                                            # (which takes a boolean mask and labels it first)
        with pytest.raises(TypeError, match=f"{name}: expected an int32 label image, got torch.bool \\(boolean masks go to "):
            _call(name, LAB > 0)
    for bad in (LAB[0, 0], LAB[None]):                                  # 1-D, 4-D
        with pytest.raises(ValueError, match=f"{name}: expected \\[H, W\\] or \\[N, H, W\\], got shape"):
            _call(name, bad)
    with pytest.raises(ValueError, match=f"{name}: empty label image"):
        _call(name, LAB[:0])
    if name in TWO:                                                     # the second image is checked alike, and against the first
        with pytest.raises(TypeError, match=f"{name}: expected an int32 label image, got torch.bool"):
            _call(name, LAB, LAB > 0)
        with pytest.raises(ValueError, match=f"{name}: expected \\[H, W\\] or \\[N, H, W\\]"):
            _call(name, LAB, LAB[None])
        for other in (LAB[0], LAB[:1], LAB[:, :3], np.zeros((2, 4, 6), np.int32)):
            with pytest.raises(ValueError, match=f"{name}: pred of shape \\(2, 4, 5\\) against truth of shape"):
                _call(name, LAB, other)


def _bad_counts(n):
    return (torch.zeros(n, dtype=torch.int64), torch.zeros(n + 1, dtype=torch.int32), torch.zeros((n, 1), dtype=torch.int32),
            np.zeros(n, np.int32), [0] * n, 0)


@pytest.mark.parametrize("name", ONE[:-1] + TWO)
def test_counts_errors_touch_no_device(name):
    # shape_labels, hull_labels and contour_labels hand their counts to measure_labels, in whose name they are refused
    who = "measure_labels" if name in ("shape_labels", "hull_labels", "contour_labels") else name
    for x, n in ((LAB, 2), (LAB[0], 1)):
        for key in (("pred_counts", "truth_counts") if name in TWO else ("counts",)):
            for bad in _bad_counts(n):
                with pytest.raises(TypeError, match=f"{who}: {key} must be an int32 tensor of shape \\({n},\\)"):
                    _call(name, x, x, **{key: bad})
    if name in TWO:                                                     # pred's counts are looked at first
        with pytest.raises(TypeError, match="pred_counts must be"):
            _call(name, LAB, pred_counts=0, truth_counts=0)


def test_size_checks_come_before_any_copy():
    wide = torch.zeros((1, 1), dtype=torch.int32).expand(1, 40000)
    with pytest.raises(ValueError, match="shape_labels: a 1x40000 image"):
        G.shape_labels(wide)
    tall = torch.zeros((1, 1), dtype=torch.int32).expand(46342, 46342)
    with pytest.raises(ValueError, match="2\\^31 pixels"):
        G.hull_labels(tall)
    with pytest.raises(ValueError, match="hausdorff_labels: squared distances"):
        G.hausdorff_labels(tall[:, :40000], tall[:, :40000])
    with pytest.raises(ValueError, match="hull_labels: max_regions 3 against a RegionTable of capacity 2"):
        z = torch.zeros((2, 2), dtype=torch.int32)
        G.hull_labels(LAB, table=G.RegionTable(z[0], 2, z, torch.zeros((2, 2, 4), dtype=torch.int32), z), max_regions=3)


def test_label_image_record():
    img = G._LabelImage("measure_labels", LAB[0])
    assert img.two_d and img.N == 1 and img.own is None and img.counts is None and tuple(img.labels.shape) == (4, 5)
    assert img.with_counts(None) is img and img.own is True
    given = torch.zeros(2, dtype=torch.int32)
    img = G._LabelImage("measure_labels", LAB).with_counts(given)
    assert not img.two_d and img.N == 2 and img.own is False and img.counts is given
    labels, counts = img.place(torch.device("cpu"))                     # (a placed record holds what the kernel calls take)
    assert tuple(labels.shape) == (2, 4, 5) and labels.is_contiguous() and counts is given and img.chunks == [(0, 2)]
    labels, counts = G._LabelImage("boundaries", LAB[0]).place(torch.device("cpu"))
    assert tuple(labels.shape) == (1, 4, 5) and counts is None


def test_pair_reader_on_a_table_made_by_hand():
    key = lambda hi, lo: (hi << 32) | lo  # noqa: E731
    keys = torch.tensor([[key(2, 3), 0, key(1, 5), key(1, 2)], [0, key(4, 1), 0, 0]], dtype=torch.int64)
    first = torch.tensor([[7, 0, 9, 4], [0, 3, 0, 0]], dtype=torch.int32)
    second = torch.tensor([[1, 0, 0, 2], [0, 8, 0, 0]], dtype=torch.int32)
    got = G._read_pairs(keys, first, second)
    assert len(got) == 5 and all(c.dtype == np.int64 for c in got)
    assert list(zip(*(c.tolist() for c in got))) == [(0, 1, 2, 4, 2), (0, 1, 5, 9, 0), (0, 2, 3, 7, 1), (1, 4, 1, 3, 8)]
    got = G._read_pairs(keys, first)
    assert list(zip(*(c.tolist() for c in got))) == [(0, 1, 2, 4), (0, 1, 5, 9), (0, 2, 3, 7), (1, 4, 1, 3)]
    assert all(len(c) == 0 and c.dtype == np.int64 for c in G._read_pairs(torch.zeros_like(keys), first, second))
    # both tables read through it
    z = torch.zeros((2, 1), dtype=torch.int32)
    over = G.OverlapTable(z[:, 0], z[:, 0], 1, 1, *([z] * 2), *([z[:, 0]] * 2), *([z] * 6), keys, first)
    assert [c.tolist() for c in over.pairs()] == [c.tolist() for c in got]
    adj = G.AdjacencyTable(z[:, 0], 1, 2, z[:, 0], z[:, 0], *([z] * 6), keys, first, second)
    assert list(zip(*(c.tolist() for c in adj.pairs())))[-1] == (1, 4, 1, 3, 8)


class _Table:
    def __init__(self, dropped):
        self.dropped = torch.tensor([0, dropped], dtype=torch.int32)


@pytest.mark.parametrize("start,most,fits,want", [(3, 100, 20, [3, 6, 12, 24]), (3, 100, 3, [3]), (3, 20, 50, [3, 6, 12, 20]),
                                                   (50, 20, 1, [20]), (50, 20, 99, [20]), (4, 16, 16, [4, 8, 16]), (1, 1, 5, [1])])
def test_the_pair_table_grows_by_doubling_and_stops_at_most(start, most, fits, want):
    sizes = []

    def run(pairs):
        sizes.append(pairs)
        return _Table(0 if pairs >= fits else fits - pairs)

    table = G._grow_pairs(run, start, most)
    assert sizes == want and int(table.dropped.max()) == (0 if want[-1] >= fits else fits - want[-1])


def test_gathering_the_chunks_tables():
    a = {"slot_keys": torch.arange(8).reshape(2, 4), "slot_counts": torch.ones((2, 4)), "area": None}
    b = {"slot_keys": torch.arange(4).reshape(1, 4), "slot_counts": torch.zeros((1, 4)), "area": None}
    one = G._gather_slots([a], ("slot_keys", "slot_counts"))
    assert list(one) == ["slot_keys", "slot_counts"] and all(one[k] is a[k] for k in one)     # one chunk: the views themselves
    both = G._gather_slots([a, b], ("slot_keys", "slot_counts"))
    assert both["slot_keys"].tolist() == [[0, 1, 2, 3], [4, 5, 6, 7], [0, 1, 2, 3]]
    assert both["slot_counts"].tolist() == [[1.0] * 4] * 2 + [[0.0] * 4]


def test_one_transfer_serves_every_score(monkeypatch):
    z = torch.zeros((1, 2), dtype=torch.int32)
    table = G.MatchTable(z[:, 0], z[:, 0], 2, 2, z, z, z, z, z)
    made = []
    inner = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda t, *a, **kw: made.append(1) or inner(t, *a, **kw))
    table.score()
    assert len(made) == 4 and len(table._host) == 4 and all(x.dtype == np.int64 for x in table._host)
    held = table._host
    table.score(iou_threshold=0.75)
    assert len(made) == 4 and table._host is held
    hausdorff = G.HausdorffTable(z[:, 0], z[:, 0], 2, 2, z, z, z[:, 0], z, z - 1, z, z - 1)
    hausdorff.score(), hausdorff.score()
    assert len(made) == 8 and len(hausdorff._host) == 4


def test_the_workspace_is_kept_while_the_chunk_size_stays():
    made = []
    workspace = G._Workspace(lambda n: made.append(n) or object())
    first = workspace(2)
    assert workspace(2) is first and workspace(1) is not first and workspace(1) is workspace(1) and made == [2, 1]
