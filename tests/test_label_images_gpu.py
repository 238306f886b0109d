"""GPU: one small batch through every call of ``regions`` that takes a label image, in every form the shared front end
(``regions._LabelImage`` / ``_LabelPair``) accepts: numpy, a host tensor, a device tensor; one image as [H, W] and as [1, H, W]; with
the counts given and with them found; and with the batch cut into kernel calls of two images.  Every form of a call has to give what
its first form gave, the counts have to be the largest label of every image, an automatic capacity the largest of those, and the
numpy restatements of tests/*_ref.py are held against the first form once.

The batch: 5 images of 3 x 66, so that a row crosses a 64-lane segment and the image boundaries (198 pixels apart) fall inside a
wave; image 1 is all background, image 0 holds a negative label, image 2 uses labels 1, 2 and 5 only (3 and 4 own no pixel).  The
labels stay below 10, inside what the dense tables of tests/overlap_ref.py and tests/adjacency_ref.py are written for."""
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import adjacency_ref as AR  # noqa: E402
import contour_ref as CR  # noqa: E402
import hausdorff_ref as HR  # noqa: E402
import hull_ref as UR  # noqa: E402
import match_ref as MR  # noqa: E402
import overlap_ref as OR  # noqa: E402
import shape_ref as SR  # noqa: E402
from cellsegmentation_amd import regions as G  # noqa: E402

pytestmark = pytest.mark.gpu

N, H, W = 5, 3, 66
ONE = ("measure_labels", "adjacency_labels", "shape_labels", "hull_labels", "contour_labels", "boundaries")
TWO = ("match_labels", "overlap_labels", "hausdorff_labels")


def _batch():
    lab = np.zeros((N, H, W), np.int32)
    lab[0, :, 2:30], lab[0, 0:2, 30:60], lab[0, 2, 30:66], lab[0, 0:2, 60:66] = 1, 2, 3, -2     # runs across column 64; a negative label
    lab[2, 0, 0:10], lab[2, 1:3, 5:40], lab[2, :, 62:66] = 1, 2, 5                            # labels 3 and 4 own no pixel
    rng = np.random.RandomState(11)
    lab[3] = np.repeat(rng.randint(-1, 7, size=(H, 11)), 6, axis=1)                          # blocks six columns wide
    lab[4] = rng.randint(0, 4, size=(H, W))                                                  # single pixels: many pairs
    truth = np.roll(lab, 3, axis=2)
    truth[1, 1, 60:66] = 4                                                                   # an object against an empty image
    truth[4] = 0                                                                             # and the other way round
    truth[3][truth[3] == 6] = 9
    return lab, truth


PRED, TRUTH = _batch()
TOP = {"pred": np.maximum(PRED.reshape(N, -1).max(axis=1), 0).astype(np.int32),
       "truth": np.maximum(TRUTH.reshape(N, -1).max(axis=1), 0).astype(np.int32)}


def test_the_batch_is_what_the_docstring_says():
    assert PRED.dtype == TRUTH.dtype == np.int32 and W > 64 and (H * W) % 64
    assert not PRED[1].any() and (PRED[0] < 0).any() and sorted(np.unique(PRED[2])) == [0, 1, 2, 5]
    assert TOP["pred"].tolist() == [3, 0, 5, 6, 3] and TOP["truth"].tolist() == [3, 4, 5, 9, 0]
    assert max(PRED.max(), TRUTH.max()) < 10


def _call(name, form, counts=False, images=slice(None)):
    """``name`` on the batch's ``images``, every label image passed through ``form``; counts: also pass the largest labels"""
    fn = getattr(G, name)
    if name in TWO:
        kw = {f"{k}_counts": torch.from_numpy(TOP[k][images].reshape(-1)) for k in ("pred", "truth")} if counts else {}
        return fn(form(PRED[images]), form(TRUTH[images]), **kw)
    kw = {"counts": torch.from_numpy(TOP["pred"][images].reshape(-1))} if counts and name != "boundaries" else {}
    return fn(form(PRED[images]), **kw)


def _flat(res, prefix=""):
    """a result -> name: tensor, int or None, the nested ``RegionTable`` included; the raw pair table is read through ``pairs()``,
    since a pair's slot depends on the order of arrival"""
    if torch.is_tensor(res):
        return {"out": res}
    out = {}
    for f in dataclasses.fields(res):
        v = getattr(res, f.name)
        if dataclasses.is_dataclass(v):
            out.update(_flat(v, f"{prefix}{f.name}."))
        elif not f.name.startswith(("_", "slot_")):
            out[prefix + f.name] = v
    if hasattr(res, "pairs"):
        out.update({f"pairs.{k}": torch.from_numpy(c) for k, c in enumerate(res.pairs())})
    return out


def _same(got, first, lifted=False):
    got, first = _flat(got), _flat(first)
    assert got.keys() == first.keys()
    for k, a in got.items():
        b = first[k]
        if torch.is_tensor(a):
            if lifted and a.dim() == b.dim() - 1:                          # an output of the input's shape: [H, W] against [1, H, W]
                b = b[0]
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.cpu(), b.cpu()), k
        else:
            assert a == b, k


_FIRST = {}


def first(name):
    """the call on numpy arrays, everything found on the device: made once, and left as it is"""
    if name not in _FIRST:
        _FIRST[name] = _call(name, lambda x: x)
    return _FIRST[name]


@pytest.mark.parametrize("name", ONE + TWO)
def test_every_form_gives_what_the_first_gave(dev, name, monkeypatch):
    want = first(name)
    _same(_call(name, torch.from_numpy), want)
    _same(_call(name, lambda x: torch.from_numpy(x).to(dev)), want)
    _same(_call(name, lambda x: x, counts=True), want)
    _same(_call(name, torch.from_numpy, images=0), _call(name, lambda x: x, images=slice(0, 1)), lifted=True)
    monkeypatch.setattr(G, "_MAX_PIXELS", 2 * H * W + 1)                  # two images per kernel call
    assert [b - a for a, b in G._chunks(torch.empty((N, H, W)))] == [2, 2, 1]
    _same(_call(name, lambda x: x), want)
    _same(_call(name, lambda x: x, counts=True), want)


@pytest.mark.parametrize("name", ONE[:-1] + TWO)
def test_counts_and_automatic_capacities(dev, name):
    t = _flat(first(name))
    sides = ("pred", "truth") if name in TWO else ("pred",)
    for side in sides:
        counts = [v for k, v in t.items() if k.split(".")[-1] in ("counts", f"counts_{side}")]
        caps = [v for k, v in t.items() if k.split(".")[-1] in ("capacity", f"cap_{side}")]
        assert len(counts) == 1 and len(caps) == 1
        assert counts[0].dtype == torch.int32 and np.array_equal(counts[0].cpu().numpy(), TOP[side])
        assert caps[0] == max(1, int(TOP[side].max()))
    if name in ("overlap_labels", "adjacency_labels"):
        assert not t["dropped"].cpu().numpy().any() and t["n_pairs"].cpu().numpy().sum() == len(t["pairs.0"]) > 0


def _equal(t, ref, keys, rename=None):
    for k in keys:
        got = t[(rename or {}).get(k, k)].cpu().numpy()
        assert got.dtype == ref[k].dtype and np.array_equal(got, ref[k]), k


def test_the_restatements_agree_once(dev):
    shape = SR.shape_labels(PRED)
    table = {"area": "table.area", "bbox": "table.bbox", "sum_rc": "table.sum_rc"}
    _equal(_flat(first("measure_labels")), shape, ("area", "bbox", "sum_rc"))
    _equal(_flat(first("shape_labels")), shape, ("area", "bbox", "sum_rc", "moments", "tallies", "edges"), table)
    assert np.array_equal(first("boundaries").cpu().numpy(), shape["edges"])
    _equal(_flat(first("hull_labels")), UR.hull_labels(PRED), ("area", "bbox", "sum_rc", "hull"), table)
    contour = CR.contour_labels(PRED)
    assert not contour["hit_bound"].any()
    _equal(_flat(first("contour_labels")), contour, ("area", "bbox", "sum_rc", "contour", "vertices"), table)
    adjacency = AR.adjacency(PRED)
    t = _flat(first("adjacency_labels"))
    _equal(t, adjacency, AR.TABLES)
    assert all(np.array_equal(t[f"pairs.{k}"].numpy(), c) for k, c in enumerate(adjacency["pairs"]))
    _equal(_flat(first("match_labels")), MR.match(PRED, TRUTH), ("area_pred", "area_truth", "match", "inter", "match_truth"))
    hausdorff = HR.hausdorff(PRED, TRUTH)
    t = _flat(first("overlap_labels"))
    _equal(t, hausdorff["overlap"], OR.TABLES)
    assert all(np.array_equal(t[f"pairs.{k}"].numpy(), c) for k, c in enumerate(hausdorff["overlap"]["pairs"]))
    _equal(_flat(first("hausdorff_labels")), hausdorff, HR.TABLES + HR.CARRIED)
