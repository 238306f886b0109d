"""Scoring of detected points against annotated ones on the GPU (csrc/score.hip through cellsegmentation_amd.score), exact against
the numpy restatement tests/score_ref.py and the vectors of the reference's own get_prf1 (tests/golden/score_vectors.npz): both
kernel paths at every size where the code takes another one, ragged batches with empty images, limits, radii, the (x, y)
convention, repeatability, graph replay, DetectResult.score and the end-to-end inference.evaluate_detection."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import score_ref as R  # noqa: E402
from cellsegmentation_amd import detect as D  # noqa: E402
from cellsegmentation_amd import kernels as K  # noqa: E402
from cellsegmentation_amd import score as S  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "score_vectors.npz"), allow_pickle=False)
NAMES = [str(n) for n in GOLD["names"]]


def check(hats, gts, limits=None, radius=16, radius2=256, force_block=False):
    """one ragged batch through score.score_points against the restatement: counts, match and the float64 bits of p, r, f1"""
    hat, hoff = R.ragged(hats)
    gt, goff = R.ragged(gts)
    want_c, want_p, want_m = R.score_batch(hat, hoff, gt, goff, limits, radius2)
    res = S.score_points(hat, gt, hoff, goff, limits=limits, radius=radius, return_match=True, _force_block=force_block)
    got_c = np.stack([res.tp, res.fp, res.fn], axis=1)
    assert got_c.dtype == np.int64 and res.match.dtype == np.int32
    bad = np.flatnonzero((got_c != want_c).any(axis=1))
    assert not len(bad), (bad[:5], got_c[bad[:5]], want_c[bad[:5]])
    assert np.array_equal(res.match, want_m)
    assert np.stack([res.precision, res.recall, res.f1], axis=1).tobytes() == want_p.tobytes()
    return res


@pytest.mark.parametrize("force_block", [False, True])
def test_golden_cases_as_one_batch_and_one_by_one(dev, force_block):
    hats, gts = [GOLD[f"{n}.hat"] for n in NAMES], [GOLD[f"{n}.gt"] for n in NAMES]
    want_c = np.stack([GOLD[f"{n}.counts"] for n in NAMES])
    want_p = np.stack([GOLD[f"{n}.prf"] for n in NAMES])
    res = check(hats, gts, force_block=force_block)
    assert np.array_equal(np.stack([res.tp, res.fp, res.fn], axis=1), want_c)
    assert np.stack([res.precision, res.recall, res.f1], axis=1).tobytes() == want_p.tobytes()
    for i, name in enumerate(NAMES):
        one = check([hats[i]], [gts[i]], force_block=force_block)
        assert (one.tp[0], one.fp[0], one.fn[0]) == tuple(want_c[i]), name
        assert np.asarray([one.precision[0], one.recall[0], one.f1[0]]).tobytes() == want_p[i].tobytes(), name
    if not force_block:
        for i in (0, 5, NAMES.index("both_empty"), NAMES.index("chain_30_shifted_by_8")):
            got = S.get_prf1(hats[i] if len(hats[i]) else np.asarray([]), gts[i] if len(gts[i]) else np.asarray([]))
            assert np.asarray(got[:3], np.float64).tobytes() == want_p[i].tobytes() and got[3:] == tuple(want_c[i])
            assert all(type(v) is float for v in got[:3]) and all(type(v) is int for v in got[3:])


@pytest.mark.parametrize("n_gt", [0, 1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097])
def test_size_sweep(dev, n_gt):
    """64 | 65: one wave | the workgroup; 4096 | 4097: LDS | global coordinates and workspace flags; 255..257: the scan's stride"""
    rng = np.random.RandomState(1000 + n_gt)
    field = R.field_for(0, n_gt)
    hats, gts = [], []
    for n_hat in (0, 1, 64, 300):
        gt = R.random_points(rng, n_gt, field)
        hats += [R.random_points(rng, n_hat, field), R.random_points(rng, n_hat, field) + 100000]     # about half match | none does
        gts += [gt, gt]
    res = check(hats, gts)
    assert not res.tp[1::2].any()
    if n_gt >= 255:
        assert 0.25 * 300 <= res.tp[6] <= 0.75 * 300, res.tp
    if n_gt <= 64:
        again = check(hats, gts, force_block=True)
        assert np.array_equal(again.match, res.match)


@pytest.mark.parametrize("force_block", [False, True])
def test_batch_of_300_ragged_images(dev, force_block):
    rng = np.random.RandomState(300)
    sizes = [(int(rng.choice([0, 3, 20, 40, 64, 65, 130])), int(rng.choice([0, 1, 10, 35, 64, 65, 200]))) for _ in range(300)]
    for i in (0, 1, 150, 151, 299):
        sizes[i] = (0, 0)
    sizes[2], sizes[149], sizes[298] = (0, 40), (25, 0), (0, 7)           # one side empty
    hats = [R.random_points(rng, a, 90) for a, _ in sizes]
    gts = [R.random_points(rng, b, 90) for _, b in sizes]
    res = check(hats, gts, force_block=force_block)
    assert res.tp.sum() > 1000 and res.fp.sum() > 100 and res.fn.sum() > 100
    assert res.precision[0] == 1.0 and res.recall[2] == 0.0 and res.precision[149] == 0.0
    for i in (0, 3, 149, 298):                                            # N = 1: empty and not
        check([hats[i]], [gts[i]], force_block=force_block)


@pytest.mark.parametrize("n_gt", [40, 100])
def test_limits(dev, n_gt):
    rng = np.random.RandomState(n_gt)
    n_hat = 23
    gt = R.random_points(rng, n_gt, 70)
    hat = R.random_points(rng, n_hat, 70)
    limits = [0, 1, n_hat, n_hat + 5, -1, -n_hat - 1, 7, -7]
    res = check([hat] * len(limits), [gt] * len(limits), limits=limits)
    m = res.match.reshape(len(limits), n_hat)
    kept = [0, 1, n_hat, n_hat, n_hat - 1, 0, 7, n_hat - 7]
    for i, k in enumerate(kept):
        assert (m[i, k:] == -2).all() and (m[i, :k] >= -1).all() and res.tp[i] + res.fp[i] == k
        assert np.array_equal(m[i, :k], m[2, :k])                         # a prefix of the greedy assignment is the assignment of the prefix
    assert res.fn[0] == n_gt and res.fn[5] == n_gt
    check([hat] * 3, [gt] * 3, limits=5)                                  # one count for every image
    check([hat] * 3, [gt] * 3, limits=np.asarray([2, -2, 100], np.int64), force_block=True)
    dev_lim = torch.tensor([3, -3, 0], dtype=torch.int32, device=dev)
    hat3, hoff3 = R.ragged([hat] * 3)
    gt3, goff3 = R.ragged([gt] * 3)
    got = S.score_points(hat3, gt3, hoff3, goff3, limits=dev_lim)
    want = R.score_batch(hat3, hoff3, gt3, goff3, [3, -3, 0])[0]
    assert np.array_equal(np.stack([got.tp, got.fp, got.fn], axis=1), want)


def test_radius(dev):
    hat = [(0, 0), (100, 100), (200, 200), (300, 300), (400, 400)]
    gt = [(0, 0), (100, 116), (204, 216), (301, 316), (400, 401)]         # d2 = 0, 256, 272, 257, 1
    for radius, radius2, tp in ((0, 0, 1), (16, 256, 3), (16.5, 272, 5), (1, 1, 2), (16.03, 256, 3), (16.04, 257, 4)):
        for force_block in (False, True):
            res = check([hat], [gt], radius=radius, radius2=radius2, force_block=force_block)
            assert res.tp[0] == tp, (radius, res.tp)
    far = [(-(1 << 31), -(1 << 31)), ((1 << 31) - 1, (1 << 31) - 1), (1 << 40, 5), (5, 5)]        # differences beyond 2^31; beyond int32
    edge = [((1 << 31) - 1, (1 << 31) - 5), (-(1 << 31), -(1 << 31) + 3), (5, 6)]
    for force_block in (False, True):
        res = check([far], [edge], force_block=force_block)
        assert res.match.tolist() == [1, 0, -1, 2]
        check([far], [edge], radius=46340, radius2=46340 ** 2, force_block=force_block)


def test_xy_annotations_and_input_kinds(dev):
    rng = np.random.RandomState(11)
    hats = [R.random_points(rng, n, 80) for n in (30, 0, 12)]
    gts = [R.random_points(rng, n, 80) for n in (25, 9, 70)]
    hat, hoff = R.ragged(hats)
    gt, goff = R.ragged(gts)
    want = check(hats, gts)
    flipped = np.ascontiguousarray(gt[:, ::-1])
    assert (flipped != gt).any()
    variants = [
        dict(points_hat=hat, points=flipped, hat_offsets=hoff, offsets=goff, gt_xy=True),
        dict(points_hat=torch.from_numpy(hat).to(dev), points=torch.from_numpy(flipped).to(dev), hat_offsets=torch.from_numpy(hoff).to(dev),
             offsets=torch.from_numpy(goff).to(dev), gt_xy=True),
        dict(points_hat=torch.from_numpy(hat), points=torch.from_numpy(gt).to(torch.int16), hat_offsets=hoff.tolist(), offsets=torch.from_numpy(goff)),
        dict(points_hat=hat.astype(np.int32), points=torch.from_numpy(gt).to(dev), hat_offsets=hoff, offsets=goff.astype(np.int32)),
    ]
    for kw in variants:
        got = S.score_points(return_match=True, **kw)
        assert np.array_equal(got.match, want.match) and np.array_equal(got.tp, want.tp) and np.array_equal(got.fn, want.fn)
        assert got.f1.tobytes() == want.f1.tobytes()
    assert S.score_points(hat, gt, hoff, goff).match is None
    # the swapped convention without the flag is another result
    assert not np.array_equal(S.score_points(hat, flipped, hoff, goff, return_match=True).match, want.match)


def test_two_runs_identical_and_graph_replay(dev):
    sizes = [(60, 30), (300, 500), (120, 4200), (0, 0)]

    def batch(seed):
        r = np.random.RandomState(seed)
        hat, hoff = R.ragged([R.random_points(r, a, R.field_for(a, b)) for a, b in sizes])
        gt, goff = R.ragged([R.random_points(r, b, R.field_for(a, b)) for a, b in sizes])
        return hat, hoff, gt.astype(np.int32), goff

    def up(x):
        return torch.from_numpy(x).to(dev)

    hat, hoff, gt, goff = batch(1)
    lim = torch.tensor([50, -1, 100, 3], dtype=torch.int32, device=dev)
    args = [up(hat), up(hoff), up(gt), up(goff)]
    c1, m1 = K.score_points(*args, limits=lim, want_match=True)
    c2, m2 = K.score_points(*args, limits=lim, want_match=True)
    assert torch.equal(c1, c2) and torch.equal(m1, m2) and int(c1[:, 0].sum()) > 100
    want_c, _, want_m = R.score_batch(hat, hoff, gt, goff, [50, -1, 100, 3])
    assert np.array_equal(c1.cpu().numpy(), want_c) and np.array_equal(m1.cpu().numpy(), want_m)
    static = [torch.zeros_like(a) for a in args]
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        K.score_points(*static, limits=lim, want_match=True)              # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gc, gm = K.score_points(*static, limits=lim, want_match=True)
    for seed in (1, 2):                                                   # same sizes, other points: the offsets stay valid
        data = batch(seed)
        for s, a in zip(static, data):
            s.copy_(up(a))
        graph.replay()
        ec, em = K.score_points(*[up(a) for a in data], limits=lim, want_match=True)
        assert torch.equal(gc, ec) and torch.equal(gm, em)
    assert torch.equal(gc, K.score_points(*static, limits=lim)[0]) and not torch.equal(gc, c1)


def test_detect_result_score(dev):
    from test_edt_gpu import mixed_batch
    maps = mixed_batch(299, 299)
    counts = [3, 0, 5, 5, 1]
    rng = np.random.RandomState(8)
    free = D.detect_points(torch.from_numpy(maps).to(dev), eps=11, method="distancetransform")
    assert free.device_points.is_cuda and free.device_offsets.is_cuda and free.device_points.dtype == torch.int64
    # annotations: every second detection moved by up to 9 pixels, a few far-away points, shuffled
    gts = []
    for pts, _ in free.per_image():
        near = pts[::2] + rng.randint(-9, 10, size=pts[::2].shape)
        g = np.concatenate([near, rng.randint(400, 500, size=(3, 2))])
        gts.append(g[rng.permutation(len(g))])
    for cc in (None, counts, 2, np.asarray([-1, 100, 0, 1, -5])):
        res = D.detect_points(torch.from_numpy(maps).to(dev), cell_counts=cc, eps=11, method="distancetransform")
        got = res.score(gts, return_match=True)
        kept = [p[0] for p in res.per_image()]
        off = res.offsets
        for i in range(len(maps)):
            tp, fp, fn, m = R.score(kept[i], gts[i])
            assert (got.tp[i], got.fp[i], got.fn[i]) == (tp, fp, fn), (cc, i)
            assert np.array_equal(got.match[off[i]:off[i] + len(kept[i])], m) and (got.match[off[i] + len(kept[i]):off[i + 1]] == -2).all()
            assert np.asarray([got.precision[i], got.recall[i], got.f1[i]]).tobytes() == R.prf(tp, fp, fn).tobytes()
        assert len(got.match) == off[-1]
        xy = res.score([g[:, ::-1] for g in gts], gt_xy=True)
        ragged = res.score(*R.ragged(gts))
        host = D.DetectResult(res.points, res.weights, res.offsets, res.n_kept, res.cell_counts).score(gts)      # no device copy kept
        for other in (xy, ragged, host):
            assert np.array_equal(other.tp, got.tp) and np.array_equal(other.fp, got.fp) and np.array_equal(other.fn, got.fn)
    assert free.score(gts).tp.sum() >= sum(len(p[0][::2]) for p in free.per_image()) * 0.5                         # the moved points are found
    one = D.detect_points(maps[0], eps=11, method="distancetransform")
    assert one.score(gts[0]).tp[0] == free.score(gts).tp[0] and one.score(gts[0][None]).tp[0] == free.score(gts).tp[0]


@pytest.mark.parametrize("reg_limit", [False, True])
def test_evaluate_detection_resnet18(dev, reg_limit):
    import detect_ref
    from cellsegmentation_amd import inference, metrics, synth
    from cellsegmentation_amd.model import resnet as RN
    m = RN.MILresnet18()
    sd = m.state_dict()
    synth.fill_state_dict(sd)
    m.load_state_dict(sd)
    m = m.to(dev).set_compute_dtype(torch.float32)
    m.setmode("segment")
    x = synth.normalise(synth.ihc_tiles(2, 299, seed=21))
    images = [x[:1], x[1:]]
    probs = inference.inference_seg(images, m, dev, mode="test")
    thr = float(np.median(probs))
    thr_for_dt = int(np.median(detect_ref.quantize(probs)))               # random weights need not straddle the default 10
    kw = dict(eps=11, method="distancetransform", thr_for_dt=thr_for_dt)
    cells = inference.detect_cells(images, m, dev, reg_limit=reg_limit, **kw)
    rng = np.random.RandomState(4)
    free = inference.detect_cells(images, m, dev, **kw)
    assert sum(len(c[0]) for c in free) > 0
    # annotations (x, y): the unlimited detections moved a little, and two far points
    pts_xy = [np.concatenate([c[0][:, ::-1] + rng.randint(-5, 6, size=c[0].shape), [[1000, 1000], [2000, 5]]]) for c in free]
    masks = (rng.rand(2, 299, 299) > 0.5).astype(np.uint8) * 255
    loader = [(images[0], torch.from_numpy(masks[:1]), [pts_xy[0]], ["breast"], ["regular"]),
              (images[1], torch.from_numpy(masks[1:]), torch.from_numpy(pts_xy[1])[None], ["colon"], ["clustered"])]
    out = inference.evaluate_detection(loader, m, dev, threshold=thr, reg_limit=reg_limit, **kw)
    assert m.mode == "segment"
    assert sorted(out) == sorted(["count", "tp", "fp", "fn", "p", "r", "f1", "dice", "mean"])
    m.setmode("image")
    with torch.no_grad():
        reg = np.concatenate([np.round(m(b.to(dev))[1][:, 0].float().cpu().numpy()).astype(int) for b in images])
    m.setmode("segment")
    assert np.array_equal(out["count"], reg)
    for i in range(2):
        tp, fp, fn, _ = R.score(cells[i][0], pts_xy[i][:, ::-1])
        assert (out["tp"][i], out["fp"][i], out["fn"][i]) == (tp, fp, fn), i
        assert np.asarray([out["p"][i], out["r"][i], out["f1"][i]]).tobytes() == R.prf(tp, fp, fn).tobytes()
    classes = inference.segment_classes(images, m, dev, thr, reg_limit=reg_limit)
    dice = metrics.dice_coef(classes.float(), torch.from_numpy(masks).to(dev).float() / 255).cpu().numpy()
    assert np.array_equal(out["dice"], dice.astype(np.float64)) and out["dice"].dtype == np.float64
    assert out["mean"] == tuple(float(out[k].mean()) for k in ("p", "r", "f1", "dice"))
    if not reg_limit:
        assert out["tp"].sum() > 0


class _CountingModel:
    """the model with its forwards counted and its setmode arguments recorded; everything else is the model's own"""

    def __init__(self, model):
        self.model, self.calls, self.modes = model, 0, []

    def __call__(self, x):
        self.calls += 1
        return self.model(x)

    def setmode(self, mode):
        self.modes.append(mode)
        self.model.setmode(mode)

    def __getattr__(self, name):
        return getattr(self.model, name)


def test_drivers_forwards_per_batch_and_final_mode(dev):
    """every driver of inference.py makes the forward passes per batch that it always made -- one in segment mode, and a second in
    image mode exactly where the count is used -- and leaves the model in segment mode and eval()"""
    from cellsegmentation_amd import inference, synth
    from cellsegmentation_amd.model import resnet as RN
    m = RN.MILresnet18()
    sd = m.state_dict()
    synth.fill_state_dict(sd)
    m.load_state_dict(sd)
    m = m.to(dev).set_compute_dtype(torch.float32)
    x = synth.normalise(synth.ihc_tiles(4, 299, seed=23))
    images = [x[:2], x[2:]]
    rng = np.random.RandomState(6)
    masks = torch.from_numpy((rng.rand(4, 299, 299) > 0.5).astype(np.uint8) * 255)
    points = [rng.randint(0, 299, size=(3, 2)) for _ in range(4)]
    with_masks = [(images[b], masks[2 * b:2 * b + 2]) for b in range(2)]
    with_points = [(images[b], masks[2 * b:2 * b + 2], points[2 * b:2 * b + 2]) for b in range(2)]
    slide = np.ascontiguousarray(synth.ihc_tiles(1, 299, seed=24)[0, :150, :170])
    slide_batches = 3                                                      # 12 patches of 64 every 48 pixels, 5 at a time
    drivers = [
        ("detect_cells", lambda c, lim: inference.detect_cells(images, c, dev, reg_limit=lim), 2, (1, 2)),
        ("segment_classes", lambda c, lim: inference.segment_classes(images, c, dev, 0.5, reg_limit=lim), 2, (1, 2)),
        ("evaluate_instances", lambda c, lim: inference.evaluate_instances(with_masks, c, dev, reg_limit=lim), 2, (1, 2)),
        ("evaluate_detection", lambda c, lim: inference.evaluate_detection(with_points, c, dev, reg_limit=lim), 2, (2, 2)),
        ("detect_slide", lambda c, lim: inference.detect_slide(slide, c, dev, batch_size=5, patch_size=64, interval=48, reg_limit=lim),
         slide_batches, (2, 2)),
    ]
    for name, run, batches, forwards in drivers:
        for lim in (False, True):
            m.setmode("segment")
            m.train()
            c = _CountingModel(m)
            run(c, lim)
            print(f"{name} reg_limit={lim}: {c.calls} forwards over {batches} batches, setmode {c.modes}")
            assert c.calls == forwards[lim] * batches, (name, lim)
            assert m.mode == "segment" and not m.training, (name, lim)
            assert c.modes.count("image") == (forwards[lim] - 1) * batches, (name, lim)
            assert not c.modes or c.modes[-1] == "segment", (name, lim)
