"""GPU: the augmented input staging (csrc/augment.hip through cellsegmentation_amd/augment.py) against the numpy restatement
(tests/augment_ref.py) and against tiles.gather_tiles.

Inputs: 3 random uint8 images of 20x24 (one with grey, all-0 and all-255 rows) and one of 67x61.  Tiles of 5 and 8 on the get_tiles
grid (border-aligned last row and column included), 40x40 tiles of the 67x61 image (1600 pixels: the contrast mean spans 4
reduction workgroups) and whole images (20x24, and 67x61 = 4087 pixels: 8 workgroups).

Bounds.  Without jitter the arithmetic is tile_gather_kernel's: bit for bit.  With jitter the fp32 output must be within 2e-5 absolute
of the restatement on the normalised output, every element compared: the fp32 restatement differs from the same code in fp64 by at
most 6.3e-6 (40 random 24x24 images x 24 orders, grey / black / white rows included), two fp32 evaluations that differ in FMA
contraction can each be that far from the exact value (1.3e-5), about 1.5x margin gives 2e-5.  The kernels compile the colour arithmetic
with contraction off, and each test prints the deviation it saw before it asserts."""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import augment_ref as R  # noqa: E402
from cellsegmentation_amd import augment as A  # noqa: E402
from cellsegmentation_amd import kernels as K  # noqa: E402
from cellsegmentation_amd import synth, tiles  # noqa: E402

F = np.float32
JITTER_ATOL = 2e-5


def _records():
    """the jitter records every case runs: all 24 orders with factors from the Maskset ranges, records of 1, 2 and 3 ops in varying
    slots, and the extreme factors"""
    rng = np.random.RandomState(7)
    lo_hi = {0: (0.9, 1.1), 1: (0.7, 1.3), 2: (0.6, 1.4), 3: (-0.05, 0.05)}
    recs = []
    for perm in itertools.permutations(range(4)):
        recs.append([(op, rng.uniform(*lo_hi[op])) for op in perm])
    for k in (1, 2, 3):
        for ops in itertools.combinations(range(4), k):
            ops = list(rng.permutation(ops))
            slots = sorted(rng.permutation(4)[:k].tolist())
            rec = [(-1, 0.0)] * 4
            for s, op in zip(slots, ops):
                rec[s] = (int(op), rng.uniform(*lo_hi[int(op)]))
            recs.append(rec)
    for ex in ([(0, 0.0)], [(0, 2.0)], [(1, 0.0)], [(2, 0.0)], [(2, 3.0)], [(3, 0.5)], [(3, -0.5)], [(3, 0.5), (1, 0.0)],
               [(2, 3.0), (0, 2.0), (3, -0.5), (1, 0.7)], [(0, 0.0), (1, 1.3), (3, 0.5)]):
        recs.append(list(ex) + [(-1, 0.0)] * (4 - len(ex)))
    order = np.asarray([[c for c, _ in r] for r in recs], np.int8)
    factors = np.asarray([[f for _, f in r] for r in recs], F)
    assert len({tuple(r) for r in order[:24].tolist()}) == 24 and {int((r >= 0).sum()) for r in order[24:38]} == {1, 2, 3}
    return order, factors


ORDER, FACTORS = _records()
SMALL, BIG = R.make_images()


def _grid(images, interval, size):
    ti, rc = tiles.tile_index(len(images), images.shape[1:3], interval, size)
    reps = -(-len(ORDER) // len(ti))                                      # every case runs every record
    return np.tile(ti, reps), np.tile(rc, (reps, 1))


def _whole(images):
    idx = np.arange(len(images))
    return np.tile(idx, -(-len(ORDER) // len(idx))), None


# name -> (images, tile_img, tile_rc or None for whole images, th, tw)
CASES = {
    "tiles5": (SMALL,) + _grid(SMALL, 4, 5) + (5, 5),
    "tiles8": (SMALL,) + _grid(SMALL, 6, 8) + (8, 8),
    "whole20x24": (SMALL,) + _whole(SMALL) + (20, 24),
    "tiles40": (BIG,) + _grid(BIG, 9, 40) + (40, 40),
    "whole67x61": (BIG,) + _whole(BIG) + (67, 61),
}
_REF = {}


def _plan(name, flips, jitter):
    """-> (flip codes or None, (order, factors) or None) of a case: all four codes mixed, record t + 1 on tile t"""
    T = len(CASES[name][1])
    fl = ((np.arange(T) * 7 + 1) // 3 % 4).astype(np.int8) if flips else None
    pick = (np.arange(T) + 1) % len(ORDER)
    return fl, ((ORDER[pick], FACTORS[pick]) if jitter else None)


def _want(name, flips, jitter):
    """the restatement of a case, computed once and left unchanged"""
    key = (name, flips, jitter)
    if key not in _REF:
        images, ti, rc, th, tw = CASES[name]
        fl, jt = _plan(name, flips, jitter)
        rc = np.zeros((len(ti), 2), np.int64) if rc is None else rc
        _REF[key] = R.stage_tiles(images, ti, rc, th, tw, fl, jt)
        _REF[key].setflags(write=False)
    return _REF[key]


def _got(name, flips, jitter, dtype, dev):
    images, ti, rc, th, tw = CASES[name]
    fl, jt = _plan(name, flips, jitter)
    d = torch.from_numpy(images).to(dev)
    if rc is None:
        return A.stage_images(d, fl, jt, ti, dtype)
    return A.stage_tiles(d, ti, rc, th, fl, jt, dtype)


def _bits(t):
    return t.cpu().view(torch.int16).numpy().view(np.uint16) if t.dtype == torch.bfloat16 else t.cpu().numpy().view(np.uint32)


def test_the_grids_hold_the_border_aligned_tiles():
    assert tiles.get_tiles((20, 24), 4, 5)[-1] == (15, 19) and (12, 16) in tiles.get_tiles((20, 24), 4, 5)
    assert tiles.get_tiles((20, 24), 6, 8)[-1] == (12, 16) and tiles.get_tiles((67, 61), 9, 40)[-1] == (27, 21)
    assert all(len(c[1]) >= len(ORDER) for c in CASES.values())
    assert (SMALL[1, 2:5, :, 0] == SMALL[1, 2:5, :, 2]).all() and not SMALL[1, 7:9].any() and (SMALL[1, 11:13] == 255).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", list(CASES))
def test_no_augmentation_is_gather_tiles_bit_for_bit(name, dtype, dev):
    images, ti, rc, th, tw = CASES[name]
    got = _got(name, False, False, dtype, dev)
    assert got.shape == (len(ti), th, tw, 8) and got.dtype == dtype
    want = _want(name, False, False)
    if rc is not None:                                                    # gather_tiles cuts square tiles only
        old = tiles.gather_tiles(torch.from_numpy(images).to(dev), ti, rc, th, dtype)
        assert torch.equal(got, old)
        zeros = A.stage_tiles(torch.from_numpy(images).to(dev), ti, rc, th, np.zeros(len(ti), np.int8), None, dtype)
        assert torch.equal(zeros, old)                                    # flip code 0 given explicitly
    assert np.array_equal(_bits(got), want.view(np.uint32) if dtype == torch.float32 else R.to_bf16_bits(want))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", list(CASES))
def test_flips_equal_the_restatement_bit_for_bit(name, dtype, dev):
    fl, _ = _plan(name, True, False)
    assert set(fl.tolist()) == {0, 1, 2, 3}
    got = _got(name, True, False, dtype, dev)
    want = _want(name, True, False)
    assert np.array_equal(_bits(got), want.view(np.uint32) if dtype == torch.float32 else R.to_bf16_bits(want))
    assert not np.array_equal(want, _want(name, False, False))


@pytest.mark.parametrize("flips", [False, True])
@pytest.mark.parametrize("name", list(CASES))
def test_jitter_fp32_is_within_2e_5_of_the_restatement(name, flips, dev):
    got = _got(name, flips, True, torch.float32, dev).cpu().numpy()
    want = _want(name, flips, True)
    assert got.shape == want.shape and np.isfinite(got).all()
    dev_abs = np.abs(got.astype(np.float64) - want.astype(np.float64))
    print(f"{name} flips={flips}: max |gpu - restatement| = {dev_abs.max():.3e}, "
          f"{int((got.view(np.uint32) != want.view(np.uint32)).sum())} of {got.size} elements differ in bits")
    assert dev_abs.max() <= JITTER_ATOL                                   # every element, padding channels included
    assert not got[..., 3:].any()
    assert np.abs(want - _want(name, flips, False)).max() > 0.1           # the records do change the pixels


@pytest.mark.parametrize("name", list(CASES))
def test_bf16_is_the_rounded_fp32_output(name, dev):
    for flips, jitter in ((True, True), (False, True)):
        a = _got(name, flips, jitter, torch.float32, dev)
        b = _got(name, flips, jitter, torch.bfloat16, dev)
        assert b.dtype == torch.bfloat16 and torch.equal(a.to(torch.bfloat16), b)


def test_two_calls_and_a_graph_replay_give_the_same_bits(dev):
    for name in ("tiles40", "whole67x61", "tiles5"):
        a, b = _got(name, True, True, torch.float32, dev), _got(name, True, True, torch.float32, dev)
        assert torch.equal(a, b)
    # the raw call with device operands, captured: memset + mean reduction + apply, one chain
    images, ti, rc, th, tw = CASES["tiles40"]
    fl, (order, factors) = _plan("tiles40", True, True)
    ops = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (images, ti.astype(np.int32), rc.astype(np.int32), fl, order, factors)]
    static = [torch.zeros_like(o) for o in ops]
    static[0].copy_(ops[0])                                               # tile origins stay zero: inside any image
    T = len(ti)
    for dtype in (torch.float32, torch.bfloat16):
        out = torch.empty((T, th, tw, 8), dtype=dtype, device=dev)
        ws = K.stage_augmented_workspace(T, dev)

        def run():
            return K.stage_augmented(static[0], static[1], static[2], th, tw, static[3], static[4], static[5], True, dtype, out=out, ws=ws)
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            run()                                                         # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(stream)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            run()
        for s, o in zip(static, ops):
            s.copy_(o)
        eager = K.stage_augmented(*ops[:3], th, tw, *ops[3:], True, dtype)
        for _ in range(2):                                                # the second replay starts from a used workspace
            out.zero_()
            graph.replay()
            assert torch.equal(out, eager)
        assert torch.equal(eager, _got("tiles40", True, True, dtype, dev))


def test_tile_train_batches(dev):
    d = torch.from_numpy(SMALL).to(dev)
    ti, rc = tiles.tile_index(3, (20, 24), 6, 8)
    rng = np.random.RandomState(3)
    pick = rng.permutation(len(ti))[:22]
    labels = rng.randint(0, 2, 22)
    rows = np.concatenate([ti[pick, None], rc[pick], labels[:, None]], axis=1)
    transform_idx = [A.FLIP_V, A.FLIP_NONE, A.FLIP_HV]
    it = A.TileTrainBatches(d, rows, transform_idx, 8, 8, torch.float32)
    assert len(it) == 3 and it.batch_size == 8
    want = R.stage_tiles(SMALL, ti[pick], rc[pick], 8, 8, [transform_idx[i] for i in ti[pick]])
    for epoch in range(2):
        batches = list(it)
        assert [tuple(x.shape) for x, _ in batches] == [(8, 8, 8, 8), (8, 8, 8, 8), (6, 8, 8, 8)]
        assert np.array_equal(torch.cat([x for x, _ in batches]).cpu().numpy().view(np.uint32), want.view(np.uint32))
        lab = torch.cat([y for _, y in batches])
        assert lab.dtype == torch.int64 and lab.cpu().tolist() == labels.tolist()
    # the reference's own row format, no flips, bf16 by default
    as_tuples = [(int(r[0]), (int(r[1]), int(r[2])), int(r[3])) for r in rows]
    it2 = A.TileTrainBatches(d, as_tuples, None, 8, 22)
    (x, y), = list(it2)
    assert len(it2) == 1 and x.dtype == torch.bfloat16 and torch.equal(x, tiles.gather_tiles(d, ti[pick], rc[pick], 8))
    assert y.cpu().tolist() == labels.tolist()


def test_mask_train_batches(dev):
    d = torch.from_numpy(SMALL).to(dev)
    masks = torch.arange(3 * 20 * 24, dtype=torch.uint8).reshape(3, 20, 24)
    labels = torch.tensor([4, 0, 17])
    plain = A.MaskTrainBatches(d, masks, labels, 2, dtype=torch.float32)
    assert len(plain) == 2 and plain.batch_size == 2
    got = list(plain)
    assert [tuple(x.shape) for x, _, _ in got] == [(2, 20, 24, 8), (1, 20, 24, 8)]
    assert torch.equal(torch.cat([x for x, _, _ in got]), A.stage_images(d, dtype=torch.float32))
    assert torch.equal(torch.cat([m for _, m, _ in got]), masks) and torch.equal(torch.cat([y for _, _, y in got]), labels)
    # augment + shuffle with a seeded generator: the same draws by hand
    it = A.MaskTrainBatches(d, masks.to(dev), labels, 2, augment=True, shuffle=True, generator=torch.Generator().manual_seed(9),
                            dtype=torch.float32)
    g = torch.Generator().manual_seed(9)
    seen = []
    for epoch in range(2):
        perm = torch.randperm(3, generator=g)
        batches = list(it)
        assert len(batches) == 2
        for b, (x, m, y) in enumerate(batches):
            idx = perm[2 * b:2 * b + 2]
            jt = A.draw_color_jitter(len(idx), generator=g)
            assert torch.equal(x, A.stage_images(d, None, jt, idx, torch.float32))
            assert m.is_cuda and torch.equal(m.cpu(), masks[idx]) and torch.equal(y, labels[idx])
            want = R.stage_images(SMALL, None, jt, idx.numpy())
            assert np.abs(x.cpu().numpy() - want).max() <= JITTER_ATOL
        seen.append(torch.cat([x for x, _, _ in batches]))
    assert not torch.equal(seen[0], seen[1])                              # fresh records every epoch


def _resnet18(mode, dtype, dev):
    from cellsegmentation_amd.model import resnet
    m = resnet.MILresnet18()
    sd = m.state_dict()
    synth.fill_state_dict(sd)
    m.load_state_dict(sd)
    m = m.to(dev).set_compute_dtype(dtype)
    m.setmode(mode)
    m.eval()
    return m


def test_resnet18_forward_on_staged_augmented_batches(dev):
    """a tile-mode and a segment-mode forward on a staged augmented batch equal the forward on the same pixels prepared by the
    restatement and uploaded as NHWC-8"""
    imgs = synth.ihc_tiles(2, 64, 5)
    d = torch.from_numpy(imgs).to(dev)
    jt = (ORDER[:16], FACTORS[:16])
    # tile mode, fp32: 16 tiles of 32x32, flipped and jittered
    ti, rc = tiles.tile_index(2, (64, 64), 16, 32)
    ti, rc = ti[1:17], rc[1:17]
    fl = (np.arange(16) % 4).astype(np.int8)
    staged = A.stage_tiles(d, ti, rc, 32, fl, jt, torch.float32)
    want = torch.from_numpy(R.stage_tiles(imgs, ti, rc, 32, 32, fl, jt)).to(dev)
    print(f"tile batch: max |staged - restatement| = {float((staged - want).abs().max()):.3e}")
    m = _resnet18("tile", torch.float32, dev)
    with torch.no_grad():
        a, b = m(staged), m(want)
    assert a.shape == (16, 2) and torch.equal(a, b)
    # segment mode, bf16: 2 whole images of 64x64, jittered
    jt2 = (ORDER[[5, 44]], FACTORS[[5, 44]])
    staged = A.stage_images(d, [A.FLIP_H, A.FLIP_V], jt2, dtype=torch.bfloat16)
    want = torch.from_numpy(R.stage_images(imgs, [A.FLIP_H, A.FLIP_V], jt2)).to(dev).to(torch.bfloat16)
    m = _resnet18("segment", torch.bfloat16, dev)
    with torch.no_grad():
        a, b = m(staged), m(want)
    assert a.shape == (2, 2, 64, 64) and torch.isfinite(a).all() and torch.equal(a, b)
