"""The segmentation decoder's data-movement kernels (csrc/resize.hip: bilinear_fwd / bilinear_bwd / concat / split), each directly
against the plain fp64 reference of tests/decoder_ref.py (itself checked on the CPU by test_decoder_ref_host.py).

Inputs are drawn in the compute dtype and widened, so for bf16 the only bf16 error is the final rounding.  Every tolerance is derived
from the number of fp32 roundings the kernel performs and is scaled by the same operator applied to the magnitudes; none of them was
tuned against the kernel's output.  Measured worst error / bound (MI355X): see DESIGN.md section 4."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import decoder_ref as R  # noqa: E402
from cellsegmentation_amd import kernels as K  # noqa: E402

DTYPES = [torch.float32, torch.bfloat16]

# The decoder of cellsegmentation_amd/model/resnet.py at 299 x 299 (encoder outputs 10, 19, 38, 75; conv1 output 150):
#   up(X4) 10->19 at 512 e channels, up 19->38 at 256 e (upconv2), 38->75 at 128 e (upconv4), 75->150 at 64 e (upconv6),
#   150->299 at 64 (upconv8); e = 1 for ResNet-18, 4 for ResNet-50.
#   cat(upconv1, X3) 256 e + 256 e at 19, cat(upconv3, X2) 128 e + 128 e at 38, cat(upconv5, X1) 64 e + 64 e at 75.
MODEL_UPS = [(10, 19, 512), (19, 38, 256), (38, 75, 128), (75, 150, 64), (150, 299, 64),          # ResNet-18
             (10, 19, 2048), (19, 38, 1024), (38, 75, 512), (75, 150, 256)]                         # ResNet-50 (150->299 is shared)
MODEL_CATS = [(19, 256), (38, 128), (75, 64), (19, 1024), (38, 512), (75, 256)]

# (N, (H, W), (P, Q), C)
SHAPES = ([(2, (a, a), (b, b), c) for a, b, c in MODEL_UPS]
          + [(2, (1, 1), (7, 7), 8), (2, (7, 7), (1, 1), 8), (2, (5, 5), (5, 5), 8), (2, (9, 9), (4, 4), 8),
             (2, (3, 11), (8, 5), 8), (2, (8, 5), (3, 11), 8), (1, (1, 6), (5, 1), 16), (3, (13, 7), (13, 20), 24)]
          # above the 16384 x 256 = 4.19 M grid cap, where the stride loop runs a second lap: 8 * 299 * 299 * 8 = 5.7 M groups in the
          # forward of the first (its backward has 1.44 M), and in the backward of the second (a downsample with an inexact scale, 298 / 139)
          + [(8, (150, 150), (299, 299), 64), (8, (299, 299), (140, 140), 64)])
SHAPE_IDS = [f"n{n}-{a[0]}x{a[1]}-{b[0]}x{b[1]}-c{c}" for n, a, b, c in SHAPES]


def _draw(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float32).to(dtype)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _check(got, ref, bound, what):
    err = (got - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"{what}: worst err/bound {ratio:.3f}, worst abs err {float(err.max()):.3e}")
    bad = err > bound
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements over the bound, worst err/bound {ratio:.3f}"
    return ratio


# ---------------------------------------------------------------------------------------------------------------- bilinear forward
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_bilinear_fwd(shape, dtype, dev):
    """|got - ref| <= 4 * 2^-24 * fwd_ref(|x|) (+ 2^-8 |ref| for the bf16 store).  The kernel evaluates
    wy0 (wx0 a + wx1 b) + wy1 (wx0 c + wx1 d): each of the four terms passes through a product, a sum, a product and a sum
    (fewer where the compiler contracts to FMA), four roundings of relative size 2^-24 on a quantity bounded by the same expression
    on |x|.  The weights themselves are the reference's, bit for bit."""
    N, in_hw, out_hw, C = shape
    x = _draw((N, in_hw[0], in_hw[1], C), dtype, 100 + C + in_hw[0])
    y = K.bilinear_fwd(x.to(dev), out_hw)
    torch.cuda.synchronize()
    assert y.shape == (N, out_hw[0], out_hw[1], C) and y.dtype == dtype
    xd = x.double()
    ref = R.bilinear_fwd_ref(xd, out_hw)
    bound = 4 * R.U32 * R.bilinear_fwd_mag(xd, out_hw)
    if dtype == torch.bfloat16:
        bound = bound + R.U16 * ref.abs()
    _check(y.cpu().double(), ref, bound, f"bilinear_fwd {SHAPE_IDS[SHAPES.index(shape)]} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_bilinear_fwd_exact_cases(dtype, dev):
    # same size: every lambda is 0, the output is the input bit for bit
    for hw in [(5, 5), (1, 1), (13, 7), (75, 75)]:
        x = _draw((2, hw[0], hw[1], 16), dtype, 7).to(dev)
        y = K.bilinear_fwd(x, hw)
        assert torch.equal(_bits(y), _bits(x)), hw
    # 3 -> 5: the scale is exactly 0.5, odd rows / columns are midpoints of small integers: exact in fp32 and in bf16
    g = torch.Generator().manual_seed(8)
    x = torch.randint(-8, 9, (2, 3, 3, 8), generator=g).to(dtype)
    y = K.bilinear_fwd(x.to(dev), (5, 5))
    ref = R.bilinear_fwd_ref(x.double(), (5, 5))
    assert torch.equal(ref.to(dtype).double(), ref)            # representable: the rounding of the reference is the identity
    assert torch.equal(_bits(y.cpu()), _bits(ref.to(dtype)))
    assert torch.equal(y[:, 1, 1].cpu().double(), x.double()[:, :2, :2].mean(dim=(1, 2)))


# ---------------------------------------------------------------------------------------------------------------- bilinear backward
def _bwd_bound(dyd, in_hw, out_hw, dtype, ref, mask=None):
    """(n_terms + 3) * 2^-24 * bwd_ref(|dy|): the kernel forms w = wy wx (one rounding; wy or wx may itself be the rounded sum
    w0 + w1 where both taps of an output land on the last pixel: one more), multiplies by dy (one) and adds the term to a running
    fp32 sum of at most n_terms terms (n_terms roundings on the path of the first)."""
    n_terms = R.bilinear_bwd_terms(in_hw, out_hw)
    bound = (n_terms + 3) * R.U32 * R.bilinear_bwd_mag(dyd, in_hw, mask)
    if dtype == torch.bfloat16:
        bound = bound + R.U16 * ref.abs()
    return bound


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_bilinear_bwd(shape, dtype, dev):
    """dx against the exact transpose of the forward (the scatter over the forward's own fp32 taps), elementwise within _bwd_bound.
    A backward weight that differs from the forward's by an ulp of the source coordinate (inexact scales: 19->38, 75->150) is many
    times the bound."""
    N, in_hw, out_hw, C = shape
    dy = _draw((N, out_hw[0], out_hw[1], C), dtype, 200 + C + in_hw[0])
    dx = K.bilinear_bwd(dy.to(dev), in_hw)
    torch.cuda.synchronize()
    assert dx.shape == (N, in_hw[0], in_hw[1], C) and dx.dtype == dtype
    dyd = dy.double()
    ref = R.bilinear_bwd_ref(dyd, in_hw)
    _check(dx.cpu().double(), ref, _bwd_bound(dyd, in_hw, out_hw, dtype, ref), f"bilinear_bwd {SHAPE_IDS[SHAPES.index(shape)]} {dtype}")


def test_bilinear_bwd_window_sweep(dev):
    """Every (H, P) with H in 1..20 and P in 1..40 (square), and a dozen seeded non-square (H, W, P, Q), at N = 1, C = 8, fp32.  The
    backward kernel gathers over a window of output rows / columns computed from the inverse scale; the forward taps come from another
    formula.  A window that drops one contributing output pixel loses a whole term (not a rounding), which the elementwise bound and
    the adjoint identity <fwd(x), dy> == <x, bwd(dy)> both see.  All inputs travel in one upload, all results come back in one."""
    rng = np.random.RandomState(5)
    cases = [((h, h), (p, p)) for h in range(1, 21) for p in range(1, 41)]
    for _ in range(12):
        h, w, p, q = (int(v) for v in (rng.randint(1, 21), rng.randint(1, 21), rng.randint(1, 41), rng.randint(1, 41)))
        cases.append(((h, w), (p, q)))
    C = 8
    g = torch.Generator().manual_seed(6)
    xs = [torch.randn(1, a[0], a[1], C, generator=g) for a, _ in cases]
    dys = [torch.randn(1, b[0], b[1], C, generator=g) for _, b in cases]
    flat = torch.cat([t.reshape(-1) for t in xs + dys]).to(dev)        # every piece is a multiple of 8 floats: 32-byte aligned views
    views, off = [], 0
    for t in xs + dys:
        views.append(flat[off:off + t.numel()].view(t.shape))
        off += t.numel()
    xv, dyv = views[:len(cases)], views[len(cases):]
    ys = [K.bilinear_fwd(xv[i], cases[i][1]) for i in range(len(cases))]
    dxs = [K.bilinear_bwd(dyv[i], cases[i][0]) for i in range(len(cases))]
    out = torch.cat([t.reshape(-1) for t in ys + dxs]).cpu().double()  # the one synchronise
    off, worst, fails = 0, [0.0, 0.0, 0.0], []
    got_y, got_dx = [], []
    for t in dys:
        got_y.append(out[off:off + t.numel()].view(t.shape))
        off += t.numel()
    for t in xs:
        got_dx.append(out[off:off + t.numel()].view(t.shape))
        off += t.numel()
    for i, (in_hw, out_hw) in enumerate(cases):
        xd, dyd = xs[i].double(), dys[i].double()
        fb = 4 * R.U32 * R.bilinear_fwd_mag(xd, out_hw)
        bb = (R.bilinear_bwd_terms(in_hw, out_hw) + 3) * R.U32 * R.bilinear_bwd_mag(dyd, in_hw)
        ef = (got_y[i] - R.bilinear_fwd_ref(xd, out_hw)).abs()
        eb = (got_dx[i] - R.bilinear_bwd_ref(dyd, in_hw)).abs()
        adj = abs(float((got_y[i] * dyd).sum()) - float((xd * got_dx[i]).sum()))
        adj_bound = float((fb * dyd.abs()).sum()) + float((xd.abs() * bb).sum())
        worst = [max(worst[0], float((ef / fb.clamp_min(1e-300)).max())), max(worst[1], float((eb / bb.clamp_min(1e-300)).max())),
                 max(worst[2], adj / max(adj_bound, 1e-300))]
        if bool((ef > fb).any()) or bool((eb > bb).any()) or adj > adj_bound:
            fails.append((in_hw, out_hw, float((ef / fb.clamp_min(1e-300)).max()), float((eb / bb.clamp_min(1e-300)).max()),
                          adj / max(adj_bound, 1e-300)))
    print(f"window sweep over {len(cases)} sizes: worst err/bound fwd {worst[0]:.3f} bwd {worst[1]:.3f} adjoint {worst[2]:.3f}")
    assert not fails, f"{len(fails)} of {len(cases)} sizes over a bound (in, out, fwd, bwd, adjoint ratio): {fails[:8]}"


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_bilinear_bwd_mask(dtype, dev):
    """The fused ReLU mask: dx = where(mask > 0, unmasked dx, +0.0), bit for bit; negative values and -0.0 mask out."""
    for in_hw, out_hw, C in [((10, 10), (19, 19), 16), ((6, 9), (4, 14), 8)]:
        dy = _draw((2, out_hw[0], out_hw[1], C), dtype, 31).to(dev)
        mask = torch.relu(_draw((2, in_hw[0], in_hw[1], C), dtype, 32))              # exact zeros like a stored ReLU output
        flat = mask.view(-1)
        flat[1::7] = -0.0
        flat[2::11] = -1.5
        flat[3] = 0.0
        assert int((mask == 0).sum()) > 100 and bool((mask < 0).any()) and bool((mask > 0).any())
        plain = K.bilinear_bwd(dy, in_hw)
        masked = K.bilinear_bwd(dy, in_hw, mask=mask.to(dev))
        torch.cuda.synchronize()
        want = torch.where(mask.to(dev) > 0, plain, torch.zeros_like(plain))
        assert torch.equal(_bits(masked), _bits(want))
        assert not bool((_bits(masked)[mask.to(dev) <= 0] != 0).any())              # +0.0, not -0.0
        ref = R.bilinear_bwd_ref(dy.cpu().double(), in_hw, mask.double())
        _check(masked.cpu().double(), ref, _bwd_bound(dy.cpu().double(), in_hw, out_hw, dtype, ref, mask.double()),
               f"bilinear_bwd masked {in_hw}->{out_hw} {dtype}")


@pytest.mark.parametrize("size", [(a, b) for a, b, _ in MODEL_UPS[:5]], ids=lambda s: f"{s[0]}-{s[1]}")
def test_bilinear_bwd_of_ones_sums_to_output_size(size, dev):
    """The weights into every output pixel sum to 1, so the backward of an all-ones gradient, summed over the input plane, is P * Q
    per channel -- within the elementwise fp32 bound summed over the plane, (n_terms + 3) 2^-24 P Q (the reference's bwd(|1|) sums to
    P Q too), plus 2^-24 P Q for the weight pairs that sum to 1 only to half an ulp."""
    H, P = size
    C = 8
    dx = K.bilinear_bwd(torch.ones(2, P, P, C, device=dev), (H, H))
    total = dx.cpu().double().sum(dim=(1, 2))
    bound = (R.bilinear_bwd_terms((H, H), (P, P)) + 3 + 1) * R.U32 * P * P
    print(f"bwd(ones) {H}->{P}: worst |sum - PQ| / bound {float((total - P * P).abs().max()) / bound:.3f}")
    assert float((total - P * P).abs().max()) <= bound


# ---------------------------------------------------------------------------------------------------------------- concat / split
def _payload(shape, dtype, seed):
    """random BIT patterns (NaNs with payloads, infinities, denormals, both zeros among them): the kernels must be pure moves"""
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.float32:
        t = torch.randint(-2 ** 31, 2 ** 31, shape, generator=g, dtype=torch.int64).to(torch.int32).view(torch.float32)
    else:
        t = torch.randint(-2 ** 15, 2 ** 15, shape, generator=g, dtype=torch.int64).to(torch.int16).view(torch.bfloat16)
    flat = t.view(-1)
    flat[0], flat[-1] = float("nan"), -0.0
    return t


CAT_CASES = ([((3, 5, 7), ca, cb) for ca, cb in [(8, 8), (8, 2040), (2040, 8), (64, 64), (512, 256)]]
             + [((2, s, s), c, c) for s, c in MODEL_CATS]
             + [((37,), 8, 16), ((1,), 8, 8), ((1,), 24, 8), ((1, 1, 1), 16, 8),
                ((270000,), 64, 64)])               # 270000 * 16 = 4.32 M groups: above the 16384 x 256 grid cap
CAT_IDS = ["x".join(str(v) for v in lead) + f"-{ca}+{cb}" for lead, ca, cb in CAT_CASES]


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", CAT_CASES, ids=CAT_IDS)
def test_concat_split_are_pure_moves(case, dtype, dev):
    lead, Ca, Cb = case
    a, b = _payload(lead + (Ca,), dtype, 41), _payload(lead + (Cb,), dtype, 42)
    ad, bd = a.to(dev), b.to(dev)
    whole = K.concat(ad, bd)
    want = torch.cat([_bits(a), _bits(b)], dim=-1)
    assert whole.shape == lead + (Ca + Cb,) and whole.dtype == dtype
    assert torch.equal(_bits(whole).cpu(), want)
    # split of an independent tensor, each side alone and both together
    w = _payload(lead + (Ca + Cb,), dtype, 43)
    wd = w.to(dev)
    wa, wb = _bits(w)[..., :Ca], _bits(w)[..., Ca:]
    sa, sb = K.split(wd, Ca)
    assert torch.equal(_bits(sa).cpu(), wa) and torch.equal(_bits(sb).cpu(), wb)
    sa, none_b = K.split(wd, Ca, want_b=False)
    assert none_b is None and torch.equal(_bits(sa).cpu(), wa)
    none_a, sb = K.split(wd, Ca, want_a=False)
    assert none_a is None and torch.equal(_bits(sb).cpu(), wb)
    assert torch.equal(_bits(wd).cpu(), _bits(w))              # the source of a split is left alone
    # round trip
    ra, rb = K.split(whole, Ca)
    assert torch.equal(_bits(ra).cpu(), _bits(a)) and torch.equal(_bits(rb).cpu(), _bits(b))
    assert torch.equal(_bits(K.concat(*K.split(wd, Ca))).cpu(), _bits(w))


# ---------------------------------------------------------------------------------------------------------------- argument checks
def test_argument_checks_raise_and_launch_nothing(dev):
    x12 = torch.zeros(1, 4, 4, 12, device=dev)
    with pytest.raises(RuntimeError, match="bad arguments"):
        K.bilinear_fwd(x12, (8, 8))
    with pytest.raises(RuntimeError, match="bad arguments"):
        K.bilinear_bwd(x12, (2, 2))
    with pytest.raises(RuntimeError, match="bad arguments"):
        K.concat(x12, torch.zeros(1, 4, 4, 8, device=dev))
    with pytest.raises(RuntimeError, match="bad arguments"):
        K.split(torch.zeros(1, 4, 4, 16, device=dev), 12)
    h = torch.zeros(1, 4, 4, 8, device=dev, dtype=torch.float16)
    for call in (lambda: K.bilinear_fwd(h, (8, 8)), lambda: K.bilinear_bwd(h, (2, 2)), lambda: K.concat(h, h), lambda: K.split(h, 8)):
        with pytest.raises(TypeError, match="unsupported activation dtype"):
            call()
    torch.cuda.synchronize()
