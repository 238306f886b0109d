"""The segmentation loss path's kernels (csrc/head.hip: softmax_channel fwd / bwd, dice sums / loss / bwd), each directly against the
plain fp64 reference of tests/decoder_ref.py, and the public entry points (functional.dice_loss / softmax_channel, train.DiceLoss,
metrics.dice_coef) over the operand dtypes and layouts a caller can hand them.

Inputs are drawn in fp32 (or bf16) and widened, so the reference sees exactly the kernel's operands.  Measured worst errors next to
their bounds (MI355X): see DESIGN.md section 4."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import decoder_ref as R  # noqa: E402
from cellsegmentation_amd import functional as HF  # noqa: E402
from cellsegmentation_amd import kernels as K  # noqa: E402
from cellsegmentation_amd import metrics as M  # noqa: E402
from cellsegmentation_amd import train as T  # noqa: E402

U = R.U32


# ====================================================================================================== softmax over channels
def _softmax_yardstick(logits, g, ch):
    """The tolerance is MEASURED ON THE REFERENCE SIDE (the error of the device expf cannot be derived from this project): ATen's own fp32
    CPU softmax(...)[:, ch] and its fp32 autograd gradient on the same inputs, their largest deviation from the fp64 reference.  The
    kernel gets 4x that (another exp implementation, another summation order over at most 5 channels), floor 8 * 2^-24 so that a
    yardstick of exactly 0 on trivial inputs does not demand bit equality.  Returns ref_p, ref_grad, tol_p, tol_grad, yard_p, yard_grad."""
    ld, gd = logits.double(), g.double()
    ref_p = R.softmax_channel_ref(ld, ch)
    ref_g = R.softmax_channel_grad_ref(ld, gd, ch)
    lg = logits.clone().requires_grad_()
    p32 = torch.softmax(lg, dim=1)[:, ch]
    p32.backward(g)
    yard_p = float((p32.detach().double() - ref_p).abs().max())
    yard_g = float((lg.grad.double() - ref_g).abs().max())
    return ref_p, ref_g, max(4 * yard_p, 8 * U), max(4 * yard_g, 8 * U), yard_p, yard_g


def _softmax_case(logits, g, ch, dev, what):
    N, C, H, W = logits.shape
    ld = logits.to(dev)
    pc = K.softmax_channel_fwd(ld, ch)
    dl = K.softmax_channel_bwd(ld, g.to(dev), ch)
    torch.cuda.synchronize()
    assert pc.shape == (N, H, W) and pc.dtype == torch.float32 and dl.shape == logits.shape and dl.dtype == torch.float32
    ref_p, ref_g, tol_p, tol_g, yard_p, yard_g = _softmax_yardstick(logits, g, ch)
    pc, dl = pc.cpu().double(), dl.cpu().double()
    err_p, err_g = float((pc - ref_p).abs().max()), float((dl - ref_g).abs().max())
    err_s = float(dl.sum(dim=1).abs().max())
    print(f"softmax_channel {what}: fwd err {err_p:.3e} (ATen fp32 {yard_p:.3e}, tol {tol_p:.3e}); "
          f"bwd err {err_g:.3e} (ATen fp32 {yard_g:.3e}, tol {tol_g:.3e}); channel sum {err_s:.3e}")
    assert not bool(torch.isnan(pc).any()) and not bool(torch.isnan(dl).any())
    assert err_p <= tol_p, f"{what}: forward {err_p:.3e} > {tol_p:.3e}"
    assert err_g <= tol_g, f"{what}: gradient {err_g:.3e} > {tol_g:.3e} (every channel of dlogits is compared)"
    # a property of its own, not implied by the line above (C values each within tol_g of a zero-sum set could sum to C * tol_g)
    assert err_s <= tol_g, f"{what}: the channels of dlogits sum to {err_s:.3e} > {tol_g:.3e} at some pixel"
    return pc, dl


def _cch():
    out = []
    for C in (2, 3, 5):
        out += [(C, ch) for ch in sorted({0, C // 2 if C >= 3 else 0, C - 1})]
    return out


@pytest.mark.parametrize("N", [1, 8])
@pytest.mark.parametrize("hw", [(1, 1), (1, 7), (299, 299)], ids=["hw1", "hw7", "hw299x299"])
@pytest.mark.parametrize("C,ch", _cch())
def test_softmax_channel(C, ch, hw, N, dev):
    """Measured over these 48 cases and the two tests below (MI355X): the forward is at most 2.34e-07 from the fp64 reference where the
    yardstick (ATen's fp32 CPU softmax on the same inputs) is at most 2.34e-07 from it; every channel of the gradient at most 5.20e-07
    where ATen's fp32 autograd is at most 6.33e-07.  Case by case the kernel used at most 0.25 (forward) and 0.28 (gradient) of its
    tolerance of 4x the yardstick, i.e. it is about as far from fp64 as ATen's fp32 path is."""
    g = torch.Generator().manual_seed(1000 * C + 10 * ch + N)
    logits = 3 * torch.randn(N, C, hw[0], hw[1], generator=g)
    dpc = torch.randn(N, hw[0], hw[1], generator=g)
    _softmax_case(logits, dpc, ch, dev, f"C{C} ch{ch} N{N} {hw}")


def test_softmax_channel_above_the_block_cap(dev):
    """N * HW = 3 * 1024^2 pixels > 8192 blocks * 256 threads: the stride loop runs a second lap for half the threads"""
    g = torch.Generator().manual_seed(77)
    logits = 3 * torch.randn(3, 2, 1024, 1024, generator=g)
    dpc = torch.randn(3, 1024, 1024, generator=g)
    assert logits.shape[0] * 1024 * 1024 > 8192 * 256
    _softmax_case(logits, dpc, 1, dev, "C2 ch1 N3 1024x1024")


def test_softmax_channel_value_edges(dev):
    g = torch.Generator().manual_seed(78)
    C, W = 3, 64
    logits = torch.randn(1, C, 6, W, generator=g)
    dpc = torch.randn(1, 6, W, generator=g)
    # row 0: a gap of 200 > 104 between channel 0 and the rest: exp of the smaller ones underflows in fp32, p is exactly 1 / 0
    logits[0, 0, 0] += 200.0
    # row 1: all channels equal: p = 1 / C
    logits[0, :, 1] = logits[0, 0, 1]
    # rows 2, 3: a large common offset, which the max subtraction cancels exactly (the operands are fp32 values near 1e4)
    logits[0, :, 2] += 1e4
    logits[0, :, 3] -= 1e4
    # rows 4, 5: -inf in a channel that is neither the maximum nor ch (ch = 0 below; channel 2 is -inf, channel 1 is lifted to the top)
    logits[0, 2, 4:] = float("-inf")
    logits[0, 1, 4:] += 5.0
    pc, dl = _softmax_case(logits, dpc, 0, dev, "value edges ch0")
    assert torch.equal(pc[0, 0], torch.ones(W, dtype=torch.float64))
    assert bool((dl[0, :, 0] == 0).all())                                  # p (1 - p) and p q with p = 1, q = 0
    assert bool((dl[0, 2, 4:] == 0).all())                                 # no gradient into the -inf channel
    pc1, dl1 = _softmax_case(logits, dpc, 1, dev, "value edges ch1")
    assert bool((pc1[0, 0] == 0).all())
    assert float((pc1[0, 1] - 1.0 / C).abs().max()) <= 8 * U


def test_softmax_channel_argument_checks(dev):
    z = torch.zeros(1, 3, 2, 2, device=dev)
    with pytest.raises(RuntimeError, match="bad arguments"):
        K.softmax_channel_fwd(z, 3)
    with pytest.raises(RuntimeError, match="bad arguments"):
        K.softmax_channel_bwd(z, z[:, 0].contiguous(), -1)
    with pytest.raises(RuntimeError, match="bad arguments"):
        K.softmax_channel_fwd(z[:, :1].contiguous(), 0)                    # C == 1
    for bad in (torch.float64, torch.bfloat16, torch.float16):             # the wrappers refuse what the kernel would read as raw bits
        with pytest.raises(TypeError):
            K.softmax_channel_fwd(z.to(bad), 1)
        with pytest.raises(TypeError):
            K.dice_fwd(z.view(1, -1).to(bad), z.view(1, -1))
    torch.cuda.synchronize()


# ====================================================================================================== Dice
def _terms_per_thread(HW):
    # the launch rule of cs_dice_fwd (csrc/head.hip):
    #     long long bx = (HW + 256 * 8 - 1) / (256 * 8);  if (bx > 256) bx = 256;   grid (bx, N), 256 threads, stride bx * 256
    bx = min((HW + 256 * 8 - 1) // (256 * 8), 256)
    return -(-HW // (bx * 256))


def _sums_rel(HW):
    """relative error bound of a per-sample sum of non-negative terms: the per-thread fp32 chain (terms_per_thread roundings on the path
    of its first term, the product's included), six wave_sum levels, two for the four wave partials (the exact accumulator: none)"""
    return (_terms_per_thread(HW) + 6 + 2) * U


def _dice_inputs(N, HW, density, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.rand(N, HW, generator=g)
    if density == 0:
        t = torch.zeros(N, HW)
    elif density == 1:
        t = torch.ones(N, HW)
    else:
        t = (torch.rand(N, HW, generator=g) < density).float()
    return p, t


def _dice_grad_bound(p, t, eps, mean, ref_grad):
    """Elementwise bound of dice_bwd, per sample n:  16 * 2^-24 * max|grad_ref[n]|  +  3 e_s * G[n, i].
    grad = -s (2 t / den - 2 p num / den^2), s = 1/N | 1, num = 2a + eps, den = b + c + eps.  The kernel's own arithmetic (three
    conversions to fp32, num, den, den^2, the division and four operations per element) is a dozen roundings on terms no larger than
    the sample's largest gradient: the first part.  The sums a, b, c arrive with relative error e_s = _sums_rel(HW) each, so num and
    den carry e_s (non-negative sums, eps exact), t / den carries e_s and p num / den^2 carries 3 e_s: the second part, with
    G = s (2 t / den + 2 p num / den^2) the same expression on the magnitudes of its two terms.  Where the two terms cancel (p near t)
    the kernel's few roundings are relative to G as well, not to the small difference; 3 e_s >= 27 * 2^-24 covers those too.
    NOTE: the second part DEPARTS from the form "everything relative to max|grad_ref| of the sample": the error of num acts on the
    single term p num / den^2, not on the difference of the two, and for p == t max|grad_ref| is ~0 while rounding 2 t den - num 2 p
    leaves a residual of size 2^-24 G, so a bound relative to max|grad_ref| alone cannot hold there.  It is a worst-case bound
    (81 * 2^-24 G at HW = 1100^2); the kernel measures below 0.1 of it."""
    N, HW = p.shape
    pd, td = p.double(), t.double()
    a, b, c = (pd * td).sum(1, keepdim=True), (pd * pd).sum(1, keepdim=True), (td * td).sum(1, keepdim=True)
    num, den = 2 * a + eps, b + c + eps
    s = 1.0 / N if mean else 1.0
    G = s * (2 * td / den + 2 * pd * num / (den * den))
    return 16 * U * ref_grad.abs().amax(dim=1, keepdim=True) + 3 * _sums_rel(HW) * G


def _dice_case(p, t, eps, dev, what):
    """p, t [N, HW] fp32 on the host; checks sums, loss (mean and sum) and gradient (mean and sum) of the kernels"""
    N, HW = p.shape
    pg, tg = p.to(dev), t.to(dev)
    pd, td = p.double().view(N, 1, HW), t.double().view(N, 1, HW)          # 3-D: rows are samples for the reference too
    for mean in (True, False):
        loss, sums = K.dice_fwd(pg, tg, eps, mean)
        vals = K.dice_sums_values(sums, N)
        dp = K.dice_bwd(pg, tg, sums, eps, mean)
        torch.cuda.synchronize()
        ref_loss, ref_sums, ref_grad = R.dice_ref(pd, td, eps, mean)
        ref_grad = ref_grad.view(N, HW)
        assert vals.shape == (N, 3) and vals.dtype == torch.float64 and dp.shape == p.shape and loss.shape == (1,)
        err_s = (vals.cpu() - ref_sums).abs()
        bound_s = _sums_rel(HW) * ref_sums
        loss_err, loss_bound = abs(float(loss.item()) - float(ref_loss)), 8 * U * (1 if mean else N)
        err_g = (dp.cpu().double() - ref_grad).abs()
        bound_g = _dice_grad_bound(p, t, eps, mean, ref_grad)
        rel_s, ratio_g = float((err_s / ref_sums.clamp_min(1e-300)).max()), float((err_g / bound_g.clamp_min(1e-300)).max())
        print(f"dice {what} {'mean' if mean else 'sum'}: sums rel err {rel_s:.3e} (bound {_sums_rel(HW):.3e}); "
              f"loss err {loss_err:.3e} (bound {loss_bound:.3e}); grad err/bound {ratio_g:.3f}")
        assert bool((err_s <= bound_s).all()), f"{what}: sums {vals.cpu().tolist()} vs {ref_sums.tolist()}"
        assert loss_err <= loss_bound, f"{what}: loss {loss.item()} vs {float(ref_loss)}"
        assert bool(torch.isfinite(dp).all()) and bool((err_g <= bound_g).all()), f"{what}: gradient err/bound {ratio_g:.3f}"


@pytest.mark.parametrize("density", [0, 0.02, 0.5, 1])
@pytest.mark.parametrize("N,HW", [(1, 1), (3, 1000), (8, 299 * 299), (64, 32 * 32), (2, 1100 * 1100)])
def test_dice_kernels(N, HW, density, dev):
    """(2, 1100^2) is above both block caps (256 blocks * 2048 and 1024 blocks * 1024 elements per sample) and makes each thread of the
    sums kernel add 19 terms.  Bounds: sums relative (terms_per_thread + 8) 2^-24; loss 8 * 2^-24 absolute per sample (a value in [0, 1]
    from three fp32 sums in four operations; times N for `sum`); gradient: _dice_grad_bound."""
    if HW == 1100 * 1100:
        assert HW > 256 * 2048 and HW > 1024 * 1024 and _terms_per_thread(HW) >= 18
    p, t = _dice_inputs(N, HW, density, 300 + N)
    _dice_case(p, t, 1e-6, dev, f"N{N} HW{HW} density {density}")


@pytest.mark.parametrize("eps", [1e-6, 1.0])
def test_dice_value_edges(eps, dev):
    N, HW = 3, 5000
    g = torch.Generator().manual_seed(9)
    zero = torch.zeros(N, HW)
    # t == 0 and p == 0 everywhere: 1 - eps / eps = 0, finite gradient
    _dice_case(zero, zero, eps, dev, f"all zero eps {eps}")
    loss, sums = K.dice_fwd(zero.to(dev), zero.to(dev), eps, True)
    assert float(loss.item()) == 0.0
    assert bool(torch.isfinite(K.dice_bwd(zero.to(dev), zero.to(dev), sums, eps, True)).all())
    # p == t: the loss is ~0 by cancellation
    t = (torch.rand(N, HW, generator=g) < 0.3).float()
    _dice_case(t.clone(), t, eps, dev, f"p == t eps {eps}")
    p, _ = _dice_inputs(N, HW, 0.5, 10)
    _dice_case(p, p.clone(), eps, dev, f"p == t (soft) eps {eps}")
    _dice_case(p, t, eps, dev, f"plain eps {eps}")


def test_dice_nan_is_per_call(dev):
    """A NaN in p makes loss, sums and gradient NaN for THAT call (the sticky flag lives in the call's own `sums` buffer); a following
    clean call on fresh inputs is clean."""
    p, t = _dice_inputs(4, 3000, 0.5, 11)
    bad = p.clone()
    bad[2, 1234] = float("nan")
    loss, sums = K.dice_fwd(bad.to(dev), t.to(dev), 1e-6, True)
    vals = K.dice_sums_values(sums, 4)
    dp = K.dice_bwd(bad.to(dev), t.to(dev), sums, 1e-6, True)
    torch.cuda.synchronize()
    assert bool(torch.isnan(loss).all()) and bool(torch.isnan(vals).all()) and bool(torch.isnan(dp).all())
    _dice_case(p, t, 1e-6, dev, "clean call after a NaN call")


# ====================================================================================================== the public entry points
def _api_operands(kind, dev):
    """p (leaf, on the device, in the caller's dtype / layout), t, and their exact fp64 values on the host"""
    g = torch.Generator().manual_seed(21)
    N, H, W = 3, 20, 30
    p32 = torch.rand(N, H, W, generator=g)
    t32 = (torch.rand(N, H, W, generator=g) < 0.4).float()
    if kind in ("t_uint8", "t_bool", "t_int64"):
        p, t = p32.to(dev), t32.to({"t_uint8": torch.uint8, "t_bool": torch.bool, "t_int64": torch.int64}[kind]).to(dev)
    elif kind == "fp64":
        p, t = p32.double().to(dev), t32.double().to(dev)
    elif kind == "bf16_p":
        p32 = p32.bfloat16().float()
        p, t = p32.bfloat16().to(dev), t32.to(dev)
    elif kind == "noncontig_p":
        probs = torch.stack([1 - p32, p32], dim=1).to(dev)               # NCHW; the caller takes a channel slice
        p, t = probs[:, 1], t32.to(dev)
        assert not p.is_contiguous()
    elif kind == "two_d":
        p32, t32 = p32[0], t32[0]
        p, t = p32.to(dev), t32.to(dev)
    else:
        raise AssertionError(kind)
    return p.detach().requires_grad_(), t, p32.double(), t32.double()


API_KINDS = ["t_uint8", "t_bool", "t_int64", "fp64", "bf16_p", "noncontig_p", "two_d"]


def _must_agree(call, p, check):
    """Every operand kind of this file is accepted (cast to fp32 on the way in, see the docstrings of functional.dice_loss /
    softmax_channel and metrics.dice_coef) and must agree with the fp64 reference; a TypeError, like a wrong number returned
    silently, fails the test."""
    out = call()
    out.sum().backward()
    torch.cuda.synchronize()
    check(out.detach().cpu().double(), p.grad)


@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("entry", ["HF.dice_loss", "train.DiceLoss"])
@pytest.mark.parametrize("kind", API_KINDS)
def test_dice_loss_public_dtypes(kind, entry, reduction, dev):
    p, t, pd, td = _api_operands(kind, dev)
    eps, mean = 1e-6, reduction == "mean"
    ref_loss, _, ref_grad = R.dice_ref(pd, td, eps, mean)
    n = 1 if pd.ndim == 2 else pd.shape[0]
    p2, t2, g2 = pd.reshape(n, -1), td.reshape(n, -1), ref_grad.reshape(n, -1)

    def check(loss, grad):
        assert abs(float(loss) - float(ref_loss)) <= 8 * U * (1 if mean else n), f"{float(loss)} vs {float(ref_loss)}"
        assert grad.shape == p.shape and grad.dtype == p.dtype                  # the caller's dtype and shape
        bound = _dice_grad_bound(p2.float(), t2.float(), eps, mean, g2)
        if grad.dtype == torch.bfloat16:
            bound = bound + R.U16 * g2.abs()
        assert bool(((grad.detach().cpu().double().reshape(n, -1) - g2).abs() <= bound).all())

    call = (lambda: HF.dice_loss(p, t, eps, reduction)) if entry == "HF.dice_loss" else (lambda: T.DiceLoss(eps, reduction)(p, t))
    _must_agree(call, p, check)


@pytest.mark.parametrize("kind", ["fp64", "bf16_p", "noncontig_p", "two_d"])      # integer targets: dice_coef asserts equal dtypes by design
def test_dice_coef_public_dtypes(kind, dev):
    p, t, pd, td = _api_operands(kind, dev)
    if kind == "bf16_p":
        t = t.bfloat16()                                                        # equal dtypes; 0 / 1 are exact in bf16
    eps = 1e-6
    ref_loss, _, ref_grad = R.dice_ref(pd, td, eps, False)                      # sum of (1 - d_n): d sums to n - loss, gradient -grad
    n = 1 if pd.ndim == 2 else pd.shape[0]
    p2, t2, g2 = pd.reshape(n, -1), td.reshape(n, -1), -ref_grad.reshape(n, -1)

    def check(d, grad):
        assert d.numel() == n and abs(float(d.sum()) - (n - float(ref_loss))) <= 8 * U * n
        assert grad.shape == p.shape and grad.dtype == p.dtype
        bound = _dice_grad_bound(p2.float(), t2.float(), eps, False, g2)
        if grad.dtype == torch.bfloat16:
            bound = bound + R.U16 * g2.abs()
        assert bool(((grad.detach().cpu().double().reshape(n, -1) - g2).abs() <= bound).all())

    _must_agree(lambda: M.dice_coef(p, t, eps), p, check)


@pytest.mark.parametrize("kind", ["fp32", "fp64", "bf16", "noncontig"])
def test_softmax_channel_public_dtypes(kind, dev):
    g = torch.Generator().manual_seed(23)
    N, C, H, W = 2, 3, 9, 11
    l32 = 3 * torch.randn(N, C, H, W, generator=g)
    dpc = torch.randn(N, H, W, generator=g)
    if kind == "bf16":
        l32 = l32.bfloat16().float()
    if kind == "noncontig":
        logits = l32.permute(0, 2, 3, 1).contiguous().to(dev).permute(0, 3, 1, 2)      # NHWC memory behind an NCHW view
        assert not logits.is_contiguous()
    else:
        logits = l32.to({"fp32": torch.float32, "fp64": torch.float64, "bf16": torch.bfloat16}[kind]).to(dev)
    logits = logits.detach().requires_grad_()
    ref_p, ref_g, tol_p, tol_g, _, _ = _softmax_yardstick(l32, dpc, 1)
    out = HF.softmax_channel(logits, 1)
    out.backward(dpc.to(dev).to(out.dtype))
    torch.cuda.synchronize()
    assert out.shape == (N, H, W)
    assert float((out.detach().cpu().double() - ref_p).abs().max()) <= tol_p
    grad = logits.grad
    assert grad.shape == logits.shape and grad.dtype == logits.dtype
    bound = tol_g + (R.U16 * ref_g.abs() if grad.dtype == torch.bfloat16 else 0)
    assert bool(((grad.cpu().double() - ref_g).abs() <= bound).all())
