"""GPU: which second-generation kernel serves a call, that it computes the exact result, and that it stays inside the rows / slabs its
query announced -- one row of tests/conv2_cases.py each (csrc/conv_v2.hip: cs_conv2d_fwd_packed, cs_conv2d_dgrad_packed;
csrc/wgrad_v2.hip through cs_conv2d_wgrad_batched).

  ledger      after each launch `cs_last_conv_variant()` equals the string `expect()` derives for the device's own compute-unit count,
              and on a 256-CU device that is the row's hand-written name (production library only: the A/B flavour's knobs re-route)
  exact       integer operands (conv2_cases.draw, two kinds): every output and gradient is an integer that bf16 / fp32 hold exactly, so
              the comparison with torch's CPU fp32 convolution is torch.equal -- no tolerance (the domain is asserted on the reference,
              and on the host by tests/test_conv2_cases_host.py)
  workspace   the C entries write every partial row / slab word they announced and leave a guard behind the buffer untouched"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

import conv2_cases as C2  # noqa: E402

from cellsegmentation_amd import _lib  # noqa: E402
from cellsegmentation_amd import kernels as K  # noqa: E402

BF = torch.bfloat16
GUARD = 4096
PRODUCTION = _lib.FLAVOUR == ""


def _variant():
    return (_lib.load().cs_last_conv_variant() or b"").decode()


def _cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _geom(case):
    N, H, W, C, Kc, R, stride, pad = case["geom"]
    return K.make_geom(N, H, W, C, Kc, R, R, stride, pad)


def _nhwc(t_nchw, dev):
    return t_nchw.permute(0, 2, 3, 1).contiguous().to(BF).to(dev)


def _nchw(t):
    return t.float().cpu().permute(0, 3, 1, 2).contiguous()


def _bits(mask_nchw, dev):
    return K.pack_bits(mask_nchw.permute(0, 2, 3, 1).contiguous().to(dev))


def _packed(geom, w_kcrs, dev, dgrad):
    """the packed operand of w [K][C][R][S] for one direction"""
    C, Kc = geom.C, geom.K
    w_khwc, w_chwk = K.weight_prep(w_kcrs.to(dev), None, BF, C, Kc, want_fwd=not dgrad, want_bwd=dgrad)
    return K.pack_conv_weights(geom, w_chwk if dgrad else w_khwc, dgrad=dgrad)


def _guarded(nbytes, dev):
    """uint8 buffer of nbytes NaN-filled workspace (every fp32 word reads as NaN) + GUARD sentinel bytes"""
    buf = torch.full((nbytes + GUARD,), 0xFF, dtype=torch.uint8, device=dev)
    sentinel = (torch.arange(GUARD, dtype=torch.int32) * 37 + 11).to(torch.uint8)
    buf[nbytes:] = sentinel.to(dev)
    return buf, sentinel


@pytest.mark.parametrize("case", C2.CASES, ids=C2.IDS)
def test_conv2_ledger(case, dev):
    """forward and data gradient of the row reach the instantiation the ledger names, and announce the partial rows the plan has"""
    lib = _lib.load()
    N, H, W, C, Kc, R, stride, pad = case["geom"]
    g = _geom(case)
    cus = _cus(dev)
    for op in ("fwd", "dgrad"):
        dg = op == "dgrad"
        want, rows = C2.expect(case, op, cus)
        assert K.packed_supported(g, BF, dgrad=dg) == (want is not None)
        assert lib.cs_conv2d_packed_partial_rows(ctypes.byref(g), int(dg)) == rows
        if cus == 256:
            assert want == case[op], (case["id"], op)
        if want is None:
            continue
        wp = torch.zeros((lib.cs_conv2d_packed_weight_bytes(ctypes.byref(g), int(dg)) // 2,), dtype=BF, device=dev)
        if dg:
            K.conv_dgrad_packed(g, torch.zeros((N, g.P, g.Q, Kc), dtype=BF, device=dev), wp)
        else:
            K.conv_fwd_packed(g, torch.zeros((N, H, W, C), dtype=BF, device=dev), wp)
        got = _variant()
        torch.cuda.synchronize()
        if PRODUCTION:
            assert got == want, (case["id"], op)


@pytest.mark.parametrize("kind", C2.KINDS)
@pytest.mark.parametrize("case", C2.CASES, ids=C2.IDS)
def test_conv2_exact_values(case, kind, dev):
    """bit equality with torch's CPU fp32 convolution and its input gradient: plain, and with every fused operand"""
    N, H, W, C, Kc, R, stride, pad = case["geom"]
    g = _geom(case)
    d = C2.reference(case, kind)
    if case["fwd"]:
        xd, wp = _nhwc(d["x"], dev), _packed(g, d["w"], dev, False)
        y = K.conv_fwd_packed(g, xd, wp)
        y_full, bits = K.conv_fwd_packed(g, xd, wp, d["shift"].to(dev), _nhwc(d["res"], dev), K.CS_ACT_RELU, want_bits=True)
        torch.cuda.synchronize()
        assert torch.equal(_nchw(y), d["y"]), f"max diff {float((_nchw(y) - d['y']).abs().max())}"
        assert torch.equal(_nchw(y_full), d["y_full"])
        assert torch.equal(K.unpack_bits(bits, Kc).cpu().permute(0, 3, 1, 2), d["y_full"] > 0)
    if not case["dgrad"]:
        return
    dyd, wpd = _nhwc(d["dy"], dev), _packed(g, d["wt"], dev, True)
    if stride == 2:
        # compact: the values of the destination pixels (2y, 2x); every other pixel of the dense gradient is zero
        comp = K.conv_dgrad_packed(g, dyd, wpd)
        torch.cuda.synchronize()
        assert isinstance(comp, K.CompactGrad) and tuple(comp.t.shape) == (N, g.P, g.Q, C)
        assert torch.equal(_nchw(comp.t), d["dx"][:, :, ::2, ::2])
        assert float(d["dx"][:, :, 1::2, :].abs().max()) == 0.0 and float(d["dx"][:, :, :, 1::2].abs().max()) == 0.0
        return
    mask_bits = _bits(d["mask"], dev)
    dx = K.conv_dgrad_packed(g, dyd, wpd)
    dx2, pc = K.conv_dgrad_packed(g, dyd, wpd, add=_nhwc(d["add"], dev), mask_bits=mask_bits, want_colsum=True)
    cs = pc.vector()
    torch.cuda.synchronize()
    assert torch.equal(_nchw(dx), d["dx"]), f"max diff {float((_nchw(dx) - d['dx']).abs().max())}"
    assert torch.equal(_nchw(dx2), d["dx2"])
    assert torch.equal(cs.cpu()[:C], d["colsum"])
    assert torch.equal(cs.cpu()[:C].double(), dx2.double().sum(dim=(0, 1, 2)).cpu())          # ... the sums of what was stored
    if "cadd" in d:
        # the consumer of a compact gradient: the operand is added at the even pixels only
        comp = K.CompactGrad(_nhwc(d["cadd"], dev), 2)
        dx2c, pc = K.conv_dgrad_packed(g, dyd, wpd, add=comp, mask_bits=mask_bits, want_colsum=True)
        cs = pc.vector()
        torch.cuda.synchronize()
        assert torch.equal(_nchw(dx2c), d["dx2c"])
        assert torch.equal(cs.cpu()[:C], d["colsum_c"])
        assert torch.equal(cs.cpu()[:C].double(), dx2c.double().sum(dim=(0, 1, 2)).cpu())


@pytest.mark.parametrize("case", [c for c in C2.CASES if c["dgrad"] and c["geom"][6] == 1], ids=lambda c: c["id"])
def test_conv2_partial_rows_are_all_written(case, dev):
    """cs_conv2d_dgrad_packed through ctypes on a NaN-filled buffer of exactly the announced rows: an announced row the launch does not
    write leaves a NaN in the folded sums; a row it writes beyond them lands in the guard"""
    lib = _lib.load()
    N, H, W, C, Kc, R, stride, pad = case["geom"]
    g = _geom(case)
    d = C2.reference(case, "sparse")
    rows = lib.cs_conv2d_packed_partial_rows(ctypes.byref(g), 1)
    assert rows == C2.expect(case, "dgrad", _cus(dev))[1] and rows > 0
    nbytes = rows * 2 * C * 4                                               # [rows][2][C] fp32: the sums, and a half the fold may use
    dyd, wpd, addd, mask_bits = _nhwc(d["dy"], dev), _packed(g, d["wt"], dev, True), _nhwc(d["add"], dev), _bits(d["mask"], dev)
    buf, sentinel = _guarded(nbytes, dev)
    dx = torch.empty((N, H, W, C), dtype=BF, device=dev)
    _lib.check(lib.cs_conv2d_dgrad_packed(ctypes.byref(g), K._p(dyd), K._p(wpd), K._p(addd), 1, K._p(mask_bits), K._p(dx), K._p(buf), K._stream()),
               "conv2d_dgrad_packed")
    torch.cuda.synchronize()
    assert torch.equal(buf[nbytes:].cpu(), sentinel)
    sums = buf[:nbytes].view(torch.float32).view(rows, 2 * C)[:, :C]
    assert bool(torch.isfinite(sums).all()), f"{int((~torch.isfinite(sums)).any(dim=1).sum())} of {rows} announced rows were not written"
    vec = torch.zeros((C,), dtype=torch.float32, device=dev)
    _lib.check(lib.cs_fold_partial_rows(K._p(buf), rows, C, K._p(vec), K._stream()), "fold_partial_rows")
    torch.cuda.synchronize()
    assert torch.equal(buf[nbytes:].cpu(), sentinel)
    assert torch.equal(vec.cpu(), d["colsum"])
    assert torch.equal(_nchw(dx), d["dx2"])


# ---------------------------------------------------------------------------------------------------------------- weight gradient
def _wgrad_launch(case, xs, dys, dev):
    """cs_conv2d_wgrad_batched through ctypes into NaN-filled slabs + guard -> ([items][nsplit][K][3][3][C] fp32, variant); every slab
    word must have been written and the guard left alone"""
    lib = _lib.load()
    N, H, W, C, Kc, items = case["geom"]
    g = K.make_geom(N, H, W, C, Kc, 3, 3, 1, 1)
    nsplit = lib.cs_conv2d_wgrad_batched_splits(ctypes.byref(g), K._code(BF), items)
    assert nsplit == C2.expect_wgrad(case)[1]
    item_bytes = nsplit * Kc * 9 * C * 4
    buf, sentinel = _guarded(items * item_bytes, dev)
    xd, dyd = [_nhwc(x, dev) for x in xs], [_nhwc(dy, dev) for dy in dys]
    arr = ctypes.c_void_p * items
    xt, dt_ = arr(*[t.data_ptr() for t in xd]), arr(*[t.data_ptr() for t in dyd])
    wt = arr(*[buf.data_ptr() + i * item_bytes for i in range(items)])
    _lib.check(lib.cs_conv2d_wgrad_batched(ctypes.byref(g), K._code(BF), xt, dt_, wt, items, 1, K._stream()), "conv2d_wgrad_batched")
    variant = _variant()
    torch.cuda.synchronize()
    assert torch.equal(buf[items * item_bytes:].cpu(), sentinel)
    slabs = buf[:items * item_bytes].view(torch.float32).view(items, nsplit, Kc, 3, 3, C)
    assert bool(torch.isfinite(slabs).all()), "a slab word was not written"
    return slabs, variant


def _kcrs(slab_sum):
    return slab_sum.float().cpu().permute(0, 3, 1, 2).contiguous()          # [K][3][3][C] -> [K][C][3][3]


@pytest.mark.parametrize("case", C2.WGRAD_CASES, ids=C2.WGRAD_IDS)
def test_wgrad2_ledger_and_exact_values(case, dev):
    """the stage class of the row; every item's slab sum is the weight gradient of ITS OWN operands; and every single slab is the weight
    gradient of the dy pixels whose padded-linear position lies in that split's stages -- the restated split plan is the kernel's"""
    N, H, W, C, Kc, items = case["geom"]
    xs, dys = C2.draw_wgrad(case)
    slabs, variant = _wgrad_launch(case, xs, dys, dev)
    want, nsplit, sps = C2.expect_wgrad(case)
    assert want == case["variant"]
    if PRODUCTION:
        assert variant == want
    assert slabs.shape[1] == nsplit
    pl = C2.plan_wgrad2(N, H, W, C, Kc, items)
    for i in range(items):
        ref = C2.wgrad_reference(xs[i], dys[i])
        got = _kcrs(slabs[i].double().sum(0))
        assert torch.equal(got, ref), f"item {i}: max diff {float((got - ref).abs().max())}"
        if pl and (i == 0 or i == items - 1):
            split = C2.split_of_pixels(N, H, W, pl["bl"], sps)
            assert int(split.max()) <= nsplit - 1
            for s in range(nsplit):                 # (a last split that holds only the zero row behind the last image owes an all-zero slab)
                part = C2.wgrad_reference(xs[i], dys[i] * (split == s))
                assert torch.equal(_kcrs(slabs[i, s]), part), f"item {i}, slab {s} of {nsplit}"


@pytest.mark.parametrize("case", C2.WGRAD_CASES, ids=C2.WGRAD_IDS)
def test_wgrad2_all_ones_closed_form(case, dev):
    """all-ones operands: dW[k][c][r][s] counts the pixel pairs of tap (r, s): N * (H - |r - 1|) * (W - |s - 1|), for every (k, c)"""
    N, H, W, C, Kc, items = case["geom"]
    xs = [torch.ones((N, C, H, W)) for _ in range(items)]
    dys = [torch.ones((N, Kc, H, W)) for _ in range(items)]
    slabs, _ = _wgrad_launch(case, xs, dys, dev)
    taps = N * torch.tensor([H - 1, H, H - 1]).view(3, 1) * torch.tensor([W - 1, W, W - 1]).view(1, 3)
    want = taps.float().view(1, 3, 3, 1).expand(Kc, 3, 3, C)
    for i in range(items):
        assert torch.equal(slabs[i].double().sum(0).float().cpu(), want), f"item {i}"
