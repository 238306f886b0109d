"""GPU: which depthwise kernel serves a call, that it computes the exact result, and that it stays inside the workspace its query
sized -- one row of tests/dw_cases.py each (csrc/dwse.hip: cs_dwconv_fwd, _fwd_stats, _dgrad, _wgrad, _wgrad_oihw).

  ledger      after each launch `cs_last_conv_variant()` equals the row's string: kernel instantiation, grid, items per workgroup, lanes
              (production routing only: the forced-mode children of test_depthwise_tiled_kernels_everywhere_the_geometry_allows
              do not select it)
  exact       integer operands (dw_cases.draw): every output, gradient and statistic is an integer that bf16 / fp32 / fp64 hold
              exactly, so the comparison with torch's CPU fp32 convolution is torch.equal -- no tolerance; the reference side is itself
              checked against an int64 restatement on the host (tests/test_dw_cases_host.py)
  workspace   the C entries write exactly the rows the plan announced, inside cs_dwconv_*_workspace bytes, and leave a guard behind
              the workspace untouched (the guard lies inside the allocation)"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

import dw_cases as DW  # noqa: E402

from cellsegmentation_amd import _lib  # noqa: E402
from cellsegmentation_amd import kernels as K  # noqa: E402

DT = {"bf16": torch.bfloat16, "f32": torch.float32}
GUARD = 4096


def _variant():
    return (_lib.load().cs_last_conv_variant() or b"").decode()


def _operands(case, dev):
    """(geom, x, w_hwc, dy) on the device in the row's dtype, NHWC"""
    C, k, s, H, W = case["geom"]
    x, w, dy, *_ = DW.reference(case)
    dt = DT[case["dtype"]]
    g = K.make_geom(DW.N, H, W, C, C, k, k, s, (k - 1) // 2)
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to(dt).to(dev)  # noqa: E731
    return g, nhwc(x), w[:, 0].permute(1, 2, 0).contiguous().to(dev), nhwc(dy)


def _nchw(t):
    return t.float().cpu().permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize("case", DW.CASES, ids=DW.IDS)
def test_dw_ledger(case, dev):
    """every operation of the row reaches the instantiation, grid, per and lanes the ledger names"""
    g, x, w, dy = _operands(case, dev)
    got = {}
    K.dwconv_fwd(g, x, w)
    got["fwd"] = _variant()
    K.dwconv_fwd_stats(g, x, w)
    got["fwd_stats"] = _variant()
    K.dwconv_dgrad(g, dy, w)
    got["dgrad"] = _variant()
    K.dwconv_wgrad(g, x, dy)
    got["wgrad"] = _variant()
    K.dwconv_wgrad(g, x, dy, param_layout=True)
    got["wgrad_oihw"] = _variant()
    torch.cuda.synchronize()
    want = {op: DW.expect(case, op)[0] for op in ("fwd", "fwd_stats", "dgrad", "wgrad")}
    want["wgrad_oihw"] = want["wgrad"]
    assert got == want


@pytest.mark.parametrize("case", DW.CASES, ids=DW.IDS)
def test_dw_exact_values(case, dev):
    """bit equality with torch's CPU fp32 convolution, its input and weight gradients, and the fp64 sums of z and z^2"""
    C, k, s, H, W = case["geom"]
    _, _, _, y, dx, dw = DW.reference(case)
    g, x, w, dy = _operands(case, dev)
    yd = K.dwconv_fwd(g, x, w)
    zd, stats = K.dwconv_fwd_stats(g, x, w)
    dxd = K.dwconv_dgrad(g, dy, w)
    dwd = K.dwconv_wgrad(g, x, dy)
    dwo = K.dwconv_wgrad(g, x, dy, param_layout=True)
    sv = K.stats_values(stats)
    torch.cuda.synchronize()
    assert torch.equal(_nchw(yd), y)
    assert torch.equal(_nchw(zd), y)
    assert torch.equal(_nchw(dxd), dx)
    assert torch.equal(dwd.cpu().permute(2, 0, 1).unsqueeze(1), dw)
    assert torch.equal(dwo.cpu(), dw)
    z = y.double().permute(1, 0, 2, 3).reshape(C, -1)
    assert torch.equal(sv[0].cpu().double(), z.sum(1)) and torch.equal(sv[1].cpu().double(), (z * z).sum(1))


def _guarded(nbytes, dev):
    """uint8 buffer of nbytes NaN-filled workspace (every fp32 / fp64 word reads as NaN) + GUARD sentinel bytes"""
    buf = torch.full((nbytes + GUARD,), 0xFF, dtype=torch.uint8, device=dev)
    sentinel = (torch.arange(GUARD, dtype=torch.int32) * 37 + 11).to(torch.uint8)
    buf[nbytes:] = sentinel.to(dev)
    return buf, sentinel


def _rows_written(buf, nbytes, row_bytes, dtype):
    """number of leading rows of the workspace that hold no NaN any more; asserts that every row behind them is still all NaN"""
    words = buf[:nbytes].view(dtype).view(-1, row_bytes // (torch.finfo(dtype).bits // 8))
    nan = torch.isnan(words)
    full = (~nan).all(dim=1).cpu()
    n = int(full.sum())
    assert bool(full[:n].all()) and bool(nan[n:].all()), "partial rows must be a dense prefix of whole rows"
    return n


@pytest.mark.parametrize("case", DW.CASES, ids=DW.IDS)
def test_dw_workspace_bound(case, dev):
    """statistics forward and weight gradient through the C entries: rows written == rows announced == the ledger's, inside the
    workspace the query sized, guard untouched"""
    C, k, s, H, W = case["geom"]
    lib = _lib.load()
    g, x, w, dy = _operands(case, dev)
    code = K._code(x.dtype)
    stream = K._stream()
    # statistics forward
    nbytes = lib.cs_dwconv_fwd_stats_workspace(ctypes.byref(g))
    buf, sentinel = _guarded(nbytes, dev)
    y = torch.empty((g.N, g.P, g.Q, C), dtype=x.dtype, device=dev)
    rows = ctypes.c_int(-1)
    _lib.check(lib.cs_dwconv_fwd_stats(ctypes.byref(g), code, K._p(x), K._p(w), K._p(y), K._p(buf), ctypes.byref(rows), stream), "dwconv_fwd_stats")
    torch.cuda.synchronize()
    want_rows = DW.expect(case, "fwd_stats")[1]
    row_bytes = 2 * C * 8
    assert torch.equal(buf[nbytes:].cpu(), sentinel)
    assert rows.value * row_bytes <= nbytes
    assert rows.value == want_rows
    assert _rows_written(buf, nbytes, row_bytes, torch.float64) == want_rows
    # weight gradient, both layouts (the entry reports no row count: the rows are read off the workspace)
    nbytes = lib.cs_dwconv_wgrad_workspace(ctypes.byref(g))
    want_rows = DW.expect(case, "wgrad")[1]
    row_bytes = k * k * C * 4
    assert want_rows * row_bytes <= nbytes
    for entry in (lib.cs_dwconv_wgrad, lib.cs_dwconv_wgrad_oihw):
        buf, sentinel = _guarded(nbytes, dev)
        dw = torch.empty((k * k * C,), dtype=torch.float32, device=dev)
        _lib.check(entry(ctypes.byref(g), code, K._p(x), K._p(dy), K._p(dw), K._p(buf), stream), "dwconv_wgrad")
        torch.cuda.synchronize()
        assert torch.equal(buf[nbytes:].cpu(), sentinel)
        assert _rows_written(buf, nbytes, row_bytes, torch.float32) == want_rows
