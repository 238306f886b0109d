"""Exact integer tests of every dispatch variant of the first-generation implicit-GEMM family (csrc/conv_igemm.hip: cs_conv2d_fwd[_bits],
cs_conv2d_dgrad[_bits], cs_conv2d_wgrad[_batched], cs_stem_*), one row of tests/igemm_cases.py each.

A row runs its launch, asserts that `cs_last_conv_variant()` names the instantiation the row expects (so a shape list that silently
stops reaching a kernel fails), then asserts BIT EQUALITY with the fp64 reference of tests/conv_ref.py cast to the stored dtype: integer
operands keep every product and every fp32 partial sum exact (conv_ref.assert_exact_domain checks that per case), so no tolerance is
needed and one mis-indexed tap, chunk, pixel, class offset, tile tail or split-K slab changes an output integer.

A/B flavour (the children of test_wave_specialised_weight_gradient_on_every_shape): the `igemm_path` fixture also walks the
register-staged kernels, and the expected string is igemm_cases.ab_variant(row) -- the full string, not just the family prefix."""
import ctypes
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import conv_ref as R  # noqa: E402
from igemm_cases import CASES, ab_variant  # noqa: E402

from cellsegmentation_amd import _lib  # noqa: E402
from cellsegmentation_amd import kernels as K  # noqa: E402

DT = {"bf16": torch.bfloat16, "f32": torch.float32}

_PATHS = ([(0, "lds_dma"), (1, "reg_staged")]
          if os.environ.get("CELLSEG_LIB_FLAVOUR") == "ab" and os.environ.get("CELLSEG_TEST_IGEMM_PATHS", "all") == "all" else [(0, "lds_dma")])
_SPEC = int(os.environ.get("CELLSEG_WGRAD_SPEC", "0")) if os.environ.get("CELLSEG_LIB_FLAVOUR") == "ab" else 0


@pytest.fixture(params=[p for p, _ in _PATHS], ids=[i for _, i in _PATHS])
def igemm_path(request):
    if len(_PATHS) == 1:
        yield request.param
        return
    old = K.set_igemm_path(request.param)
    yield request.param
    K.set_igemm_path(old)


def _variant():
    return (_lib.load().cs_last_conv_variant() or b"").decode()


def _pad_c(t_nchw, Cp):
    """NCHW fp64 -> NHWC fp64 with the channels zero-padded to Cp"""
    n, c, h, w = t_nchw.shape
    out = torch.zeros((n, h, w, Cp), dtype=torch.float64)
    out[..., :c] = t_nchw.permute(0, 2, 3, 1)
    return out


def _dev(t_nchw, Cp, dtype, dev):
    return _pad_c(t_nchw, Cp).to(dtype).to(dev)


def _tile_of(variant):
    parts = variant[variant.index("<") + 1:-1].split(",")
    return int(parts[1]), int(parts[2])


def _assert_equal(got_nhwc, ref_nchw, dtype, case, what, stride=1, variant=""):
    """bit equality of a stored NHWC tensor with the zero-padded fp64 reference cast to the stored dtype; on a mismatch, the first
    differing (n, h, w, c), its tile and its parity class"""
    ref = _pad_c(ref_nchw, got_nhwc.shape[-1]).to(dtype)
    got = got_nhwc.cpu()
    if torch.equal(got, ref):
        return
    diff = (got.double() != ref.double()).nonzero()
    n, h, w, c = [int(v) for v in diff[0]]
    bm, bn = _tile_of(variant) if variant.startswith("igemm") else (0, 0)
    m = (n * got.shape[1] + h) * got.shape[2] + w
    where = f"M tile {m // bm} row {m % bm}, N tile {c // bn}" if bm else ""
    raise AssertionError(f"{case['id']} {what}: {len(diff)} elements differ; first at (n, h, w, c) = ({n}, {h}, {w}, {c}): got {float(got[n, h, w, c])}, "
                         f"want {float(ref[n, h, w, c])}; {where}; parity class ({h % stride}, {w % stride}) of stride {stride}; {variant}")


def _expect(case, igemm_path):
    return ab_variant(case["variant"], igemm_path, _SPEC, case["ab_reg"]) if os.environ.get("CELLSEG_LIB_FLAVOUR") == "ab" else case["variant"]


def _seed(case):
    return torch.Generator().manual_seed(sum(ord(ch) * (i + 1) for i, ch in enumerate(case["id"])))


def _rows(M, variant):
    bm = _tile_of(variant)[0]
    return (M + bm - 1) // bm


# ------------------------------------------------------------------------------------------------ forward
def _run_fwd(case, dev, igemm_path):
    N, H, W, Cin, Cout, Rf, s, p, G = case["geom"]
    dtype, flags = DT[case["dtype"]], case["op"].split("+")[1:]
    g = _seed(case)
    Cp, Kp = K.pad_channels(Cin), K.pad_channels(Cout)
    geom = K.make_geom(N, H, W, Cp, Kp, Rf, Rf, s, p)
    P, Q = geom.P, geom.Q
    x = R.activations((N, Cin, H, W), g)
    w = R.fwd_filters(Cout, Cin // G, Rf, Rf, 12, g)
    fused = "fused" in flags or "bits" in flags
    scale = R.ints((Cout,), 1, 2, g) if "fused" in flags else None
    shift = R.ints((Cout,), -8, 8, g) if fused else None
    res = R.ints((N, Cout, P, Q), -16, 16, g) if fused else None
    ref = R.conv_fwd(x, w, s, p, G, scale, shift, res, relu=fused)
    bound = R.conv_fwd(x.abs(), w.abs(), s, p, G, scale, None if shift is None else shift.abs(), None if res is None else res.abs())
    R.assert_exact_domain(stored=[ref], abs_sums=[bound], stats_of=ref if "stats" in flags else None)
    xd = _dev(x, Cp, dtype, dev)
    if G > 1:
        wk, _ = K.weight_prep_grouped(w.float().to(dev), None, dtype, True, False)
    else:
        wk, _ = K.weight_prep(w.float().to(dev), None, dtype, Cp, Kp, want_fwd=True, want_bwd=False)

    def vec(v, fill):
        out = torch.full((Kp,), fill, dtype=torch.float32)
        out[:Cout] = v.float()
        return out.to(dev)
    sc = vec(scale, 1.0) if scale is not None else None
    sh = vec(shift, 0.0) if shift is not None else None
    rd = _dev(res, Kp, dtype, dev) if res is not None else None
    act = K.CS_ACT_RELU if fused else K.CS_ACT_NONE
    stats = K.new_stats(Kp, dev) if "stats" in flags else None
    bits = None
    if "bits" in flags:
        y, bits = K.conv_fwd(geom, xd, wk, sc, sh, rd, act, grouped=G > 1, want_bits=True)
    else:
        y = K.conv_fwd(geom, xd, wk, sc, sh, rd, act, stats=stats, grouped=G > 1)
    if stats is not None:
        # which statistics path ran: the slab path writes `rows` partial rows of the workspace, the atomic path leaves it alone
        # (the same launch again through the C ABI, on a workspace of NaN and a second accumulator)
        ws = torch.full((_lib.load().cs_conv2d_stats_workspace(N * P * Q, Kp) // 4,), float("nan"), dtype=torch.float32, device=dev)
        y2, stats2 = torch.empty_like(y), K.new_stats(Kp, dev)
        _lib.check(_lib.load().cs_conv2d_fwd(ctypes.byref(geom), K._code(dtype), K._p(xd), K._p(wk), None, None, None, act, K._p(y2), K._p(stats2),
                                             K._p(ws), K._stream()), "conv2d_fwd")
        written = ~torch.isnan(ws[:case["rows"] * 2 * Kp])
        assert bool(written.all()) if case["rows"] > 512 else not bool(written.any()), \
            f"{case['id']}: {case['rows']} rows took the {'atomic' if case['rows'] > 512 else 'slab'} path"
        assert torch.equal(y2, y) and torch.equal(K.stats_values(stats2), K.stats_values(stats))
    got_variant = _variant()
    torch.cuda.synchronize()
    assert got_variant == _expect(case, igemm_path), f"{case['id']}: launched {got_variant}"
    _assert_equal(y, ref, dtype, case, "y", 1, got_variant)                 # (padded output channels: exactly zero)
    if bits is not None:
        assert torch.equal(K.unpack_bits(bits, Kp).cpu(), _pad_c(ref, Kp) > 0), f"{case['id']}: sign bits"
    if stats is not None:
        assert _rows(N * P * Q, got_variant) == case["rows"], f"{case['id']}: {_rows(N * P * Q, got_variant)} statistics rows"
        want = torch.zeros((2, Kp), dtype=torch.float64)
        want[:, :Cout] = R.channel_stats(ref)
        assert torch.equal(K.stats_values(stats).cpu(), want), f"{case['id']}: statistics ({'atomic' if case['rows'] <= 512 else 'slab'} path)"


# ------------------------------------------------------------------------------------------------ data gradient
def _run_dgrad(case, dev, igemm_path):
    N, H, W, Cin, Cout, Rf, s, p, G = case["geom"]
    dtype, flags = DT[case["dtype"]], case["op"].split("+")[1:]
    g = _seed(case)
    Cp, Kp = K.pad_channels(Cin), K.pad_channels(Cout)
    geom = K.make_geom(N, H, W, Cp, Kp, Rf, Rf, s, p)
    P, Q = geom.P, geom.Q
    dy = R.gradients((N, Cout, P, Q), g)
    w = R.dgrad_filters_grouped(Cin, Cin // G, Rf, Rf, 12, g) if G > 1 else R.dgrad_filters(Cout, Cin, Rf, Rf, 12, g)
    add = R.ints((N, Cin, H, W), -16, 16, g) if "add" in flags else None
    mask = (torch.rand((N, Cin, H, W), generator=g) > 0.4) if ("mask" in flags or "bits" in flags) else None
    ref = R.conv_dgrad(dy, w, (H, W), s, p, G, add, mask)
    bound = R.conv_dgrad(dy.abs(), w.abs(), (H, W), s, p, G, None if add is None else add.abs())
    want_cs = "colsum" in flags or "defer" in flags
    R.assert_exact_domain(stored=[ref], abs_sums=[bound], colsum_of=ref if want_cs else None)
    dyd = _dev(dy, Kp, dtype, dev)
    if G > 1:
        _, wc = K.weight_prep_grouped(w.float().to(dev), None, dtype, False, True)
    else:
        _, wc = K.weight_prep(w.float().to(dev), None, dtype, Cp, Kp, want_fwd=False, want_bwd=True)
    addd = _dev(add, Cp, dtype, dev) if add is not None else None
    maskd = bitsd = None
    if "mask" in flags:
        maskd = _dev(torch.where(mask, 1.0, -1.0).double(), Cp, dtype, dev)          # kept where the mask operand is > 0
    if "bits" in flags:
        bitsd = K.pack_bits((_pad_c(mask.double(), Cp) > 0).to(dev))
    lib = _lib.load()
    cgeom = K._grouped_geom(geom, G > 1)
    # deferred column sums: stride 1, or a stride-2 launch whose classes merge (not on the register-staged path: immediate sums there)
    defer = "defer" in flags and (s == 1 or lib.cs_conv2d_dgrad_partial_rows(ctypes.byref(cgeom)) > 0)
    cs = torch.zeros((Cp,), dtype=torch.float32, device=dev) if (want_cs and not defer) else None
    out = K.conv_dgrad(geom, dyd, wc, addd, maskd, cs, grouped=G > 1, defer_colsum=defer, mask_bits=bitsd)
    got_variant = _variant()
    dx = out
    if defer:
        dx, pc = out
        assert isinstance(pc, K.PartialColsum) and pc.rows == case["rows"], f"{case['id']}: {pc.rows} partial rows"
        cs = pc.vector()
    torch.cuda.synchronize()
    assert got_variant == _expect(case, igemm_path), f"{case['id']}: launched {got_variant}"
    _assert_equal(dx, ref, dtype, case, "dx", s, got_variant)
    if want_cs:
        want = torch.zeros((Cp,), dtype=torch.float64)
        want[:Cin] = R.column_sums(ref)
        assert torch.equal(cs.cpu().double(), want), f"{case['id']}: column sums differ at channels {(cs.cpu().double() != want).nonzero().flatten().tolist()[:8]}"


# ------------------------------------------------------------------------------------------------ weight gradient
def _run_wgrad(case, dev, igemm_path):
    N, H, W, Cin, Cout, Rf, s, p, G = case["geom"]
    dtype, flags = DT[case["dtype"]], case["op"].split("+")[1:]
    op = case["op"].split("+")[0]
    n_items = int(op[5:]) if len(op) > 5 else 0
    tr = "tr" in flags
    g = _seed(case)
    Cp, Kp = K.pad_channels(Cin), K.pad_channels(Cout)
    geom = K.make_geom(N, H, W, Cp, Kp, Rf, Rf, s, p)
    P, Q = geom.P, geom.Q
    items = []
    for _ in range(max(1, n_items)):
        x = R.activations((N, Cin, H, W), g)
        dy = R.gradients((N, Cout, P, Q), g, for_wgrad=True)
        # grouped: the slab-dense kernel computes, per 64-channel slab, the DENSE gradient of its output channels against the slab's
        # input channels (cs_wgrad_finalize_grouped reads the block diagonal): the reference is the ungrouped gradient
        ref = R.conv_wgrad(x, dy, Rf, Rf, s, p)
        R.assert_exact_domain(abs_sums=[R.conv_wgrad(x.abs(), dy.abs(), Rf, Rf, s, p)])
        items.append((_dev(x, Cp, dtype, dev), _dev(dy, Kp, dtype, dev), ref))
    if n_items:
        assert not K.wgrad2_serves(geom, dtype), f"{case['id']}: the second-generation weight gradient takes this geometry"
        slabs = K.wgrad_batched(geom, [i[0] for i in items], [i[1] for i in items], use_tr_read=tr)
    else:
        raw = K.new_wgrad_buffer(geom, dev, grouped=G > 1)
        raw.fill_(float("nan"))                          # every slab element must be overwritten by the kernel
        K.conv_wgrad(geom, items[0][0], items[0][1], raw, use_tr_read=tr, grouped=G > 1)
        slabs = raw.unsqueeze(0)
    got_variant = _variant()
    torch.cuda.synchronize()
    assert got_variant == _expect(case, igemm_path), f"{case['id']}: launched {got_variant}"
    for i, (_, _, ref) in enumerate(items):
        got = slabs[i].double().sum(0).cpu()             # [Kp][R][S][Cp | 64]
        want = torch.zeros((Kp, Rf, Rf, Cp), dtype=torch.float64)
        want[:Cout, :, :, :Cin] = ref.permute(0, 2, 3, 1)
        if G > 1:
            want = torch.stack([want[k, :, :, (k // 64) * 64:(k // 64) * 64 + 64] for k in range(Kp)])
        assert torch.equal(got, want), (f"{case['id']} item {i}: {int((got != want).sum())} of {got.numel()} elements differ, first at [k][r][s][c] = "
                                        f"{(got != want).nonzero()[0].tolist()}; {slabs.shape[1]} slices; {got_variant}")


# ------------------------------------------------------------------------------------------------ pixel-paired stem
def _run_stem(case, dev, igemm_path):
    N, H, W, Cin, Cout, Rf, s, p, G = case["geom"]
    dtype, flags = DT[case["dtype"]], case["op"].split("+")[1:]
    g = _seed(case)
    geom = K.make_geom(N, H, W, 8, Cout, 7, 7, 2, 3)
    assert K.is_stem_geom(geom) and Cin == 3
    x = R.activations((N, 3, H, W), g)
    xp = K.stem_pair_input(_dev(x, 8, dtype, dev))
    if case["op"].startswith("stem_fwd"):
        w = R.fwd_filters(Cout, 3, 7, 7, 12, g)
        shift = R.ints((Cout,), -8, 8, g)
        ref = R.conv_fwd(x, w, 2, 3, 1, None, shift)
        R.assert_exact_domain(stored=[ref], abs_sums=[R.conv_fwd(x.abs(), w.abs(), 2, 3, 1, None, shift.abs())], stats_of=ref if "stats" in flags else None)
        wk, _ = K.weight_prep(w.float().to(dev), None, dtype, 8, Cout, True, False)
        stats = K.new_stats(Cout, dev) if "stats" in flags else None
        y = K.stem_fwd(geom, xp, K.stem_pair_weights(wk), None, shift.float().to(dev), K.CS_ACT_NONE, stats=stats)
        got_variant = _variant()
        torch.cuda.synchronize()
        assert got_variant == _expect(case, igemm_path), f"{case['id']}: launched {got_variant}"
        _assert_equal(y, ref, dtype, case, "y", 1, got_variant)
        if stats is not None:
            assert _rows(N * geom.P * geom.Q, got_variant) == case["rows"]
            assert torch.equal(K.stats_values(stats).cpu(), R.channel_stats(ref)), f"{case['id']}: statistics"
        return
    dy = R.gradients((N, Cout, geom.P, geom.Q), g, for_wgrad=True)
    ref = R.conv_wgrad(x, dy, 7, 7, 2, 3)
    R.assert_exact_domain(abs_sums=[R.conv_wgrad(x.abs(), dy.abs(), 7, 7, 2, 3)])
    lib = _lib.load()
    nsplit = lib.cs_stem_wgrad_splits(N, H, W, Cout)
    pair = torch.full((nsplit, Cout, 7, 4, 8), float("nan"), dtype=torch.float32, device=dev)      # every paired slab element is overwritten
    _lib.check(lib.cs_stem_wgrad(N, H, W, Cout, K._code(dtype), K._p(xp), K._p(_dev(dy, Cout, dtype, dev)), K._p(pair), 1 if "tr" in flags else 0,
                                 K._stream()), "stem_wgrad")
    got_variant = _variant()
    raw = torch.empty((1, Cout, 7, 7, 8), dtype=torch.float32, device=dev)
    _lib.check(lib.cs_stem_unpair_slabs(K._p(pair), nsplit, Cout, K._p(raw), K._stream()), "stem_unpair_slabs")
    torch.cuda.synchronize()
    assert got_variant == _expect(case, igemm_path), f"{case['id']}: launched {got_variant}"
    want = torch.zeros((Cout, 7, 7, 8), dtype=torch.float64)
    want[..., :3] = ref.permute(0, 2, 3, 1)
    assert torch.equal(raw[0].cpu().double(), want), f"{case['id']}: {int((raw[0].cpu().double() != want).sum())} elements differ; {nsplit} slices"
    assert not bool(torch.isnan(pair).any()), f"{case['id']}: a paired slab element was not written"


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_first_generation_kernels_are_exact_on_integer_data(case, dev, igemm_path):
    op = case["op"].split("+")[0]
    if op == "fwd":
        _run_fwd(case, dev, igemm_path)
    elif op == "dgrad":
        _run_dgrad(case, dev, igemm_path)
    elif op.startswith("wgrad"):
        _run_wgrad(case, dev, igemm_path)
    elif op.startswith("stem"):
        _run_stem(case, dev, igemm_path)
    else:
        raise AssertionError(f"unknown operation {case['op']}")
