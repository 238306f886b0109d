"""GPU: the two-source ring forward (csrc/conv_v2.hip conv2_ring_kernel S2, cs_conv2d_fwd_shortcut_packed) -- the last 1x1 convolution
of a bottleneck and the block's 1x1 projection shortcut in one launch -- against the fp64 host
reference of tests/conv_ref.py and against the library's own two launches (shortcut, then the main convolution with a residual).

Exact cases: integer operands in -2..2, sparse +-1 / +-2 weights (12 per output channel and source), integer shifts in -8..8: every
pre-activation value is an integer of magnitude <= 2 * 12 * 2 * 2 + 16 = 112 (asserted on the reference: <= 256), so fp32 accumulation
is exact in any order, the shortcut's bf16 round trip of the two-launch path loses nothing, and all three results owe equality.
Random cases: the tolerance tests/test_conv_packed_gpu.py applies to a forward with residual (its TOL, relative to max|ref|); and,
because the launch rounds the shortcut's product to bf16 exactly where the two launches did, equality with those wherever both of
them ran on the ring kernel (the wide kernel sums two chunks at a time: another order)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import conv_ref as R  # noqa: E402
from test_conv_packed_gpu import TOL  # noqa: E402

from cellsegmentation_amd import _lib, kernels as K  # noqa: E402

BF = torch.bfloat16

#        N  Hs  Ws  stride Ca    Cb    K      what the case is there for (source B is [N][Hs][Ws][Cb]; P = (Hs - 1) / stride + 1)
CASES = [
    (1, 7, 6, 1, 64, 64, 256),        # chunks (1, 1): an epilogue every second step; stride 1; M = 42, less than one tile
    (2, 9, 9, 2, 64, 128, 128),       # (1, 2); stride 2 from an odd source, 9 -> 5; M = 50: no multiple of 32, less than one tile; one channel tile
    (2, 19, 19, 2, 128, 256, 256),    # (2, 4); 19 -> 10; M = 200: a full and a partial pixel tile
    (1, 11, 9, 1, 512, 1024, 128),    # (8, 16): the step wait covers the epilogue's operands
    (2, 95, 95, 2, 64, 64, 2048),     # K = 2048, 95 -> 48: 36 pixel tiles x 16 channel tiles > 512: a workgroup walks two pixel tiles (B -> A)
    (2, 95, 95, 2, 64, 128, 1024),    # 36 x 8 workgroups of 128 px in 257..512, 48 x 8 of 96 px <= 512: pick_tm answers 3
]
TM = [4, 4, 4, 4, 4, 3]
# (activation, bit plane, shift of the main convolution present, shift of the shortcut present)
CONFIGS = [
    (K.CS_ACT_RELU, True, True, True),
    (K.CS_ACT_NONE, False, True, True),
    (K.CS_ACT_RELU, False, False, True),
    (K.CS_ACT_NONE, True, True, False),
]
# every configuration on the four small cases, two each on the large ones
EXACT = [(ci, cf) for ci in range(4) for cf in range(4)] + [(4, 0), (4, 3), (5, 0), (5, 2)]


def _geoms(case):
    N, Hs, Ws, stride, Ca, Cb, Kc = case
    gv = K.make_geom(N, Hs, Ws, Cb, Kc, 1, 1, stride, 0)
    gm = K.make_geom(N, gv.P, gv.Q, Ca, Kc, 1, 1, 1, 0)
    return gm, gv


@functools.lru_cache(maxsize=None)
def _operands(ci, exact):
    """CPU operands (NCHW / KCRS) of a case and the fp64 products of both sources, computed once and shared (read-only)."""
    case = CASES[ci]
    N, Hs, Ws, stride, Ca, Cb, Kc = case
    gm, _ = _geoms(case)
    g = torch.Generator().manual_seed(4242 + 17 * ci + (0 if exact else 1000))
    if exact:
        z = R.ints((N, Ca, gm.P, gm.Q), -2, 2, g)
        x = R.ints((N, Cb, Hs, Ws), -2, 2, g)
        w3 = R.fwd_filters(Kc, Ca, 1, 1, 12, g)
        wd = R.fwd_filters(Kc, Cb, 1, 1, 12, g)
        s3 = R.ints((Kc,), -8, 8, g)
        sd = R.ints((Kc,), -8, 8, g)
    else:
        q = lambda t: t.to(BF).double()       # noqa: E731  (operands pre-rounded to bf16, as test_conv_packed_gpu.py does)
        z = q(torch.randn((N, Ca, gm.P, gm.Q), generator=g))
        x = q(torch.randn((N, Cb, Hs, Ws), generator=g))
        w3 = q(torch.randn((Kc, Ca, 1, 1), generator=g) / Ca ** 0.5)
        wd = q(torch.randn((Kc, Cb, 1, 1), generator=g) / Cb ** 0.5)
        s3 = (torch.randn((Kc,), generator=g) * 0.1).float().double()
        sd = (torch.randn((Kc,), generator=g) * 0.1).float().double()
    ya = R.conv_fwd(z, w3, 1, 0)
    yb = R.conv_fwd(x, wd, stride, 0)
    assert ya.shape == yb.shape
    abs_sum = R.conv_fwd(z.abs(), w3.abs(), 1, 0) + R.conv_fwd(x.abs(), wd.abs(), stride, 0) + s3.abs().view(1, -1, 1, 1) + sd.abs().view(1, -1, 1, 1)
    return z, x, w3, wd, s3, sd, ya, yb, abs_sum


def _nhwc(t, dev):
    return t.permute(0, 2, 3, 1).contiguous().to(BF).to(dev)


def _from_nhwc(t):
    return t.double().cpu().permute(0, 3, 1, 2).contiguous()


def _packed(geom, w, dev):
    w_khwc, _ = K.weight_prep(w.float().to(dev), None, BF, geom.C, geom.K, want_fwd=True, want_bwd=False)
    return K.pack_conv_weights(geom, w_khwc, dgrad=False)


def _run(ci, cf, exact, dev, two_launch):
    case = CASES[ci]
    act, want_bits, has3, hasd = CONFIGS[cf]
    z, x, w3, wd, s3, sd, ya, yb, abs_sum = _operands(ci, exact)
    gm, gv = _geoms(case)
    assert K.conv_fwd_shortcut_supported(gm, gv, BF)
    pre = ya + yb
    if has3:
        pre = pre + s3.view(1, -1, 1, 1)
    if hasd:
        pre = pre + sd.view(1, -1, 1, 1)
    ref = torch.relu(pre) if act == K.CS_ACT_RELU else pre
    if exact:
        # the condition of the equalities below, on the reference itself: integers of magnitude <= 256, partial sums below 2^24
        r_two = yb + (sd.view(1, -1, 1, 1) if hasd else 0)
        R.assert_exact_domain(stored=[pre, r_two], abs_sums=[abs_sum])
        assert float(pre.abs().max()) <= 256
    zd, xd = _nhwc(z, dev), _nhwc(x, dev)
    wp3, wpd = _packed(gm, w3, dev), _packed(gv, wd, dev)
    s3d = s3.float().to(dev) if has3 else None
    sdd = sd.float().to(dev) if hasd else None
    out = K.conv_fwd_shortcut_packed(gm, zd, wp3, s3d, gv, xd, wpd, sdd, act, want_bits=want_bits)
    variant = (_lib.load().cs_last_conv_variant() or b"").decode()
    y, bits = out if want_bits else (out, None)
    y2 = None
    _run.two_on_ring = False
    if two_launch:
        last = lambda: (_lib.load().cs_last_conv_variant() or b"").decode()       # noqa: E731
        r = K.conv_fwd_packed(gv, xd, wpd, sdd, None, K.CS_ACT_NONE)
        v1 = last()
        y2 = K.conv_fwd_packed(gm, zd, wp3, s3d, r, act)
        _run.two_on_ring = v1.startswith("conv2_ring_kernel<") and last().startswith("conv2_ring_kernel<")
    torch.cuda.synchronize()
    assert variant == f"conv2_ring_kernel<{TM[ci]},1,4,false,false,true>", variant
    return ref, y, bits, y2, gm


@pytest.mark.parametrize("ci,cf", EXACT)
def test_two_source_forward_is_exact_on_integer_data(ci, cf, dev):
    ref, y, bits, y2, gm = _run(ci, cf, True, dev, two_launch=True)
    got = _from_nhwc(y)
    assert torch.equal(got, ref), f"max diff {float((got - ref).abs().max())} at {int((got != ref).sum())} elements"
    assert torch.equal(y, y2), "fused and two-launch outputs differ"
    if bits is not None:
        assert torch.equal(K.unpack_bits(bits, gm.K).cpu().permute(0, 3, 1, 2), ref > 0)


@pytest.mark.parametrize("ci,cf", [(0, 2), (1, 0), (2, 1), (3, 0), (4, 0), (5, 3)])
def test_two_source_forward_on_random_data(ci, cf, dev):
    ref, y, bits, y2, gm = _run(ci, cf, False, dev, two_launch=True)
    got = _from_nhwc(y)
    assert _run.two_on_ring or ci == 3, "only the deep stride-1 contractions of case 3 may take the wide kernel"
    if _run.two_on_ring:
        assert torch.equal(y, y2), f"fused and two-launch outputs differ at {int((y != y2).sum())} elements"
    err = float((got - ref).abs().max() / (ref.abs().max() + 1e-12))
    print(f"case {CASES[ci]}: relative error {err:.3e} (bound {TOL})")
    assert err < TOL
    if bits is not None:
        assert torch.equal(K.unpack_bits(bits, gm.K).cpu().permute(0, 3, 1, 2), got > 0)
