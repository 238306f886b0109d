"""GPU: the weight-staging entries of csrc/prep.hip (K.weight_prep = cs_weight_prep, K.stage_layer = cs_stage_conv_bn_one) against the
operands' definition in torch (conv_ref.staged_operands), bit for bit.

Every entry runs ONE kernel body, so none of them can serve as the other's reference.  A staged element is one fp32 product
w * scale[k] rounded once to the operand dtype: torch's elementwise multiply and its round-to-nearest-even conversion are that
definition, so the bound is equality of the bits, padding (exact zeros) included.  The folded scale / shift / rstd rows are held
against cs_bn_fold, a separate kernel with the same expressions; the packed orders against cs_pack_conv_weights applied to the torch
reference.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from conv_ref import same_bits, staged_operands  # noqa: E402

from cellsegmentation_amd import kernels as K  # noqa: E402

BF, F32 = torch.bfloat16, torch.float32

#        K    Cin  R   Cp   Kp
SHAPES = [
    (64, 3, 7, 8, 64),            # the stem: 3 input channels stored as 8
    (20, 16, 3, 16, 24),          # K not a multiple of 8: padded filter rows
    (20, 24, 1, 24, 24),          # the same, 1x1
    (64, 256, 1, 256, 64),        # unpadded 1x1 (bf16: through the LDS tile)
    (128, 64, 3, 64, 128),        # unpadded 3x3 (bf16: through the LDS tile)
    (120, 60, 3, 64, 128),        # both extents padded up to packable ones
    (512, 512, 3, 512, 512),      # 2.4 M staged elements per operand: above the 2^21 of the former tiled kernel, unpadded
    (516, 515, 3, 520, 520),      # above it with both extents padded (element-wise path on a large tensor)
]


def _weights(K_, Cin, R, dev, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn((K_, Cin, R, R), generator=g) / (Cin * R * R) ** 0.5
    scale = torch.rand((K_,), generator=g) + 0.5
    return w.to(dev), scale.to(dev)


@pytest.mark.parametrize("want_bwd", [False, True])
@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES)
def test_weight_prep_equals_the_torch_definition(shape, dtype, scaled, want_bwd, dev):
    K_, Cin, R, Cp, Kp = shape
    w, scale = _weights(K_, Cin, R, dev, 11 + K_ + Cin + R)
    if not scaled:
        scale = None
    t_khwc, t_chwk = staged_operands(w, scale, dtype, Cp, Kp)
    w_khwc, w_chwk = K.weight_prep(w, scale, dtype, Cp, Kp, want_fwd=True, want_bwd=want_bwd)
    torch.cuda.synchronize()
    assert tuple(w_khwc.shape) == (Kp, R, R, Cp) and same_bits(w_khwc, t_khwc)
    assert bool((w_khwc[K_:] == 0).all()) and bool((w_khwc[..., Cin:] == 0).all()), "padding must be exact zeros"
    if want_bwd:
        assert tuple(w_chwk.shape) == (Cp, R, R, Kp) and same_bits(w_chwk, t_chwk)
        assert bool((w_chwk[Cin:] == 0).all()) and bool((w_chwk[..., K_:] == 0).all()), "padding must be exact zeros"
    else:
        assert w_chwk is None
        only_bwd = K.weight_prep(w, scale, dtype, Cp, Kp, want_fwd=False, want_bwd=True)       # the data-gradient operand alone
        torch.cuda.synchronize()
        assert only_bwd[0] is None and same_bits(only_bwd[1], t_chwk)


def _layer(K_, Cin, R, bias, fold, dev, seed):
    torch.manual_seed(seed)
    conv = torch.nn.Conv2d(Cin, K_, R, 1, R // 2, bias=bias).to(dev)
    bn = None
    if fold:
        bn = torch.nn.BatchNorm2d(K_).to(dev)
        with torch.no_grad():
            bn.weight.uniform_(0.5, 1.5); bn.bias.normal_(); bn.running_mean.normal_(); bn.running_var.uniform_(0.5, 2.0)
    return conv, bn


@pytest.mark.parametrize("want_bwd", [False, True])
@pytest.mark.parametrize("fold", [False, True], ids=["plain", "fold"])
@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES)
def test_stage_layer_equals_the_torch_definition_and_bn_fold(shape, dtype, fold, want_bwd, dev):
    """One launch: operands as the torch definition gives them from cs_bn_fold's scale; the scale / shift / rstd rows equal
    cs_bn_fold's bit for bit, rows k >= K are zero.  Without a BatchNorm: scale = rstd = 1, shift = the convolution's bias or 0."""
    K_, Cin, R, Cp, Kp = shape
    bias = (K_ + R) % 2 == 0 or not fold            # both bias settings occur among the fold cases; every plain case has one
    conv, bn = _layer(K_, Cin, R, bias, fold, dev, 5 + K_ + Cin + R)
    w = conv.weight.detach()
    b = conv.bias.detach() if bias else None
    if fold:
        scale_ref, shift_ref, rstd_ref = K.bn_fold(bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var, bn.eps, b)
    else:
        scale_ref, shift_ref, rstd_ref = torch.ones_like(b), b, torch.ones_like(b)
    t_khwc, t_chwk = staged_operands(w, scale_ref if fold else None, dtype, Cp, Kp)
    w_khwc, w_chwk, scale, shift, rstd = K.stage_layer(conv, bn, dtype, Cp, Kp, want_bwd=want_bwd)
    torch.cuda.synchronize()
    assert same_bits(w_khwc, t_khwc)
    assert bool((w_khwc[K_:] == 0).all()) and bool((w_khwc[..., Cin:] == 0).all()), "padding must be exact zeros"
    if want_bwd:
        assert same_bits(w_chwk, t_chwk)
        assert bool((w_chwk[Cin:] == 0).all()) and bool((w_chwk[..., K_:] == 0).all()), "padding must be exact zeros"
    else:
        assert w_chwk is None
    for got, ref in ((scale, scale_ref), (shift, shift_ref), (rstd, rstd_ref)):
        assert tuple(got.shape) == (Kp,) and same_bits(got[:K_].contiguous(), ref.contiguous())
        assert same_bits(got[K_:].contiguous(), torch.zeros_like(got[K_:])), "rows k >= K must be zero"


#                K    Cin  R   Cp   Kp
@pytest.mark.parametrize("shape", [(128, 64, 3, 64, 128), (64, 256, 1, 256, 64), (120, 60, 3, 64, 128), (64, 3, 1, 64, 64)])
@pytest.mark.parametrize("fold", [False, True], ids=["plain", "fold"])
def test_stage_layer_writes_the_packed_orders(shape, fold, dev):
    """fwd_packed / bwd_packed: the MFMA-fragment order, from the LDS tile (unpadded layers) and element by element (padded ones),
    equals cs_pack_conv_weights of the torch reference."""
    K_, Cin, R, Cp, Kp = shape
    conv, bn = _layer(K_, Cin, R, False, fold, dev, 9 + K_ + Cin + R)
    scale_ref = K.bn_fold(bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var, bn.eps)[0] if fold else None
    t_khwc, t_chwk = staged_operands(conv.weight.detach(), scale_ref, BF, Cp, Kp)
    geom = K.make_geom(2, 19, 19, Cp, Kp, R, R, 1, R // 2)
    ref_f = K.pack_conv_weights(geom, t_khwc, dgrad=False)
    ref_b = K.pack_conv_weights(geom, t_chwk, dgrad=True)
    w_f, w_b = K.stage_layer(conv, bn, BF, Cp, Kp, want_bwd=True, fwd_packed=True, bwd_packed=True)[:2]
    u_f, u_b = K.stage_layer(conv, bn, BF, Cp, Kp, want_bwd=True, fwd_packed=True, bwd_packed=False)[:2]      # mixed orders
    torch.cuda.synchronize()
    assert same_bits(w_f, ref_f) and same_bits(w_b, ref_b)
    assert same_bits(u_f, ref_f) and same_bits(u_b, t_chwk)


def test_stage_layer_refuses_what_it_cannot_pack(dev):
    conv, _ = _layer(20, 16, 3, False, False, dev, 1)
    with pytest.raises(ValueError, match="packed layouts"):
        K.stage_layer(conv, None, BF, 16, 24, want_bwd=True, fwd_packed=True)
