"""GPU: the stem forward fused with its max-pool (csrc/stem_pool.hip, kernels.stem_pool_fwd) gives the VALUES of the two launches it
replaces -- cs_stem_fwd_packed (ring kernel, gathered rows) then cs_maxpool3x3s2_fwd --, pooled map and tap plane, with torch.equal;
and a ResNet step through the engine is the same with engine.FUSE_STEM_POOL on and off.

Shapes (N, H, W) are chosen for edges, not size: the smallest served; even everywhere; odd W with the last pool window half outside
the stem map; several tiles both ways with ragged last tiles; pooled extents (6, 16), one more than a multiple of the 5 x 15 tile both
ways.  Two draws per shape: bf16 normal data under a shift that is negative on some channels (whole windows tie at zero), and the
ledger's exact draw (integers |x| <= 4, |w| <= 1: every fp32 sum is exact, non-zero ties are common), the latter also held to an fp64
conv2d -> relu -> bf16 -> max-pool on the CPU under tests/pool_ref.py's tap rule."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pool_ref as PR  # noqa: E402
from cellsegmentation_amd import engine as E  # noqa: E402
from cellsegmentation_amd import functional as HF  # noqa: E402
from cellsegmentation_amd import kernels as K  # noqa: E402
from cellsegmentation_amd import synth  # noqa: E402
from cellsegmentation_amd.model import resnet as R  # noqa: E402

SHAPES = [(1, 7, 9), (2, 32, 32), (3, 37, 41), (1, 67, 131), (2, 23, 63)]
KC = 64


def _draw(shape, kind):
    """(x[N,3,H,W], w[64,3,7,7], shift[64]) in fp32 on the CPU"""
    N, H, W = shape
    seed = 1000 * H + W
    if kind == "exact":
        x = PR.ints((N, 3, H, W), seed, -4, 4).float()
        w = PR.ints((KC, 3, 7, 7), seed + 1, -1, 1).float()
        shift = PR.ints((KC,), seed + 2, -6, 6).float()
    else:
        g = torch.Generator().manual_seed(seed)
        x = torch.randn((N, 3, H, W), generator=g)
        w = torch.randn((KC, 3, 7, 7), generator=g) * 0.1
        shift = torch.randn((KC,), generator=g)
        shift[::5] = -50.0                           # these channels are zero after the ReLU: every window ties, the first valid tap stands
    return x, w, shift


@pytest.mark.parametrize("kind", ["normal", "exact"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fused_stem_pool_equals_the_two_launches(dev, shape, kind):
    N, H, W = shape
    geom = K.make_geom(N, H, W, 8, KC, 7, 7, 2, 3)
    assert K.stem_pool_fwd_supported(geom, torch.bfloat16) and K.stem_fwd_packed_supported(geom, torch.bfloat16)
    x, w, shift = _draw(shape, kind)
    x8 = torch.zeros((N, H, W, 8))
    x8[..., :3] = x.permute(0, 2, 3, 1)
    xp = K.stem_pair_input(x8.to(dev).to(torch.bfloat16))
    wk, _ = K.weight_prep(w.to(dev), None, torch.bfloat16, 8, KC, True, False)
    wp = K.stem_pair_weights(wk)
    sh = shift.to(dev)
    z = K.stem_fwd_packed(geom, xp, K.stem_pack_weights(wp), sh, K.CS_ACT_RELU)
    y_ref, am_ref = K.maxpool_fwd(z, want_argmax=True)
    y, am = K.stem_pool_fwd(geom, xp, wp, sh, want_argmax=True)
    from cellsegmentation_amd import _lib
    variant = (_lib.load().cs_last_conv_variant() or b"").decode()
    y_only, none = K.stem_pool_fwd(geom, xp, wp, sh, want_argmax=False)
    torch.cuda.synchronize()
    assert variant.startswith("stem_pool_fwd_kernel<") and none is None
    assert y.shape == y_ref.shape and am.shape == am_ref.shape and am.dtype == torch.uint8
    assert torch.equal(y, y_ref)
    assert torch.equal(am, am_ref)
    assert torch.equal(y_only, y_ref)
    if kind == "exact":
        # fp64 on the CPU: exact integers; the one rounding to bf16 comes before the pool, as in the kernels
        s = torch.nn.functional.conv2d(x.double(), w.double(), stride=2, padding=3) + shift.double()[None, :, None, None]
        s = torch.relu(s).float().to(torch.bfloat16)
        want_y, want_tap = PR.maxpool_fwd(s)
        assert torch.equal(y.cpu().double().permute(0, 3, 1, 2), want_y)
        assert torch.equal(am.cpu().long().permute(0, 3, 1, 2), want_tap)


def _model(arch, dev):
    m = {"resnet18": R.MILresnet18, "resnet50": R.MILresnet50}[arch]()
    sd = m.state_dict()
    synth.fill_state_dict(sd)
    m.load_state_dict(sd)
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    return m.to(dev).set_compute_dtype(torch.bfloat16)


@pytest.mark.parametrize("arch", ["resnet18", "resnet50"])
def test_engine_step_is_the_same_with_and_without_the_fusion(dev, arch, monkeypatch):
    """tile mode, bf16, freeze_bn, the whole trunk training: logits, loss and every parameter gradient, then the eval forward."""
    m = _model(arch, dev)
    m.setmode("tile")
    m.set_encoder_grads(True)
    g = torch.Generator().manual_seed(11)
    x = torch.randn((2, 3, 75, 77), generator=g).to(dev)
    y = torch.tensor([1, 0], device=dev)
    fused_calls = []
    real = K.stem_pool_fwd
    monkeypatch.setattr(K, "stem_pool_fwd", lambda *a, **k: (fused_calls.append(1), real(*a, **k))[1])

    def step(flag):
        monkeypatch.setattr(E, "FUSE_STEM_POOL", flag)
        m.train()
        m.zero_grad(set_to_none=True)
        logits = m(x, freeze_bn=True)
        loss = HF.cross_entropy(logits, y)
        loss.backward()
        grads = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
        m.eval()
        with torch.no_grad():
            ev = m(x).clone()
        torch.cuda.synchronize()
        return logits.detach().clone(), loss.detach().clone(), grads, ev

    a = step(True)
    assert len(fused_calls) == 2, "the training and the eval forward both take the fused launch"
    b = step(False)
    assert len(fused_calls) == 2
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[3], b[3])
    assert a[2].keys() == b[2].keys() and len(a[2]) > 10
    bad = [k for k in a[2] if not torch.equal(a[2][k], b[2][k])]
    assert not bad, bad[:8]
