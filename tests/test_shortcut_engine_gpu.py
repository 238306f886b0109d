"""GPU: one bottleneck stage (a down-sampling block with a 1x1 projection shortcut, then an identity block) through the engine, bag of
2 at 35 x 35, eval-mode BN, bf16, with engine.FUSE_SHORTCUT on and off: output, input gradient and every parameter gradient.

The fused launch rounds the shortcut's product to bf16 in LDS exactly where the separate launch rounded it on its way to memory, and
adds it to the same fp32 sum, so at these extents (both passes on ring launches) the two passes owe the same bits: asserted with
torch.equal on normal data and on integer data (sparse +-1 / +-2 weights, inputs in -2..2, identity BN with integer shifts; every
tensor of the down-sampling block an integer of magnitude <= 256, asserted on an fp64 host forward, so that a difference there cannot
hide behind rounding).  On normal data the bounds tests/test_parity_bf16_gpu.py holds this library's bf16 step to against the
reference are checked as well -- 5e-2 of max|ref| on the output (its logits bound), cosine / relative L2 within ABS_COS_FLOOR /
ABS_REL_CEIL on every gradient -- and printed; equality implies them.
A no-grad forward gives the training forward's output; the step replayed through GraphedStep gives the eager step's bits."""
import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

import conv_ref as CR  # noqa: E402
from test_parity_bf16_gpu import ABS_COS_FLOOR, ABS_REL_CEIL  # noqa: E402

from cellsegmentation_amd import engine as E  # noqa: E402
from cellsegmentation_amd import kernels as K  # noqa: E402
from cellsegmentation_amd.graphed import GraphedStep  # noqa: E402
from cellsegmentation_amd.model import resnet as R  # noqa: E402

BF = torch.bfloat16
N, HW, CIN, PLANES = 2, 35, 128, 64
OUT_BOUND = 5e-2          # tests/test_parity_bf16_gpu.py: |logits - reference| <= 5e-2 max|reference|


class _Stage(nn.Module):
    def __init__(self):
        super().__init__()
        self.blocks = nn.ModuleList([R._Block("bottleneck", CIN, PLANES, 2), R._Block("bottleneck", 4 * PLANES, PLANES, 1)])


def _plan(stage):
    """the units model/resnet.py plans for a stage: conv1, conv2, [downsample], conv3 (+ residual) per block"""
    units, cur, nxt = [], 0, 1
    for bi, blk in enumerate(stage.blocks):
        x_in = cur
        for ci in (1, 2):
            units.append(E.ConvUnit(f"b{bi}.conv{ci}", getattr(blk, f"conv{ci}"), getattr(blk, f"bn{ci}"), E.ACT_RELU, cur, nxt))
            cur, nxt = nxt, nxt + 1
        res = x_in
        if blk.downsample is not None:
            res, nxt = nxt, nxt + 1
            units.append(E.ConvUnit(f"b{bi}.downsample", blk.downsample[0], blk.downsample[1], E.ACT_NONE, x_in, res))
        units.append(E.ConvUnit(f"b{bi}.conv3", blk.conv3, blk.bn3, E.ACT_RELU, cur, nxt, res=res))
        cur, nxt = nxt, nxt + 1
    return E.Plan(units, [0], [cur])


def _fill(stage, exact, g):
    with torch.no_grad():
        for mod in stage.modules():
            if isinstance(mod, nn.Conv2d):
                Kc, C, Rr, S = mod.weight.shape
                if exact:
                    mod.weight.copy_(CR.fwd_filters(Kc, C, Rr, S, 3, g).float())
                else:
                    mod.weight.copy_(torch.randn(mod.weight.shape, generator=g) * (2.0 / (C * Rr * S)) ** 0.5)
            elif isinstance(mod, nn.BatchNorm2d):
                C = mod.weight.numel()
                if exact:      # scale = 1 * (1 / sqrt(1 + 0)) = 1, shift = an integer
                    mod.eps = 0.0
                    mod.weight.fill_(1.0); mod.running_mean.zero_(); mod.running_var.fill_(1.0)
                    mod.bias.copy_(CR.ints((C,), -2, 1, g).float())
                else:
                    mod.weight.copy_(torch.rand((C,), generator=g) + 0.5); mod.bias.copy_(torch.randn((C,), generator=g) * 0.1)
                    mod.running_mean.copy_(torch.randn((C,), generator=g) * 0.1); mod.running_var.copy_(torch.rand((C,), generator=g) * 1.5 + 0.5)


def _host_forward_tensors(stage, x):
    """every tensor the forward of the down-sampling block stores (and the shortcut's output, which only the two-launch pass stores),
    in fp64 on the CPU"""
    stored, cur = [], x.double()
    for blk in stage.blocks[:1]:
        x_in = cur
        for ci in (1, 2):
            conv, bn = getattr(blk, f"conv{ci}"), getattr(blk, f"bn{ci}")
            cur = CR.conv_fwd(cur, conv.weight.detach().cpu(), conv.stride[0], conv.padding[0], shift=bn.bias.detach().cpu(), relu=True)
            stored.append(cur)
        res = x_in
        if blk.downsample is not None:
            conv, bn = blk.downsample
            res = CR.conv_fwd(x_in, conv.weight.detach().cpu(), conv.stride[0], 0, shift=bn.bias.detach().cpu())
            stored.append(res)
        pre = CR.conv_fwd(cur, blk.conv3.weight.detach().cpu(), 1, 0, shift=blk.bn3.bias.detach().cpu(), residual=res)
        stored.append(pre)
        cur = torch.relu(pre)
    return stored


def _setup(exact, dev):
    g = torch.Generator().manual_seed(2024 + int(exact))
    stage = _Stage()
    _fill(stage, exact, g)
    x = CR.ints((N, CIN, HW, HW), -2, 2, g).float() if exact else torch.randn((N, CIN, HW, HW), generator=g)
    if exact:
        CR.assert_exact_domain(stored=_host_forward_tensors(stage, x))
    stage = stage.to(dev)
    plan = _plan(stage)
    xd = x.permute(0, 2, 3, 1).contiguous().to(BF).to(dev)
    P = (HW - 1) // 2 + 1
    gout = torch.randint(-2, 3, (N, P, P, 4 * PLANES), generator=g).to(BF).to(dev)
    return stage, plan, xd, gout


def _step_fn(plan, gout):
    params = plan.param_tensors()

    def step(xb):
        xi = xb.detach().requires_grad_(True)
        y, = E.run_plan(plan, [xi], BF, bn_train=False)
        # (the engine's convention: the gradient of a post-ReLU tensor arrives already masked)
        grads = torch.autograd.grad(y, [xi] + params, grad_outputs=gout * (y.detach() > 0).to(BF))
        return (y.detach(),) + tuple(grads)
    return step


def _count_fused(monkeypatch):
    calls = []
    real = K.conv_fwd_shortcut_packed
    monkeypatch.setattr(K, "conv_fwd_shortcut_packed", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


@pytest.mark.parametrize("exact", [False, True], ids=["normal", "integers"])
def test_stage_is_the_same_with_and_without_the_fusion(dev, exact, monkeypatch):
    stage, plan, xd, gout = _setup(exact, dev)
    assert list(E.shortcut_pairs(plan, False).items()) == [(2, 3)]
    calls = _count_fused(monkeypatch)
    step = _step_fn(plan, gout)
    monkeypatch.setattr(E, "FUSE_SHORTCUT", True)
    a = [t.clone() for t in step(xd)]
    with torch.no_grad():
        y_nograd, = E.run_plan(plan, [xd], BF, bn_train=False)
        y_nograd = y_nograd.clone()
    assert len(calls) == 2, "the training and the no-grad forward both take the fused launch"
    monkeypatch.setattr(E, "FUSE_SHORTCUT", False)
    b = [t.clone() for t in step(xd)]
    torch.cuda.synchronize()
    assert len(calls) == 2 and len(a) == len(b) == 2 + len(plan.param_tensors())
    assert torch.equal(y_nograd, a[0]), "a no-grad forward stores the training forward's output"
    names = ["y", "dx"] + [f"{plan.units[ui].name}.{role}" for ui, role, _ in plan.param_list]
    if exact:
        bad = [n for n, s, t in zip(names, a, b) if not torch.equal(s, t)]
        assert not bad, bad
        return
    errs = []
    # (at these extents both passes run ring launches, and the fused one rounds the shortcut exactly as they do: the same bits)
    differ = [n for n, s, t in zip(names, a, b) if not torch.equal(s, t)]
    assert not differ, differ
    for n, s, t in zip(names, a, b):
        s, t = s.double().flatten(), t.double().flatten()
        if n == "y":
            d = float((s - t).abs().max() / t.abs().max())
            print(f"{n}: max |fused - two launches| / max |two launches| = {d:.3e} (bound {OUT_BOUND})")
            if not d <= OUT_BOUND:
                errs.append(f"{n}: {d}")
            continue
        cos = float(s @ t / (s.norm() * t.norm() + 1e-300))
        rel = float((s - t).norm() / (t.norm() + 1e-300))
        print(f"{n:24s} cos {cos:.6f} rel {rel:.3e}")
        if not (cos >= ABS_COS_FLOOR and rel <= ABS_REL_CEIL):
            errs.append(f"{n}: cos {cos:.4f} rel {rel:.3f}")
    assert not errs, errs


def test_graphed_stage_step_equals_eager_bit_for_bit(dev, monkeypatch):
    stage, plan, xd, gout = _setup(False, dev)
    calls = _count_fused(monkeypatch)
    step = _step_fn(plan, gout)
    g = torch.Generator().manual_seed(5)
    x2 = torch.randn(xd.shape, generator=g).to(BF).to(dev)
    eager = [[t.clone() for t in step(x)] for x in (xd, x2)]
    assert len(calls) == 2
    graphed = GraphedStep(step, (xd,), warmup=2)
    replayed = [[t.clone() for t in graphed(x)] for x in (xd, x2)]
    torch.cuda.synchronize()
    for e, r in zip(eager, replayed):
        assert len(e) == len(r) and all(torch.equal(s, t) for s, t in zip(e, r))
    assert not torch.equal(eager[0][0], eager[1][0])
