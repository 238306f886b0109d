"""CPU: the two-source ring forward (cs_conv2d_fwd_shortcut_packed, csrc/conv_v2.hip) -- what its planner serves and declines, the
argument checks of the entry point (nothing is launched), and which unit pairs of the ResNet / ResNeXt plans the engine hands to it."""
import ctypes
import os
import re

import torch

from cellsegmentation_amd import _lib, engine as E, kernels as K
from cellsegmentation_amd.model import resnet as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cs_conv2d_fwd_shortcut_supported", "cs_conv2d_fwd_shortcut_packed")
BF = torch.bfloat16


def _pair(N, Hs, Ws, stride, Ca, Cb, Kc, Kb=None, pad_b=0):
    gv = K.make_geom(N, Hs, Ws, Cb, Kc if Kb is None else Kb, 1, 1, stride, pad_b)
    gm = K.make_geom(N, (Hs - 1) // stride + 1, (Ws - 1) // stride + 1, Ca, Kc, 1, 1, 1, 0)
    return gm, gv


def test_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "cellseg_hip.h")).read()
    lib = _lib.load()
    for name in NAMES:
        assert re.search(rf"\bint {name}\s*\(", header), name
        assert name in _lib._SIGNATURES and name in _lib.exported_symbols() and hasattr(lib, name)
    assert callable(K.conv_fwd_shortcut_packed) and callable(K.conv_fwd_shortcut_supported)
    assert E.FUSE_SHORTCUT is True


def test_planner_decisions():
    ok = lambda gm, gv: K.conv_fwd_shortcut_supported(gm, gv, BF)      # noqa: E731
    # the four down-sampling blocks of ResNet-50 at the classifier's bag of 64 tiles of 299 x 299
    for Hs, stride, Ca, Cb, Kc in ((75, 1, 64, 64, 256), (75, 2, 128, 256, 512), (38, 2, 256, 512, 1024), (19, 2, 512, 1024, 2048)):
        assert ok(*_pair(64, Hs, Hs, stride, Ca, Cb, Kc)), (Hs, stride, Ca, Cb, Kc)
    assert ok(*_pair(1, 7, 6, 1, 64, 64, 128)) and ok(*_pair(2, 9, 9, 2, 64, 128, 128))
    assert not K.conv_fwd_shortcut_supported(*_pair(1, 7, 6, 1, 64, 64, 128), torch.float32)
    # declined: the two outputs differ in K; K = 64 (no 128-channel tile); stride 3; a padded shortcut; a contraction that is no multiple of 64
    assert not ok(*_pair(1, 8, 8, 1, 64, 64, 256, Kb=128))
    assert not ok(*_pair(1, 8, 8, 1, 64, 64, 64))
    assert not ok(*_pair(1, 9, 9, 3, 64, 64, 128))
    gm, _ = _pair(1, 8, 8, 1, 64, 64, 128)
    assert not ok(gm, K.make_geom(1, 6, 6, 64, 128, 1, 1, 1, 1))              # 6 + 2 * 1 = 8: the extents agree, the padding is refused
    assert not ok(*_pair(1, 8, 8, 1, 96, 64, 128)) and not ok(*_pair(1, 8, 8, 1, 64, 32, 128))
    # also: other pixel grids, a strided main convolution, a 3x3, one destination row under stride 2, a source beyond 31 bits
    assert not ok(gm, K.make_geom(1, 9, 8, 64, 128, 1, 1, 1, 0))
    assert not ok(K.make_geom(1, 15, 15, 64, 128, 1, 1, 2, 0), K.make_geom(1, 15, 15, 64, 128, 1, 1, 2, 0))
    assert not ok(K.make_geom(1, 8, 8, 64, 128, 3, 3, 1, 1), K.make_geom(1, 8, 8, 64, 128, 1, 1, 1, 0))
    assert not ok(*_pair(4, 1, 9, 2, 64, 64, 128))
    assert ok(*_pair(64, 150, 150, 2, 64, 256, 128)) and not ok(*_pair(256, 300, 300, 2, 64, 256, 128))       # 0.74 GB / 11.8 GB of block input
    lib = _lib.load()
    assert lib.cs_conv2d_fwd_shortcut_supported(None, ctypes.byref(gm)) == 0 and lib.cs_conv2d_fwd_shortcut_supported(ctypes.byref(gm), None) == 0


def test_argument_errors_without_a_launch():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    ptr = ctypes.c_void_p(ctypes.addressof(buf))
    gm, gv = _pair(1, 7, 6, 1, 64, 64, 128)
    a, b = ctypes.byref(gm), ctypes.byref(gv)
    call = lib.cs_conv2d_fwd_shortcut_packed
    assert call(None, ptr, ptr, None, b, ptr, ptr, None, 0, ptr, None, None) == -1 and b"NULL geometry" in lib.cs_last_error()
    assert call(a, ptr, ptr, None, None, ptr, ptr, None, 0, ptr, None, None) == -1 and b"NULL geometry" in lib.cs_last_error()
    for hole in range(5):
        t = [ptr] * 5
        t[hole] = None
        x, w, x_in, w_sc, y = t
        assert call(a, x, w, None, b, x_in, w_sc, None, 0, y, None, None) == -1
        assert lib.cs_last_error() == b"conv2d_fwd_shortcut_packed: NULL tensor"
    assert call(a, ptr, ptr, None, b, ptr, ptr, None, K.CS_ACT_SILU, ptr, None, None) == -1 and b"activation" in lib.cs_last_error()
    gm64, gv64 = _pair(1, 7, 6, 1, 64, 64, 64)
    rc = call(ctypes.byref(gm64), ptr, ptr, None, ctypes.byref(gv64), ptr, ptr, None, 0, ptr, None, None)
    assert rc != 0 and b"not served" in lib.cs_last_error()


def _encoder_plan(make):
    m = make()
    return m, m._encoder_plan(False)


def test_engine_eligibility_on_the_model_plans(monkeypatch):
    for make in (R.MILresnet50, R.MILresnext50_32x4d):
        m, plan = _encoder_plan(make)
        m.eval()
        pairs = E.shortcut_pairs(plan, bn_train=True)          # (eval-mode modules: nothing runs on batch statistics)
        names = [(plan.units[vi].name, plan.units[ui].name) for vi, ui in sorted(pairs.items())]
        assert names == [(f"layer{i}.0.downsample", f"layer{i}.0.conv3") for i in (1, 2, 3, 4)], names
        assert E.shortcut_pairs(plan, bn_train=False) == pairs                 # freeze_bn
        # ... and the library serves each of them at the classifier's tile size (the geometry ConvUnit.fwd asks with)
        hw = 75
        for i, (vi, ui) in enumerate(sorted(pairs.items())):
            v, u = plan.units[vi], plan.units[ui]
            s = v.conv.stride[0]
            gv = K.make_geom(2, hw, hw, v.conv.in_channels, v.conv.out_channels, 1, 1, s, 0)
            gm = K.make_geom(2, gv.P, gv.Q, u.conv.in_channels, u.conv.out_channels, 1, 1, 1, 0)
            assert K.conv_fwd_shortcut_supported(gm, gv, BF), (v.name, u.name)
            hw = gv.P
        m.train()
        assert E.shortcut_pairs(plan, bn_train=True) == {}, "batch statistics: the two launches"
        assert E.shortcut_pairs(plan, bn_train=False) == pairs
        monkeypatch.setattr(E, "FUSE_SHORTCUT", False)
        assert E.shortcut_pairs(plan, bn_train=False) == {}
        monkeypatch.setattr(E, "FUSE_SHORTCUT", True)
        monkeypatch.setattr(E, "PACKED", False)
        assert E.shortcut_pairs(plan, bn_train=False) == {}
        monkeypatch.setattr(E, "PACKED", True)
    # basic blocks end in a 3x3: no pair
    m, plan = _encoder_plan(R.MILresnet18)
    m.eval()
    assert E.shortcut_pairs(plan, bn_train=False) == {}


def test_a_shortcut_with_another_reader_or_an_activation_keeps_its_launch():
    m, plan = _encoder_plan(R.MILresnet50)
    m.eval()
    pairs = E.shortcut_pairs(plan, False)
    vi, ui = sorted(pairs.items())[0]
    v = plan.units[vi]
    # the shortcut's output is also a plan output
    assert vi not in E.shortcut_pairs(E.Plan(plan.units, plan.inputs, plan.outputs + [v.dst]), False)
    # a second reader
    extra = E.PoolUnit(v.dst, 10 ** 6)
    assert vi not in E.shortcut_pairs(E.Plan(plan.units + [extra], plan.inputs, plan.outputs), False)
    # the shortcut planned before the block's first two convolutions: the main convolution's input does not exist yet when it runs
    units = list(plan.units)
    units.insert(vi - 2, units.pop(vi))
    moved = E.Plan(units, plan.inputs, plan.outputs)
    assert moved.units[vi - 2] is v and (vi - 2) not in E.shortcut_pairs(moved, False) and len(E.shortcut_pairs(moved, False)) == len(pairs) - 1
    # an activation on the shortcut
    v.act = E.ACT_RELU
    try:
        assert vi not in E.shortcut_pairs(E.Plan(plan.units, plan.inputs, plan.outputs), False)
    finally:
        v.act = E.ACT_NONE
