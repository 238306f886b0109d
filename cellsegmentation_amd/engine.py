"""Plan executor: the explicit forward/backward kernel schedule of a CNN trunk on MI355X.

A *plan* is a list of fused units over numbered tensor slots (NHWC, bf16 or fp32):

* ``ConvUnit``     Conv2d (+bias) [+ BatchNorm2d] [+ residual add] [+ ReLU]
                   - BN in eval mode (``freeze_bn`` / ``model.eval()``): BN is folded into the
                     staged weights + a per-channel shift, everything fused in the conv epilogue;
                     its backward derives dgamma/dbeta from the raw weight gradient (no conv
                     output is kept).
                   - BN in train mode: conv (+fused per-channel fp64 statistics) -> finalize ->
                     normalise+residual+ReLU kernel; backward = 2-pass BN backward + dgrad/wgrad.
* ``PoolUnit``     MaxPool2d(3,2,1)
* ``UpsampleUnit`` bilinear, align_corners=True
* ``ConcatUnit``   channel concat

Gradient convention: a gradient w.r.t. a post-ReLU tensor is always stored already multiplied
by [tensor > 0]; the kernel producing the LAST contribution to a slot applies the mask (dgrad and
bilinear-backward epilogues), so ReLU backward never costs a separate pass, and residual
gradients are passed as the ``add`` operand of the dgrad epilogue instead of a separate add.

Each unit has a forward step ``fwd`` and a backward step ``bwd``; ``_Forward`` / ``_Backward`` hold the state of a pass.
The whole plan is ONE torch.autograd.Function: torch only sees (inputs, parameters) -> outputs.
"""
from collections import namedtuple
from types import SimpleNamespace

import torch

from . import _capture
from . import kernels as K

ACT_NONE, ACT_RELU, ACT_SILU = K.CS_ACT_NONE, K.CS_ACT_RELU, K.CS_ACT_SILU

PACKED = True              # packed-operand conv kernels (False: first-generation igemm everywhere; tests flip it for a reference path)
PACKED_TRAIN_BN = True     # ... also for heavy 3x3 convolutions under batch-statistics BN
FUSE_STEM_POOL = True      # eval-BN bf16 stem + ReLU + the max-pool behind it in one launch (False: the two launches; tests compare the two)
FUSE_SHORTCUT = True       # eval-BN bf16 1x1 projection shortcut inside the block's last 1x1 forward (False: the two launches; tests compare the two)


class ConvUnit:
    kind = "conv"

    def __init__(self, name, conv, bn, act, src, dst, res=None):
        self.name, self.conv, self.bn, self.act = name, conv, bn, act
        self.src, self.dst, self.res = src, dst, res
        self.grouped = conv.groups != 1
        if self.grouped:
            cg = conv.in_channels // conv.groups
            if conv.in_channels != conv.out_channels or conv.in_channels % 64 != 0 or 64 % cg != 0 or conv.bias is not None:
                raise NotImplementedError(f"{name}: grouped convolution needs C == K, C % 64 == 0, (C/groups) | 64, no bias "
                                          "(the ResNeXt 32x4d / 32x8d 3x3 layers)")
        self._cache = None

    def params(self):
        out = [("weight", self.conv.weight)]
        if self.conv.bias is not None:
            out.append(("bias", self.conv.bias))
        if self.bn is not None:
            out += [("gamma", self.bn.weight), ("beta", self.bn.bias)]
        return out

    def inputs(self):
        return [self.src] + ([self.res] if self.res is not None else [])

    def fwd(self, f, ui):
        x = f.t[self.src]
        N, H, W, Cp = x.shape
        conv = self.conv
        Kp = K.pad_channels(conv.out_channels)
        R, S = conv.kernel_size
        geom = K.make_geom(N, H, W, Cp, Kp, R, S, conv.stride[0], conv.padding[0])
        # (a projection shortcut fused into this launch left its operands instead of a residual tensor: see below)
        sc = f.fused_sc.pop(ui, None)
        res = f.t[self.res] if (self.res is not None and sc is None) else None
        batch_stats = _bn_uses_batch_stats(self.bn, f.bn_train)
        st = f.staged(ui, self, geom, batch_stats)
        # the stem runs on a pixel-paired image (kernels.stem_*): 28 instead of 49 K chunks
        stem = _is_paired_stem(self) and K.is_stem_geom(geom)
        xp = wp = None
        if ui == 0 and f.nchw_for_stem is not None:
            if not stem:
                raise RuntimeError("engine: the stem was expected to take the NCHW image (placeholder input would be read)")
            xp = K.stem_pair_from_nchw(f.nchw_for_stem, f.dtype)
        elif stem:
            xp = K.stem_pair_input(x)
        if stem:
            wp = K.stem_pair_weights(st.w_khwc)
        if batch_stats:
            stats = f.take_stats(Kp)
            if stem:
                z = K.stem_fwd(geom, xp, wp, None, st.shift, ACT_NONE, stats=stats)
            elif st.fwd_packed:
                # halo kernel + one statistics pass over the stored z (the statistics of exactly the values bn_apply normalises)
                z = K.conv_fwd_packed(geom, x, st.w_khwc, st.shift, None, ACT_NONE)
                K.bn_stats(z, stats)
            else:
                z = K.conv_fwd(geom, x, st.w_khwc, None, st.shift, None, ACT_NONE, stats=stats, grouped=self.grouped)
            y, mean, rstd = f.bn_train_fwd(self.bn, z, stats, res, self.act)
            f.aux[ui] = SimpleNamespace(geom=geom, st=st, train=True, z=z if f.save else None, mean=mean, rstd=rstd, xp=xp)
        else:
            # one bit per output next to a ReLU output of a pass that will run backward: the data gradient that later masks with
            # this tensor reads 1 byte per 16 (the bf16 masks are ~1/8 of a training step's HBM traffic)
            want_bits = f.save and self.act == ACT_RELU
            main_ui = f.sc_pairs.get(ui)
            if main_ui is not None and st.fwd_packed:
                # this unit is the 1x1 projection shortcut of a block whose last 1x1 convolution (unit main_ui) is its only reader:
                # that launch multiplies both (kernels.conv_fwd_shortcut_packed).  Staged here, aux recorded for backward (which
                # needs the block input and the incoming gradient only), the slot never materialised.  The operands travel in
                # fused_sc, so the block input outlives its release in a no-grad pass until the main unit has run.
                um = f.plan.units[main_ui]
                zN, zH, zW, zC = f.t[um.src].shape
                gm = K.make_geom(zN, zH, zW, zC, K.pad_channels(um.conv.out_channels), 1, 1, 1, 0)
                # (both operands staged packed -- the main unit's flag is the one its own f.staged() will compute -- and the pair served)
                main_packed = _packed_flags(f.plan, um, gm, f.dtype, False, False, f.bits, f.bn_train)[0]
                if main_packed and K.conv_fwd_shortcut_supported(gm, geom, f.dtype):
                    f.fused_sc[main_ui] = (geom, st, x)
                    f.aux[ui] = SimpleNamespace(geom=geom, st=st, train=False, xp=None)
                    return
            if sc is not None:
                if not st.fwd_packed:
                    raise RuntimeError(f"{self.name}: a shortcut was left for this launch but its operand is not staged packed")
                gv, stv, x_in = sc
                y = K.conv_fwd_shortcut_packed(geom, x, st.w_khwc, st.shift, gv, x_in, stv.w_khwc, stv.shift, self.act, want_bits=want_bits)
                if want_bits:
                    y, f.bits[self.dst] = y
                f.aux[ui] = SimpleNamespace(geom=geom, st=st, train=False, xp=None)
                f.t[self.dst] = y
                return
            pool_ui = None
            if stem and PACKED and FUSE_STEM_POOL and self.act == ACT_RELU and K.stem_pool_fwd_supported(geom, f.dtype):
                pool_ui = _sole_pool_consumer(f.plan, self)
            if pool_ui is not None:
                # stem + max-pool in one launch: the pool's slot and aux are stored here, this unit's own slot is never materialised
                # (backward needs the pooled gradient, the tap plane and xp only); the PoolUnit finds its work done
                f.t[f.plan.units[pool_ui].dst], am = K.stem_pool_fwd(geom, xp, wp, st.shift, want_argmax=f.save)
                f.aux[pool_ui] = SimpleNamespace(argmax=am, in_hw=(geom.P, geom.Q))
                f.aux[ui] = SimpleNamespace(geom=geom, st=st, train=False, xp=xp)
                return
            if stem and PACKED and K.stem_fwd_packed_supported(geom, f.dtype):
                y = K.stem_fwd_packed(geom, xp, K.stem_pack_weights(wp), st.shift, self.act)       # ring kernel, gathered rows
            elif stem:
                y = K.stem_fwd(geom, xp, wp, None, st.shift, self.act)
            elif st.fwd_packed and want_bits:
                y, f.bits[self.dst] = K.conv_fwd_packed(geom, x, st.w_khwc, st.shift, res, self.act, want_bits=True)
            elif st.fwd_packed:
                y = K.conv_fwd_packed(geom, x, st.w_khwc, st.shift, res, self.act)
            elif want_bits and Kp % 32 == 0:
                y, f.bits[self.dst] = K.conv_fwd(geom, x, st.w_khwc, None, st.shift, res, self.act, grouped=self.grouped, want_bits=True)
            else:
                y = K.conv_fwd(geom, x, st.w_khwc, None, st.shift, res, self.act, grouped=self.grouped)
            f.aux[ui] = SimpleNamespace(geom=geom, st=st, train=False, xp=xp)
        f.t[self.dst] = y

    def bwd(self, b, ui, g):
        a = b.aux[ui]
        x = b.t[self.src]
        if self.res is not None and b.requires.get(self.res, False):
            b.contribute(self.res, g, masked=False)
        if self.act == ACT_SILU and not a.train:
            raise NotImplementedError(f"{self.name}: backward through a folded (eval-mode) BN + SiLU is not supported; "
                                      "EfficientNet trains with batch statistics (efficientnet.py:308-312)")
        dz = b.bn_bwd(ui, self, g, a, self.conv.out_channels) if a.train else g
        if _defers(self, a, b.need, ui):
            b.defer_wgrad(ui, self, a, x, g, dz)
        elif b.need(ui, "weight") or b.need(ui, "bias") or (not a.train and (b.need(ui, "gamma") or b.need(ui, "beta"))):
            b.conv_wgrad(ui, self, a, x, g, dz)
        b.gsum_cache.pop(self.dst, None)
        if b.requires.get(self.src, False):
            b.grads[self.src] = b.conv_dgrad(self, a, x, dz)


class DwConvUnit:
    """Depthwise k x k Conv2d(groups=C, bias=False) + BatchNorm2d + activation (MBConv, efficientnet.py:101-103)."""
    kind = "dw"

    def __init__(self, name, conv, bn, act, src, dst):
        self.name, self.conv, self.bn, self.act, self.src, self.dst = name, conv, bn, act, src, dst
        if conv.groups != conv.in_channels or conv.in_channels != conv.out_channels or conv.bias is not None:
            raise ValueError(f"{name}: not a bias-free depthwise convolution")

    def params(self):
        return [("weight", self.conv.weight), ("gamma", self.bn.weight), ("beta", self.bn.bias)]

    def inputs(self):
        return [self.src]

    def fwd(self, f, ui):
        x = f.t[self.src]
        N, H, W, C = x.shape
        conv, bn = self.conv, self.bn
        R = conv.kernel_size[0]
        geom = K.make_geom(N, H, W, C, C, R, R, conv.stride[0], conv.padding[0])
        w_hwc = f.dw_hwc[ui] if ui in f.dw_hwc else conv.weight.detach()[:, 0].permute(1, 2, 0).contiguous()
        if _bn_uses_batch_stats(bn, f.bn_train):
            z, zstats = K.dwconv_fwd_stats(geom, x, w_hwc)
            f.t[self.dst], mean, rstd = f.bn_train_fwd(bn, z, zstats, None, self.act)
            f.aux[ui] = SimpleNamespace(geom=geom, train=True, z=z if f.save else None, mean=mean, rstd=rstd, w_hwc=w_hwc)
        else:
            scale, shift, _ = K.bn_fold(bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var, bn.eps)
            f.t[self.dst] = K.dwconv_fwd(geom, x, w_hwc, scale, shift, self.act)
            f.aux[ui] = SimpleNamespace(geom=geom, train=False)

    def bwd(self, b, ui, g):
        a = b.aux[ui]
        if not a.train:
            raise NotImplementedError(f"{self.name}: backward through an eval-mode depthwise block is not supported")
        x = b.t[self.src]
        dz = b.bn_bwd(ui, self, g, a)
        if b.need(ui, "weight"):
            b.emit(ui, "weight", K.dwconv_wgrad(a.geom, x, dz, param_layout=True))
        if b.requires.get(self.src, False):
            b.left[self.src] -= 1
            dx = K.dwconv_dgrad(a.geom, dz, a.w_hwc)
            pending = b.grads.pop(self.src, None)
            b.grads[self.src] = dx if pending is None else K.rowscale_add(dx, None, pending)


class SEUnit:
    """torchvision SqueezeExcitation: x * sigmoid(fc2(silu(fc1(avgpool(x)))))  (efficientnet.py:105-107)."""
    kind = "se"

    def __init__(self, name, fc1, fc2, src, dst):
        self.name, self.fc1, self.fc2, self.src, self.dst = name, fc1, fc2, src, dst

    def params(self):
        return [("w1", self.fc1.weight), ("b1", self.fc1.bias), ("w2", self.fc2.weight), ("b2", self.fc2.bias)]

    def inputs(self):
        return [self.src]

    def fwd(self, f, ui):
        x = f.t[self.src]
        C = x.shape[-1]
        w1 = self.fc1.weight.detach().view(self.fc1.out_channels, C)
        w2 = self.fc2.weight.detach().view(C, self.fc2.in_channels)
        avg, _ = K.gap_fwd(x, with_max=False)
        h1, u1 = K.linear_fwd(avg, w1, self.fc1.bias.detach(), K.CS_ACT_SILU, want_preact=True)
        sc = K.linear_fwd(h1, w2, self.fc2.bias.detach(), K.CS_ACT_SIGMOID)
        f.t[self.dst] = K.se_scale(x, sc)
        f.aux[ui] = SimpleNamespace(avg=avg, h1=h1, u1=u1, s=sc, w1=w1, w2=w2)

    def bwd(self, b, ui, g):
        a = b.aux[ui]
        ds = K.se_scale_bwd_ds(g, b.t[self.src])
        want2 = b.need(ui, "w2") or b.need(ui, "b2")
        want1 = b.need(ui, "w1") or b.need(ui, "b1")
        dh1, dw2, db2 = K.linear_bwd(a.h1, a.w2, ds, a.s, K.CS_ACT_SIGMOID, True, want2, want2)
        davg, dw1, db1 = K.linear_bwd(a.avg, a.w1, dh1, a.u1, K.CS_ACT_SILU, True, want1, want1)
        if b.need(ui, "w2"):
            b.emit(ui, "w2", dw2.view_as(self.fc2.weight))
        if b.need(ui, "b2"):
            b.emit(ui, "b2", db2)
        if b.need(ui, "w1"):
            b.emit(ui, "w1", dw1.view_as(self.fc1.weight))
        if b.need(ui, "b1"):
            b.emit(ui, "b1", db1)
        if b.requires.get(self.src, False):
            b.sole_consumer(self.src, "SE")
            b.grads[self.src] = K.se_scale_bwd_dx(g, a.s, davg)


class RowScaleAddUnit:
    """StochasticDepth(p, "row") on `a`, then + `b` (efficientnet.py:116-121); only planned when training with p > 0."""
    kind = "sd"

    def __init__(self, a, b, dst, p):
        self.a, self.b, self.dst, self.p = a, b, dst, p

    def params(self):
        return []

    def inputs(self):
        return [self.a, self.b]

    def fwd(self, f, ui):
        a = f.t[self.a]
        keep = 1.0 - self.p
        noise = torch.empty((a.shape[0],), dtype=torch.float32, device=a.device).bernoulli_(keep)
        if keep > 0:
            noise.div_(keep)
        f.t[self.dst] = K.rowscale_add(a, noise, f.t[self.b])
        f.aux[ui] = SimpleNamespace(noise=noise)

    def bwd(self, b, ui, g):
        if b.requires.get(self.b, False):
            b.contribute(self.b, g, masked=True)
        if b.requires.get(self.a, False):
            b.contribute(self.a, K.rowscale_add(g, b.aux[ui].noise, None), masked=True)


class PoolUnit:
    kind = "pool"

    def __init__(self, src, dst):
        self.src, self.dst = src, dst

    def params(self):
        return []

    def inputs(self):
        return [self.src]

    def fwd(self, f, ui):
        if f.aux[ui] is not None:
            return          # the stem in front pooled its own output (ConvUnit.fwd, FUSE_STEM_POOL)
        x = f.t[self.src]
        f.t[self.dst], am = K.maxpool_fwd(x, want_argmax=f.save)
        f.aux[ui] = SimpleNamespace(argmax=am, in_hw=tuple(x.shape[1:3]))

    def bwd(self, b, ui, g):
        if b.requires.get(self.src, False):
            b.sole_consumer(self.src, "pool")
            a = b.aux[ui]
            # dy is masked by [pool_out>0]; the argmax element equals pool_out, so dx is masked too
            b.grads[self.src] = K.maxpool_bwd(g, a.argmax, None, a.in_hw)


class UpsampleUnit:
    kind = "up"

    def __init__(self, src, dst, size_like=None, size_fn=None):
        """output size = spatial size of slot ``size_like`` or ``size_fn(input_hw_of_plan)``"""
        self.src, self.dst, self.size_like, self.size_fn = src, dst, size_like, size_fn

    def params(self):
        return []

    def inputs(self):
        return [self.src]

    def fwd(self, f, ui):
        x = f.t[self.src]
        size = tuple(f.t[self.size_like].shape[1:3]) if self.size_like is not None else tuple(self.size_fn(f.in_hw))
        f.t[self.dst] = K.bilinear_fwd(x, size)
        f.aux[ui] = SimpleNamespace(in_hw=tuple(x.shape[1:3]))

    def bwd(self, b, ui, g):
        if b.requires.get(self.src, False):
            b.sole_consumer(self.src, "upsample")
            mask = b.t[self.src] if self.src in b.plan.relu_slots else None
            b.grads[self.src] = K.bilinear_bwd(g, b.aux[ui].in_hw, mask=mask)


class ConcatUnit:
    kind = "cat"

    def __init__(self, a, b, dst):
        self.a, self.b, self.dst = a, b, dst

    def params(self):
        return []

    def inputs(self):
        return [self.a, self.b]

    def fwd(self, f, ui):
        a, b = f.t[self.a], f.t[self.b]
        f.t[self.dst] = K.concat(a, b)
        f.aux[ui] = SimpleNamespace(ca=a.shape[-1])

    def bwd(self, b, ui, g):
        na, nb = b.requires.get(self.a, False), b.requires.get(self.b, False)
        if na or nb:
            ga, gb = K.split(g, b.aux[ui].ca, want_a=na, want_b=nb)
            if na:
                b.contribute(self.a, ga, masked=True)
            if nb:
                b.contribute(self.b, gb, masked=True)


class Plan:
    def __init__(self, units, inputs, outputs, relu_inputs=()):
        self.units, self.inputs, self.outputs = units, list(inputs), list(outputs)
        self.relu_slots = set(relu_inputs)
        for u in units:
            if u.kind == "conv" and u.act == ACT_RELU:
                self.relu_slots.add(u.dst)
            elif u.kind == "pool" and u.src in self.relu_slots:
                self.relu_slots.add(u.dst)       # max of non-negative values; see PoolUnit backward
            elif u.kind == "cat" and u.a in self.relu_slots and u.b in self.relu_slots:
                self.relu_slots.add(u.dst)
        self.consumers = {}
        for u in units:
            for s in u.inputs():
                self.consumers[s] = self.consumers.get(s, 0) + 1
        self.param_list = []          # [(unit_index, role, tensor)]
        for ui, u in enumerate(units):
            for role, t in u.params():
                self.param_list.append((ui, role, t))

    def param_tensors(self):
        return [t for _, _, t in self.param_list]


def _bn_uses_batch_stats(bn, bn_train):
    return bn is not None and bn_train and bn.training


def _is_paired_stem(u):
    """Conv2d(<= 3 -> K, 7x7, stride 2, padding 3) without groups or residual: the stem the pixel-paired kernels (kernels.stem_*) run."""
    if u.kind != "conv":
        return False
    c = u.conv
    return (not u.grouped and u.res is None and c.in_channels <= 3 and c.kernel_size == (7, 7)
            and c.stride == (2, 2) and c.padding == (3, 3))


def _sole_pool_consumer(plan, u):
    """Index of the PoolUnit that is the ONLY reader of conv unit u's output (which is no plan output either), else None."""
    if plan.consumers.get(u.dst, 0) != 1 or u.dst in plan.outputs:
        return None
    for vi, v in enumerate(plan.units):
        if u.dst in v.inputs():
            return vi if v.kind == "pool" else None
    return None


def shortcut_pairs(plan, bn_train):
    """{index of a projection-shortcut unit v: index of the unit u that takes v's output as its residual} for every pair one launch can
    serve (FUSE_SHORTCUT): both ungrouped 1x1 convolutions without padding, u of stride 1 and v of stride 1 or 2, v without
    activation or residual of its own, v's output read by u alone and no plan output, u's input already there when v runs, a folded
    (not batch-statistics) BN or none on both.  What depends on the pass -- bf16, packed staging, the extents the library serves --
    is asked in ConvUnit.fwd.  Decided once per plan and BN mode (cached on the plan)."""
    if not (PACKED and FUSE_SHORTCUT):
        return {}
    key = (bool(bn_train), tuple(u.bn.training for u in plan.units if u.kind == "conv" and u.bn is not None))
    cache = plan.__dict__.setdefault("_shortcut_pairs", {})
    if key not in cache:
        cache[key] = _find_shortcut_pairs(plan, bn_train)
    return cache[key]


def _find_shortcut_pairs(plan, bn_train):
    producer = {v.dst: vi for vi, v in enumerate(plan.units) if v.kind == "conv"}
    made_by = {w.dst: wi for wi, w in enumerate(plan.units)}
    pairs = {}
    for ui, u in enumerate(plan.units):
        vi = producer.get(u.res) if u.kind == "conv" and u.res is not None else None
        if vi is None or vi >= ui:
            continue
        v = plan.units[vi]

        def one_by_one(w, strides):
            c = w.conv
            return not w.grouped and c.kernel_size == (1, 1) and c.padding == (0, 0) and c.stride in strides
        if not (one_by_one(u, ((1, 1),)) and one_by_one(v, ((1, 1), (2, 2)))):
            continue
        if v.act != ACT_NONE or v.res is not None or u.act not in (ACT_NONE, ACT_RELU):
            continue
        if plan.consumers.get(v.dst, 0) != 1 or v.dst in plan.outputs:
            continue
        if u.src not in plan.inputs and made_by.get(u.src, len(plan.units)) >= vi:
            continue          # (v asks the library with u's input extents, and hands its operands to the NEXT launch of u)
        if _bn_uses_batch_stats(u.bn, bn_train) or _bn_uses_batch_stats(v.bn, bn_train):
            continue
        pairs[vi] = ui
    return pairs


def _stem_takes_nchw(plan, dtype):
    """True when the plan's input feeds exactly one unit and that unit is the pixel-paired bf16 stem: the fp32 NCHW image can go
    straight to the paired operand (cs_stem_pair_from_nchw) and the NHWC8 tensor is never made."""
    if not (dtype == torch.bfloat16 and len(plan.inputs) == 1 and plan.units):
        return False
    u = plan.units[0]
    return (_is_paired_stem(u) and u.conv.in_channels == 3 and u.src == plan.inputs[0]
            and plan.consumers.get(u.src, 0) == 1)


def _packed_flags(plan, u, geom, dtype, need_bwd, batch_stats, bits, bn_train=False):
    """(forward operand packed?, data-gradient operand packed?) for the packed-operand kernels of csrc/conv_v2.hip.
    The data gradient only qualifies when its ReLU mask (if it applies one) exists as a bit tensor."""
    if not PACKED or u.grouped or u.act not in (ACT_NONE, ACT_RELU):
        return False, False
    if batch_stats:
        # Batch-statistics BN: the packed kernels have no statistics epilogue (16 more live registers spill under their cap), so
        # z is written first and one cs_bn_stats pass reads it back.  Only where that pass is noise next to the MFMA work: dense
        # stride-1 3x3 convolutions of >= 128 channels (the segmentation decoder, resnet.py:195-200 -- 86 % of segment-mode FLOPs).
        # Their ReLU masks, where no bit plane exists, are made on demand in backward (kernels.positive_bits).
        # (Round 4 tried the forward-only 1x1 convolutions of the frozen encoder too -- 21 us launches at 0.08 of HBM on the
        # first-generation kernel at B = 8: with the ring kernel + the statistics pass C5 went 1454 -> 1407 img/s, 512 x 512 580 -> 562.)
        if not (PACKED_TRAIN_BN and geom.R == 3 and geom.S == 3 and geom.stride == 1 and min(geom.C, geom.K) >= 128):
            return False, False
        pkf = K.packed_supported(geom, dtype, dgrad=False)
        pkb = bool(need_bwd) and K.packed_supported(geom, dtype, dgrad=True) and geom.C % 32 == 0
        return pkf, pkb
    pkf = K.packed_supported(geom, dtype, dgrad=False)
    pkb = bool(need_bwd) and K.packed_supported(geom, dtype, dgrad=True) and (u.src not in plan.relu_slots or u.src in bits)
    if pkb and geom.stride != 1:
        # a strided 1x1 data gradient is served in COMPACT form (kernels.CompactGrad): only where the other consumer of the block
        # input is the stride-1 1x1 convolution whose packed data gradient runs AFTER this one in backward order and adds it
        pkb = _compact_partner(plan, u, geom, dtype, bits, bn_train) is not None
    return pkf, pkb


def _compact_partner(plan, u, geom, dtype, bits, bn_train=False):
    """The unit whose data gradient will take u's compact gradient as its strided add operand, or None.  The partner must itself
    be staged bwd_packed in this pass: same eligibility as _packed_flags applies to it, including ITS BatchNorm mode (a model
    with mixed frozen / train-mode BN layers falls back to the dense strided gradient instead of raising in backward)."""
    others = [(i, v) for i, v in enumerate(plan.units) if v is not u and v.kind == "conv" and v.src == u.src]
    if len(others) != 1 or plan.consumers.get(u.src, 0) != 2:
        return None
    iv, v = others[0]
    iu = plan.units.index(u)
    c = v.conv
    if iv > iu or v.grouped or v.act not in (ACT_NONE, ACT_RELU) or c.kernel_size != (1, 1) or c.stride != (1, 1) or c.padding != (0, 0):
        return None
    if not PACKED or _bn_uses_batch_stats(v.bn, bn_train):
        return None
    if u.src in plan.relu_slots and u.src not in bits:
        return None
    gv = K.make_geom(geom.N, geom.H, geom.W, geom.C, K.pad_channels(c.out_channels), 1, 1, 1, 0)
    if not K.packed_supported(gv, dtype, dgrad=True):
        return None
    return v


_STAGE_EPOCH = [0]


def invalidate_staged():
    """Drop every cached staged-weight set (of every plan).  Needed whenever parameters or BN buffers change behind the
    host's back: a HIP-graph replay of a training step updates them without running any Python (graphed.GraphedStep)."""
    _STAGE_EPOCH[0] += 1


# How a convolution is staged: channel extents, data-gradient operand or not, packed orders, batch-statistics BN (nothing folded in).
# The one-launch staging (kernels.StagePack) serves a layer only under the spec it recorded.
_StageSpec = namedtuple("_StageSpec", "Cp Kp need_bwd pkf pkb batch_stats")


class _Staged:
    """Staged operands of one convolution: w_khwc (forward), w_chwk (data gradient, or None), [Kp] scale / rstd (None unless an
    eval-mode BN is folded in) and shift; *_packed: that operand is in the order of the packed-operand kernels (conv_v2.hip)."""
    __slots__ = ("w_khwc", "w_chwk", "scale", "shift", "rstd", "fwd_packed", "bwd_packed")

    def __init__(self, w_khwc, w_chwk, scale, shift, rstd, pkf, pkb):
        self.w_khwc, self.w_chwk, self.scale, self.shift, self.rstd = w_khwc, w_chwk, scale, shift, rstd
        self.fwd_packed, self.bwd_packed = bool(pkf), bool(pkb and w_chwk is not None)


def _stage_weights(u, dtype, spec, fresh):
    """BN folding + weight staging, layer by layer.  Cached only for frozen parameters and for no-grad passes: `fresh` (a forward
    that will be followed by an optimizer step, of a layer whose staging depends on a trainable parameter) always stages afresh
    and leaves the cache invalid, because tensor version counters cannot be trusted to see the update -- torch's fused optimizers
    (`Adam(fused=True)`) write the parameters without bumping `_version`."""
    conv, bn = u.conv, u.bn
    # (a batch-statistics pass folds nothing of the BatchNorm into the operands: they depend on the convolution's own tensors only, so a
    # frozen encoder under train-mode BN -- the segmentation stage -- stages once, not once per step)
    fold = bn is not None and not spec.batch_stats
    key_t = [conv.weight, conv.bias] + ([bn.weight, bn.bias, bn.running_mean, bn.running_var] if fold else [])
    key = (_STAGE_EPOCH[0], dtype, spec) + tuple((t._version, t.data_ptr()) if t is not None else None for t in key_t)
    if fresh:
        key = None
    elif u._cache is not None and u._cache[0] == key:
        return u._cache[1]
    if u.grouped:
        w = conv.weight.detach()
        scale = rstd = None
        shift = conv.bias.detach() if conv.bias is not None else None
        if fold:
            scale, shift, rstd = K.bn_fold(bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var, bn.eps, shift)
        w_khwc, w_chwk = K.weight_prep_grouped(w, scale, dtype, want_fwd=True, want_bwd=spec.need_bwd)
    else:
        # one launch: BN fold, both operands, packed order where the packed-operand kernels take them (as kernels.StagePack does)
        w_khwc, w_chwk, scale, shift, rstd = K.stage_layer(conv, bn if fold else None, dtype, spec.Cp, spec.Kp, want_bwd=spec.need_bwd,
                                                           fwd_packed=spec.pkf, bwd_packed=spec.pkb)
        if not fold:                        # nothing folded: no scale, no rstd, a shift only where the convolution has a bias
            scale = rstd = None
            if conv.bias is None:
                shift = None
    st = _Staged(w_khwc, w_chwk, scale, shift, rstd, spec.pkf, spec.pkb)
    u._cache = (key, st)
    return st


class _Arena:
    """Zeroed tensors bump-allocated from one zero-filled buffer (one fill per pass); take() is None when the request does not fit."""

    def __init__(self, n, dtype, device, align):
        self.buf = torch.zeros((n,), dtype=dtype, device=device) if n else None
        self.pos, self.align = 0, align

    def take(self, n):
        step = (n + self.align - 1) // self.align * self.align
        if self.buf is None or self.pos + step > self.buf.numel():
            return None
        v = self.buf[self.pos:self.pos + n]
        self.pos += step
        return v


class _Forward:
    """State of one forward pass: slot tensors `t`, per-unit `aux` for backward, ReLU bit planes, weight staging, BN bookkeeping."""

    def __init__(self, plan, feeds, dtype, bn_train, save, requires, image_hw, input_nchw):
        self.plan, self.dtype, self.bn_train, self.save, self.requires = plan, dtype, bn_train, save, requires
        self.t = t = dict(feeds)
        self.nchw_for_stem = None
        if input_nchw is not None:
            if _stem_takes_nchw(plan, dtype):
                self.nchw_for_stem = input_nchw
            else:
                t[plan.inputs[0]] = K.to_nhwc(input_nchw, dtype, K.pad_channels(3))
        self.aux = [None] * len(plan.units)
        self.remaining = dict(plan.consumers)
        self.in_hw = image_hw if image_hw is not None else tuple(t[plan.inputs[0]].shape[1:3])
        self.dev = dev = t[plan.inputs[0]].device
        self.capturing = _capture.capturing()

        # Training passes re-stage every folded Conv+BN after each optimizer update: one launch for the whole plan (the first such
        # pass stages layer by layer and records the layout; see kernels.StagePack)
        # (one pack per (dtype, input shape): which layers take packed operands depends on the geometry, and a ragged last batch must
        # not evict the pack of the full batches -- a captured step keeps replaying into it)
        self.packs = plan.__dict__.setdefault("_stage_packs", {})
        self.pack_key = (dtype, tuple(t[plan.inputs[0]].shape))
        pack = self.packs.get(self.pack_key) if save else None
        self.prestaged, self.record = {}, None          # record: [(unit index, unit, _StageSpec)] for the pack built at the end
        if save:
            if pack is not None and pack.valid():
                pack.launch()
                self.prestaged = pack.by_unit
                if self.capturing:
                    _capture.keep(pack)
            else:
                self.packs.pop(self.pack_key, None)
                while len(self.packs) >= 4:
                    self.packs.pop(next(iter(self.packs)))
                self.record = []

        # train-mode BN bookkeeping for the whole plan in two launches instead of two per layer: one zero-filled fp64 arena for the
        # per-channel statistics, one foreach-add for the num_batches_tracked counters (this path is host-bound: ~1000 launches/step)
        self.bumped = []
        if bn_train and save:
            K.begin_pass(dev)
        self.bits = {}       # slot -> uint8 "output > 0" bit tensor (folded Conv+BN+ReLU outputs of a pass that will run backward)
        # projection shortcuts that ride in their block's last 1x1 launch (shortcut_pairs: cached on the plan), and the operands a
        # shortcut unit left for that launch {main unit index: (geometry, staged set, block input)}
        self.sc_pairs = shortcut_pairs(plan, bn_train) if dtype == torch.bfloat16 else {}
        self.fused_sc = {}
        n_stats = sum(K.accum_words(K.pad_channels(u.conv.out_channels)) for u in plan.units
                      if u.kind == "conv" and _bn_uses_batch_stats(u.bn, bn_train)) if bn_train else 0
        self.stats = _Arena(n_stats, torch.float64, dev, 1)
        self.dw_hwc = self._stage_depthwise()

    def _stage_depthwise(self):
        """{unit index: [R, S, C] filter} of every depthwise layer, restaged by one launch per pass (a permute + strided copy per
        layer: 26 launches of 4.4 us on EfficientNet-B3)."""
        plan = self.plan
        units = [ui for ui, u in enumerate(plan.units) if u.kind == "dw"]
        if not units:
            return {}
        ws = [plan.units[ui].conv.weight.detach() for ui in units]
        if not all(w.is_contiguous() and w.dtype == torch.float32 and w.dim() == 4 and w.shape[1] == 1 for w in ws):
            return {}
        dpack = plan.__dict__.get("_dw_stage_pack")
        if dpack is None or dpack.key != tuple(w.data_ptr() for w in ws):
            dpack = plan.__dict__["_dw_stage_pack"] = K.DwStagePack(ws)
        dpack.run()
        if self.capturing:
            _capture.keep(dpack)
        return dict(zip(units, dpack.hwc))

    def take_stats(self, C):
        v = self.stats.take(K.accum_words(C))
        return v if v is not None else K.new_stats(C, self.dev)

    def staged(self, ui, u, geom, batch_stats):
        """The staged operands of conv unit u: from this pass's one-launch pack when its spec matches, else layer by layer."""
        need_bwd = self.save and self.requires.get(u.src, False)
        pkf, pkb = _packed_flags(self.plan, u, geom, self.dtype, need_bwd, batch_stats, self.bits, self.bn_train)
        spec = _StageSpec(geom.C, geom.K, need_bwd, pkf, pkb, batch_stats)
        ps = (u.conv.weight, u.conv.bias) + ((u.bn.weight, u.bn.bias) if (u.bn is not None and not batch_stats) else ())
        trainable = any(p is not None and p.requires_grad for p in ps)       # does the staging depend on a trainable parameter?
        # A pass that will be followed by an optimizer step, or that updates BN running statistics in place, must not leave
        # a version-keyed cache behind: fused optimizers and our own kernels write those tensors without bumping `_version`
        # (a later no-grad pass would be served the old weights; the one-launch pack path never touches `_cache`)
        if self.save and trainable:
            u._cache = None
        pre = self.prestaged.get(ui)
        if pre is not None and pre[0] == spec:
            return pre[1]
        if pre is not None:
            self.packs.pop(self.pack_key, None)       # the layout changed (other requires_grad pattern): rebuild next time
        st = _stage_weights(u, self.dtype, spec, fresh=self.save and trainable)
        if self.capturing:
            _capture.keep(st)               # (a cached staged set may be replaced by a later eager pass: the graph keeps this one)
        # (a batch-statistics layer joins the one-launch staging with bn = None: its operands depend on the convolution only)
        if self.record is not None and not u.grouped and (batch_stats or u.bn is not None) and trainable:
            self.record.append((ui, u, spec))
        return st

    def bn_train_fwd(self, bn, z, stats, res, act):
        """Train-mode BatchNorm of z (+ residual, activation): finalize + apply in one launch (mean / rstd derived inside)."""
        momentum = bn.momentum if bn.momentum is not None else 0.1
        track = bn.track_running_stats
        y, mean, rstd = K.bn_apply_stats(z, stats, bn.eps, momentum, bn.running_mean if track else None,
                                         bn.running_var if track else None, bn.weight.detach(), bn.bias.detach(), res, act)
        if track and bn.num_batches_tracked is not None:
            self.bumped.append(bn.num_batches_tracked)
        return y, mean, rstd

    def release(self, s):
        if self.save or s in self.plan.outputs:
            return
        self.remaining[s] -= 1
        if self.remaining[s] == 0:
            self.t.pop(s, None)

    def finish(self):
        if self.bumped:
            torch._foreach_add_(self.bumped, 1)
        if self.record:
            pk = K.StagePack([(u.conv, None if s.batch_stats else u.bn, s.Cp, s.Kp, s.need_bwd, s.pkf, s.pkb)
                              for _, u, s in self.record], self.dtype)
            # (batch statistics: the consumers expect no folded scale and no rstd)
            pk.by_unit = {ui: (s, _Staged(w, wb, None if s.batch_stats else sc, sh, None if s.batch_stats else r, s.pkf, s.pkb))
                          for (ui, _, s), (w, wb, sc, sh, r) in zip(self.record, pk.staged)}
            self.packs[self.pack_key] = pk


def forward(plan, feeds, dtype, bn_train, save, requires, image_hw=None, input_nchw=None):
    """feeds: {slot: NHWC tensor}.  Returns state with .t (slot tensors) and .aux (per unit).
    input_nchw: the network input as the contiguous fp32 [N,3,H,W] image instead (feeds then holds an UNINITIALISED placeholder of
    the NHWC8 shape for that slot): converted here -- directly into the paired stem operand where the stem takes it."""
    f = _Forward(plan, feeds, dtype, bn_train, save, requires, image_hw, input_nchw)
    for ui, u in enumerate(plan.units):
        u.fwd(f, ui)
        for s in u.inputs():
            f.release(s)
    f.finish()
    return SimpleNamespace(t=f.t, aux=f.aux, in_hw=f.in_hw, bits=f.bits)


def compute_requires(plan, param_needs, input_needs):
    """requires[slot]: does anything upstream of (and including the producer of) slot need a gradient?"""
    requires = {s: bool(input_needs.get(s, False)) for s in plan.inputs}
    pi = 0
    unit_trainable = []
    for u in plan.units:
        n = len(u.params())
        unit_trainable.append(any(param_needs[pi:pi + n]))
        pi += n
    for ui, u in enumerate(plan.units):
        requires[u.dst] = unit_trainable[ui] or any(requires.get(s, False) for s in u.inputs())
    return requires, unit_trainable


def _defers(u, a, need, ui):
    """Ungrouped convolutions under a BatchNorm take the batched weight-gradient path (one split-K launch + ONE fused finalize per group of
    identical geometry; the fused finalize turns the [rs][c] slabs into torch's [c][rs] order through LDS): eval-BN layers without a
    bias whose weight AND BN gradients are wanted (the finalize also writes dgamma / dbeta), and batch-statistics layers whose weight
    gradient is wanted (their BN gradients come from the BN backward pass; the finalize only folds the slabs) -- round 5: also the
    biased 3x3 convolutions of the decoder (resnet.py:195-200), whose bias gradient is the column sum of dz, taken on its own."""
    if not (u.kind == "conv" and need(ui, "weight") and not u.grouped and u.bn is not None):
        return False
    if a.train:
        return True
    return u.conv.bias is None and not need(ui, "bias") and bool(need(ui, "gamma") or need(ui, "beta"))


def _group_key(geom, a):
    return ((geom.N, geom.H, geom.W, geom.C, geom.K, geom.R, geom.S, geom.stride, geom.pad), bool(a.train))


_grad_sink = None


def set_grad_sink(sink):
    """Data-parallel hook (parallel.GradReducer.attach): `sink.view_for(param)` may hand out the tensor a parameter
    gradient is to be written into (a slice of a flat all-reduce bucket) and `sink.deliver(param, grad)` is called, in
    the order gradients are finished inside backward, as soon as the kernels producing `grad` are enqueued -- so the
    bucket's collective can start while the rest of backward still runs.  Returns the previous sink."""
    global _grad_sink
    prev, _grad_sink = _grad_sink, sink
    return prev


class _Backward:
    """State of one backward pass: slot and parameter gradients, column sums left by dgrads, batched weight-gradient groups."""

    def __init__(self, plan, state, grad_feeds, param_needs, requires, use_tr_read):
        self.plan, self.t, self.aux, self.bits = plan, state.t, state.aux, state.bits
        self.param_needs, self.requires, self.use_tr_read = param_needs, requires, use_tr_read
        self.grads = dict(grad_feeds)
        self.gsum_cache = {}
        self.sink = _grad_sink
        # One zero-filled fp32 arena for every raw weight-gradient buffer and column-sum vector of this backward pass
        # (a single fill kernel instead of ~2 per convolution).
        self.dev = next(iter(grad_feeds.values())).device if grad_feeds else None
        n = sum(a.geom.C + a.geom.K + 16 for u, a in zip(plan.units, self.aux) if u.kind == "conv" and a is not None)
        self.arena = _Arena(n if self.dev is not None else 0, torch.float32, self.dev, 8)
        self.left = dict(plan.consumers)
        self.pgrads = [None] * len(plan.param_list)
        self.pindex = {(ui, role): i for i, (ui, role, _) in enumerate(plan.param_list)}
        # how many layers of each geometry will ask for a batched weight gradient: a group is launched as soon as it is complete
        # (or holds 8 layers), so its gradients are final -- and its activations released -- long before backward ends
        self.group_total, self.group_seen, self.deferred = {}, {}, {}
        for ui, (u, a) in enumerate(zip(plan.units, self.aux)):
            if a is not None and _defers(u, a, self.need, ui):
                k = _group_key(a.geom, a)
                self.group_total[k] = self.group_total.get(k, 0) + 1

    def need(self, ui, role):
        i = self.pindex.get((ui, role))
        return i is not None and self.param_needs[i]

    def emit(self, ui, role, g):
        """Record a finished parameter gradient (and hand it to the data-parallel sink straight away)."""
        i = self.pindex[(ui, role)]
        self.pgrads[i] = g if self.sink is None else self.sink.deliver(self.plan.param_list[i][2], g)

    def emit_bn(self, ui, dgamma, dbeta, n=None):
        """dgamma / dbeta where wanted (their first n channels: the padded ones are not the parameter's)."""
        if self.need(ui, "gamma"):
            self.emit(ui, "gamma", dgamma if n is None else dgamma[:n])
        if self.need(ui, "beta"):
            self.emit(ui, "beta", dbeta if n is None else dbeta[:n])

    def grad_buffer(self, param):
        """Destination for a parameter gradient: the sink's bucket slice when there is one."""
        v = self.sink.view_for(param) if self.sink is not None else None
        return v if v is not None else torch.empty_like(param)

    def take(self, n):
        v = self.arena.take(n)
        return v if v is not None else torch.zeros((n,), dtype=torch.float32, device=self.dev)

    def contribute(self, slot, g, masked):
        """Non-fused contribution (alias when first)."""
        self.left[slot] -= 1
        if slot in self.grads:
            raise NotImplementedError("engine: unfused gradient accumulation is not expected for these networks")
        if self.left[slot] == 0 and slot in self.plan.relu_slots and not masked:
            raise NotImplementedError("engine: last contribution to a post-ReLU slot must come from a masking kernel")
        self.grads[slot] = g

    def sole_consumer(self, slot, what):
        """Count the one contribution to `slot` of a unit that cannot add to a gradient already there."""
        self.left[slot] -= 1
        if slot in self.grads:
            raise NotImplementedError(f"engine: {what} input with several consumers")

    def bn_bwd(self, ui, u, g, a, n=None):
        """Train-mode BatchNorm backward (through the activation) -> dz; dgamma / dbeta emitted where wanted (see emit_bn)."""
        bn, want = u.bn, self.need(ui, "gamma") or self.need(ui, "beta")
        dz, dgamma, dbeta = K.bn_bwd(g, a.z, a.mean, a.rstd, bn.weight.detach(), want_param_grads=want, beta=bn.bias.detach(),
                                     act=ACT_SILU if u.act == ACT_SILU else ACT_NONE)
        self.emit_bn(ui, dgamma, dbeta, n)
        return dz

    def colsums(self, u, a, g, dz, partial):
        """Column sums of dz for u's BN / bias gradients (eval-mode BN: those the dgrad that finished g left), else taken now as a
        PartialColsum (`partial`) or a vector; shared with the residual slot when it receives the very same gradient tensor."""
        cached = self.gsum_cache.pop(u.dst, None) if not a.train else None
        if partial:
            gsum = cached if cached is not None else K.colsum_partial(dz)
        else:
            gsum = K.colsum_vector(cached) if cached is not None else K.colsum(dz)
        if not a.train and u.res is not None and self.grads.get(u.res) is g:
            self.gsum_cache[u.res] = gsum
        return gsum

    def defer_wgrad(self, ui, u, a, x, g, dz):
        """Weight gradients of identical-geometry layers are launched together (one batched split-K launch per shape group:
        proportionally fewer partial slabs to write and fold)."""
        gsum = None
        if not a.train:
            gsum = self.colsums(u, a, g, dz, partial=True)
        elif self.need(ui, "bias"):
            # the bias of a convolution in front of a batch-statistics BN: d bias = column sums of dz (analytically zero --
            # the BN backward removes the batch mean --, the reference computes the same rounding noise: train_seg.py decoder)
            dbias = self.grad_buffer(u.conv.bias)
            dbias.copy_(K.colsum(dz)[:u.conv.out_channels])
            self.emit(ui, "bias", dbias)
        key = _group_key(a.geom, a)
        items = self.deferred.setdefault(key, [])
        items.append(SimpleNamespace(ui=ui, u=u, a=a, x=x, dz=dz, gsum=gsum))
        self.group_seen[key] = self.group_seen.get(key, 0) + 1
        if len(items) == 8 or self.group_seen[key] == self.group_total.get(key, 0):      # kernel-argument tables hold at most 8 layers
            self.flush(self.deferred.pop(key))

    def flush(self, items):
        geom = items[0].a.geom
        convs = [it.u.conv for it in items]
        Cin = convs[0].in_channels
        train = bool(items[0].a.train)                   # (a group is all eval-BN or all batch-statistics: _group_key)
        dws = [self.grad_buffer(c.weight) for c in convs]
        dgs = None if train else [self.grad_buffer(it.u.bn.weight) for it in items]
        dbs = None if train else [self.grad_buffer(it.u.bn.bias) for it in items]
        # (single layers take the same path: its finalize folds deferred column sums, the stand-alone one does not)
        if len(items) == 1 and items[0].a.xp is not None:
            slabs = K.stem_wgrad(geom, items[0].a.xp, items[0].dz, use_tr_read=self.use_tr_read).unsqueeze(0)     # [1, 1, K, 7, 7, 8]
        else:
            slabs = K.wgrad_batched(geom, [it.x for it in items], [it.dz for it in items], use_tr_read=self.use_tr_read)
        if train:
            K.wgrad_finalize_batched(slabs, None, None, None, None, None, dws, None, None, Cin)
            for it, dw in zip(items, dws):
                self.emit(it.ui, "weight", dw)
            return
        K.wgrad_finalize_batched(slabs, [c.weight.detach() for c in convs], [it.a.st.scale for it in items],
                                 [it.a.st.rstd for it in items], [it.u.bn.running_mean for it in items], [it.gsum for it in items],
                                 dws, dgs, dbs, Cin)
        for it, dw, dg, db in zip(items, dws, dgs, dbs):
            self.emit(it.ui, "weight", dw)
            self.emit_bn(it.ui, dg, db)

    def conv_wgrad(self, ui, u, a, x, g, dz):
        """Weight (+ bias, + eval-mode BN) gradients of one convolution, launched now."""
        conv, geom = u.conv, a.geom
        want_b = self.need(ui, "bias")
        want_bn = not a.train and (self.need(ui, "gamma") or self.need(ui, "beta"))
        gsum = self.colsums(u, a, g, dz, partial=False) if (want_b or want_bn) else None
        if a.xp is not None:
            raw = K.stem_wgrad(geom, a.xp, dz, use_tr_read=self.use_tr_read)
        elif not u.grouped and K.wgrad2_serves(geom, x.dtype):
            raw = K.wgrad_batched(geom, [x], [dz], use_tr_read=self.use_tr_read)[0]      # wgrad_v2.hip (the batched entry routes to it)
        else:
            raw = K.new_wgrad_buffer(geom, x.device, u.grouped)
            K.conv_wgrad(geom, x, dz, raw, use_tr_read=self.use_tr_read, grouped=u.grouped)
        dw = self.grad_buffer(conv.weight)
        dbias = self.grad_buffer(conv.bias) if want_b else None
        dgamma, dbeta = (self.grad_buffer(u.bn.weight), self.grad_buffer(u.bn.bias)) if want_bn else (None, None)
        dot = self.take(conv.out_channels) if want_bn else None
        w = conv.weight.detach() if want_bn else None
        scale, rstd = (None, None) if a.train else (a.st.scale, a.st.rstd)
        mean = u.bn.running_mean if want_bn else None
        if u.grouped:
            K.wgrad_finalize_grouped(raw, w, scale, rstd, mean, gsum, dw, dgamma=dgamma, dbeta=dbeta, dot=dot)
        else:
            K.wgrad_finalize(raw, w, scale, rstd, mean, gsum, conv.in_channels, dw, dbias=dbias, dgamma=dgamma, dbeta=dbeta, dot=dot)
        if self.need(ui, "weight"):
            self.emit(ui, "weight", dw)
        if want_b:
            self.emit(ui, "bias", dbias)
        if want_bn:
            self.emit_bn(ui, dgamma, dbeta)

    def conv_dgrad(self, u, a, x, dz):
        """Data gradient of conv unit u (packed or dense route); the one finishing the slot masks it and leaves its column sums."""
        geom, st = a.geom, a.st
        self.left[u.src] -= 1
        final = self.left[u.src] == 0
        pending = self.grads.pop(u.src, None)
        mask = x if (u.src in self.plan.relu_slots and final) else None
        mbits = self.bits.get(u.src) if mask is not None else None
        if mbits is not None:
            mask = None
        if st.bwd_packed and geom.stride != 1:
            if final or pending is not None:
                raise RuntimeError(f"{u.name}: compact strided data gradient out of order (it must be the first contribution)")
            return K.conv_dgrad_packed(geom, dz, st.w_chwk)          # kernels.CompactGrad: consumed as a strided add operand
        if st.bwd_packed:
            if mask is not None and a.train:
                mbits, mask = K.positive_bits(mask), None          # (a train-mode BN + ReLU output / a concatenation of such)
            if mask is not None:
                raise RuntimeError(f"{u.name}: packed data-gradient operand staged but the ReLU mask is not a bit tensor")
            if not final:
                return K.conv_dgrad_packed(geom, dz, st.w_chwk, add=pending, mask_bits=mbits)
            dx, self.gsum_cache[u.src] = K.conv_dgrad_packed(geom, dz, st.w_chwk, add=pending, mask_bits=mbits, want_colsum=True)
            return dx
        if isinstance(pending, K.CompactGrad):
            raise RuntimeError(f"{u.name}: a compact gradient reached a data gradient that cannot add it")
        if not final:
            return K.conv_dgrad(geom, dz, st.w_chwk, add=pending, mask=mask, grouped=u.grouped, mask_bits=mbits)
        # column sums of the finished gradient feed its producer's BN/bias gradients: left as per-workgroup partial
        # rows where the launch allows it (the batched finalize folds them; one small launch less per layer)
        cs = self.take(geom.C) if (geom.stride != 1 or u.grouped) else None
        dx, self.gsum_cache[u.src] = K.conv_dgrad(geom, dz, st.w_chwk, add=pending, mask=mask, colsum=cs, grouped=u.grouped,
                                                  defer_colsum=True, mask_bits=mbits)
        return dx


def backward(plan, state, grad_feeds, param_needs, requires, use_tr_read=True):
    """grad_feeds: {output slot: grad (already ReLU-masked where the slot is post-ReLU)}.
    Returns ({input slot: grad}, [param grads in plan.param_list order])."""
    b = _Backward(plan, state, grad_feeds, param_needs, requires, use_tr_read)
    for ui in reversed(range(len(plan.units))):
        u = plan.units[ui]
        g = b.grads.pop(u.dst, None)
        if g is not None:
            u.bwd(b, ui, g)
    for items in list(b.deferred.values()):       # groups whose count fell short of the forecast (defensive; not expected)
        b.flush(items)
    return {s: b.grads.get(s) for s in plan.inputs}, b.pgrads


class _PlanFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, plan, cfg, n_inputs, *tensors):
        inputs, params = tensors[:n_inputs], tensors[n_inputs:]
        feeds = {s: x for s, x in zip(plan.inputs, inputs)}
        input_needs = {s: ctx.needs_input_grad[3 + i] for i, s in enumerate(plan.inputs)}
        param_needs = [ctx.needs_input_grad[3 + n_inputs + i] for i in range(len(params))]
        save = any(param_needs) or any(input_needs.values())
        requires, _ = compute_requires(plan, param_needs, input_needs)
        state = forward(plan, feeds, cfg.dtype, cfg.bn_train, save, requires, cfg.image_hw, getattr(cfg, "input_nchw", None))
        ctx.plan, ctx.cfg, ctx.n_inputs = plan, cfg, n_inputs
        ctx.param_needs, ctx.requires = param_needs, requires
        ctx.state = state if save else None
        outs = tuple(state.t[s] for s in plan.outputs)
        return outs

    @staticmethod
    def backward(ctx, *gouts):
        plan = ctx.plan
        grad_feeds = {}
        for s, g in zip(plan.outputs, gouts):
            if g is not None:
                grad_feeds[s] = g.contiguous()
        in_grads, pgrads = backward(plan, ctx.state, grad_feeds, ctx.param_needs, ctx.requires, ctx.cfg.use_tr_read)
        ctx.state = None
        return (None, None, None) + tuple(in_grads[s] for s in plan.inputs) + tuple(pgrads)


def run_plan(plan, inputs, dtype, bn_train, use_tr_read=True, image_hw=None, input_nchw=None):
    """Differentiable execution of a plan. inputs: NHWC tensors for plan.inputs; returns NHWC outputs.
    image_hw: spatial size of the network input (for UpsampleUnit.size_fn).
    input_nchw: a contiguous fp32 [N,3,H,W] image that does NOT require a gradient, given INSTEAD of the single NHWC input (inputs is
    then ignored): the engine converts it itself, straight into the paired stem operand where the first unit is that stem."""
    cfg = SimpleNamespace(dtype=dtype, bn_train=bn_train, use_tr_read=use_tr_read, image_hw=image_hw, input_nchw=None)
    if input_nchw is not None:
        if len(plan.inputs) != 1 or input_nchw.requires_grad or input_nchw.dtype != torch.float32 or input_nchw.dim() != 4 or input_nchw.shape[1] != 3:
            raise ValueError("run_plan: input_nchw is a single fp32 [N,3,H,W] image without gradient")
        cfg.input_nchw = input_nchw.contiguous()
        N, _, H, W = input_nchw.shape
        inputs = [torch.empty((N, H, W, K.pad_channels(3)), dtype=dtype, device=input_nchw.device)]      # shape carrier only (never read, never filled)
    return _PlanFunction.apply(plan, cfg, len(inputs), *inputs, *plan.param_tensors())
