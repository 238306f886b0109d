"""Tensor-level wrappers over the C ABI (no autograd here).

Every function checks that its operands live on the GPU and are contiguous, then enqueues the HIP
kernel on torch's current stream.  Activations are NHWC tensors of dtype float32 (parity mode) or
bfloat16 (throughput mode) whose channel count is already padded (see ``pad_channels``).
"""
import ctypes

import torch

from . import _lib
from ._lib import (CS_ACT_NONE, CS_ACT_RELU, CS_ACT_SIGMOID, CS_ACT_SILU, CS_BF16, CS_BN_BWD_FROZEN, CS_BN_BWD_OWN_RELU, CS_F32,  # noqa: F401
                   CsConvGeom)


def _code(dtype):
    if dtype == torch.float32:
        return CS_F32
    if dtype == torch.bfloat16:
        return CS_BF16
    raise TypeError(f"unsupported activation dtype {dtype}; use torch.float32 or torch.bfloat16")


def _f32(*tensors):
    """the loss kernels read `const float*` only: any other dtype would be read as raw bits"""
    for t in tensors:
        if t.dtype != torch.float32:
            raise TypeError(f"this kernel reads torch.float32 only, got {t.dtype}; cast on the way in (functional.py does)")


def chunk(dtype):
    """Elements per 16-byte chunk."""
    return 4 if dtype == torch.float32 else 8


def pad_channels(c, dtype=None):
    """Stored channel count: multiple of 8 (a multiple of both chunk sizes)."""
    return (c + 7) // 8 * 8


def _p(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("cellsegmentation_amd kernels need GPU tensors: the HIP path has no CPU fallback")
    if not t.is_contiguous():
        raise RuntimeError("cellsegmentation_amd kernels need contiguous tensors")
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    # the raw handle of torch's current stream; ~10x cheaper than building a torch.cuda.Stream object per launch (the
    # BN-train image path issues ~1000 launches per step and is host-bound)
    return ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice()))


def make_geom(N, H, W, C, K, R, S, stride, pad, groups=1):
    P = (H + 2 * pad - R) // stride + 1
    Q = (W + 2 * pad - S) // stride + 1
    return CsConvGeom(N, H, W, C, K, R, S, stride, pad, P, Q, groups)


# ---------------------------------------------------------------- layout
def to_nhwc(x, dtype, Cp):
    """x[N,C,H,W] fp32 -> [N,H,W,Cp] dtype (zero padded channels)."""
    N, C, H, W = x.shape
    if x.dtype != torch.float32:
        raise TypeError("to_nhwc expects an fp32 NCHW tensor")
    y = torch.empty((N, H, W, Cp), dtype=dtype, device=x.device)
    _lib.check(_lib.load().cs_nchw_to_nhwc(_p(x), _p(y), _code(dtype), N, C, H, W, Cp, _stream()), "nchw_to_nhwc")
    return y


def to_nchw(y, C):
    """y[N,H,W,Cp] -> [N,C,H,W] fp32 (first C channels)."""
    N, H, W, Cp = y.shape
    x = torch.empty((N, C, H, W), dtype=torch.float32, device=y.device)
    _lib.check(_lib.load().cs_nhwc_to_nchw(_p(y), _code(y.dtype), _p(x), N, C, H, W, Cp, _stream()), "nhwc_to_nchw")
    return x


# ---------------------------------------------------------------- parameters
def bn_fold(gamma, beta, mean, var, eps, conv_bias=None):
    C = mean.numel()
    out = torch.empty((3, C), dtype=torch.float32, device=mean.device)
    _lib.check(_lib.load().cs_bn_fold(_p(gamma), _p(beta), _p(mean), _p(var), eps, _p(conv_bias), _p(out[0]), _p(out[1]), _p(out[2]),
                                      C, _stream()), "bn_fold")
    return out[0], out[1], out[2]


def _stage_desc(d, conv, bn, Cp, Kp, want_bwd, fwd_packed, bwd_packed, dtype):
    """Fill the CsStageDesc `d` for one ungrouped Conv2d and allocate what it writes.  bn: the eval-mode BatchNorm2d folded into
    the operands, or None (scale 1, shift = the convolution's bias or 0).  *_packed: that operand is written in the MFMA-fragment
    order of the packed-operand kernels (conv_v2.hip).  Returns (w_khwc, w_chwk or None, scale, shift, rstd), the last three [Kp]."""
    K_, Cin, R, S = conv.weight.shape
    dev = conv.weight.device
    bwd_packed = bool(bwd_packed and want_bwd)
    if (fwd_packed and (Kp % 32 or Cp % 64)) or (bwd_packed and (Cp % 32 or Kp % 64)):
        raise ValueError("weight staging: packed layouts need 32-row tiles and 64-channel chunks")
    w_khwc = torch.empty((Kp, R, S, Cp), dtype=dtype, device=dev)
    w_chwk = torch.empty((Cp, R, S, Kp), dtype=dtype, device=dev) if want_bwd else None
    vec = torch.empty((3, Kp), dtype=torch.float32, device=dev)

    def ptr(t):
        return None if t is None else _p(t).value

    d.w, d.conv_bias = ptr(conv.weight), ptr(conv.bias)
    if bn is not None:
        d.gamma, d.beta, d.mean, d.var = ptr(bn.weight), ptr(bn.bias), ptr(bn.running_mean), ptr(bn.running_var)
    else:
        d.gamma = d.beta = d.mean = d.var = None
    d.w_khwc, d.w_chwk = ptr(w_khwc), ptr(w_chwk)
    d.scale, d.shift, d.rstd = ptr(vec[0]), ptr(vec[1]), ptr(vec[2])
    d.eps = float(bn.eps) if bn is not None else 0.0
    d.K, d.Cin, d.R, d.S, d.Cp, d.Kp, d.block0 = K_, Cin, R, S, Cp, Kp, 0
    d.fwd_packed, d.bwd_packed = int(bool(fwd_packed)), int(bwd_packed)
    return w_khwc, w_chwk, vec[0], vec[1], vec[2]


def stage_layer(conv, bn, dtype, Cp, Kp, want_bwd=False, fwd_packed=False, bwd_packed=False):
    """BN fold (bn = None: nothing folded) + both weight operands of ONE ungrouped Conv2d, plain or packed, in one launch whose
    descriptor travels as the kernel argument (no device table, no copy: it may run inside a stream capture).
    Returns w_khwc, w_chwk, scale, shift, rstd as _stage_desc does."""
    d = _lib.CsStageDesc()
    staged = _stage_desc(d, conv, bn, Cp, Kp, want_bwd, fwd_packed, bwd_packed, dtype)
    _lib.check(_lib.load().cs_stage_conv_bn_one(ctypes.byref(d), _code(dtype), _stream()), "stage_conv_bn_one")
    return staged


class StagePack:
    """Every Conv2d(+eval-mode BatchNorm2d) of a network staged by ONE launch (cs_stage_conv_bn_multi).

    layers: [(conv, bn, Cp, Kp, want_bwd, fwd_packed, bwd_packed)] as _stage_desc takes them; bn = None for a layer whose BatchNorm
    runs on batch statistics.  The staging buffers and the device descriptor table are allocated once and rewritten by every
    launch(); valid() tells whether the parameter tensors are still the ones the table points at."""

    def __init__(self, layers, dtype):
        lib = _lib.load()
        dev = layers[0][0].weight.device
        self.dtype, self.layers, self.staged = dtype, layers, []
        arr = (_lib.CsStageDesc * len(layers))()
        block = 0
        for d, (conv, bn, Cp, Kp, want_bwd, pkf, pkb) in zip(arr, layers):
            self.staged.append(_stage_desc(d, conv, bn, Cp, Kp, want_bwd, pkf, pkb, dtype))
            nb = lib.cs_stage_conv_bn_blocks(d.K, d.Cin, d.R, d.S, Cp, Kp, 1, 1 if want_bwd else 0)
            if nb < 1:
                raise ValueError("StagePack: bad layer extents")
            d.block0 = block
            block += nb
        self.total_blocks = block
        self.table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
        self.key = self._key()

    def _key(self):
        out = []
        for conv, bn, *_ in self.layers:
            for t in (conv.weight, conv.bias) + ((bn.weight, bn.bias, bn.running_mean, bn.running_var) if bn is not None else ()):
                out.append(t.data_ptr() if t is not None else 0)
        return tuple(out)

    def valid(self):
        return self._key() == self.key

    def launch(self):
        _lib.check(_lib.load().cs_stage_conv_bn_multi(self.table.data_ptr(), len(self.layers), self.total_blocks, _code(self.dtype), _stream()),
                   "stage_conv_bn_multi")


def weight_prep(w, scale, dtype, Cp, Kp, want_fwd=True, want_bwd=False):
    K, Cin, R, S = w.shape
    w_khwc = torch.empty((Kp, R, S, Cp), dtype=dtype, device=w.device) if want_fwd else None
    w_chwk = torch.empty((Cp, R, S, Kp), dtype=dtype, device=w.device) if want_bwd else None
    _lib.check(_lib.load().cs_weight_prep(_p(w), _p(scale), _code(dtype), K, Cin, R, S, Cp, Kp, _p(w_khwc), _p(w_chwk),
                                          _stream()), "weight_prep")
    return w_khwc, w_chwk


# ---------------------------------------------------------------- convolution family
class LaunchTimer:
    """Optional per-launch HIP-event timing of the conv family (used by bench.py for the roofline
    object).  Events are recorded on torch's current stream = the stream the kernels run on."""

    def __init__(self):
        self.records = []      # (kind, geom tuple, dtype, start, end)
        self.enabled = True    # the caller may switch the bracketing off for some steps

    def __enter__(self):
        global _timer
        _timer = self
        return self

    def __exit__(self, *exc):
        global _timer
        _timer = None

    def results(self):
        """[(kind, geom dict, dtype, milliseconds)] -- call after torch.cuda.synchronize()."""
        return [(k, g, d, s.elapsed_time(e)) for k, g, d, s, e in self.records]


_timer = None


def _timed(kind, geom, dtype, fn, extra_tensors=0, batch=1):
    """extra_tensors: how many destination-shaped tensors the epilogue also reads (residual / add / mask)."""
    if _timer is None or not _timer.enabled:
        return fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    rc = fn()
    e.record()
    g = {f: getattr(geom, f) for f, _ in geom._fields_}
    g["extra"] = extra_tensors
    g["batch"] = batch
    g["variant"] = (_lib.load().cs_last_conv_variant() or b"").decode()      # what the library actually launched
    _timer.records.append((kind, g, dtype, s, e))
    return rc


def _stats_ws(M, n_out, device):
    nbytes = _lib.load().cs_conv2d_stats_workspace(int(M), int(n_out))
    return torch.empty((nbytes // 4,), dtype=torch.float32, device=device)


def set_igemm_path(path):
    """0 = LDS-DMA staging (default), 1 = register staging; any other value is refused. Returns the previous value.
    A/B flavour of the library only (CELLSEG_LIB_FLAVOUR=ab, `make AB=1`): the production library has no such switch."""
    if _lib.FLAVOUR != "ab":
        raise RuntimeError("set_igemm_path: the production library has no A/B switches; run with CELLSEG_LIB_FLAVOUR=ab")
    old = _lib.load().cs_set_igemm_path(int(path))
    if old < 0:
        _lib.check(old, "set_igemm_path")
    return old


def igemm_tile(M, n_out):
    """(BM, BN) the fwd/dgrad dispatcher picks."""
    v = _lib.load().cs_igemm_tile(int(M), int(n_out))
    return v // 1000, v % 1000


def weight_prep_grouped(w, scale, dtype, want_fwd=True, want_bwd=False):
    """w[K][Cg][R][S] (groups = K // Cg... i.e. Conv2d(groups=G).weight) -> slab-dense operands [K][R][S][64]."""
    K_, Cg, R, S = w.shape
    w_khwc = torch.empty((K_, R, S, 64), dtype=dtype, device=w.device) if want_fwd else None
    w_chwk = torch.empty((K_, R, S, 64), dtype=dtype, device=w.device) if want_bwd else None
    _lib.check(_lib.load().cs_weight_prep_grouped(_p(w), _p(scale), _code(dtype), K_, Cg, R, S, _p(w_khwc), _p(w_chwk), _stream()),
               "weight_prep_grouped")
    return w_khwc, w_chwk


def wgrad_finalize_grouped(dw_slab, w, scale, rstd, mean, gsum, dw, dgamma=None, dbeta=None, dot=None):
    K_, Cg, R, S = dw.shape
    if dgamma is not None and dot is None:
        dot = torch.zeros((K_,), dtype=torch.float32, device=dw.device)
    _lib.check(_lib.load().cs_wgrad_finalize_grouped(_p(dw_slab), dw_slab.shape[0], _p(w), _p(scale), _p(rstd), _p(mean), _p(gsum), K_, Cg, R, S, _p(dw),
                                                     _p(dgamma), _p(dbeta), _p(dot), _stream()), "wgrad_finalize_grouped")


def _grouped_geom(geom, grouped):
    """The geometry the C side sees: `groups > 1` selects the slab-dense grouped kernels (an explicit field of CsConvGeom; the
    library keeps no per-thread state between calls)."""
    if not grouped or geom.groups > 1:
        return geom
    g = CsConvGeom.from_buffer_copy(geom)
    g.groups = max(2, geom.C // 64 if geom.C >= 128 else 2)      # any value > 1: the staged weights carry the block structure
    return g


def conv_fwd(geom, x, w_khwc, scale=None, shift=None, residual=None, act=CS_ACT_NONE, stats=None, out=None, grouped=False,
             want_bits=False):
    """want_bits: also return a uint8 [N,P,Q,K/8] tensor with one bit per output element (> 0), the 1-byte-per-16 form of the
    ReLU mask a later data gradient needs -> (y, bits)."""
    y = out if out is not None else torch.empty((geom.N, geom.P, geom.Q, geom.K), dtype=x.dtype, device=x.device)
    lib = _lib.load()
    geom = _grouped_geom(geom, grouped)
    if want_bits:
        if stats is not None:
            raise ValueError("conv_fwd: want_bits and stats are separate entry points")
        bits = torch.empty((geom.N, geom.P, geom.Q, geom.K // 8), dtype=torch.uint8, device=x.device)
        _lib.check(_timed("fwd", geom, x.dtype, lambda: lib.cs_conv2d_fwd_bits(
            ctypes.byref(geom), _code(x.dtype), _p(x), _p(w_khwc), _p(scale), _p(shift), _p(residual), act, _p(y), _p(bits), _stream()),
            extra_tensors=int(residual is not None) + 1.0 / (8 * y.element_size())), "conv2d_fwd_bits")
        return y, bits
    ws = _stats_ws(geom.N * geom.P * geom.Q, geom.K, x.device) if stats is not None else None
    _lib.check(_timed("fwd", geom, x.dtype, lambda: lib.cs_conv2d_fwd(
        ctypes.byref(geom), _code(x.dtype), _p(x), _p(w_khwc), _p(scale), _p(shift), _p(residual), act, _p(y), _p(stats), _p(ws),
        _stream()), extra_tensors=int(residual is not None)), "conv2d_fwd")
    return y


# ---------------------------------------------------------------- packed-operand bf16 convolutions (csrc/conv_v2.hip)
def packed_supported(geom, dtype, dgrad=False):
    """Does the halo-tile / packed-weight kernel serve this geometry (bf16 only)?"""
    return dtype == torch.bfloat16 and bool(_lib.load().cs_conv2d_packed_supported(ctypes.byref(geom), 1 if dgrad else 0))


def pack_conv_weights(geom, w_staged, dgrad=False, out=None):
    """staged w_khwc (forward) / w_chwk (data gradient) -> MFMA-fragment order (a flat bf16 tensor)."""
    lib = _lib.load()
    n = lib.cs_conv2d_packed_weight_bytes(ctypes.byref(geom), 1 if dgrad else 0) // 2
    if out is None:
        out = torch.empty((n,), dtype=torch.bfloat16, device=w_staged.device)
    _lib.check(lib.cs_pack_conv_weights(ctypes.byref(geom), 1 if dgrad else 0, _p(w_staged), _p(out), _stream()), "pack_conv_weights")
    return out


def conv_fwd_packed(geom, x, w_packed, shift=None, residual=None, act=CS_ACT_NONE, want_bits=False, out=None):
    y = out if out is not None else torch.empty((geom.N, geom.P, geom.Q, geom.K), dtype=x.dtype, device=x.device)
    bits = torch.empty((geom.N, geom.P, geom.Q, geom.K // 8), dtype=torch.uint8, device=x.device) if want_bits else None
    lib = _lib.load()
    _lib.check(_timed("fwd", geom, x.dtype, lambda: lib.cs_conv2d_fwd_packed(
        ctypes.byref(geom), _p(x), _p(w_packed), _p(shift), _p(residual), act, _p(y), _p(bits), _stream()),
        extra_tensors=int(residual is not None) + (1.0 / 16 if want_bits else 0.0)), "conv2d_fwd_packed")
    return (y, bits) if want_bits else y


def conv_fwd_shortcut_supported(geom, geom_sc, dtype):
    """Does one launch serve the 1x1 convolution `geom` together with the 1x1 projection shortcut `geom_sc` that feeds its residual
    (conv_fwd_shortcut_packed; bf16 only)?"""
    return dtype == torch.bfloat16 and bool(_lib.load().cs_conv2d_fwd_shortcut_supported(ctypes.byref(geom), ctypes.byref(geom_sc)))


def conv_fwd_shortcut_packed(geom, x, w_packed, shift, geom_sc, x_in, w_packed_sc, shift_sc, act=CS_ACT_NONE, want_bits=False, out=None):
    """y = act(conv(x, w) + shift + bf16(conv(x_in, w_sc) + shift_sc)): the two 1x1 convolutions in one launch -- the shortcut's
    output never reaches memory, the values are those of the two launches.  Timed under the main geometry: the row's byte and FLOP
    model (that of a one-source forward) does not count the second source."""
    y = out if out is not None else torch.empty((geom.N, geom.P, geom.Q, geom.K), dtype=x.dtype, device=x.device)
    bits = torch.empty((geom.N, geom.P, geom.Q, geom.K // 8), dtype=torch.uint8, device=x.device) if want_bits else None
    lib = _lib.load()
    _lib.check(_timed("fwd", geom, x.dtype, lambda: lib.cs_conv2d_fwd_shortcut_packed(
        ctypes.byref(geom), _p(x), _p(w_packed), _p(shift), ctypes.byref(geom_sc), _p(x_in), _p(w_packed_sc), _p(shift_sc), act, _p(y), _p(bits),
        _stream()), extra_tensors=1.0 / 16 if want_bits else 0.0), "conv2d_fwd_shortcut_packed")
    return (y, bits) if want_bits else y


class CompactGrad:
    """The data gradient of a stride-2 1x1 convolution in compact form: `t` [N][P][Q][C] holds the values of the destination pixels
    (2y, 2x); every other pixel of that gradient is zero and was never written.  Only a packed 1x1 data gradient can consume it
    (conv_dgrad_packed(add=CompactGrad))."""

    def __init__(self, t, stride):
        self.t, self.stride = t, stride


def conv_dgrad_packed(geom, dy, w_packed, add=None, mask_bits=None, want_colsum=False):
    """-> dx, or (dx, PartialColsum) with want_colsum.  A stride-2 1x1 geometry returns a CompactGrad (no add / mask / column sums);
    `add` may be such a CompactGrad of the same destination."""
    lib = _lib.load()
    if geom.stride != 1:
        if add is not None or mask_bits is not None or want_colsum:
            raise ValueError("conv_dgrad_packed: a strided 1x1 data gradient is compact -- no add, mask or column sums")
        dxc = torch.empty((geom.N, geom.P, geom.Q, geom.C), dtype=dy.dtype, device=dy.device)
        _lib.check(_timed("dgrad", geom, dy.dtype, lambda: lib.cs_conv2d_dgrad_packed(
            ctypes.byref(geom), _p(dy), _p(w_packed), None, 1, None, _p(dxc), None, _stream()), extra_tensors=-0.75), "conv2d_dgrad_packed")
        return CompactGrad(dxc, geom.stride)
    add_stride = 1
    if isinstance(add, CompactGrad):
        add_stride, add = add.stride, add.t
        if tuple(add.shape) != (geom.N, (geom.H + 1) // 2, (geom.W + 1) // 2, geom.C):
            raise ValueError("conv_dgrad_packed: compact add operand of another destination")
    dx = torch.empty((geom.N, geom.H, geom.W, geom.C), dtype=dy.dtype, device=dy.device)
    rows = lib.cs_conv2d_packed_partial_rows(ctypes.byref(geom), 1) if want_colsum else 0
    ws = torch.empty((rows, 2 * geom.C), dtype=torch.float32, device=dy.device) if want_colsum else None
    _lib.check(_timed("dgrad", geom, dy.dtype, lambda: lib.cs_conv2d_dgrad_packed(
        ctypes.byref(geom), _p(dy), _p(w_packed), _p(add), add_stride, _p(mask_bits), _p(dx), _p(ws), _stream()),
        extra_tensors=(int(add is not None) if add_stride == 1 else 0.25) + (1.0 / 16 if mask_bits is not None else 0.0)), "conv2d_dgrad_packed")
    if want_colsum:
        return dx, PartialColsum(ws, rows, geom.C)
    return dx


# ---------------------------------------------------------------- stem on a pixel-paired image (cs_stem_*)
def is_stem_geom(geom):
    """Conv2d(3 -> K, 7x7, stride 2, padding 3) on an NHWC8 image: the layer the paired path replaces."""
    return geom.R == 7 and geom.S == 7 and geom.stride == 2 and geom.pad == 3 and geom.C == 8


def stem_pair_input(x):
    """x[N,H,W,8] (channels 3.. zero) -> [N,H,ceil(W/2),8]: two neighbouring pixels x 4 channels per 16-byte chunk."""
    N, H, W, C = x.shape
    if C != 8:
        raise ValueError("stem_pair_input expects an NHWC image with 8 stored channels")
    out = torch.empty((N, H, (W + 1) // 2, 8), dtype=x.dtype, device=x.device)
    _lib.check(_lib.load().cs_stem_pair_input(_p(x), _code(x.dtype), N, H, W, _p(out), _stream()), "stem_pair_input")
    return out


def stem_pair_from_nchw(x_nchw, dtype):
    """fp32 NCHW image [N,3,H,W] -> the paired stem operand [N,H,ceil(W/2),8] of `dtype` (bf16), without the NHWC8 intermediate."""
    N, C, H, W = x_nchw.shape
    if C != 3 or x_nchw.dtype != torch.float32 or not x_nchw.is_contiguous():
        raise ValueError("stem_pair_from_nchw expects a contiguous fp32 [N,3,H,W] image")
    out = torch.empty((N, H, (W + 1) // 2, 8), dtype=dtype, device=x_nchw.device)
    _lib.check(_lib.load().cs_stem_pair_from_nchw(_p(x_nchw), _code(dtype), N, H, W, _p(out), _stream()), "stem_pair_from_nchw")
    return out


def stem_pair_weights(w_khwc):
    """staged [K,7,7,8] -> paired [K,7,4,8]."""
    K_ = w_khwc.shape[0]
    out = torch.empty((K_, 7, 4, 8), dtype=w_khwc.dtype, device=w_khwc.device)
    _lib.check(_lib.load().cs_stem_pair_weights(_p(w_khwc), _code(w_khwc.dtype), K_, _p(out), _stream()), "stem_pair_weights")
    return out


def stem_fwd(geom, x_pair, w_pair, scale=None, shift=None, act=CS_ACT_NONE, stats=None):
    """cs_conv2d_fwd of the stem geometry `geom` (the 7x7 one: it names the launch for the timers) on paired operands."""
    y = torch.empty((geom.N, geom.P, geom.Q, geom.K), dtype=x_pair.dtype, device=x_pair.device)
    lib = _lib.load()
    ws = _stats_ws(geom.N * geom.P * geom.Q, geom.K, x_pair.device) if stats is not None else None
    _lib.check(_timed("fwd", geom, x_pair.dtype, lambda: lib.cs_stem_fwd(
        geom.N, geom.H, geom.W, geom.K, _code(x_pair.dtype), _p(x_pair), _p(w_pair), _p(scale), _p(shift), act, _p(y), _p(stats), _p(ws),
        _stream())), "stem_fwd")
    return y


def stem_pack_weights(w_pair):
    """paired stem weights [K][7][4][8] bf16 -> the packed operand of stem_fwd_packed: one zero filter row appended ([K][256]) and
    re-ordered like a 1x1 convolution's forward weights."""
    K_ = w_pair.shape[0]
    w256 = torch.zeros((K_, 1, 1, 256), dtype=w_pair.dtype, device=w_pair.device)
    w256.view(K_, 256)[:, :224] = w_pair.reshape(K_, 224)
    return pack_conv_weights(make_geom(1, 2, 2, 256, K_, 1, 1, 1, 0), w256, dgrad=False)


def stem_fwd_packed_supported(geom, dtype):
    return dtype == torch.bfloat16 and is_stem_geom(geom) and geom.K == 64 and geom.P >= 2 and geom.Q >= 2


def stem_fwd_packed(geom, x_pair, w_packed, shift=None, act=CS_ACT_NONE, want_bits=False):
    """The stem forward on the ring kernel (bf16): y, or (y, bits)."""
    y = torch.empty((geom.N, geom.P, geom.Q, geom.K), dtype=x_pair.dtype, device=x_pair.device)
    bits = torch.empty((geom.N, geom.P, geom.Q, geom.K // 8), dtype=torch.uint8, device=x_pair.device) if want_bits else None
    lib = _lib.load()
    _lib.check(_timed("fwd", geom, x_pair.dtype, lambda: lib.cs_stem_fwd_packed(
        geom.N, geom.H, geom.W, geom.K, _p(x_pair), _p(w_packed), _p(shift), act, _p(y), _p(bits), _stream()),
        extra_tensors=1.0 / 16 if want_bits else 0), "stem_fwd_packed")
    return (y, bits) if want_bits else y


def stem_pool_fwd_supported(geom, dtype):
    """Does cs_stem_pool_fwd (stem forward + ReLU + MaxPool2d(3, 2, 1) in one launch) serve this stem geometry?"""
    return (dtype == torch.bfloat16 and is_stem_geom(geom)
            and bool(_lib.load().cs_stem_pool_fwd_supported(geom.N, geom.H, geom.W, geom.K)))


def stem_pool_fwd(geom, x_pair, w_pair, shift, want_argmax=True):
    """max_pool(relu(stem(x) + shift)) of the stem geometry `geom` without the stem map in between: (y_pool, argmax or None), the
    values maxpool_fwd(stem_fwd_packed(...)) returns.  w_pair: the paired weights [K,7,4,8] of stem_pair_weights."""
    PP, PQ = (geom.P - 1) // 2 + 1, (geom.Q - 1) // 2 + 1
    y = torch.empty((geom.N, PP, PQ, geom.K), dtype=x_pair.dtype, device=x_pair.device)
    am = torch.empty((geom.N, PP, PQ, geom.K), dtype=torch.uint8, device=x_pair.device) if want_argmax else None
    lib = _lib.load()
    _lib.check(_timed("fwd", geom, x_pair.dtype, lambda: lib.cs_stem_pool_fwd(
        geom.N, geom.H, geom.W, geom.K, _p(x_pair), _p(w_pair), _p(shift), _p(y), _p(am), _stream())), "stem_pool_fwd")
    return y, am


def stem_wgrad(geom, x_pair, dy, use_tr_read=True):
    """Raw weight gradient of the stem in the ORDINARY slab layout [1, K, 7, 7, 8] (one slab: the paired split-K slabs are summed
    while they are un-paired), ready for wgrad_finalize / wgrad_finalize_batched."""
    lib = _lib.load()
    nsplit = lib.cs_stem_wgrad_splits(geom.N, geom.H, geom.W, geom.K)
    pair = torch.empty((nsplit, geom.K, 7, 4, 8), dtype=torch.float32, device=dy.device)
    _lib.check(_timed("wgrad", geom, dy.dtype, lambda: lib.cs_stem_wgrad(
        geom.N, geom.H, geom.W, geom.K, _code(dy.dtype), _p(x_pair), _p(dy), _p(pair), 1 if use_tr_read else 0, _stream())), "stem_wgrad")
    raw = torch.empty((1, geom.K, 7, 7, 8), dtype=torch.float32, device=dy.device)
    _lib.check(lib.cs_stem_unpair_slabs(_p(pair), nsplit, geom.K, _p(raw), _stream()), "stem_unpair_slabs")
    return raw


class PartialColsum:
    """Column sums of a dgrad output still in per-workgroup partial rows (cs_conv2d_dgrad with colsum == NULL): the batched
    weight-gradient finalize folds them itself; vector() folds them now for any other consumer."""

    def __init__(self, buf, rows, n_out):
        self.buf, self.rows, self.n_out = buf, rows, n_out
        self._vec = None
        self._vec_stream = None      # the stream the fold ran on (weight gradients may run on a side stream)

    def _set(self, vec):
        self._vec, self._vec_stream = vec, torch.cuda.current_stream()

    def _sync(self):
        cur = torch.cuda.current_stream()
        if self._vec_stream is not None and cur != self._vec_stream:
            cur.wait_stream(self._vec_stream)
        return self._vec

    def vector(self):
        if self._vec is None:
            vec = torch.zeros((self.n_out,), dtype=torch.float32, device=self.buf.device)
            _lib.check(_lib.load().cs_fold_partial_rows(_p(self.buf), self.rows, self.n_out, _p(vec), _stream()), "fold_partial_rows")
            self._set(vec)
        return self._sync()


def colsum_vector(g):
    """A [C] fp32 tensor from either form of column sums."""
    return g.vector() if isinstance(g, PartialColsum) else g


def conv_dgrad(geom, dy, w_chwk, add=None, mask=None, colsum=None, grouped=False, defer_colsum=False, mask_bits=None):
    """colsum: zeroed fp32 [C] to accumulate the column sums of dx into; or defer_colsum=True (stride 1, ungrouped) to get
    (dx, PartialColsum) with the fold left to the consumer.  mask_bits: uint8 [N,H,W,C/8] from conv_fwd(want_bits=True), used
    instead of `mask`."""
    dx = torch.empty((geom.N, geom.H, geom.W, geom.C), dtype=dy.dtype, device=dy.device)
    lib = _lib.load()
    geom = _grouped_geom(geom, grouped)
    # (stride 2: deferrable when the library merges the parity classes into one launch -- it then reports the row count, else 0)
    defer = defer_colsum and not grouped and (geom.stride == 1 or lib.cs_conv2d_dgrad_partial_rows(ctypes.byref(geom)) > 0)
    ws = _stats_ws(geom.N * geom.H * geom.W, geom.C, dy.device) if (colsum is not None or defer) else None
    if mask_bits is not None:
        _lib.check(_timed("dgrad", geom, dy.dtype, lambda: lib.cs_conv2d_dgrad_bits(
            ctypes.byref(geom), _code(dy.dtype), _p(dy), _p(w_chwk), _p(add), _p(mask_bits), _p(dx), None if defer else _p(colsum), _p(ws),
            _stream()), extra_tensors=int(add is not None) + 1.0 / (8 * dx.element_size())), "conv2d_dgrad_bits")
    else:
        _lib.check(_timed("dgrad", geom, dy.dtype, lambda: lib.cs_conv2d_dgrad(
            ctypes.byref(geom), _code(dy.dtype), _p(dy), _p(w_chwk), _p(add), _p(mask), _p(dx), None if defer else _p(colsum), _p(ws), _stream()),
            extra_tensors=int(add is not None) + int(mask is not None)), "conv2d_dgrad")
    if defer_colsum:
        if defer:
            return dx, PartialColsum(ws, lib.cs_conv2d_dgrad_partial_rows(ctypes.byref(geom)), geom.C)
        return dx, colsum
    return dx


def wgrad_splits(geom, grouped=False):
    return _lib.load().cs_conv2d_wgrad_splits(ctypes.byref(geom), 1 if grouped else 0)


def new_wgrad_buffer(geom, device, grouped=False):
    """[nsplit, K, R, S, Cp|64] fp32 split-K partial slabs (no zero-fill needed)."""
    return torch.empty((wgrad_splits(geom, grouped), geom.K, geom.R, geom.S, 64 if grouped else geom.C), dtype=torch.float32, device=device)


def conv_wgrad(geom, x, dy, dw_raw, use_tr_read=True, grouped=False):
    """dw_raw = new_wgrad_buffer(...): every slab is fully written by the kernel."""
    if dw_raw.dim() != 5 or dw_raw.shape[0] != wgrad_splits(geom, grouped):
        raise ValueError("conv_wgrad: dw_raw must come from new_wgrad_buffer(geom, ...)")
    lib = _lib.load()
    geom = _grouped_geom(geom, grouped)
    _lib.check(_timed("wgrad", geom, x.dtype, lambda: lib.cs_conv2d_wgrad(
        ctypes.byref(geom), _code(x.dtype), _p(x), _p(dy), _p(dw_raw), 1 if use_tr_read else 0, _stream())), "conv2d_wgrad")
    return dw_raw


def wgrad2_serves(geom, dtype):
    """True when the batched weight-gradient entry runs this geometry on the second-generation kernel (csrc/wgrad_v2.hip)."""
    return bool(_lib.load().cs_conv2d_wgrad2_supported(ctypes.byref(geom), _code(dtype)))


def wgrad_batched(geom, xs, dys, use_tr_read=True):
    """Batched wgrad over len(xs) <= 8 layers of identical geometry.  Returns the split-K slab buffer [n, nsplit, K, R, S, Cp]."""
    n = len(xs)
    lib = _lib.load()
    nsplit = lib.cs_conv2d_wgrad_batched_splits(ctypes.byref(geom), _code(xs[0].dtype), n)
    slabs = torch.empty((n, nsplit, geom.K, geom.R, geom.S, geom.C), dtype=torch.float32, device=xs[0].device)
    for t in list(xs) + list(dys):
        _p(t)                                  # device / contiguity checks
    arr = ctypes.c_void_p * n
    xt, dt_, wt = arr(*[t.data_ptr() for t in xs]), arr(*[t.data_ptr() for t in dys]), arr(*[slabs[i].data_ptr() for i in range(n)])
    _lib.check(_timed("wgrad", geom, xs[0].dtype, lambda: lib.cs_conv2d_wgrad_batched(
        ctypes.byref(geom), _code(xs[0].dtype), xt, dt_, wt, n, 1 if use_tr_read else 0, _stream()), batch=n), "conv2d_wgrad_batched")
    return slabs


def wgrad_finalize_batched(slabs, ws, scales, rstds, means, gsums, dws, dgammas, dbetas, Cin):
    """Batched finalize for the eval-BN trunk: lists of n <= 8 tensors each, ONE launch.  gsums: [K] vectors or PartialColsum objects
    (deferred column sums of a data-gradient launch: the kernel folds the partial rows of its channel itself)."""
    n, nsplit, Kp, R, S, Cp = slabs.shape
    K_ = dws[0].shape[0]
    want_bn = dgammas is not None

    def ptrs(lst):
        return [None] * n if lst is None else [t.data_ptr() for t in lst]

    grows, gstride, gptr = [0] * n, 0, [None] * n
    if gsums is not None:
        for i, g in enumerate(gsums):
            if isinstance(g, PartialColsum) and g._vec is None:
                grows[i], gptr[i] = g.rows, g.buf.data_ptr()
                if gstride not in (0, 2 * g.n_out):
                    raise ValueError("wgrad_finalize_batched: mixed partial-row strides")
                gstride = 2 * g.n_out           # partial rows are [rows][2][n_out] in every producer
            else:
                gptr[i] = colsum_vector(g).data_ptr()
    flat = [slabs[i].data_ptr() for i in range(n)] + ptrs(ws) + ptrs(scales) + ptrs(rstds) + ptrs(means) + gptr + ptrs(dws) + \
        ptrs(dgammas) + ptrs(dbetas)
    table = (ctypes.c_void_p * len(flat))(*flat)
    rows_arr = (ctypes.c_int * n)(*grows)
    _lib.check(_lib.load().cs_wgrad_finalize_batched(table, rows_arr, gstride, n, nsplit, Kp, K_, Cin, R, S, Cp, 1 if want_bn else 0,
                                                     _stream()), "wgrad_finalize_batched")


def wgrad_finalize(dw_raw, w, scale, rstd, mean, gsum, Cin, dw, dbias=None, dgamma=None, dbeta=None, accumulate=False, dot=None):
    """dot: zeroed fp32 [K] scratch (allocated here when omitted)."""
    nsplit, Kp, R, S, Cp = dw_raw.shape
    K = dw.shape[0]
    if dgamma is not None and dot is None:
        dot = torch.zeros((K,), dtype=torch.float32, device=dw.device)
    _lib.check(_lib.load().cs_wgrad_finalize(_p(dw_raw), nsplit, Kp, _p(w), _p(scale), _p(rstd), _p(mean), _p(gsum), K, Cin, R, S, Cp,
                                             _p(dw), _p(dbias), _p(dgamma), _p(dbeta), _p(dot), 1 if accumulate else 0, _stream()),
               "wgrad_finalize")


def colsum(g, out=None):
    """Per-channel sums of an NHWC tensor.  Without `out`: per-workgroup partial rows + one fold (no atomics: 512 adds per
    address serialise at the memory side and cost 3x the streaming time); with `out`: accumulated into it atomically."""
    C = g.shape[-1]
    M = g.numel() // C
    if out is None:
        return colsum_partial(g).vector()
    _lib.check(_lib.load().cs_colsum(_p(g), _code(g.dtype), M, C, _p(out), _stream()), "colsum")
    return out


def positive_bits(x):
    """Bit plane of a bf16 NHWC tensor: bit = x[..., c] > 0, in the channel-block-major layout of the convolution epilogues (the 32-bit
    word (c // 32) * M + pixel holds channels 32 (c // 32) .. + 31 of that pixel; unpack_bits / pack_bits translate) -- the `mask_bits`
    operand of the packed data gradients for a post-ReLU tensor that no convolution epilogue produced (train-mode BN + ReLU outputs,
    their concatenation).  Returned as uint8 [..., C/8] (a shape carrier: the bytes are NOT in NHWC order)."""
    C = x.shape[-1]
    if x.dtype != torch.bfloat16 or C % 32 or not x.is_contiguous():
        raise ValueError("positive_bits: contiguous bf16 tensor with a channel count that is a multiple of 32")
    bits = torch.empty(x.shape[:-1] + (C // 8,), dtype=torch.uint8, device=x.device)
    _lib.check(_lib.load().cs_positive_bits(_p(x), _code(x.dtype), x.numel() // C, C, _p(bits), _stream()), "positive_bits")
    return bits


def unpack_bits(bits, C):
    """bool [..., C] from a bit plane of the library (uint8, M * C / 8 bytes, channel-block-major: see positive_bits)."""
    M = bits.numel() * 8 // C
    words = bits.contiguous().view(-1).view(C // 32, M, 4)                       # [block][pixel][byte of the little-endian word]
    sh = torch.arange(8, dtype=torch.uint8, device=bits.device)
    b = ((words.unsqueeze(-1) >> sh) & 1).bool()                                  # [block][pixel][byte][bit]
    return b.permute(1, 0, 2, 3).reshape(tuple(bits.shape[:-1]) + (C,))


def pack_bits(mask):
    """The inverse: a bool / 0-1 tensor [..., C] (C % 32 == 0) -> uint8 [..., C/8] in the library's bit-plane layout."""
    C = mask.shape[-1]
    M = mask.numel() // C
    b = mask.reshape(M, C // 32, 4, 8).to(torch.uint8)
    w = (b << torch.arange(8, dtype=torch.uint8, device=mask.device)).sum(-1).to(torch.uint8)       # [pixel][block][byte]
    return w.permute(1, 0, 2).contiguous().view(tuple(mask.shape[:-1]) + (C // 8,))


def colsum_partial(g):
    """Column sums as a PartialColsum (per-workgroup partial rows, folded later together with its group's other sums)."""
    C = g.shape[-1]
    M = g.numel() // C
    lib = _lib.load()
    rows = lib.cs_colsum_partial_rows(M)
    buf = torch.empty((rows, 2 * C), dtype=torch.float32, device=g.device)
    _lib.check(lib.cs_colsum_partial(_p(g), _code(g.dtype), M, C, _p(buf), _stream()), "colsum_partial")
    return PartialColsum(buf, rows, C)


# ---------------------------------------------------------------- BatchNorm (train mode)
# Zero-initialised fp64 accumulators ([2, C] per BatchNorm reduction) come out of one pool per device that the engine clears ONCE
# per training pass (begin_pass) instead of one fill launch per accumulator (EfficientNet-B3: 104 fills of 4.8 us per step).
# Every user consumes its accumulator inside the call that took it (stream order), so clearing the whole pool at the start of the
# next pass is safe; without begin_pass (direct calls from tests / tools) the pool is used once and then falls back to torch.zeros.
_STATS_POOL_ELEMS = 1 << 21           # 8-byte words (16 MB): an exact accumulator takes 6 C + 1 of them (cs_bn_accum_words)
_stats_pools = {}


def accum_words(C):
    """8-byte words of the exact per-channel accumulator of a C-channel BatchNorm reduction (cs_bn_accum_words: three fp64 limbs per sum
    and channel, each added to exactly, + one flag word; order-independent adds, so batch statistics repeat bit for bit)."""
    return 6 * C + 1


def begin_pass(device):
    pool = _stats_pools.get(device)
    if pool is None:
        _stats_pools[device] = [torch.zeros((_STATS_POOL_ELEMS,), dtype=torch.float64, device=device), 0]
    else:
        pool[0].zero_()
        pool[1] = 0


def new_stats(C, device):
    """A zeroed exact accumulator for C channels (opaque words, dtype float64 for history; stats_values() reads the totals)."""
    n = accum_words(C)
    pool = _stats_pools.get(device)
    if pool is not None and pool[1] + n <= _STATS_POOL_ELEMS:
        v = pool[0][pool[1]:pool[1] + n]
        pool[1] += n
        return v
    return torch.zeros((n,), dtype=torch.float64, device=device)


def stats_channels(stats):
    n = stats.numel()
    if n < 7 or (n - 1) % 6:
        raise ValueError("not a BatchNorm accumulator (kernels.new_stats)")
    return (n - 1) // 6


def stats_values(stats):
    """fp64 [2, C]: the two per-channel totals an exact accumulator holds (cs_bn_accum_read; tests and tools)."""
    C = stats_channels(stats)
    out = torch.empty((2, C), dtype=torch.float64, device=stats.device)
    _lib.check(_lib.load().cs_bn_accum_read(_p(stats), C, _p(out), _stream()), "bn_accum_read")
    return out


def bn_stats(z, stats=None):
    C = z.shape[-1]
    M = z.numel() // C
    if stats is None:
        stats = new_stats(C, z.device)
    _lib.check(_lib.load().cs_bn_stats(_p(z), _code(z.dtype), M, C, _p(stats), _p(_bn_ws(M, C, z.device)), _stream()), "bn_stats")
    return stats


def _bn_ws(M, C, device):
    """Partial-sum workspace of the BN reductions, or None where the library wants none (cs_bn_partial_workspace returns 0: few
    workgroups, fp64 atomics -- nearly every layer; the decision is the library's alone)."""
    nbytes = _lib.load().cs_bn_partial_workspace(M, C)
    if nbytes == 0:
        return None
    return torch.empty((nbytes // 8,), dtype=torch.float64, device=device)


def bn_finalize(stats, M, eps, momentum, running_mean=None, running_var=None):
    C = stats_channels(stats)
    out = torch.empty((2, C), dtype=torch.float32, device=stats.device)
    _lib.check(_lib.load().cs_bn_finalize(_p(stats), M, eps, momentum, _p(running_mean), _p(running_var), _p(out[0]), _p(out[1]), C,
                                          _stream()), "bn_finalize")
    return out[0], out[1]


def bn_apply(z, mean, rstd, gamma, beta, residual=None, act=CS_ACT_NONE, out=None):
    C = z.shape[-1]
    M = z.numel() // C
    y = out if out is not None else torch.empty_like(z)
    _lib.check(_lib.load().cs_bn_apply(_p(z), _code(z.dtype), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(residual), act, _p(y), M, C,
                                       _stream()), "bn_apply")
    return y


def bn_apply_stats(z, stats, eps, momentum, running_mean, running_var, gamma, beta, residual=None, act=CS_ACT_NONE):
    """bn_finalize + bn_apply as one launch: returns (y, mean, rstd); the running statistics (nullable) are updated in place."""
    C = z.shape[-1]
    M = z.numel() // C
    y = torch.empty_like(z)
    out = torch.empty((2, C), dtype=torch.float32, device=z.device)
    _lib.check(_lib.load().cs_bn_apply_stats(_p(z), _code(z.dtype), _p(stats), eps, momentum, _p(running_mean), _p(running_var), _p(gamma),
                                             _p(beta), _p(residual), act, _p(y), _p(out[0]), _p(out[1]), M, C, _stream()), "bn_apply_stats")
    return y, out[0], out[1]


def bn_bwd(dy, z, mean, rstd, gamma, want_param_grads=True, beta=None, act=CS_ACT_NONE):
    """returns dz, dgamma, dbeta.  act=CS_ACT_SILU differentiates through the SiLU that follows the BN."""
    C = z.shape[-1]
    M = z.numel() // C
    sums = new_stats(C, z.device)
    lib = _lib.load()
    _lib.check(lib.cs_bn_bwd_reduce(_p(dy), _p(z), _code(z.dtype), _p(mean), _p(rstd), _p(gamma), _p(beta), act, M, C, _p(sums),
                                    _p(_bn_ws(M, C, z.device)), _stream()), "bn_bwd_reduce")
    dz = torch.empty_like(z)
    dg = torch.empty((2, C), dtype=torch.float32, device=z.device) if want_param_grads else None
    _lib.check(lib.cs_bn_bwd_apply(_p(dy), _p(z), _code(z.dtype), _p(mean), _p(rstd), _p(gamma), _p(beta), act, _p(sums), M, C, _p(dz),
                                   _p(dg[0]) if dg is not None else None, _p(dg[1]) if dg is not None else None, _stream()),
               "bn_bwd_apply")
    return dz, (dg[0] if dg is not None else None), (dg[1] if dg is not None else None)


# ---------------------------------------------------------------- decoder data movement
def bilinear_fwd(x, out_hw):
    N, H, W, C = x.shape
    P, Q = out_hw
    y = torch.empty((N, P, Q, C), dtype=x.dtype, device=x.device)
    _lib.check(_lib.load().cs_bilinear_ac_fwd(_p(x), _code(x.dtype), _p(y), N, H, W, C, P, Q, _stream()), "bilinear_fwd")
    return y


def bilinear_bwd(dy, in_hw, mask=None):
    N, P, Q, C = dy.shape
    H, W = in_hw
    dx = torch.empty((N, H, W, C), dtype=dy.dtype, device=dy.device)
    _lib.check(_lib.load().cs_bilinear_ac_bwd(_p(dy), _p(mask), _code(dy.dtype), _p(dx), N, H, W, C, P, Q, _stream()), "bilinear_bwd")
    return dx


def concat(a, b):
    Ca, Cb = a.shape[-1], b.shape[-1]
    M = a.numel() // Ca
    out = torch.empty(tuple(a.shape[:-1]) + (Ca + Cb,), dtype=a.dtype, device=a.device)
    _lib.check(_lib.load().cs_concat_channels(_p(a), _p(b), _code(a.dtype), _p(out), M, Ca, Cb, _stream()), "concat")
    return out


def split(whole, Ca, want_a=True, want_b=True):
    C = whole.shape[-1]
    Cb = C - Ca
    M = whole.numel() // C
    a = torch.empty(tuple(whole.shape[:-1]) + (Ca,), dtype=whole.dtype, device=whole.device) if want_a else None
    b = torch.empty(tuple(whole.shape[:-1]) + (Cb,), dtype=whole.dtype, device=whole.device) if want_b else None
    _lib.check(_lib.load().cs_split_channels(_p(whole), _code(whole.dtype), _p(a), _p(b), M, Ca, Cb, _stream()), "split")
    return a, b


# ---------------------------------------------------------------- MBConv pieces
def dwconv_fwd(geom, x, w_hwc, scale=None, shift=None, act=CS_ACT_NONE):
    y = torch.empty((geom.N, geom.P, geom.Q, geom.C), dtype=x.dtype, device=x.device)
    _lib.check(_lib.load().cs_dwconv_fwd(ctypes.byref(geom), _code(x.dtype), _p(x), _p(w_hwc), _p(scale), _p(shift), act, _p(y), _stream()),
               "dwconv_fwd")
    return y


def dwconv_fwd_stats(geom, x, w_hwc):
    """Raw depthwise output z and its train-mode BN statistics (fp64 [2, C]) from one pass."""
    lib = _lib.load()
    y = torch.empty((geom.N, geom.P, geom.Q, geom.C), dtype=x.dtype, device=x.device)
    ws = torch.empty((lib.cs_dwconv_fwd_stats_workspace(ctypes.byref(geom)) // 8,), dtype=torch.float64, device=x.device)
    rows = ctypes.c_int(0)
    _lib.check(lib.cs_dwconv_fwd_stats(ctypes.byref(geom), _code(x.dtype), _p(x), _p(w_hwc), _p(y), _p(ws), ctypes.byref(rows), _stream()),
               "dwconv_fwd_stats")
    stats = new_stats(geom.C, x.device)
    _lib.check(lib.cs_bn_partial_fold(_p(ws), rows.value, geom.C, _p(stats), _stream()), "bn_partial_fold")
    return y, stats


def dwconv_dgrad(geom, dy, w_hwc):
    dx = torch.empty((geom.N, geom.H, geom.W, geom.C), dtype=dy.dtype, device=dy.device)
    _lib.check(_lib.load().cs_dwconv_dgrad(ctypes.byref(geom), _code(dy.dtype), _p(dy), _p(w_hwc), _p(dx), _stream()), "dwconv_dgrad")
    return dx


def dwconv_wgrad(geom, x, dy, param_layout=False):
    """fp32 [R, S, C]; param_layout: [C, 1, R, S], the layout of nn.Conv2d(groups=C).weight (no permute + copy afterwards)."""
    lib = _lib.load()
    ws = torch.empty((max(lib.cs_dwconv_wgrad_workspace(ctypes.byref(geom)) // 4, 1),), dtype=torch.float32, device=x.device)
    if param_layout:
        dw = torch.empty((geom.C, 1, geom.R, geom.S), dtype=torch.float32, device=x.device)
        _lib.check(lib.cs_dwconv_wgrad_oihw(ctypes.byref(geom), _code(x.dtype), _p(x), _p(dy), _p(dw), _p(ws), _stream()), "dwconv_wgrad_oihw")
        return dw
    dw = torch.empty((geom.R, geom.S, geom.C), dtype=torch.float32, device=x.device)
    _lib.check(lib.cs_dwconv_wgrad(ctypes.byref(geom), _code(x.dtype), _p(x), _p(dy), _p(dw), _p(ws), _stream()), "dwconv_wgrad")
    return dw


class DwStagePack:
    """The depthwise filters of a plan in the layout the depthwise kernels read ([R, S, C] fp32), restaged from the parameters by ONE launch
    per forward (cs_dw_weights_hwc_multi).  `weights`: the nn.Conv2d(groups=C).weight parameters, [C, 1, R, S] fp32 contiguous."""

    def __init__(self, weights):
        dev = weights[0].device
        sizes = [w.numel() for w in weights]
        self.flat = torch.empty((sum(sizes),), dtype=torch.float32, device=dev)
        self.key = tuple(w.data_ptr() for w in weights)
        self.hwc, rows, first = [], [], 0
        for w, n in zip(weights, sizes):
            C, RS = w.shape[0], w.shape[2] * w.shape[3]
            dst = self.flat[first:first + n].view(w.shape[2], w.shape[3], C)
            self.hwc.append(dst)
            rows.append([w.data_ptr(), dst.data_ptr(), C, RS, first])
            first += n
        self.total = first
        self.desc = torch.tensor(rows, dtype=torch.int64).to(dev)
        self.n = len(rows)

    def run(self):
        _lib.check(_lib.load().cs_dw_weights_hwc_multi(_p(self.desc), self.n, self.total, _stream()), "dw_weights_hwc_multi")


def se_scale(x, s):
    N, H, W, C = x.shape
    y = torch.empty_like(x)
    _lib.check(_lib.load().cs_se_scale(_p(x), _code(x.dtype), _p(s), _p(y), N, H * W, C, _stream()), "se_scale")
    return y


def sample_sum(a, b=None, scale=1.0):
    """fp32 [N, C]: scale * sum over the pixels of a (* b) per sample and channel (cs_sample_sum: row-strided, fixed-order fold)."""
    N, H, W, C = a.shape
    lib = _lib.load()
    out = torch.empty((N, C), dtype=torch.float32, device=a.device)
    ws = torch.empty((lib.cs_sample_sum_workspace(N, H * W, C) // 4,), dtype=torch.float32, device=a.device)
    _lib.check(lib.cs_sample_sum(_p(a), _p(b), _code(a.dtype), float(scale), _p(out), _p(ws), N, H * W, C, _stream()), "sample_sum")
    return out


def se_scale_bwd_ds(dy, x):
    return sample_sum(dy, x)


def se_scale_bwd_dx(dy, s, davg):
    N, H, W, C = dy.shape
    dx = torch.empty_like(dy)
    _lib.check(_lib.load().cs_se_scale_bwd_dx(_p(dy), _code(dy.dtype), _p(s), _p(davg), _p(dx), N, H * W, C, _stream()), "se_scale_bwd_dx")
    return dx


def rowscale_add(a, row_scale, b):
    N = a.shape[0]
    y = torch.empty_like(a)
    _lib.check(_lib.load().cs_rowscale_add(_p(a), _code(a.dtype), _p(row_scale), _p(b), _p(y), N, a.numel() // N, _stream()), "rowscale_add")
    return y


# ---------------------------------------------------------------- pooling
def maxpool_fwd(x, want_argmax=True):
    N, H, W, C = x.shape
    P, Q = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.empty((N, P, Q, C), dtype=x.dtype, device=x.device)
    am = torch.empty((N, P, Q, C), dtype=torch.uint8, device=x.device) if want_argmax else None
    _lib.check(_lib.load().cs_maxpool3x3s2_fwd(_p(x), _code(x.dtype), _p(y), _p(am), N, H, W, C, P, Q, _stream()), "maxpool_fwd")
    return y, am


def maxpool_bwd(dy, argmax, y_mask, in_hw):
    N, P, Q, C = dy.shape
    H, W = in_hw
    dx = torch.empty((N, H, W, C), dtype=dy.dtype, device=dy.device)
    _lib.check(_lib.load().cs_maxpool3x3s2_bwd(_p(dy), _p(argmax), _p(y_mask), _code(dy.dtype), _p(dx), N, H, W, C, P, Q,
                                               _stream()), "maxpool_bwd")
    return dx


def gap_fwd(x, with_max=True):
    N, H, W, C = x.shape
    if not with_max:
        return sample_sum(x, None, 1.0 / (H * W)), None          # the squeeze-excitation average pool
    feat = torch.empty((N, C), dtype=torch.float32, device=x.device)
    am = torch.empty((N, C), dtype=torch.int32, device=x.device) if with_max else None
    _lib.check(_lib.load().cs_gap_avgmax_fwd(_p(x), _code(x.dtype), _p(feat), _p(am), N, H * W, C, 1 if with_max else 0, _stream()),
               "gap_fwd")
    return feat, am


def gap_bwd(dfeat, argmax, x, relu_mask, with_max=True):
    N, H, W, C = x.shape
    dx = torch.empty_like(x)
    _lib.check(_lib.load().cs_gap_avgmax_bwd(_p(dfeat), _p(argmax), _p(x), _code(x.dtype), _p(dx), N, H * W, C,
                                             1 if relu_mask else 0, 1 if with_max else 0, _stream()), "gap_bwd")
    return dx


# ---------------------------------------------------------------- heads / losses
_LOSS_WORDS = 16            # cs_loss_words(): floats behind a CE / MSE value (the value + the exact accumulator of its partial sums)
def linear_fwd(x, w, b, act=CS_ACT_NONE, want_preact=False):
    M, K = x.shape
    N = w.shape[0]
    y = torch.empty((M, N), dtype=torch.float32, device=x.device)
    pre = torch.empty_like(y) if want_preact else None
    _lib.check(_lib.load().cs_linear_fwd(_p(x), _p(w), _p(b), _p(y), _p(pre), M, N, K, act, _stream()), "linear_fwd")
    return (y, pre) if want_preact else y


def linear_bwd(x, w, dy, y=None, act=CS_ACT_NONE, need_dx=True, need_dw=True, need_db=True):
    M, K = x.shape
    N = w.shape[0]
    dx = torch.empty((M, K), dtype=torch.float32, device=x.device) if need_dx else None
    dw = torch.empty((N, K), dtype=torch.float32, device=x.device) if (need_dw or need_db) else None
    db = torch.empty((N,), dtype=torch.float32, device=x.device) if need_db else None
    lib = _lib.load()
    nws = lib.cs_linear_bwd_workspace(M, N, K) if dw is not None else 0          # (> 512 rows: row slices of the weight gradient)
    ws = torch.empty((nws // 4,), dtype=torch.float32, device=x.device) if nws else None
    _lib.check(lib.cs_linear_bwd(_p(x), _p(w), _p(dy), _p(y), act, _p(dx), _p(dw), _p(db), M, N, K, 0, _p(ws), _stream()),
               "linear_bwd")
    return dx, dw, db


def softmax_ce(logits, labels, gamma=1.0, want_grad=True):
    M, C = logits.shape
    loss = torch.empty((_LOSS_WORDS,), dtype=torch.float32, device=logits.device)      # [0] = the value, the rest: its exact accumulator
    dl = torch.empty_like(logits) if want_grad else None
    _lib.check(_lib.load().cs_softmax_ce(_p(logits), _p(labels), float(gamma), _p(loss), _p(dl), M, C, _stream()), "softmax_ce")
    return loss[:1], dl


def softmax_prob1(logits):
    M, C = logits.shape
    p1 = torch.empty((M,), dtype=torch.float32, device=logits.device)
    _lib.check(_lib.load().cs_softmax_prob1(_p(logits), _p(p1), M, C, _stream()), "softmax_prob1")
    return p1


def softmax_argmax(logits):
    """np.argmax(F.softmax(logits, 1), axis=1) of inference.py:72-76 on the device: int64 [M], first index on probability ties."""
    M, C = logits.shape
    idx = torch.empty((M,), dtype=torch.int64, device=logits.device)
    _lib.check(_lib.load().cs_softmax_argmax(_p(logits), _p(idx), M, C, _stream()), "softmax_argmax")
    return idx


def mse(x, t, weighted=False, mean=True, want_grad=True):
    M = x.numel()
    loss = torch.empty((_LOSS_WORDS,), dtype=torch.float32, device=x.device)
    dx = torch.empty_like(x) if want_grad else None
    _lib.check(_lib.load().cs_mse(_p(x), _p(t), 1 if weighted else 0, 1 if mean else 0, _p(loss), _p(dx), M, _stream()), "mse")
    return loss[:1], dx


def dice_fwd(p, t, eps=1e-6, mean=True):
    """p, t: [N, HW] fp32 contiguous. returns loss[1], sums: the per-sample (sum p t, sum p^2, sum t^2) as an exact accumulator of
    accum_words(3 N) opaque words (cleared by the call, read by dice_bwd)"""
    _f32(p, t)
    N, HW = p.shape
    sums = torch.empty((accum_words(3 * N),), dtype=torch.float64, device=p.device)
    loss = torch.empty((1,), dtype=torch.float32, device=p.device)
    _lib.check(_lib.load().cs_dice_fwd(_p(p), _p(t), N, HW, eps, 1 if mean else 0, _p(sums), _p(loss), _stream()), "dice_fwd")
    return loss, sums


def dice_sums_values(sums, N):
    """fp64 [N, 3]: the per-sample (sum p t, sum p^2, sum t^2) that dice_fwd left in its exact accumulator."""
    return stats_values(sums)[0].view(N, 3)


def dice_bwd(p, t, sums, eps=1e-6, mean=True):
    _f32(p, t)
    N, HW = p.shape
    dp = torch.empty_like(p)
    _lib.check(_lib.load().cs_dice_bwd(_p(p), _p(t), _p(sums), N, HW, eps, 1 if mean else 0, _p(dp), _stream()), "dice_bwd")
    return dp


def softmax_channel_fwd(logits, ch=1):
    """logits [N,C,H,W] fp32 -> softmax over C, channel ch: [N,H,W]"""
    _f32(logits)
    N, C, H, W = logits.shape
    pc = torch.empty((N, H, W), dtype=torch.float32, device=logits.device)
    _lib.check(_lib.load().cs_softmax_channel_fwd(_p(logits), _p(pc), N, C, H * W, ch, _stream()), "softmax_channel_fwd")
    return pc


def softmax_channel_bwd(logits, dpc, ch=1):
    _f32(logits, dpc)
    N, C, H, W = logits.shape
    dl = torch.empty_like(logits)
    _lib.check(_lib.load().cs_softmax_channel_bwd(_p(logits), _p(dpc), _p(dl), N, C, H * W, ch, _stream()), "softmax_channel_bwd")
    return dl


def _select_buffers(probs):
    """(lib, T, workspace, out_idx[T] int64, count[1] int64) of one compaction over the T tiles of probs"""
    T = probs.numel()
    lib = _lib.load()
    ws = torch.empty((lib.cs_segmented_topk_workspace(T),), dtype=torch.uint8, device=probs.device)
    out = torch.empty((T,), dtype=torch.int64, device=probs.device)
    cnt = torch.zeros((1,), dtype=torch.int64, device=probs.device)
    return lib, T, ws, out, cnt


def segmented_topk(probs, groups, k_per_tile, seg_offsets, max_run):
    """Device-side order[index] of inference.py:31-43. Returns (out_idx[T] int64, count[1] int64)."""
    lib, T, ws, out, cnt = _select_buffers(probs)
    _lib.check(lib.cs_segmented_topk(_p(probs), _p(groups), _p(k_per_tile), _p(seg_offsets), seg_offsets.numel() - 1,
                                     int(max_run), T, _p(out), _p(cnt), _p(ws), ws.numel(), _stream()), "segmented_topk")
    return out, cnt


# ---------------------------------------------------------------- either side of the top-k
def segmented_order(probs, seg_offsets, max_run):
    """np.lexsort((probs, groups)) for non-decreasing groups: int64 [T] on the device."""
    T = probs.numel()
    order = torch.empty((T,), dtype=torch.int64, device=probs.device)
    _lib.check(_lib.load().cs_segmented_order(_p(probs), _p(seg_offsets), seg_offsets.numel() - 1, int(max_run), T, _p(order), _stream()),
               "segmented_order")
    return order


def threshold_select(probs, order, threshold):
    """order[probs[order] > threshold] -> (out_idx[T] int64, count[1] int64)."""
    lib, T, ws, out, cnt = _select_buffers(probs)
    _lib.check(lib.cs_threshold_select(_p(probs), _p(order), T, float(threshold), _p(out), _p(cnt), _p(ws), ws.numel(), _stream()), "threshold_select")
    return out, cnt


def evaluate_tile_counts(probs, order, groups, pos_from, threshold):
    """int64 [4] on the device: #(pred != real), #(pred & !real), #(!pred & real), #real."""
    counts = torch.zeros((4,), dtype=torch.int64, device=probs.device)
    _lib.check(_lib.load().cs_evaluate_tile_counts(_p(probs), _p(order), _p(groups), _p(pos_from), float(threshold), probs.numel(), _p(counts),
                                                   _stream()), "evaluate_tile_counts")
    return counts


def paint_tile_masks(selected, n_selected, groups, tile_xy, tile_size, n_images, H, W):
    """uint8 [n_images, H, W] masks with a tile_size^2 block of ones per selected tile."""
    masks = torch.zeros((n_images, H, W), dtype=torch.uint8, device=groups.device)
    _lib.check(_lib.load().cs_paint_tile_masks(_p(selected) if n_selected else None, int(n_selected), _p(groups), _p(tile_xy), int(tile_size), H, W,
                                               _p(masks), _stream()), "paint_tile_masks")
    return masks


def prune_excess(labels, flag, n_excess):
    """Positions that survive deleting the first n_excess entries with labels == flag -> (kept[n] int64, count[1] int64)."""
    n = labels.numel()
    kept = torch.empty((n,), dtype=torch.int64, device=labels.device)
    cnt = torch.zeros((1,), dtype=torch.int64, device=labels.device)
    _lib.check(_lib.load().cs_prune_excess(_p(labels), n, int(flag), int(n_excess), _p(kept), _p(cnt), _stream()), "prune_excess")
    return kept, cnt


# ---------------------------------------------------------------- cell localisation (csrc/detect.hip; detect.py is the public API)
def _aligned16(t):
    """contiguous and 16-byte aligned (a view into the middle of a buffer may not be)."""
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def detect_quantize(probs):
    """fp32 probabilities of any shape -> uint8 trunc(255 p), same shape."""
    p = _aligned16(probs)
    out = torch.empty(p.shape, dtype=torch.uint8, device=p.device)
    if p.numel():
        _lib.check(_lib.load().cs_detect_quantize(_p(p), p.numel(), _p(out), _stream()), "detect_quantize")
    return out


def detect_blur(src, taps_x, taps_y):
    """src [N,H,W] uint8 or fp32 probabilities (quantised on the way in) -> uint8 [N,H,W]; taps: host int sequences."""
    N, H, W = src.shape
    s = _aligned16(src)
    out = torch.empty((N, H, W), dtype=torch.uint8, device=s.device)
    tx = (ctypes.c_int32 * len(taps_x))(*[int(v) for v in taps_x])
    ty = (ctypes.c_int32 * len(taps_y))(*[int(v) for v in taps_y])
    _lib.check(_lib.load().cs_detect_blur(_p(s), int(s.dtype == torch.float32), N, H, W, tx, len(taps_x), ty, len(taps_y), _p(out), _stream()),
               "detect_blur")
    return out


def _workspace(size_fn, device, why, *args):
    """the caller-owned scratch of one library call: ``size_fn(*args)`` bytes as uint8; 0 = the library refuses these sizes (``why``)"""
    nbytes = size_fn(*args)
    if nbytes == 0:
        raise ValueError(why)
    return torch.empty((nbytes,), dtype=torch.uint8, device=device)


def stitch_patches(patches, corners, H, W):
    """patches uint8 [M,ph,pw], corners int32 [M,2] (device) -> uint8 [H,W], the highest patch index winning overlaps."""
    M, ph, pw = patches.shape
    lib = _lib.load()
    ws = _workspace(lib.cs_stitch_workspace, patches.device, f"stitch_patches: a {H}x{W} image has no pixels", H, W)
    out = torch.empty((H, W), dtype=torch.uint8, device=patches.device)
    _lib.check(lib.cs_stitch_patches(_p(patches.contiguous()) if M else None, M, ph, pw, _p(corners.contiguous()) if M else None, H, W, _p(out),
                                     _p(ws), ws.numel(), _stream()), "stitch_patches")
    return out


def stitch_logits(mask, logits, corners, ch=1):
    """logits fp32 [B,C,ph,pw], corners int32 [B,2] (device) -> mask uint8 [H,W] (device), in place: quantised softmax channel ch of
    every patch, the highest patch index of the batch winning overlaps; one launch, no workspace, no synchronisation."""
    _f32(logits)
    B, C, ph, pw = logits.shape
    H, W = mask.shape
    if B:
        _lib.check(_lib.load().cs_stitch_logits(_p(logits), B, C, ph, pw, int(ch), _p(corners), H, W, _p(mask), _stream()), "stitch_logits")
    return mask


def stitch_blend_add(num, den, logits, corners, taps_r, taps_c, flips=None, ch=1):
    """logits fp32 [B,C,ph,pw], corners int32 [B,2], flips uint8 [B] or None, taps int32 [ph] / [pw] (all device) -> num int64 [H,W]
    += w q and den int32 [H,W] += w in place, for every patch that covers a pixel (csrc/detect.hip); one launch, no workspace, no
    synchronisation."""
    _f32(logits)
    B, C, ph, pw = logits.shape
    H, W = num.shape
    if B:
        _lib.check(_lib.load().cs_stitch_blend_add(_p(logits), B, C, ph, pw, int(ch), _p(corners), _p(flips), _p(taps_r), _p(taps_c), H, W,
                                                   _p(num), _p(den), _stream()), "stitch_blend_add")
    return num, den


def stitch_blend_finish(num, den, out=None):
    """num int64 [H,W], den int32 [H,W] -> uint8 [H,W] = den ? num // (256 den) : 0 (into ``out`` when given); one launch."""
    H, W = num.shape
    if out is None:
        out = torch.empty((H, W), dtype=torch.uint8, device=num.device)
    _lib.check(_lib.load().cs_stitch_blend_finish(_p(num), _p(den), H, W, _p(out), _stream()), "stitch_blend_finish")
    return out


def detect_grid_size(H, W, interval, window):
    return _lib.load().cs_detect_grid_size(int(H), int(W), int(interval), int(window))


def detect_meanshift(blurred, interval, window, thr255, max_iter):
    """blurred uint8 [N,H,W] -> (pts int32 [N,G,2] final window centres, n_pts int32 [N] windows kept per map)."""
    N, H, W = blurred.shape
    G = detect_grid_size(H, W, interval, window)
    if G <= 0:
        raise ValueError(f"window {window} does not fit a {H}x{W} map (or interval {interval} is not positive)")
    pts = torch.empty((N, G, 2), dtype=torch.int32, device=blurred.device)
    n_pts = torch.empty((N,), dtype=torch.int32, device=blurred.device)
    _lib.check(_lib.load().cs_detect_meanshift(_p(blurred.contiguous()), N, H, W, int(interval), int(window), float(thr255), int(max_iter), _p(pts),
                                               _p(n_pts), _stream()), "detect_meanshift")
    return pts, n_pts


def detect_cluster(pts, n_pts, eps, blurred, force_global=False):
    """pts int32 [N,cap,2], n_pts int32 [N] -> (points int64 [N cap,2], weights int32 [N cap], offsets int64 [N+1]) on the device;
    the clusters of map n are rows offsets[n]:offsets[n+1]."""
    N, cap, _ = pts.shape
    _, H, W = blurred.shape
    lib = _lib.load()
    ws = _workspace(lib.cs_detect_cluster_workspace, pts.device, f"detect_cluster: no workspace for {(N, cap)}", N, cap)
    out_pts = torch.empty((N * cap, 2), dtype=torch.int64, device=pts.device)
    out_w = torch.empty((N * cap,), dtype=torch.int32, device=pts.device)
    out_off = torch.empty((N + 1,), dtype=torch.int64, device=pts.device)
    _lib.check(lib.cs_detect_cluster(_p(pts.contiguous()), _p(n_pts.contiguous()), N, cap, float(eps), _p(blurred.contiguous()), H, W,
                                     int(bool(force_global)), _p(out_pts), _p(out_w), _p(out_off), _p(ws), ws.numel(), _stream()), "detect_cluster")
    return out_pts, out_w, out_off


# cs_detect_edt_* live in csrc/morph.hip: the distance transform shares the nearest-site transform's column pass and row search
def _detect_edt(src, thr, smooth):
    N, H, W = src.shape
    lib = _lib.load()
    ws = _workspace(lib.cs_detect_edt_workspace, src.device,
                    f"distance transform: a call takes 0 < N <= 65535 maps with H^2 + W^2 < 2^31, got {(N, H, W)}", N, H, W, int(smooth))
    s = _aligned16(src)
    out = torch.empty((N, H, W), dtype=torch.uint8 if smooth else torch.int32, device=s.device)
    fn = lib.cs_detect_edt_smooth if smooth else lib.cs_detect_edt_sq
    _lib.check(fn(_p(s), int(s.dtype == torch.float32), N, H, W, int(thr), _p(out), _p(ws), ws.numel(), _stream()),
               "detect_edt_smooth" if smooth else "detect_edt_sq")
    return out


def detect_edt_sq(src, thr=10):
    """src [N,H,W] uint8 or fp32 probabilities (quantised on the way in); foreground = u8 > thr -> int32 [N,H,W] exact squared
    Euclidean distance to the nearest background pixel of the map (-1 everywhere in a map without background)."""
    return _detect_edt(src, thr, False)


def detect_edt_smooth(src, thr=10):
    """src as detect_edt_sq -> uint8 [N,H,W] = 255 sqrt(D2 / max D2 of the map), rounded half to even in integer arithmetic."""
    return _detect_edt(src, thr, True)


# ---------------------------------------------------------------- nearest-site transform and disk morphology (csrc/morph.hip; morph.py
# is the public API)
def morph_max_site_width():
    """the widest row the calls that return or follow a site take (a row of packed words has to fit the LDS)"""
    return _lib.load().cs_morph_max_site_width()


def morph_workspace(N, H, W, device):
    """the caller-owned scratch of one cs_morph_* call on [N,H,W] (reusable by later calls of the same shape)"""
    return _workspace(_lib.load().cs_morph_workspace, device,
                      f"morph: a call takes 0 < N <= 65535 images with H^2 + W^2 < 2^31, got {(N, H, W)}", N, H, W)


def _morph_args(x, dtypes, ws):
    if x.dtype not in dtypes or x.dim() != 3:
        raise TypeError(f"morph kernels read [N,H,W] of {' or '.join(str(d) for d in dtypes)}, got {x.dtype} {tuple(x.shape)}")
    N, H, W = x.shape
    if ws is None:
        ws = morph_workspace(N, H, W, x.device)
    return N, H, W, ws


def morph_nearest(src, background=False, d2=None, site=None, ws=None):
    """src uint8 [N,H,W] (sites: != 0, or == 0 with ``background``) or int32 labels (sites: != 0) -> (d2, site) int32 [N,H,W]: the
    exact squared distance to the nearest site and its flat index row W + col, the lowest index among equally near sites; both -1
    in an image without a site."""
    N, H, W, ws = _morph_args(src, (torch.uint8, torch.int32), ws)
    t = _regions_outputs("morph_nearest", {"d2": ((N, H, W), torch.int32), "site": ((N, H, W), torch.int32)}, {"d2": d2, "site": site},
                         src.device)
    _lib.check(_lib.load().cs_morph_nearest(_p(src), int(src.dtype == torch.int32), int(bool(background)), N, H, W, _p(t["d2"]),
                                            _p(t["site"]), _p(ws), ws.numel(), _stream()), "morph_nearest")
    return t["d2"], t["site"]


def morph_binary(mask, erode, r2, outside_is_site=False, out=None, ws=None):
    """mask uint8 [N,H,W] -> uint8 0/1: ``D2 to the nearest nonzero pixel <= r2`` (dilation), or with ``erode`` ``mask != 0 and D2 to
    the nearest zero pixel > r2``; with ``outside_is_site`` the pixels beyond the edge count as nonzero / zero respectively."""
    N, H, W, ws = _morph_args(mask, (torch.uint8,), ws)
    if out is None:
        out = torch.empty((N, H, W), dtype=torch.uint8, device=mask.device)
    _lib.check(_lib.load().cs_morph_binary(_p(mask), N, H, W, int(bool(erode)), int(r2), int(bool(outside_is_site)), _p(out), _p(ws),
                                           ws.numel(), _stream()), "morph_binary")
    return out


def morph_expand_labels(labels, r2, out=None, ws=None):
    """labels int32 [N,H,W] -> int32: a zero pixel whose nearest nonzero pixel lies within r2 takes that pixel's label"""
    N, H, W, ws = _morph_args(labels, (torch.int32,), ws)
    if out is None:
        out = torch.empty((N, H, W), dtype=torch.int32, device=labels.device)
    _lib.check(_lib.load().cs_morph_expand_labels(_p(labels), N, H, W, int(r2), _p(out), _p(ws), ws.numel(), _stream()),
               "morph_expand_labels")
    return out


# ---------------------------------------------------------------- small-region clean-up (csrc/regions.hip; regions.py is the public API)
def regions_workspace(N, H, W, device):
    """the caller-owned scratch of one cs_regions_* call on [N,H,W] (reusable by later calls of the same shape)"""
    return _workspace(_lib.load().cs_regions_workspace, device,
                      f"regions: a call takes 0 < N <= 65535 images with N H W < 2^31 pixels, got {(N, H, W)}", N, H, W)


def _regions_args(mask, ws):
    if mask.dtype != torch.uint8 or mask.dim() != 3:
        raise TypeError("regions kernels read uint8 [N,H,W] masks")
    N, H, W = mask.shape
    if ws is None:
        ws = regions_workspace(N, H, W, mask.device)
    return N, H, W, ws


def _regions_outputs(what, want, given, device):
    """name -> tensor for every (shape, dtype) of ``want``: the one given (checked: written in place), else a new one"""
    t = {}
    for name, (shape, dtype) in want.items():
        x = given.get(name)
        if x is None:
            x = torch.empty(shape, dtype=dtype, device=device)
        elif x.dtype != dtype or tuple(x.shape) != shape:
            raise TypeError(f"{what}: {name} must be {dtype} of shape {shape}, got {x.dtype} {tuple(x.shape)}")
        t[name] = x
    return t


def regions_label(mask, connectivity=1, out=None, ws=None):
    """uint8 [N,H,W] -> int32 [N,H,W] scipy.ndimage.label per image"""
    N, H, W, ws = _regions_args(mask, ws)
    if out is None:
        out = torch.empty((N, H, W), dtype=torch.int32, device=mask.device)
    _lib.check(_lib.load().cs_regions_label(_p(mask), N, H, W, int(connectivity), _p(out), _p(ws), ws.numel(), _stream()), "regions_label")
    return out


def regions_number(mask, connectivity=1, counts=None, ws=None):
    """uint8 [N,H,W] -> counts int32 [N], the number of foreground components per image; ``ws`` keeps the roots and numbers for a
    regions_measure(..., numbered=True) of the same mask"""
    N, H, W, ws = _regions_args(mask, ws)
    if counts is None:
        counts = torch.empty((N,), dtype=torch.int32, device=mask.device)
    _lib.check(_lib.load().cs_regions_number(_p(mask), N, H, W, int(connectivity), _p(counts), _p(ws), ws.numel(), _stream()), "regions_number")
    return counts


def regions_measure(mask, capacity, intensity=None, connectivity=1, numbered=False, counts=None, area=None, bbox=None, sums=None,
                    isum=None, imax=None, ws=None):
    """uint8 [N,H,W] (and uint8 intensity [N,H,W] or None) -> (counts int32 [N], area int32 [N,cap], bbox int32 [N,cap,4],
    sums int64 [N,cap,2], isum int64 [N,cap] | None, imax int32 [N,cap] | None); row k = component k + 1, zero from
    min(count, cap) on.  Tables that are given are written in place (contiguous, of these shapes).  numbered=True: ``counts`` and
    ``ws`` are what regions_number left for this mask."""
    N, H, W, ws = _regions_args(mask, ws)
    cap = int(capacity)
    if numbered and counts is None:
        raise ValueError("regions_measure: numbered=True needs the counts of regions_number")
    if intensity is not None and (intensity.dtype != torch.uint8 or tuple(intensity.shape) != (N, H, W)):
        raise TypeError("regions_measure: the intensity image is uint8 of the mask's shape")
    want = {"counts": ((N,), torch.int32), "area": ((N, cap), torch.int32), "bbox": ((N, cap, 4), torch.int32),
            "sums": ((N, cap, 2), torch.int64)}
    if intensity is not None:
        want.update(isum=((N, cap), torch.int64), imax=((N, cap), torch.int32))
    t = _regions_outputs("regions_measure", want, {"counts": counts, "area": area, "bbox": bbox, "sums": sums, "isum": isum, "imax": imax},
                         mask.device)
    _lib.check(_lib.load().cs_regions_measure(_p(mask), _p(intensity), N, H, W, int(connectivity), cap, int(bool(numbered)), _p(t["counts"]),
                                              _p(t["area"]), _p(t["bbox"]), _p(t["sums"]), _p(t.get("isum")), _p(t.get("imax")), _p(ws),
                                              ws.numel(), _stream()), "regions_measure")
    return t["counts"], t["area"], t["bbox"], t["sums"], t.get("isum"), t.get("imax")


def regions_split_workspace(N, H, W, P, device):
    """the caller-owned scratch of one cs_regions_split call on [N,H,W] with a points buffer of P rows"""
    why = f"regions_split: a call takes 0 < N <= 65535 images with N H W < 2^31 pixels and P >= 0 points, got {(N, H, W, P)}"
    return _workspace(_lib.load().cs_regions_split_workspace, device, why, N, H, W, int(P))


def _split_operands(what, mask, points, offsets, limits):
    """the operand checks the two split wrappers share -> N, H, W, the contiguous point set, P, and none_if_empty: the pointer of a
    tensor of P rows, None when P == 0 (an empty tensor has no storage to point at)"""
    if mask.dtype != torch.uint8 or mask.dim() != 3:
        raise TypeError("regions kernels read uint8 [N,H,W] masks")
    N, H, W = mask.shape
    points, offsets, limits, _ = _point_operands(what, points, offsets, limits, N, "points", device=mask.device)
    P = int(points.shape[0])
    if P + H * W >= 1 << 31:
        raise ValueError(f"{what}: {P} points and {H}x{W} pixels do not leave room for int32 labels")
    return N, H, W, points, offsets, limits, P, (lambda x: _p(x) if P else None)


def regions_split(mask, points, offsets, limits=None, connectivity=1, labels=None, counts=None, live=None, ws=None):
    """uint8 [N,H,W], points int64 [P,2] (row, col), offsets int64 [N+1], limits int32 [N] | None -> (labels int32 [N,H,W],
    counts int32 [N], live uint8 [P]): every foreground pixel labelled 1 + the index of the nearest live seed of its own component,
    components without one numbered after the image's seeds (cs_regions_split in include/cellseg_hip.h)"""
    N, H, W, points, offsets, limits, P, none_if_empty = _split_operands("regions_split", mask, points, offsets, limits)
    want = {"labels": ((N, H, W), torch.int32), "counts": ((N,), torch.int32), "live": ((P,), torch.uint8)}
    t = _regions_outputs("regions_split", want, {"labels": labels, "counts": counts, "live": live}, mask.device)
    if ws is None:
        ws = regions_split_workspace(N, H, W, P, mask.device)
    _lib.check(_lib.load().cs_regions_split(_p(mask), N, H, W, int(connectivity), none_if_empty(points), _p(offsets), _p(limits), P,
                                            _p(t["labels"]), _p(t["counts"]), none_if_empty(t["live"]), _p(ws), ws.numel(), _stream()),
               "regions_split")
    return t["labels"], t["counts"], t["live"]


def regions_geodesic_workspace(N, H, W, P, device):
    """the caller-owned scratch of one cs_regions_split_geodesic call on [N,H,W] with a points buffer of P rows; a call with
    ``resume`` takes the one its first call ran on"""
    why = (f"regions_split_geodesic: a call takes 0 < N <= 65535 images with N H W < 2^31 and 7 H W < 2^31 pixels and P >= 0 points, "
           f"got {(N, H, W, P)}")
    return _workspace(_lib.load().cs_regions_geodesic_workspace, device, why, N, H, W, int(P))


def regions_split_geodesic(mask, points, offsets, limits=None, connectivity=1, rounds=1, resume=False, labels=None, counts=None,
                           live=None, distance=None, converged=None, want_distance=False, ws=None):
    """regions_split's arguments -> (labels int32 [N,H,W], counts int32 [N], live uint8 [P], distance int32 [N,H,W] | None, converged
    uint8 [N], ws): every foreground pixel labelled 1 + the index of the live seed of its component that is nearest along 5-7 chamfer
    paths inside the component, after ``rounds`` relaxation rounds (cs_regions_split_geodesic in include/cellseg_hip.h).  ``resume``:
    ``ws`` and the outputs are those of an earlier call with the same arguments; ``rounds`` more rounds run on them."""
    N, H, W, points, offsets, limits, P, none_if_empty = _split_operands("regions_split_geodesic", mask, points, offsets, limits)
    if resume and (ws is None or labels is None or counts is None or live is None):
        raise ValueError("regions_split_geodesic: resume needs the workspace and the outputs of the call it resumes")
    want = {"labels": ((N, H, W), torch.int32), "counts": ((N,), torch.int32), "live": ((P,), torch.uint8), "converged": ((N,), torch.uint8)}
    if want_distance or distance is not None:
        want["distance"] = ((N, H, W), torch.int32)
    t = _regions_outputs("regions_split_geodesic", want, {"labels": labels, "counts": counts, "live": live, "distance": distance,
                                                          "converged": converged}, mask.device)
    if ws is None:
        ws = regions_geodesic_workspace(N, H, W, P, mask.device)
    _lib.check(_lib.load().cs_regions_split_geodesic(_p(mask), N, H, W, int(connectivity), none_if_empty(points), _p(offsets), _p(limits), P,
                                                     int(rounds), int(bool(resume)), _p(t["labels"]), _p(t["counts"]),
                                                     none_if_empty(t["live"]), _p(t.get("distance")), _p(t["converged"]), _p(ws), ws.numel(),
                                                     _stream()), "regions_split_geodesic")
    return t["labels"], t["counts"], t["live"], t.get("distance"), t["converged"], ws


def _label_images(what, labels):
    """the label-image operand of the wrapper ``what`` -> N, H, W"""
    if labels.dtype != torch.int32 or labels.dim() != 3:
        raise TypeError(f"{what} reads int32 [N,H,W] label images")
    return labels.shape


def _bbox_operand(what, bbox, N, cap):
    """the bounding boxes of regions_measure_labels for the same image, as the wrapper ``what`` takes them"""
    if bbox.dtype != torch.int32 or tuple(bbox.shape) != (N, cap, 4):
        raise TypeError(f"{what}: bbox must be torch.int32 of shape {(N, cap, 4)}, got {bbox.dtype} {tuple(bbox.shape)}")


def regions_measure_labels(labels, capacity, intensity=None, counts=None, area=None, bbox=None, sums=None, isum=None, imax=None,
                           want_counts=True):
    """int32 label image [N,H,W] (and uint8 intensity [N,H,W] or None) -> the tuple of regions_measure with row k = label k + 1; a
    label without a pixel leaves an all-zero row.  counts is written with the largest label of every image, or left out
    (``want_counts=False`` -> None) by a caller that has the counts already."""
    N, H, W = _label_images("regions_measure_labels", labels)
    cap = int(capacity)
    if intensity is not None and (intensity.dtype != torch.uint8 or tuple(intensity.shape) != (N, H, W)):
        raise TypeError("regions_measure_labels: the intensity image is uint8 of the label image's shape")
    want = {"area": ((N, cap), torch.int32), "bbox": ((N, cap, 4), torch.int32), "sums": ((N, cap, 2), torch.int64)}
    if want_counts:
        want["counts"] = ((N,), torch.int32)
    if intensity is not None:
        want.update(isum=((N, cap), torch.int64), imax=((N, cap), torch.int32))
    t = _regions_outputs("regions_measure_labels", want,
                         {"counts": counts, "area": area, "bbox": bbox, "sums": sums, "isum": isum, "imax": imax}, labels.device)
    _lib.check(_lib.load().cs_regions_measure_labels(_p(labels), _p(intensity), N, H, W, cap, _p(t.get("counts")), _p(t["area"]),
                                                     _p(t["bbox"]), _p(t["sums"]), _p(t.get("isum")), _p(t.get("imax")), _stream()),
               "regions_measure_labels")
    return t.get("counts"), t["area"], t["bbox"], t["sums"], t.get("isum"), t.get("imax")


REGIONS_SHAPE_MAX_SIDE = 32768       # cs_regions_shape_labels: Sxx <= area (H - 1)^2 < 2^61 stays inside int64


def regions_edges_labels(labels, edges=None):
    """int32 label image [N,H,W] -> edges uint8 [N,H,W]: 1 where the pixel's object id max(label, 0) is positive and one of its four
    neighbours (outside the image: id 0) has another id (cs_regions_edges_labels in include/cellseg_hip.h)."""
    N, H, W = _label_images("regions_edges_labels", labels)
    t = _regions_outputs("regions_edges_labels", {"edges": ((N, H, W), torch.uint8)}, {"edges": edges}, labels.device)
    _lib.check(_lib.load().cs_regions_edges_labels(_p(labels), N, H, W, _p(t["edges"]), _stream()), "regions_edges_labels")
    return t["edges"]


def regions_shape_labels(labels, edges, capacity, bbox, moments=None, tallies=None):
    """int32 label image [N,H,W], its edges uint8 [N,H,W] (regions_edges_labels) and bbox int32 [N,cap,4] (regions_measure_labels of
    the same image) -> (moments int64 [N,cap,3] = Sxx, Syy, Sxy about the box corner, tallies int32 [N,cap,4] = edge pixels,
    straight, diagonal, mixed); row k = label k + 1 (cs_regions_shape_labels in include/cellseg_hip.h)."""
    N, H, W = _label_images("regions_shape_labels", labels)
    cap = int(capacity)
    if edges.dtype != torch.uint8 or tuple(edges.shape) != (N, H, W):
        raise TypeError("regions_shape_labels: the edge map is uint8 of the label image's shape")
    _bbox_operand("regions_shape_labels", bbox, N, cap)
    if max(H, W) > REGIONS_SHAPE_MAX_SIDE:
        raise ValueError(f"regions_shape_labels: a {H}x{W} image: H, W <= {REGIONS_SHAPE_MAX_SIDE} keep the second moments inside int64")
    t = _regions_outputs("regions_shape_labels", {"moments": ((N, cap, 3), torch.int64), "tallies": ((N, cap, 4), torch.int32)},
                         {"moments": moments, "tallies": tallies}, labels.device)
    _lib.check(_lib.load().cs_regions_shape_labels(_p(labels), _p(edges), N, H, W, cap, _p(bbox), _p(t["moments"]), _p(t["tallies"]),
                                                   _stream()), "regions_shape_labels")
    return t["moments"], t["tallies"]


REGIONS_HULL_MAX_SIDE = 1024         # cs_regions_hull_max_side: a larger bounding box is counted, not measured (its row is -1)


def regions_hull_labels(labels, capacity, bbox, hull=None):
    """int32 label image [N,H,W] and bbox int32 [N,cap,4] (regions_measure_labels of the same image) -> hull int32 [N,cap,5] =
    n_vertices, area2, feret_max2, width_cross, width_len2 of the convex hull of every label's pixel squares; row k = label k + 1,
    all -1 where the box has more than REGIONS_HULL_MAX_SIDE rows or columns (cs_regions_hull_labels in include/cellseg_hip.h)."""
    N, H, W = _label_images("regions_hull_labels", labels)
    cap = int(capacity)
    _bbox_operand("regions_hull_labels", bbox, N, cap)
    t = _regions_outputs("regions_hull_labels", {"hull": ((N, cap, 5), torch.int32)}, {"hull": hull}, labels.device)
    _lib.check(_lib.load().cs_regions_hull_labels(_p(labels), N, H, W, cap, _p(bbox), _p(t["hull"]), _stream()), "regions_hull_labels")
    return t["hull"]


REGIONS_CONTOUR_MAX_SIDE = 512       # cs_regions_contour_max_side: a larger bounding box is counted, not traced (its row is -1)


def regions_contour_labels(labels, capacity, bbox, connectivity, max_vertices, contour=None, vertices=None):
    """int32 label image [N,H,W] and bbox int32 [N,cap,4] (regions_measure_labels of the same image) -> (contour int32 [N,cap,4] =
    n_vertices, n_cracks, area2, cracks_all of the outer boundary ring of every label, vertices int32 [N,cap,max_vertices,2] = the
    ring's first vertices as (row, col), then (-1, -1)); row k = label k + 1, all -1 where the box has more than
    REGIONS_CONTOUR_MAX_SIDE rows or columns.  ``max_vertices=0`` only counts: vertices is None
    (cs_regions_contour_labels in include/cellseg_hip.h)."""
    N, H, W = _label_images("regions_contour_labels", labels)
    cap, maxv = int(capacity), int(max_vertices)
    _bbox_operand("regions_contour_labels", bbox, N, cap)
    if maxv < 0:
        raise ValueError(f"regions_contour_labels: max_vertices must be >= 0, got {max_vertices!r}")
    want = {"contour": ((N, cap, 4), torch.int32)}
    if maxv > 0:
        want["vertices"] = ((N, cap, maxv, 2), torch.int32)
    elif vertices is not None:
        raise TypeError("regions_contour_labels: max_vertices=0 only counts and takes no vertices")
    t = _regions_outputs("regions_contour_labels", want, {"contour": contour, "vertices": vertices}, labels.device)
    _lib.check(_lib.load().cs_regions_contour_labels(_p(labels), N, H, W, cap, _p(bbox), int(connectivity), maxv, _p(t["contour"]),
                                                     _p(t.get("vertices")), _stream()), "regions_contour_labels")
    return t["contour"], t.get("vertices")


TEXTURE_LEVELS = (8, 16, 32)         # cs_regions_texture_labels: the grey levels L of a co-occurrence matrix
TEXTURE_MAX_DISTANCE = 8
TEXTURE_MAX_PIXELS = 1 << 30         # H W per image: every direction then has fewer than 2^30 pairs and the int32 counts hold


def texture_labels(labels, capacity, bbox, plane=None, images_u8=None, od_q=None, Mq=None, levels=16, distance=1, want_matrix=False,
                   **tables):
    """int32 label image [N,H,W], bbox int32 [N,cap,4] (regions_measure_labels of the same image) and either ``plane`` uint8 [N,H,W]
    or ``images_u8`` uint8 [N,H,W,3] with od_q int32 [256] and Mq int32 [N,3] (one stain row per image) -> dict of pairs int32
    [N,cap,4]; diff, marg int32 [N,cap,4,L]; sum int32 [N,cap,4,2L-1]; sq, cross int64 [N,cap,4] and, with ``want_matrix``, matrix
    int32 [N,cap,4,L,L]: the symmetric grey-level co-occurrence of every label at ``distance`` in the four directions, L =
    ``levels``; row k = label k + 1.  ``tables``: tensors to write instead of new ones (cs_regions_texture_labels in
    include/cellseg_hip.h)."""
    what = "texture_labels"
    N, H, W = _label_images(what, labels)
    cap, L, d = int(capacity), int(levels), int(distance)
    _bbox_operand(what, bbox, N, cap)
    if (plane is None) == (images_u8 is None):
        raise ValueError(f"{what}: exactly one of plane and images_u8 is given")
    if L not in TEXTURE_LEVELS:
        raise ValueError(f"{what}: levels must be one of {TEXTURE_LEVELS}, got {levels}")
    if not 1 <= d <= TEXTURE_MAX_DISTANCE:
        raise ValueError(f"{what}: distance must lie in [1, {TEXTURE_MAX_DISTANCE}], got {distance}")
    if H * W > TEXTURE_MAX_PIXELS:
        raise ValueError(f"{what}: a {H}x{W} image: H W <= 2^30 keeps the pair counts inside int32")
    if plane is not None:
        if not torch.is_tensor(plane) or plane.dtype != torch.uint8 or tuple(plane.shape) != (N, H, W):
            raise TypeError(f"{what}: the plane is uint8 of the label image's shape")
        if od_q is not None or Mq is not None:
            raise ValueError(f"{what}: od_q and Mq go with images_u8")
    else:
        if tuple(_rgb_images(what, images_u8, whole_batch=True)) != (N, H, W):
            raise ValueError(f"{what}: images of shape {tuple(images_u8.shape)} for labels of {(N, H, W)}")
        if not torch.is_tensor(od_q) or od_q.dtype != torch.int32 or tuple(od_q.shape) != (256,):
            raise ValueError(f"{what}: od_q must be an int32 tensor shaped (256,) (stain.od_table)")
        if not torch.is_tensor(Mq) or Mq.dtype != torch.int32 or tuple(Mq.shape) != (N, 3):
            raise ValueError(f"{what}: Mq must be an int32 tensor shaped {(N, 3)}: one stain row per image")
    want = {"pairs": ((N, cap, 4), torch.int32), "diff": ((N, cap, 4, L), torch.int32), "sum": ((N, cap, 4, 2 * L - 1), torch.int32),
            "marg": ((N, cap, 4, L), torch.int32), "sq": ((N, cap, 4), torch.int64), "cross": ((N, cap, 4), torch.int64)}
    if want_matrix or tables.get("matrix") is not None:
        want["matrix"] = ((N, cap, 4, L, L), torch.int32)
    unknown = sorted(set(tables) - set(want) - {"matrix"})
    if unknown:
        raise TypeError(f"{what}: no table named {unknown[0]!r}")
    t = _regions_outputs(what, want, tables, labels.device)
    _lib.check(_lib.load().cs_regions_texture_labels(_p(labels), _p(plane), _p(images_u8), _p(od_q), _p(Mq), N, H, W, cap, _p(bbox), L, d,
                                                     _p(t["pairs"]), _p(t["diff"]), _p(t["sum"]), _p(t["marg"]), _p(t["sq"]),
                                                     _p(t["cross"]), _p(t.get("matrix")), _stream()), what)
    return t


def _label_pair_args(what, pred, truth, want_counts):
    """two int32 [N,H,W] label images of one shape -> (N, H, W, the ``_regions_outputs`` entries of the counts asked for)"""
    if pred.dtype != torch.int32 or pred.dim() != 3 or truth.dtype != torch.int32 or tuple(truth.shape) != tuple(pred.shape):
        raise TypeError(f"{what} reads two int32 [N,H,W] label images of one shape")
    N, H, W = pred.shape
    return N, H, W, {k: ((N,), torch.int32) for k, wanted in zip(("counts_pred", "counts_truth"), want_counts) if wanted}


def regions_match_workspace(N, cap_pred, cap_truth, device):
    """the caller-owned scratch of one cs_regions_match_labels call on N images with these capacities"""
    why = ("regions_match_labels: a call takes 0 < N <= 65535 images and capacities >= 1 with N cap_pred "
           f"bit_length(cap_truth) < 2^31 and N cap_truth < 2^31, got {(N, cap_pred, cap_truth)}")
    return _workspace(_lib.load().cs_regions_match_workspace, device, why, int(N), int(cap_pred), int(cap_truth))


def regions_match_labels(pred, truth, cap_pred, cap_truth, counts_pred=None, counts_truth=None, area_pred=None, area_truth=None,
                         match=None, inter=None, match_truth=None, want_counts=(True, True), ws=None):
    """int32 label images pred, truth [N,H,W] -> (counts_pred int32 [N] | None, counts_truth int32 [N] | None, area_pred int32
    [N,cap_pred], area_truth int32 [N,cap_truth], match int32 [N,cap_pred], inter int32 [N,cap_pred], match_truth int32
    [N,cap_truth]): the partner of every label at IoU > 1/2 (cs_regions_match_labels in include/cellseg_hip.h).  The counts of a
    side are written with the largest label of every image, or left out (``want_counts`` False for that side -> None)."""
    N, H, W, counts = _label_pair_args("regions_match_labels", pred, truth, want_counts)
    cp, ct = int(cap_pred), int(cap_truth)
    want = {"area_pred": ((N, cp), torch.int32), "area_truth": ((N, ct), torch.int32), "match": ((N, cp), torch.int32),
            "inter": ((N, cp), torch.int32), "match_truth": ((N, ct), torch.int32), **counts}
    if ws is None:
        ws = regions_match_workspace(N, cp, ct, pred.device)
    t = _regions_outputs("regions_match_labels", want,
                         {"counts_pred": counts_pred, "counts_truth": counts_truth, "area_pred": area_pred, "area_truth": area_truth,
                          "match": match, "inter": inter, "match_truth": match_truth}, pred.device)
    _lib.check(_lib.load().cs_regions_match_labels(_p(pred), _p(truth), N, H, W, cp, ct, _p(t.get("counts_pred")), _p(t.get("counts_truth")),
                                                   _p(t["area_pred"]), _p(t["area_truth"]), _p(t["match"]), _p(t["inter"]),
                                                   _p(t["match_truth"]), _p(ws), ws.numel(), _stream()), "regions_match_labels")
    return (t.get("counts_pred"), t.get("counts_truth"), t["area_pred"], t["area_truth"], t["match"], t["inter"], t["match_truth"])


def regions_overlap_slots(max_pairs):
    """the entries of one image's pair table: the smallest power of two >= 2 max_pairs"""
    return 1 << max(1, (2 * int(max_pairs) - 1).bit_length())


def _int_max_pairs(size_fn, at):
    """``size_fn`` with its ``max_pairs``, argument ``at``, kept to what the library's int holds: any other is refused here (0)"""
    return lambda *a: size_fn(*a) if 1 <= a[at] < 1 << 31 else 0


def _pair_table_views(ws, N, max_pairs, n_counts):
    """The pair table of a call as views of its workspace ``ws``: (slot_keys int64 [N,slots], then ``n_counts`` int32 [N,slots] count
    arrays).  The table leads the workspace, 8 bytes per slot of keys and then 4 per slot of every count array, and N slots is even,
    so nothing pads them apart (pair_table_layout in csrc/regions.hip)."""
    cells = N * regions_overlap_slots(max_pairs)
    keys = ws[:8 * cells].view(torch.int64).view(N, -1)
    return (keys, *(ws[(8 + 4 * k) * cells:(12 + 4 * k) * cells].view(torch.int32).view(N, -1) for k in range(n_counts)))


def regions_overlap_workspace(N, cap_pred, cap_truth, max_pairs, device):
    """the caller-owned scratch of one cs_regions_overlap_labels call on N images with these capacities; it starts with the pair
    table, which the call's result views"""
    why = ("regions_overlap_labels: a call takes 0 < N <= 65535 images, capacities >= 1 and 1 <= max_pairs <= 2^29 with "
           f"N cap_pred, N cap_truth and N slots < 2^31, got {(N, cap_pred, cap_truth, max_pairs)}")
    return _workspace(_int_max_pairs(_lib.load().cs_regions_overlap_workspace, 3), device, why, int(N), int(cap_pred), int(cap_truth),
                      int(max_pairs))


_OVERLAP_TABLES = (("area_pred", 0), ("area_truth", 1), ("iou_partner", 1), ("iou_inter", 1), ("inter_partner_truth", 1), ("inter_truth", 1),
                   ("inter_partner_pred", 0), ("inter_pred", 0))


def regions_overlap_labels(pred, truth, cap_pred, cap_truth, max_pairs, counts_pred=None, counts_truth=None, area_pred=None,
                           area_truth=None, n_pairs=None, dropped=None, iou_partner=None, iou_inter=None, inter_partner_truth=None,
                           inter_truth=None, inter_partner_pred=None, inter_pred=None, want_counts=(True, True), ws=None):
    """int32 label images pred, truth [N,H,W] -> a dict of int32 tensors: counts_pred, counts_truth [N] (None where ``want_counts``
    is False for that side), area_pred [N,cap_pred], area_truth [N,cap_truth], n_pairs, dropped [N], iou_partner, iou_inter,
    inter_partner_truth, inter_truth [N,cap_truth], inter_partner_pred, inter_pred [N,cap_pred], and the pair table itself as views
    of ``ws``: slot_keys int64 [N,slots] ((pred << 32) | truth, 0 = empty) and slot_counts int32 [N,slots]
    (cs_regions_overlap_labels in include/cellseg_hip.h)."""
    N, H, W, counts = _label_pair_args("regions_overlap_labels", pred, truth, want_counts)
    cp, ct, mp = int(cap_pred), int(cap_truth), int(max_pairs)
    caps = (cp, ct)
    want = {name: ((N, caps[side]), torch.int32) for name, side in _OVERLAP_TABLES}
    want.update(n_pairs=((N,), torch.int32), dropped=((N,), torch.int32), **counts)
    if ws is None:
        ws = regions_overlap_workspace(N, cp, ct, mp, pred.device)
    given = {"counts_pred": counts_pred, "counts_truth": counts_truth, "area_pred": area_pred, "area_truth": area_truth, "n_pairs": n_pairs,
             "dropped": dropped, "iou_partner": iou_partner, "iou_inter": iou_inter, "inter_partner_truth": inter_partner_truth,
             "inter_truth": inter_truth, "inter_partner_pred": inter_partner_pred, "inter_pred": inter_pred}
    t = _regions_outputs("regions_overlap_labels", want, given, pred.device)
    _lib.check(_lib.load().cs_regions_overlap_labels(
        _p(pred), _p(truth), N, H, W, cp, ct, mp, _p(t.get("counts_pred")), _p(t.get("counts_truth")), _p(t["area_pred"]),
        _p(t["area_truth"]), _p(t["n_pairs"]), _p(t["dropped"]), _p(t["iou_partner"]), _p(t["iou_inter"]), _p(t["inter_partner_truth"]),
        _p(t["inter_truth"]), _p(t["inter_partner_pred"]), _p(t["inter_pred"]), _p(ws), ws.numel(), _stream()), "regions_overlap_labels")
    t["slot_keys"], t["slot_counts"] = _pair_table_views(ws, N, mp, 1)
    t.setdefault("counts_pred", None)
    t.setdefault("counts_truth", None)
    return t


def regions_adjacency_workspace(N, capacity, max_pairs, device):
    """the caller-owned scratch of one cs_regions_adjacency_labels call on N images with this capacity; it starts with the pair
    table, which the call's result views"""
    why = ("regions_adjacency_labels: a call takes 0 < N <= 65535 images, a capacity >= 1 and 1 <= max_pairs <= 2^29 with "
           f"N capacity and N slots < 2^31, got {(N, capacity, max_pairs)}")
    return _workspace(_int_max_pairs(_lib.load().cs_regions_adjacency_workspace, 2), device, why, int(N), int(capacity), int(max_pairs))


_ADJACENCY_TABLES = ("n_neighbors", "contact", "background", "outside", "partner", "partner_sides")


def regions_adjacency_labels(labels, capacity, max_pairs, connectivity=1, counts=None, n_pairs=None, dropped=None, n_neighbors=None,
                             contact=None, background=None, outside=None, partner=None, partner_sides=None, want_counts=True, ws=None):
    """int32 label image [N,H,W] -> a dict of int32 tensors: counts [N] (the largest label of every image; None with
    ``want_counts=False``), n_pairs, dropped [N], n_neighbors, contact, background, outside, partner, partner_sides [N,capacity], and
    the pair table itself as views of ``ws``: slot_keys int64 [N,slots] ((a << 32) | b with a < b, 0 = empty), slot_sides and
    slot_corners int32 [N,slots] (cs_regions_adjacency_labels in include/cellseg_hip.h)."""
    N, H, W = _label_images("regions_adjacency_labels", labels)
    cap, mp = int(capacity), int(max_pairs)
    want = {name: ((N, cap), torch.int32) for name in _ADJACENCY_TABLES}
    want.update(n_pairs=((N,), torch.int32), dropped=((N,), torch.int32))
    if want_counts:
        want["counts"] = ((N,), torch.int32)
    if ws is None:
        ws = regions_adjacency_workspace(N, cap, mp, labels.device)
    given = {"counts": counts, "n_pairs": n_pairs, "dropped": dropped, "n_neighbors": n_neighbors, "contact": contact,
             "background": background, "outside": outside, "partner": partner, "partner_sides": partner_sides}
    t = _regions_outputs("regions_adjacency_labels", want, given, labels.device)
    _lib.check(_lib.load().cs_regions_adjacency_labels(
        _p(labels), N, H, W, cap, mp, int(connectivity), _p(t.get("counts")), _p(t["n_pairs"]), _p(t["dropped"]), _p(t["n_neighbors"]),
        _p(t["contact"]), _p(t["background"]), _p(t["outside"]), _p(t["partner"]), _p(t["partner_sides"]), _p(ws), ws.numel(), _stream()),
        "regions_adjacency_labels")
    t["slot_keys"], t["slot_sides"], t["slot_corners"] = _pair_table_views(ws, N, mp, 2)
    t.setdefault("counts", None)
    return t


def regions_seed_labels(points, offsets, H, W, limits=None, labels=None):
    """points int64 [P,2] (row, col) with offsets int64 [N+1] and limits int32 [N] | None -> labels int32 [N,H,W]: 0 everywhere and
    k + 1 at the pixel of point k of its image (within the limit, inside the image), the lowest k of a pixel
    (cs_regions_seed_labels in include/cellseg_hip.h)"""
    points, offsets, limits, N = _point_operands("regions_seed_labels", points, offsets, limits, name="points")
    P = int(points.shape[0])
    labels = _regions_outputs("regions_seed_labels", {"labels": ((N, int(H), int(W)), torch.int32)}, {"labels": labels},
                              points.device)["labels"]
    _lib.check(_lib.load().cs_regions_seed_labels(_p(points) if P else None, _p(offsets), _p(limits), P, N, int(H), int(W), _p(labels),
                                                  _stream()), "regions_seed_labels")
    return labels


def regions_hausdorff_stage_runs():
    """the horizontal runs of an object that one stage of cs_regions_hausdorff_labels holds; an object with more is taken in chunks"""
    return int(_lib.load().cs_regions_hausdorff_stage_runs())


def regions_hausdorff_workspace(N, cap_pred, cap_truth, device):
    """the caller-owned scratch of one cs_regions_hausdorff_labels call on N images with these capacities"""
    why = ("regions_hausdorff_labels: a call takes 0 < N <= 65535 images and capacities >= 1 with N (cap_pred + cap_truth) < 2^31, "
           f"got {(N, cap_pred, cap_truth)}")
    return _workspace(_lib.load().cs_regions_hausdorff_workspace, device, why, int(N), int(cap_pred), int(cap_truth))


def regions_hausdorff_labels(pred, truth, cap_pred, cap_truth, inter_partner_truth, inter_partner_pred, partner_truth=None, d2_truth=None,
                             partner_pred=None, d2_pred=None, ws=None):
    """int32 label images pred, truth [N,H,W] and the best-intersection partners of regions_overlap_labels for the same pair
    (inter_partner_truth int32 [N,cap_truth], inter_partner_pred int32 [N,cap_pred]) -> a dict of int32 tensors: partner_truth,
    d2_truth [N,cap_truth], partner_pred, d2_pred [N,cap_pred] (cs_regions_hausdorff_labels in include/cellseg_hip.h)."""
    N, H, W, _ = _label_pair_args("regions_hausdorff_labels", pred, truth, (False, False))
    cp, ct = int(cap_pred), int(cap_truth)
    if (H - 1) ** 2 + (W - 1) ** 2 >= 1 << 31:
        raise ValueError(f"regions_hausdorff_labels: squared distances in a {H}x{W} image do not fit int32")
    for x, cap, name in ((inter_partner_truth, ct, "inter_partner_truth"), (inter_partner_pred, cp, "inter_partner_pred")):
        if x.dtype != torch.int32 or tuple(x.shape) != (N, cap):
            raise TypeError(f"regions_hausdorff_labels: {name} must be torch.int32 of shape {(N, cap)}, got {x.dtype} {tuple(x.shape)}")
    want = {"partner_truth": ((N, ct), torch.int32), "d2_truth": ((N, ct), torch.int32), "partner_pred": ((N, cp), torch.int32),
            "d2_pred": ((N, cp), torch.int32)}
    if ws is None:
        ws = regions_hausdorff_workspace(N, cp, ct, pred.device)
    t = _regions_outputs("regions_hausdorff_labels", want, {"partner_truth": partner_truth, "d2_truth": d2_truth,
                                                            "partner_pred": partner_pred, "d2_pred": d2_pred}, pred.device)
    _lib.check(_lib.load().cs_regions_hausdorff_labels(
        _p(pred), _p(truth), N, H, W, cp, ct, _p(inter_partner_truth), _p(inter_partner_pred), _p(t["partner_truth"]), _p(t["d2_truth"]),
        _p(t["partner_pred"]), _p(t["d2_pred"]), _p(ws), ws.numel(), _stream()), "regions_hausdorff_labels")
    return t


def regions_areas(mask, connectivity=1, out=None, ws=None):
    """uint8 [N,H,W] -> int32 [N,H,W]: the area of the component of equal-valued pixels under every pixel"""
    N, H, W, ws = _regions_args(mask, ws)
    if out is None:
        out = torch.empty((N, H, W), dtype=torch.int32, device=mask.device)
    _lib.check(_lib.load().cs_regions_areas(_p(mask), N, H, W, int(connectivity), _p(out), _p(ws), ws.numel(), _stream()), "regions_areas")
    return out


def regions_filter(mask, value, min_area, connectivity=1, out=None, ws=None):
    """components of `value` (0 / 1) smaller than min_area flipped; out may be mask itself"""
    N, H, W, ws = _regions_args(mask, ws)
    if out is None:
        out = torch.empty_like(mask)
    _lib.check(_lib.load().cs_regions_filter(_p(mask), N, H, W, int(connectivity), int(value), int(min_area), _p(out), _p(ws), ws.numel(),
                                             _stream()), "regions_filter")
    return out


def regions_remove_small(mask, min_object_size, hole_area_threshold, connectivity=1, out=None, ws=None):
    """remove_small_objects then remove_small_holes of the result; out may be mask itself"""
    N, H, W, ws = _regions_args(mask, ws)
    if out is None:
        out = torch.empty_like(mask)
    _lib.check(_lib.load().cs_regions_remove_small(_p(mask), N, H, W, int(min_object_size), int(hole_area_threshold), int(connectivity), _p(out),
                                                   _p(ws), ws.numel(), _stream()), "regions_remove_small")
    return out


def regions_threshold(probs, threshold):
    """fp32 probabilities of any shape -> uint8 (probs > float32(threshold)), same shape"""
    _f32(probs)
    out = torch.empty(probs.shape, dtype=torch.uint8, device=probs.device)
    if probs.numel():
        _lib.check(_lib.load().cs_regions_threshold(_p(probs), probs.numel(), float(threshold), _p(out), _stream()), "regions_threshold")
    return out


def regions_hsv_gate(images_hwc, mask, v_max=170):
    """images uint8 [..., 3], mask uint8 [...] -> uint8 (mask != 0) & (max over the 3 channels <= v_max)"""
    if images_hwc.dtype != torch.uint8 or mask.dtype != torch.uint8 or tuple(images_hwc.shape) != tuple(mask.shape) + (3,):
        raise TypeError("regions_hsv_gate: expected uint8 images [..., 3] and a uint8 mask of the leading shape")
    out = torch.empty_like(mask)
    if mask.numel():
        _lib.check(_lib.load().cs_regions_hsv_gate(_p(images_hwc), _p(mask), mask.numel(), int(v_max), _p(out), _stream()), "regions_hsv_gate")
    return out


# ---------------------------------------------------------------- detections against annotations (csrc/score.hip; score.py is the public API)
def score_workspace(N, total_gt, device):
    """the caller-owned scratch of one cs_score_points call on N images with total_gt annotations in all"""
    return _workspace(_lib.load().cs_score_workspace, device, f"score_points: a call takes 0 < N <= 65535 images, got {N}",
                      int(N), int(total_gt))


def score_points(hat, hat_off, gt, gt_off, limits=None, radius2=256, want_match=False, force_block=False, ws=None):
    """hat int64 [T,2] with hat_off int64 [N+1] (detect_cluster's points and offsets as they are), gt int32 [G,2] with gt_off int64
    [N+1], limits int32 [N] or None (Python's [:c] per image) -> (counts int32 [N,3] = tp, fp, fn; match int32 [T] or None) on the
    device.  match: the annotation index within the image, -1 = false positive, -2 = not scored (beyond the limit, or a row of hat
    that hat_off does not cover).  force_block (tests): the 256-thread path for images of at most 64 annotations too."""
    hat, hat_off, limits, N = _point_operands("score_points", hat, hat_off, limits, name="hat")
    gt, gt_off, _, _ = _point_operands("score_points", gt, gt_off, None, N, "gt", torch.int32, hat_off.device)
    radius2 = int(radius2)
    if radius2 < 0 or radius2 >= 1 << 31:
        raise ValueError(f"score_points: radius2 must be in [0, 2^31), got {radius2}")
    if ws is None:
        ws = score_workspace(N, gt.shape[0], hat.device)
    counts = torch.empty((N, 3), dtype=torch.int32, device=hat.device)
    match = torch.full((hat.shape[0],), -2, dtype=torch.int32, device=hat.device) if want_match else None
    _lib.check(_lib.load().cs_score_points(_p(hat) if hat.numel() else None, _p(hat_off), _p(limits), _p(gt) if gt.numel() else None, _p(gt_off),
                                           N, radius2, int(bool(force_block)), _p(counts), _p(match) if want_match and match.numel() else None,
                                           _p(ws), ws.numel(), _stream()), "score_points")
    return counts, match


# ---------------------------------------------------------------- neighbourhood queries over points (csrc/spatial.hip; spatial.py is the public API)
def spatial_workspace(N, H, W, bucket, P, P_other, device):
    """the caller-owned scratch of one cs_spatial_nearest / cs_spatial_count_within call; P_other = -1 without a second point set"""
    why = (f"spatial: a call takes 0 < N <= 65535 images with H^2 + W^2 < 2^31 and at most 2^22 buckets, got "
           f"{(N, H, W)} with buckets of side {bucket}")
    return _workspace(_lib.load().cs_spatial_workspace, device, why, int(N), int(H), int(W), int(bucket), int(P), int(P_other))


def _point_operands(what, pts, off, limits, n_images=None, name="pts", dtype=torch.int64, device=None):
    """the operand check of one ragged point set (csrc/cs_points.h): ``pts`` dtype [P,2], ``off`` int64 [N+1], ``limits`` int32 [N] |
    None, device tensors on the device of ``off`` -> (pts, off, limits) contiguous, N; ``n_images``, ``device``: the N it must
    have and the device it must live on (those of the call's first set)"""
    names = (name, "off", "limits") if name == "pts" else (name, f"{name}_off", f"{name}_limits")

    def need(t, name, dtype, tail):
        if not torch.is_tensor(t):
            raise TypeError(f"{what}: {name} must be a torch tensor")
        if t.dtype != dtype:
            raise TypeError(f"{what}: {name} must be {dtype}, got {t.dtype}")
        if t.dim() != 1 + len(tail) or tuple(t.shape[1:]) != tail:
            raise ValueError(f"{what}: {name} must be shaped [n{''.join(f', {v}' for v in tail)}], got {tuple(t.shape)}")
        if not t.is_cuda or t.device != off.device:
            raise ValueError(f"{what}: {name} must live on the device of {names[1]}")
        return t.contiguous()

    if not torch.is_tensor(off) or not off.is_cuda or (device is not None and off.device != device):
        raise ValueError(f"{what}: {names[1]} must be a device tensor{'' if device is None else f' on {device}'}")
    off = need(off, names[1], torch.int64, ())
    N = off.numel() - 1
    if N < 1 or N > 65535:
        raise ValueError(f"{what}: a call takes 0 < N <= 65535 images, got {N}")
    if n_images is not None and N != n_images:
        raise ValueError(f"{what}: {n_images} images but {N + 1} offsets of {name}")
    pts = need(pts, name, dtype, (2,))
    if limits is not None:
        limits = need(limits, names[2], torch.int32, ())
        if limits.numel() != N:
            raise ValueError(f"{what}: {N} images but {limits.numel()} limits of {name}")
    return pts, off, limits, N


def _spatial_args(what, pts, off, limits, other, other_off, other_limits):
    """the operand checks the two query wrappers share -> (pts, off, limits, other, other_off, other_limits) contiguous, N"""
    pts, off, limits, N = _point_operands(what, pts, off, limits)
    if other_off is None:
        if other is not None or other_limits is not None:
            raise ValueError(f"{what}: a second point set needs its offsets")
    else:
        other, other_off, other_limits, _ = _point_operands(what, other, other_off, other_limits, N, "other", device=off.device)
    return pts, off, limits, other, other_off, other_limits, N


def _spatial_common(a, H, W, bucket, ws):
    """-> the leading arguments of both query entry points, the workspace"""
    pts, off, limits, other, other_off, other_limits, N = a
    P, Q = int(pts.shape[0]), -1 if other_off is None else int(other.shape[0])
    if ws is None:
        ws = spatial_workspace(N, H, W, bucket, P, Q, pts.device)
    head = (_p(pts) if P else None, _p(off), _p(limits), P, _p(other) if Q > 0 else None, _p(other_off), _p(other_limits), max(Q, 0), N,
            int(H), int(W), int(bucket))
    return head, ws


def spatial_nearest(pts, off, H, W, bucket, k=1, limits=None, other=None, other_off=None, other_limits=None, other_xy=False,
                    index=None, d2=None, ws=None):
    """pts int64 [P,2] (row, col) with off int64 [N+1] and limits int32 [N] | None; optionally a second set other / other_off /
    other_limits of the same layout (other_xy: its rows are (col, row)) -> (index int32 [P,k], d2 int32 [P,k]) on the device: the
    k smallest keys (d2, index within the image) among the live targets of every live point, (-1, -1) beyond their number, (-2, -1)
    in the rows that are not live (cs_spatial_nearest in include/cellseg_hip.h)"""
    a = _spatial_args("spatial_nearest", pts, off, limits, other, other_off, other_limits)
    k = int(k)
    if not 1 <= k <= 8:
        raise ValueError(f"spatial_nearest: k must be in 1..8, got {k}")
    head, ws = _spatial_common(a, H, W, bucket, ws)
    P = int(a[0].shape[0])
    t = _regions_outputs("spatial_nearest", {"index": ((P, k), torch.int32), "d2": ((P, k), torch.int32)}, {"index": index, "d2": d2},
                         a[0].device)
    _lib.check(_lib.load().cs_spatial_nearest(*head, k, int(bool(other_xy)), _p(t["index"]) if P else None, _p(t["d2"]) if P else None,
                                              _p(ws), ws.numel(), _stream()), "spatial_nearest")
    return t["index"], t["d2"]


def spatial_count_within(pts, off, H, W, bucket, radii2, limits=None, other=None, other_off=None, other_limits=None, other_xy=False,
                         counts=None, pair_counts=None, ws=None):
    """spatial_nearest's operands and radii2, 1 to 8 host integers in [0, 2^31) -> (counts int32 [P,R], pair_counts int64 [N,R]) on
    the device: the live targets with d2 <= radii2[j] of every live point (-1 in the rows that are not live) and their per-image
    sums (cs_spatial_count_within in include/cellseg_hip.h)"""
    a = _spatial_args("spatial_count_within", pts, off, limits, other, other_off, other_limits)
    r2 = [int(v) for v in radii2]
    if not 1 <= len(r2) <= 8 or any(v < 0 or v >= 1 << 31 for v in r2):
        raise ValueError(f"spatial_count_within: 1 to 8 radii2 in [0, 2^31), got {r2}")
    head, ws = _spatial_common(a, H, W, bucket, ws)
    P, N, R = int(a[0].shape[0]), a[6], len(r2)
    t = _regions_outputs("spatial_count_within", {"counts": ((P, R), torch.int32), "pair_counts": ((N, R), torch.int64)},
                         {"counts": counts, "pair_counts": pair_counts}, a[0].device)
    _lib.check(_lib.load().cs_spatial_count_within(*head, (ctypes.c_int32 * R)(*r2), R, int(bool(other_xy)), _p(t["counts"]) if P else None,
                                                   _p(t["pair_counts"]), _p(ws), ws.numel(), _stream()), "spatial_count_within")
    return t["counts"], t["pair_counts"]


def spatial_cluster_workspace(N, H, W, bucket, P, device):
    """the caller-owned scratch of one cs_spatial_cluster call"""
    why = (f"spatial: a call takes 0 < N <= 65535 images with H^2 + W^2 < 2^31 and at most 2^22 buckets, got "
           f"{(N, H, W)} with buckets of side {bucket}")
    return _workspace(_lib.load().cs_spatial_cluster_workspace, device, why, int(N), int(H), int(W), int(bucket), int(P))


def spatial_cluster(pts, off, H, W, bucket, radius2, min_samples, limits=None, labels=None, core=None, n_clusters=None, size=None,
                    n_core=None, sums=None, bbox=None, ws=None):
    """pts int64 [P,2] with off int64 [N+1] and limits int32 [N] | None, radius2 in [0, 2^31) and min_samples >= 1 host integers ->
    (labels int32 [P], core uint8 [P], n_clusters int32 [N], size int32 [P], n_core int32 [P], sums int64 [P,2], bbox int32 [P,4])
    on the device: DBSCAN of every image's live points; cluster c of image n is row off[n] + c of the four tables
    (cs_spatial_cluster in include/cellseg_hip.h)"""
    pts, off, limits, N = _point_operands("spatial_cluster", pts, off, limits)
    radius2, min_samples = int(radius2), int(min_samples)
    if not 0 <= radius2 < 1 << 31:
        raise ValueError(f"spatial_cluster: radius2 must be in [0, 2^31), got {radius2}")
    if not 1 <= min_samples < 1 << 31:
        raise ValueError(f"spatial_cluster: min_samples must be in [1, 2^31), got {min_samples}")
    P = int(pts.shape[0])
    if ws is None:
        ws = spatial_cluster_workspace(N, H, W, bucket, P, pts.device)
    want = {"labels": ((P,), torch.int32), "core": ((P,), torch.uint8), "n_clusters": ((N,), torch.int32), "size": ((P,), torch.int32),
            "n_core": ((P,), torch.int32), "sums": ((P, 2), torch.int64), "bbox": ((P, 4), torch.int32)}
    t = _regions_outputs("spatial_cluster", want, {"labels": labels, "core": core, "n_clusters": n_clusters, "size": size, "n_core": n_core,
                                                   "sums": sums, "bbox": bbox}, pts.device)
    out = [_p(t[name]) if P or name == "n_clusters" else None for name in want]
    _lib.check(_lib.load().cs_spatial_cluster(_p(pts) if P else None, _p(off), _p(limits), P, N, int(H), int(W), int(bucket), radius2,
                                              min_samples, *out, _p(ws), ws.numel(), _stream()), "spatial_cluster")
    return tuple(t[name] for name in want)


def spatial_bin_counts(pts, off, H, W, bin, limits=None, out=None):
    """pts int64 [P,2] with off int64 [N+1] and limits int32 [N] | None -> int32 [N, ceil(H/bin), ceil(W/bin)] on the device: the live
    points per square bin (cs_spatial_bin_counts in include/cellseg_hip.h)"""
    pts, off, limits, N = _point_operands("spatial_bin_counts", pts, off, limits)
    bin = int(bin)
    if bin < 1:
        raise ValueError(f"spatial_bin_counts: bin must be positive, got {bin}")
    P = int(pts.shape[0])
    shape = (N, -(-int(H) // bin), -(-int(W) // bin))
    out = _regions_outputs("spatial_bin_counts", {"out": (shape, torch.int32)}, {"out": out}, pts.device)["out"]
    _lib.check(_lib.load().cs_spatial_bin_counts(_p(pts) if P else None, _p(off), _p(limits), P, N, int(H), int(W), bin, _p(out), _stream()),
               "spatial_bin_counts")
    return out


# ---------------------------------------------------------------- tissue detection (csrc/tissue.hip; tissue.py is the public API)
CS_TISSUE_CHROMA, CS_TISSUE_DARKNESS = 0, 1


def _rgb_images(what, images_u8, name="images", whole_batch=False):
    """the check of every pass over uint8 RGB images (csrc/cs_pixels.h) -> (N, H, W); ``whole_batch``: the pass walks the batch as
    one run of pixels, so all of them together stay below 2^31"""
    if not torch.is_tensor(images_u8) or images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or images_u8.shape[-1] != 3:
        raise TypeError(f"{what}: {name} must be a uint8 tensor shaped [N, H, W, 3]")
    N, H, W, _ = images_u8.shape
    if not 1 <= N <= 65535 or H < 1 or W < 1 or (N if whole_batch else 1) * H * W >= 1 << 31:
        limit = "with N H W < 2^31" if whole_batch else "of 0 < H W < 2^31"
        raise ValueError(f"{what}: a call takes 0 < N <= 65535 images {limit} pixels, got {(N, H, W)}")
    return N, H, W


def tissue_histogram(images_u8, channel=CS_TISSUE_CHROMA, hist=None):
    """images uint8 [N,H,W,3] (device) -> int64 [N,256] on the device: the pixels of every image per value of the feature
    ``channel``.  ``hist``: an int64 [N,256] device tensor to ADD into instead of a zeroed one (cs_tissue_histogram)."""
    N, H, W = _rgb_images("tissue_histogram", images_u8)
    if hist is None:
        hist = torch.zeros((N, 256), dtype=torch.int64, device=images_u8.device)
    elif not torch.is_tensor(hist) or hist.dtype != torch.int64 or tuple(hist.shape) != (N, 256):
        raise ValueError(f"tissue_histogram: hist must be an int64 tensor shaped {(N, 256)}")
    _lib.check(_lib.load().cs_tissue_histogram(_p(images_u8), N, H, W, int(channel), _p(hist), _stream()), "tissue_histogram")
    return hist


def tissue_mask(images_u8, thr, channel=CS_TISSUE_CHROMA, out=None):
    """images uint8 [N,H,W,3], thr int32 [N] (both on the device) -> uint8 [N,H,W]: feature > thr[n] as 0 / 1 (cs_tissue_mask)"""
    N, H, W = _rgb_images("tissue_mask", images_u8)
    if not torch.is_tensor(thr) or thr.dtype != torch.int32 or tuple(thr.shape) != (N,):
        raise ValueError(f"tissue_mask: thr must be an int32 tensor shaped {(N,)}")
    out = _regions_outputs("tissue_mask", {"out": ((N, H, W), torch.uint8)}, {"out": out}, images_u8.device)["out"]
    _lib.check(_lib.load().cs_tissue_mask(_p(images_u8), N, H, W, int(channel), _p(thr), _p(out), _stream()), "tissue_mask")
    return out


def tissue_coverage(mask, tile_img, tile_rc, ph, pw):
    """mask uint8 [N,H,W], tile_img int32 [T], tile_rc int32 [T,2] (device) -> int32 [T]: the non-zero mask pixels under every
    ph x pw window, clamped to the image (cs_tissue_coverage)"""
    if not torch.is_tensor(mask) or mask.dtype != torch.uint8 or mask.dim() != 3:
        raise TypeError("tissue_coverage: mask must be a uint8 tensor shaped [N, H, W]")
    N, H, W = mask.shape
    T = int(tile_img.numel())
    if tile_img.dtype != torch.int32 or tile_rc.dtype != torch.int32 or tuple(tile_rc.shape) != (T, 2):
        raise ValueError(f"tissue_coverage: tile_img int32 [T] and tile_rc int32 [T, 2], got {tuple(tile_img.shape)} and {tuple(tile_rc.shape)}")
    cover = torch.empty((T,), dtype=torch.int32, device=mask.device)
    _lib.check(_lib.load().cs_tissue_coverage(_p(mask), N, H, W, _p(tile_img) if T else None, _p(tile_rc) if T else None, T, int(ph), int(pw),
                                              _p(cover) if T else None, _stream()), "tissue_coverage")
    return cover


def tissue_select(cover, min_pixels):
    """cover int32 [T] (device) -> (selected int32 [T], n_selected int32 [1]) on the device: the indices with cover >= min_pixels
    in rising order, -1 from their number on (cs_tissue_select)"""
    if not torch.is_tensor(cover) or cover.dtype != torch.int32 or cover.dim() != 1:
        raise TypeError("tissue_select: cover must be an int32 tensor shaped [T]")
    T = int(cover.numel())
    selected = torch.empty((T,), dtype=torch.int32, device=cover.device)
    n_selected = torch.empty((1,), dtype=torch.int32, device=cover.device)
    _lib.check(_lib.load().cs_tissue_select(_p(cover) if T else None, T, int(min_pixels), _p(selected) if T else None, _p(n_selected), _stream()),
               "tissue_select")
    return selected, n_selected


# ---------------------------------------------------------------- stain separation and normalisation (csrc/stain.hip; stain.py is the public API)
def _stain_args(what, images_u8, od_q, mask=None, **mats):
    """the checks every stain wrapper shares; ``mats``: name -> (fp32 device tensor, its shape after N)"""
    N, H, W = _rgb_images(what, images_u8)
    if not torch.is_tensor(od_q) or od_q.dtype != torch.int32 or tuple(od_q.shape) != (256,):
        raise ValueError(f"{what}: od_q must be an int32 tensor shaped (256,) (stain.od_table)")
    if mask is not None and (not torch.is_tensor(mask) or mask.dtype != torch.uint8 or tuple(mask.shape) != (N, H, W)):
        raise ValueError(f"{what}: mask must be a uint8 tensor shaped {(N, H, W)}")
    for name, (m, shape) in mats.items():
        if not torch.is_tensor(m) or m.dtype != torch.float32 or tuple(m.shape) != (N,) + shape:
            raise ValueError(f"{what}: {name} must be a float32 tensor shaped {(N,) + shape}")
    return N, H, W


def _stain_sums(what, given, shape, device):
    if given is None:
        return torch.zeros(shape, dtype=torch.int64, device=device)
    if not torch.is_tensor(given) or given.dtype != torch.int64 or tuple(given.shape) != shape:
        raise ValueError(f"{what}: out must be an int64 tensor shaped {shape}")
    return given


def stain_moments(images_u8, od_q, beta_q, mask=None, out=None):
    """images uint8 [N,H,W,3], od_q int32 [256], mask uint8 [N,H,W] or None (device) -> int64 [N,10]: over the kept pixels their
    number and the sums of od_q r, g, b, rr, rg, rb, gg, gb, bb.  ``out``: an int64 [N,10] tensor to ADD into instead of a zeroed
    one (cs_stain_moments)."""
    N, H, W = _stain_args("stain_moments", images_u8, od_q, mask)
    out = _stain_sums("stain_moments", out, (N, 10), images_u8.device)
    _lib.check(_lib.load().cs_stain_moments(_p(images_u8), N, H, W, _p(od_q), int(beta_q), _p(mask), _p(out), _stream()), "stain_moments")
    return out


def stain_angle_hist(images_u8, od_q, beta_q, V, bins, mask=None, out=None):
    """V fp32 [N,3,2] -> int64 [N,bins]: the kept pixels by the angle atan2f(p1, p0) of p = od V over [-pi/2, pi/2); ADDS into
    ``out`` where given (cs_stain_angle_hist)"""
    N, H, W = _stain_args("stain_angle_hist", images_u8, od_q, mask, V=(V, (3, 2)))
    out = _stain_sums("stain_angle_hist", out, (N, int(bins)), images_u8.device)
    _lib.check(_lib.load().cs_stain_angle_hist(_p(images_u8), N, H, W, _p(od_q), int(beta_q), _p(mask), _p(V), int(bins), _p(out), _stream()),
               "stain_angle_hist")
    return out


def stain_conc_hist(images_u8, od_q, beta_q, P, bins, conc_max, mask=None, out=None):
    """P fp32 [N,2,3] -> int64 [N,2,bins]: the kept pixels by each concentration of c = P od over [0, conc_max); ADDS into ``out``
    where given (cs_stain_conc_hist)"""
    N, H, W = _stain_args("stain_conc_hist", images_u8, od_q, mask, P=(P, (2, 3)))
    out = _stain_sums("stain_conc_hist", out, (N, 2, int(bins)), images_u8.device)
    _lib.check(_lib.load().cs_stain_conc_hist(_p(images_u8), N, H, W, _p(od_q), int(beta_q), _p(mask), _p(P), int(bins), float(conc_max),
                                              _p(out), _stream()), "stain_conc_hist")
    return out


def stain_apply(images_u8, od_q, A, Io, out=None):
    """A fp32 [N,3,3] -> uint8 [N,H,W,3]: clamp(rint(Io expf(-(A od))), 0, 255) for every pixel; ``out`` must not be the images
    (cs_stain_apply)"""
    N, H, W = _stain_args("stain_apply", images_u8, od_q, A=(A, (3, 3)))
    out = _regions_outputs("stain_apply", {"out": ((N, H, W, 3), torch.uint8)}, {"out": out}, images_u8.device)["out"]
    if out.data_ptr() == images_u8.data_ptr():
        raise ValueError("stain_apply: out must not be the images")
    _lib.check(_lib.load().cs_stain_apply(_p(images_u8), N, H, W, _p(od_q), _p(A), float(Io), _p(out), _stream()), "stain_apply")
    return out


def stain_separate(images_u8, od_q, P, as_u8=False, conc_max=1.0, out=None):
    """P fp32 [N,K,3], K = 2 or 3 -> the concentrations P od of every pixel: fp32 [N,H,W,K], or with ``as_u8`` uint8
    clamp(rint(255 c / conc_max), 0, 255) (cs_stain_separate)"""
    if not torch.is_tensor(P) or P.dim() != 3 or P.shape[1] not in (2, 3):
        raise ValueError("stain_separate: P must be a float32 tensor shaped [N, K, 3] with K = 2 or 3")
    Kn = int(P.shape[1])
    N, H, W = _stain_args("stain_separate", images_u8, od_q, P=(P, (Kn, 3)))
    out = _regions_outputs("stain_separate", {"out": ((N, H, W, Kn), torch.uint8 if as_u8 else torch.float32)}, {"out": out},
                           images_u8.device)["out"]
    _lib.check(_lib.load().cs_stain_separate(_p(images_u8), N, H, W, _p(od_q), _p(P), Kn, int(bool(as_u8)), float(conc_max), _p(out),
                                             _stream()), "stain_separate")
    return out


STAIN_QUANTIFY_BINS = (0, 16, 32, 64, 128, 256)


def stain_quantify_labels(images_u8, labels, od_q, Mq, capacity, expanded=None, pos_levels=None, bins=0, counts=None, want_counts=True,
                          **tables):
    """images uint8 [N,H,W,3], labels (and expanded or None) int32 [N,H,W], od_q int32 [256], Mq int32 [N,K,3] (device) -> dict of
    n int32 [N,cap,C]; sum, sumsq int64 and max, pos int32 [N,cap,C,K]; hist int32 [N,cap,C,K,bins] (with bins) and counts int32 [N]
    (with ``want_counts``): the integer stain levels of every (label, compartment), C = 2 with ``expanded``.  ``pos_levels``: K host
    integers in [0, 256] or None; ``tables``: tensors to write instead of new ones (cs_stain_quantify_labels in
    include/cellseg_hip.h)."""
    what = "stain_quantify_labels"
    N, H, W = _rgb_images(what, images_u8, whole_batch=True)
    if not torch.is_tensor(od_q) or od_q.dtype != torch.int32 or tuple(od_q.shape) != (256,):
        raise ValueError(f"{what}: od_q must be an int32 tensor shaped (256,) (stain.od_table)")
    if not torch.is_tensor(Mq) or Mq.dtype != torch.int32 or Mq.dim() != 3 or tuple(Mq.shape) not in ((N, 2, 3), (N, 3, 3)):
        raise ValueError(f"{what}: Mq must be an int32 tensor shaped [{N}, K, 3] with K = 2 or 3")
    Kn, cap, bins = int(Mq.shape[1]), int(capacity), int(bins)
    for name, x in (("labels", labels), ("expanded", expanded)):
        if x is not None and (tuple(_label_images(what, x)) != (N, H, W)):
            raise ValueError(f"{what}: {name} of shape {tuple(x.shape)} for images of {(N, H, W)}")
    if bins not in STAIN_QUANTIFY_BINS:
        raise ValueError(f"{what}: bins must be one of {STAIN_QUANTIFY_BINS}, got {bins}")
    levels = None
    if pos_levels is not None:
        if len(pos_levels) != Kn:
            raise ValueError(f"{what}: {Kn} stains but {len(pos_levels)} positive levels")
        levels = (ctypes.c_int32 * Kn)(*[int(v) for v in pos_levels])
    C = 1 if expanded is None else 2
    want = {"n": ((N, cap, C), torch.int32), "sum": ((N, cap, C, Kn), torch.int64), "sumsq": ((N, cap, C, Kn), torch.int64),
            "max": ((N, cap, C, Kn), torch.int32), "pos": ((N, cap, C, Kn), torch.int32)}
    if bins:
        want["hist"] = ((N, cap, C, Kn, bins), torch.int32)
    if want_counts:
        want["counts"] = ((N,), torch.int32)
    t = _regions_outputs(what, want, dict(tables, counts=counts), images_u8.device)
    _lib.check(_lib.load().cs_stain_quantify_labels(_p(images_u8), _p(labels), _p(expanded), N, H, W, _p(od_q), _p(Mq), Kn, levels, bins,
                                                    cap, _p(t.get("counts")), _p(t["n"]), _p(t["sum"]), _p(t["sumsq"]), _p(t["max"]),
                                                    _p(t["pos"]), _p(t.get("hist")), _stream()), what)
    return t


# ---------------------------------------------------------------- annotated images (csrc/render.hip; render.py is the public API)
CS_RENDER_FILL_NONE, CS_RENDER_FILL_MASK, CS_RENDER_FILL_HEAT_U8, CS_RENDER_FILL_HEAT_F32 = 0, 1, 2, 3
CS_RENDER_POINTS_XY, CS_RENDER_POINTS_TAIL = 1, 2
RENDER_MAX_RADIUS = 64


def _render_rgb(what, name, rgb):
    """three integers in [0, 255] -> r | g << 8 | b << 16"""
    try:
        r, g, b = (int(v) for v in rgb)
        ok = all(not isinstance(v, bool) and int(v) == v for v in rgb)
    except (TypeError, ValueError):
        ok = False
    if not ok or not all(0 <= v <= 255 for v in (r, g, b)):
        raise ValueError(f"{what}: {name} must be three integers in [0, 255], got {rgb!r}")
    return r | g << 8 | b << 16


def render_compose(images_u8, fill=CS_RENDER_FILL_NONE, fill_map=None, threshold=0.0, invert=True, colormap=None, labels=None,
                   outline_color=(255, 255, 0), palette=None, out=None):
    """images uint8 [N,H,W,3] -> uint8 [N,H,W,3], one launch: the fill ``fill`` from ``fill_map`` (uint8 [N,H,W]; fp32 for
    CS_RENDER_FILL_HEAT_F32, with ``threshold``) through ``colormap`` uint8 [256,3], then the outline of ``labels`` int32 [N,H,W] in
    ``outline_color`` or ``palette`` uint8 [P,3]; ``out`` may be the images (cs_render_compose in include/cellseg_hip.h)"""
    N, H, W = _rgb_images("render_compose", images_u8, whole_batch=True)
    if fill not in (CS_RENDER_FILL_NONE, CS_RENDER_FILL_MASK, CS_RENDER_FILL_HEAT_U8, CS_RENDER_FILL_HEAT_F32):
        raise ValueError(f"render_compose: unknown fill {fill!r}")
    if (fill == CS_RENDER_FILL_NONE) != (fill_map is None):
        raise ValueError("render_compose: a fill needs its map, no fill takes none")
    heat = fill in (CS_RENDER_FILL_HEAT_U8, CS_RENDER_FILL_HEAT_F32)
    if fill_map is not None:
        want = torch.float32 if fill == CS_RENDER_FILL_HEAT_F32 else torch.uint8
        if not torch.is_tensor(fill_map) or fill_map.dtype != want or tuple(fill_map.shape) != (N, H, W):
            raise TypeError(f"render_compose: the map of this fill must be a {want} tensor shaped {(N, H, W)}")
    if heat and (not torch.is_tensor(colormap) or colormap.dtype != torch.uint8 or tuple(colormap.shape) != (256, 3)):
        raise TypeError("render_compose: a heat fill needs a uint8 colour table shaped (256, 3)")
    if labels is not None and (not torch.is_tensor(labels) or labels.dtype != torch.int32 or tuple(labels.shape) != (N, H, W)):
        raise TypeError(f"render_compose: labels must be an int32 tensor shaped {(N, H, W)}")
    rows = 0
    if palette is not None:
        if labels is None:
            raise ValueError("render_compose: a palette needs the labels")
        if not torch.is_tensor(palette) or palette.dtype != torch.uint8 or palette.dim() != 2 or palette.shape[1] != 3:
            raise TypeError("render_compose: palette must be a uint8 tensor shaped [P, 3]")
        rows = int(palette.shape[0])
        if not 1 <= rows <= 256:
            raise ValueError(f"render_compose: a palette has 1 to 256 rows, got {rows}")
    rgb = _render_rgb("render_compose", "outline_color", outline_color)
    out = _regions_outputs("render_compose", {"out": ((N, H, W, 3), torch.uint8)}, {"out": out}, images_u8.device)["out"]
    a, b, n = images_u8.data_ptr(), out.data_ptr(), 3 * N * H * W
    if a != b and a < b + n and b < a + n:
        raise ValueError("render_compose: out may be the images themselves, or must not overlap them")
    _lib.check(_lib.load().cs_render_compose(_p(images_u8), N, H, W, int(fill), _p(fill_map), float(threshold), int(bool(invert)),
                                             _p(colormap) if heat else None, _p(labels), rgb, _p(palette), rows, _p(out), _stream()),
               "render_compose")
    return out


def render_points(canvas_u8, pts, off, limits=None, radius=4, color=(255, 0, 0), thickness=-1, xy=False, tail=False):
    """draws into canvas uint8 [N,H,W,3] in place and returns it: pts int64 [P,2] with off int64 [N+1] and limits int32 [N] | None
    (the triple of spatial_bin_counts), every kept row -- with ``tail`` every row that limits does not keep -- as a disc of
    ``radius`` (thickness < 0) or a ring of that thickness (cs_render_points in include/cellseg_hip.h)"""
    N, H, W = _rgb_images("render_points", canvas_u8, "canvas", whole_batch=True)
    radius, thickness = int(radius), int(thickness)
    if not 0 <= radius <= RENDER_MAX_RADIUS:
        raise ValueError(f"render_points: radius must be in [0, {RENDER_MAX_RADIUS}], got {radius}")
    if thickness == 0 or thickness > 2 * radius:
        raise ValueError(f"render_points: thickness must be negative (filled) or in [1, 2 radius = {2 * radius}], got {thickness}")
    rgb = _render_rgb("render_points", "color", color)
    if not canvas_u8.is_cuda:
        raise ValueError("render_points: the canvas must be a device tensor")
    pts, off, limits, _ = _point_operands("render_points", pts, off, limits, N, device=canvas_u8.device)
    if tail and limits is None:
        raise ValueError("render_points: tail draws the points from limits[n] on: it needs limits")
    P = int(pts.shape[0])
    flags = (CS_RENDER_POINTS_XY if xy else 0) | (CS_RENDER_POINTS_TAIL if tail else 0)
    if P:
        _lib.check(_lib.load().cs_render_points(_p(canvas_u8), N, H, W, _p(pts), _p(off), _p(limits), P, radius, max(thickness, -1), rgb, flags,
                                                _stream()), "render_points")
    return canvas_u8


# ---------------------------------------------------------------- polygons to pixels (csrc/polygons.hip; polygons.py is the public API)
CS_POLYGON_EVENODD, CS_POLYGON_NONZERO = 0, 1
CS_POLYGON_LABELS, CS_POLYGON_MASK = 0, 1
POLYGON_MAX_SUB = 8
POLYGON_MAX_COORD = 1 << 28           # of a quantised vertex coordinate, either sign


def polygons_check_size(what, N, H, W, sub):
    """the sizes cs_polygons_rasterize takes, checked without the library"""
    if isinstance(sub, bool) or not isinstance(sub, int) or not 0 <= sub <= POLYGON_MAX_SUB:
        raise ValueError(f"{what}: sub must be an integer in [0, {POLYGON_MAX_SUB}], got {sub!r}")
    if not 1 <= N <= 65535 or H < 1 or W < 1 or H * W >= 1 << 31:
        raise ValueError(f"{what}: a call takes 0 < N <= 65535 images of 0 < H W < 2^31 pixels, got {(N, H, W)}")
    if max(H, W) << (sub + 1) >= 1 << 30:
        raise ValueError(f"{what}: max(H, W) << (sub + 1) must stay below 2^30, got {(H, W)} at sub={sub}")


def polygons_rasterize(vertices, ring_start, ring_count, shape_rings, image_shapes, out, sub, rule=CS_POLYGON_EVENODD, items=None):
    """paints into ``out`` (int32 [N,H,W]: labels by maximum; uint8 [N,H,W]: 1 where covered) and returns it.  vertices int32 [V,2],
    ring_start / ring_count int32 [R], shape_rings int32 [S+1], image_shapes int32 [N+1], items int32 [I,3] | None, all on the device
    of ``out``; pixels that no shape takes are not written (cs_polygons_rasterize in include/cellseg_hip.h)."""
    if not torch.is_tensor(out) or out.dim() != 3 or out.dtype not in (torch.int32, torch.uint8):
        raise TypeError("polygons_rasterize: out must be an int32 (labels) or uint8 (mask) tensor shaped [N, H, W]")
    N, H, W = (int(v) for v in out.shape)
    polygons_check_size("polygons_rasterize", N, H, W, sub)
    if rule not in (CS_POLYGON_EVENODD, CS_POLYGON_NONZERO):
        raise ValueError(f"polygons_rasterize: unknown rule {rule!r}")
    tabs = {"vertices": vertices, "ring_start": ring_start, "ring_count": ring_count, "shape_rings": shape_rings,
            "image_shapes": image_shapes}
    if items is not None:
        tabs["items"] = items
    for name, t in tabs.items():
        if not torch.is_tensor(t) or t.dtype != torch.int32:
            raise TypeError(f"polygons_rasterize: {name} must be an int32 tensor")
    V, R, S = int(vertices.numel()) // 2, int(ring_start.numel()), int(shape_rings.numel()) - 1
    I = 0 if items is None else int(items.numel()) // 3
    if (vertices.numel() % 2 or int(ring_count.numel()) != R or S < 0 or int(image_shapes.numel()) != N + 1
            or (items is not None and items.numel() % 3)):
        raise ValueError("polygons_rasterize: vertices [V,2], ring_start and ring_count [R], shape_rings [S+1], image_shapes [N+1], "
                         f"items [I,3]; got {[tuple(t.shape) for t in tabs.values()]} for {N} images")
    if items is not None and I == 0:
        return out
    mode = CS_POLYGON_LABELS if out.dtype == torch.int32 else CS_POLYGON_MASK
    _lib.check(_lib.load().cs_polygons_rasterize(_p(vertices) if V else None, V, _p(ring_start) if R else None, _p(ring_count) if R else None,
                                                 R, _p(shape_rings), S, _p(image_shapes), _p(items), I, N, H, W, sub, rule, mode, _p(out),
                                                 _stream()), "polygons_rasterize")
    return out


# ---------------------------------------------------------------- augmented input staging (csrc/augment.hip; augment.py is the public API)
def stage_augmented_workspace(n_tiles, device):
    """the caller-owned scratch of one cs_stage_augmented call whose records hold a contrast op"""
    ws_bytes = _lib.load().cs_stage_augmented_workspace(int(n_tiles))
    if ws_bytes == 0:
        raise ValueError(f"stage_augmented: a call takes 0 < T < 2^31 tiles, got {n_tiles}")
    return torch.empty((ws_bytes // 8,), dtype=torch.float64, device=device)


def stage_augmented(images_u8, tile_img, tile_rc, th, tw, flips=None, ops=None, factors=None, has_contrast=False, dtype=torch.bfloat16,
                    mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), out=None, ws=None):
    """Device operands as they are (nothing is validated against the images here: augment.py does that on the host): images_u8 uint8
    [n,H,W,3], tile_img int32 [T], tile_rc int32 [T,2], flips int8 [T] or None, ops int8 [T,4] with factors float32 [T,4] or None ->
    NHWC [T,th,tw,8] dtype.  has_contrast: some record holds op code 1 (the mean reduction runs, into ws).  Enqueues 1 or 3 stream
    operations and never synchronises: with out (and ws) given it can be captured into a graph."""
    def need(t, what, dt, shape):
        if not torch.is_tensor(t) or t.dtype != dt or tuple(t.shape) != shape:
            raise TypeError(f"stage_augmented: {what} must be a {dt} tensor shaped {list(shape)}")
        return t

    if not torch.is_tensor(images_u8) or images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or images_u8.shape[-1] != 3:
        raise TypeError("stage_augmented expects uint8 images shaped [n, H, W, 3]")
    n, H, W, _ = images_u8.shape
    T = int(tile_img.numel()) if torch.is_tensor(tile_img) else -1
    need(tile_img, "tile_img", torch.int32, (T,))
    need(tile_rc, "tile_rc", torch.int32, (T, 2))
    if flips is not None:
        need(flips, "flips", torch.int8, (T,))
    if (ops is None) != (factors is None):
        raise TypeError("stage_augmented: ops and factors come together")
    if ops is not None:
        need(ops, "ops", torch.int8, (T, 4))
        need(factors, "factors", torch.float32, (T, 4))
    if has_contrast and ops is None:
        raise ValueError("stage_augmented: has_contrast without a jitter record")
    code = _code(dtype)
    if out is None:
        out = torch.empty((T, th, tw, 8), dtype=dtype, device=images_u8.device)
    elif out.dtype != dtype or tuple(out.shape) != (T, th, tw, 8):
        raise TypeError(f"stage_augmented: out must be {dtype} shaped {[T, th, tw, 8]}")
    if has_contrast and ws is None:
        ws = stage_augmented_workspace(T, images_u8.device)
    m = (ctypes.c_float * 3)(*[float(v) for v in mean])
    s = (ctypes.c_float * 3)(*[float(v) for v in std])
    _lib.check(_lib.load().cs_stage_augmented(_p(images_u8), n, H, W, _p(tile_img), _p(tile_rc), _p(flips), _p(ops), _p(factors),
                                              int(bool(has_contrast)), T, int(th), int(tw), m, s, code, _p(out),
                                              _p(ws) if has_contrast else None, ws.numel() * 8 if has_contrast else 0, _stream()),
               "stage_augmented")
    return out
