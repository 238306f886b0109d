"""GPU: the row passes over NHWC rows [M][C] -- BatchNorm statistics / finalize / apply / backward and the per-sample row sums -- give
the SAME BITS as the digests recorded in tests/golden/row_passes_digests.json (SHA-256 of the raw output bytes).  The file was recorded
from the library as it stood before these kernels were moved onto the shared row placement of csrc/cs_rows.h (the commit and compiler
are named in the file), so a change to the placement, the row walk or the folds that alters a summation order, a rounding or which
multiply-adds the compiler fuses shows here, on every decomposition the launch rules produce.

Inputs are integer hashes of the flat index scaled by a power of two and cast on the CPU: the same bits on any host.

    python tests/test_row_passes_bits_gpu.py --record [--out FILE] [--commit HASH]      rewrites the digests from the loaded library
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

from cellsegmentation_amd import kernels as K  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "row_passes_digests.json")

# tests/test_bn_reductions_gpu.py::SHAPES (one chunk / 16-, 32-, 64-group chunks with a ragged last one, atomics and partial rows, row
# counts that are no multiple of a row block) ...
BN_SHAPES = [(6400, 1392), (6400, 2304), (9001, 288), (5000, 816), (23104, 576), (37, 8), (1000, 40), (300, 520), (8, 512), (70001, 24),
             (6400, 232), (2000, 136), (123457, 64)]
# ... + a single row (forward only), width 3 / rpar 85 / one dead lane / fewer rows than rpar, and CG = 257 (last element-wise chunk 1 wide)
EXTRA_SHAPES = [(1, 8), (3, 24), (300, 2056)]
F32_BWD_APPLY_SHAPES = EXTRA_SHAPES + [(5000, 816)]
SUM_SHAPES = [(2, 10, 10, 144), (3, 19, 19, 1392), (2, 40, 40, 24), (1, 150, 150, 40)]
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
EPS, MOMENTUM = 1e-3, 0.1


def _hash16(n, seed):
    """n values in [0, 65536): a multiplicative hash of the flat index (uint32 arithmetic, i.e. mod 2^32, only)."""
    h = np.arange(n, dtype=np.uint32) * np.uint32(2654435761) + np.uint32((seed * 0x9E3779B1) & 0xFFFFFFFF)
    h ^= h >> np.uint32(15)
    h *= np.uint32(0x2C1B3C6D)
    h ^= h >> np.uint32(13)
    return ((h >> np.uint32(8)) & np.uint32(0xFFFF)).astype(np.int32)


def _signed(shape, seed, dtype, dev):
    """values k * 2^-14, k in [-32768, 32768), cast to `dtype` on the CPU"""
    n = int(np.prod(shape))
    v = torch.from_numpy((_hash16(n, seed) - 32768).astype(np.float32) * np.float32(2.0 ** -14)).view(*shape)
    return v.to(dtype).to(dev)


def _positive(n, seed, dev):
    """fp32 values 0.5 + k * 2^-16, k in [0, 65536)"""
    return torch.from_numpy(_hash16(n, seed).astype(np.float32) * np.float32(2.0 ** -16) + np.float32(0.5)).to(dev)


def _digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        t = t.contiguous()
        if t.dtype == torch.bfloat16:
            t = t.view(torch.int16)
        h.update(t.cpu().numpy().tobytes())
    return h.hexdigest()


_cache = {}


def _bn_inputs(M, C, tname):
    """z / dy / res in the element type, fp32 gamma / beta, batch mean / rstd from the library's own statistics -- each made when first
    asked for.  One (shape, dtype) is kept: its groups run next to each other."""
    key = (M, C, tname)
    if _cache.get("key") != key:
        _cache.clear()
        _cache["key"] = key
    dev, dtype, seed = torch.device("cuda:0"), DTYPES[tname], 7 * M + C
    make = {"z": lambda: _signed((M, C), seed, dtype, dev), "dy": lambda: _signed((M, C), seed + 1, dtype, dev),
            "res": lambda: _signed((M, C), seed + 2, dtype, dev), "gamma": lambda: _positive(C, seed + 3, dev),
            "beta": lambda: _signed((C,), seed + 4, torch.float32, dev) * 0.125,
            "moments": lambda: K.bn_finalize(K.bn_stats(get("z")), M, EPS, MOMENTUM)}

    def get(name):
        if name not in _cache:
            _cache[name] = make[name]()
        return _cache[name]
    return get


def _running(C, seed, dev):
    return _signed((C,), seed + 5, torch.float32, dev), _positive(C, seed + 6, dev)


def group_bn_fwd(M, C, tname):
    d = _bn_inputs(M, C, tname)
    stats = K.bn_stats(d("z"))
    rm, rv = _running(C, 7 * M + C, stats.device)
    mean, rstd = K.bn_finalize(stats, M, EPS, MOMENTUM, rm, rv)
    return {"stats": _digest(K.stats_values(stats)), "finalize": _digest(mean, rstd, rm, rv)}


def group_bn_apply(M, C, tname):
    d = _bn_inputs(M, C, tname)
    out = {}
    for aname, act in (("none", K.CS_ACT_NONE), ("relu", K.CS_ACT_RELU), ("silu", K.CS_ACT_SILU)):
        for rname, res in (("plain", None), ("res", d("res"))):
            y = K.bn_apply(d("z"), *d("moments"), d("gamma"), d("beta"), residual=res, act=act)
            out["apply/%s/%s" % (aname, rname)] = _digest(y)
            rm, rv = _running(C, 7 * M + C, y.device)
            y, mean, rstd = K.bn_apply_stats(d("z"), K.bn_stats(d("z")), EPS, MOMENTUM, rm, rv, d("gamma"), d("beta"), residual=res, act=act)
            out["apply_stats/%s/%s" % (aname, rname)] = _digest(y, mean, rstd, rm, rv)
    return out


def group_bn_bwd(M, C, tname):
    d = _bn_inputs(M, C, tname)
    out = {}
    for aname, act in (("none", K.CS_ACT_NONE), ("silu", K.CS_ACT_SILU), ("own_relu", K.CS_BN_BWD_OWN_RELU), ("frozen", K.CS_BN_BWD_FROZEN)):
        dz, dgamma, dbeta = K.bn_bwd(d("dy"), d("z"), *d("moments"), d("gamma"), True, beta=d("beta"), act=act)
        out[aname] = _digest(dz, dgamma, dbeta)
    return out


def group_sample_sum(N, H, W, C, tname):
    dev, dtype = torch.device("cuda:0"), DTYPES[tname]
    seed = 11 * H + C
    a, b = _signed((N, H, W, C), seed, dtype, dev), _signed((N, H, W, C), seed + 1, dtype, dev)
    return {"a": _digest(K.sample_sum(a)), "ab": _digest(K.sample_sum(a, b))}


def _groups():
    g = []
    for M, C in BN_SHAPES + EXTRA_SHAPES:
        for tname in ("bf16", "f32"):
            f32_too = (M, C) in F32_BWD_APPLY_SHAPES
            g.append(("bn_fwd/%dx%d/%s" % (M, C, tname), group_bn_fwd, (M, C, tname)))
            if tname == "bf16" or f32_too:
                g.append(("bn_apply/%dx%d/%s" % (M, C, tname), group_bn_apply, (M, C, tname)))
                if M > 1:
                    g.append(("bn_bwd/%dx%d/%s" % (M, C, tname), group_bn_bwd, (M, C, tname)))
    for shape in SUM_SHAPES:
        for tname in ("bf16", "f32"):
            g.append(("sample_sum/%dx%dx%dx%d/%s" % (shape + (tname,)), group_sample_sum, shape + (tname,)))
    return g


GROUPS = _groups()


def _run(group):
    name, fn, args = group
    return {name + "/" + k: v for k, v in fn(*args).items()}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["digests"]


@pytest.mark.parametrize("group", GROUPS, ids=[g[0] for g in GROUPS])
def test_bits_match_recorded_digests(group, golden):
    got = _run(group)
    want = {k: v for k, v in golden.items() if k.startswith(group[0] + "/")}
    assert sorted(got) == sorted(want)                                   # every case of the group is recorded, none is extra
    assert got == want, "changed bits: " + ", ".join(k for k in got if got[k] != want[k])


def test_every_recorded_case_is_run(golden):
    names = tuple(g[0] + "/" for g in GROUPS)
    assert all(k.startswith(names) for k in golden)


def _record(argv):
    import subprocess
    out = argv[argv.index("--out") + 1] if "--out" in argv else GOLDEN
    commit = argv[argv.index("--commit") + 1] if "--commit" in argv else ""
    digests = {}
    for g in GROUPS:
        digests.update(_run(g))
    hipcc = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--version"], capture_output=True, text=True).stdout.splitlines()
    doc = {"recorded_from_commit": commit, "hipcc": next((ln for ln in hipcc if "HIP version" in ln), hipcc[0] if hipcc else ""),
           "device": torch.cuda.get_device_name(0), "digests": digests}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded %d digests -> %s" % (len(digests), out))


if __name__ == "__main__":
    if "--record" not in sys.argv:
        sys.exit("usage: test_row_passes_bits_gpu.py --record [--out FILE] [--commit HASH]")
    _record(sys.argv)
