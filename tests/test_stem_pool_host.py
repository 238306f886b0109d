"""CPU: the fused stem + max-pool entry points (csrc/stem_pool.hip) are declared, bound and exported; the host query refuses what the
kernel does not serve; the launcher refuses NULL operands with a message before anything is launched."""
import ctypes
import os
import re

from cellsegmentation_amd import _lib, engine, kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cs_stem_pool_fwd", "cs_stem_pool_fwd_supported")


def test_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "cellseg_hip.h")).read()
    lib = _lib.load()
    for name in NAMES:
        assert re.search(rf"\bint {name}\s*\(", header), name
        assert name in _lib._SIGNATURES and name in _lib.exported_symbols()
        assert hasattr(lib, name)
    assert "stem_pool.hip" in open(os.path.join(ROOT, "cellsegmentation_amd", "csrc", "Makefile")).read()
    assert callable(kernels.stem_pool_fwd) and callable(kernels.stem_pool_fwd_supported)
    assert engine.FUSE_STEM_POOL is True


def test_supported_query():
    ok = _lib.load().cs_stem_pool_fwd_supported
    assert ok(64, 299, 299, 64) == 1                 # the classifier's bag of tiles
    assert ok(40960, 32, 32, 64) == 1                # 64-bit image bases: many small images are served
    assert ok(1, 7, 7, 64) == 1
    assert ok(1, 299, 299, 128) == 0 and ok(1, 299, 299, 32) == 0      # K != 64
    assert ok(1, 6, 299, 64) == 0 and ok(1, 299, 6, 64) == 0           # H, W < 7
    assert ok(0, 299, 299, 64) == 0
    assert ok(1, 65536, 65536, 64) == 0              # offsets inside one image are 32-bit: 2^35 bytes of pairs
    assert ok(1, 8192, 16384, 64) == 1 and ok(1, 16384, 16384, 64) == 0    # 2^30 / 2^31 bytes of pairs
    assert ok(1 << 30, 299, 299, 64) == 0            # the workgroup count


def test_null_operands_are_refused_without_a_launch():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    ptr = ctypes.c_void_p(ctypes.addressof(buf))
    for args in ((None, ptr, ptr), (ptr, None, ptr), (ptr, ptr, None)):
        x, w, y = args
        assert lib.cs_stem_pool_fwd(1, 32, 32, 64, x, w, None, y, None, None) == -1
        assert lib.cs_last_error() == b"stem_pool_fwd: x_pair, w_pair and y_pool must not be NULL"
    assert lib.cs_stem_pool_fwd(1, 32, 32, 32, ptr, ptr, None, ptr, None, None) == -1 and b"64 output channels" in lib.cs_last_error()
    assert lib.cs_stem_pool_fwd(1, 6, 32, 64, ptr, ptr, None, ptr, None, None) == -1 and b"out of range" in lib.cs_last_error()
