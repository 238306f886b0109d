"""Device arrays at chosen addresses, for the GPU tests of the kernels that ask no alignment of their tensors (csrc/cs_pixels.h)."""
import numpy as np
import torch

GUARD = 0xA5


def shifted(a, shift, dev, fill=None):
    """the array on the device, its first byte `shift` bytes (a multiple of the item size) past a 16-byte boundary, inside a buffer
    of GUARD bytes -> (the view, the buffer, the view's byte range in it); fill: a constant instead of the array's values"""
    assert shift % a.dtype.itemsize == 0
    flat = torch.full((a.nbytes + 64,), GUARD, dtype=torch.uint8, device=dev)
    lead = (-flat.data_ptr()) % 16 + 16 + shift
    view = flat[lead:lead + a.nbytes].view(torch.from_numpy(a[:0].copy()).dtype).view(a.shape)
    if fill is None:
        view.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    else:
        view.fill_(fill)
    assert view.data_ptr() % 16 == shift % 16 and view.is_contiguous()
    return view, flat, (lead, lead + a.nbytes)


def guards_intact(flat, span):
    """nothing was written around the view: the buffer outside the byte range is still GUARD"""
    f = flat.cpu().numpy()
    return bool((f[:span[0]] == GUARD).all() and (f[span[1]:] == GUARD).all())
