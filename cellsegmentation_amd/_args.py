"""Image arguments of the post-processing API (regions.py, detect.py, inference.py): numpy or torch in, a checked torch tensor out."""
import numpy as np
import torch

MAX_PIXELS = (1 << 31) - 1            # per image, and per kernel call
_SHAPES = {2: "[H, W]", 3: "[N, H, W]"}


def _device(*xs):
    """the device of the first device tensor among xs, else the current one"""
    for x in xs:
        if torch.is_tensor(x) and x.is_cuda:
            return x.device
    return torch.device("cuda", torch.cuda.current_device())


def _tensor(x):
    return torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x


def _images(x, what, dtype, wrong_dtype, ranks=(2, 3), noun=None, subject="expected", lift=False, to_device=False):
    """numpy / torch image(s) -> the checked torch tensor; argument errors before any device work.

    ``wrong_dtype``: the rest of the message for another dtype, ``{}`` = the dtype given (it carries the caller's hint).  ``ranks``:
    the dimensions allowed, None = not checked here.  ``noun``: what an image is called; with it an empty image and one of 2^31
    pixels or more are refused.  ``lift``: [H, W] -> [1, H, W].  ``to_device``: a host tensor is moved to the current device."""
    t = _tensor(x)
    if not torch.is_tensor(t):
        raise TypeError(f"{what}: {subject} a numpy array or a torch tensor")
    if t.dtype != dtype:
        raise TypeError(f"{what}: {subject} {wrong_dtype.format(t.dtype)}")
    if ranks is not None and t.dim() not in ranks:
        raise ValueError(f"{what}: expected {' or '.join(_SHAPES[r] for r in ranks)}, got shape {tuple(t.shape)}")
    if noun is not None:
        if t.numel() == 0:
            raise ValueError(f"{what}: empty {noun} of shape {tuple(t.shape)}")
        if t.shape[-1] * t.shape[-2] > MAX_PIXELS:
            raise ValueError(f"{what}: one image of {t.shape[-2]}x{t.shape[-1]} has 2^31 pixels or more")
    if lift and t.dim() == 2:
        t = t.unsqueeze(0)
    if to_device and not t.is_cuda:
        t = t.to(_device())
    return t
