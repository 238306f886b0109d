"""CPU: the C ABI of the one-launch SGD (include/cellseg_hip.h against the ctypes table of _lib.py) and what
cellsegmentation_amd.optim.SGD decides on the host before any device work: constructor validation, the defaults schedulers look
for, state interchange with torch.optim.SGD through load_state_dict."""
import copy
import os
import re

import pytest
import torch

from cellsegmentation_amd import _lib
from cellsegmentation_amd.optim import SGD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_sgd_entry_point_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "cellseg_hip.h")).read()
    declared = sorted(set(re.findall(r"\b(cs_sgd_[a-z0-9_]+)\s*\(", header)))
    assert declared == ["cs_sgd_step", "cs_sgd_step_dev"]
    assert sorted(n for n in _lib._SIGNATURES if n.startswith("cs_sgd_")) == declared
    lib = _lib.load()
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/cellseg_hip.h but not exported"
        # one ctypes argument per declared parameter, doubles where the header says double
        params = re.search(rf"\bint {name}\s*\((.*?)\);", header, flags=re.S).group(1).split(",")
        restype, argtypes = _lib._SIGNATURES[name]
        assert restype is _lib.c_int and len(argtypes) == len(params), name
        for decl, ct in zip(params, argtypes):
            want = _lib.c_double if decl.strip().startswith("double ") else _lib.c_int if decl.strip().startswith("int ") else _lib._P
            assert ct is want, (name, decl.strip())
    assert re.search(r"typedef struct CsSgdTensor \{ float\* p; float\* buf; long long n; \} CsSgdTensor;", header)


def test_sgd_entry_points_check_their_arguments_before_launching():
    lib = _lib.load()
    # NULL tables: refused by CS_CHECK_ARG, nothing is enqueued
    assert lib.cs_sgd_step(None, None, 0, 1, None, 1, 0.1, 0.9, 0.0, 0.0, 0, 0, None) == -1
    assert b"sgd_step" in lib.cs_last_error()
    assert lib.cs_sgd_step_dev(None, None, 0, 1, None, 1, None, 0.0, 0.0, 0, 0, None) == -1
    assert b"sgd_step_dev" in lib.cs_last_error()


def _param():
    return torch.arange(6, dtype=torch.float32).reshape(2, 3).requires_grad_()


def test_sgd_constructor_validates_like_torch():
    for bad in (dict(lr=-1e-3), dict(momentum=-0.1), dict(weight_decay=-1e-4), dict(nesterov=True), dict(nesterov=True, momentum=0.9, dampening=0.1),
                dict(maximize=True), dict(foreach=True), dict(fused=True)):
        with pytest.raises(ValueError):
            SGD([_param()], **bad)
        if not ({"maximize", "foreach", "fused"} & set(bad)):        # (what torch implements and this class does not)
            with pytest.raises(ValueError):
                torch.optim.SGD([_param()], **{"lr": 1e-3, **bad})
    opt = SGD([_param()], lr=0.1, momentum=0.9, weight_decay=1e-4, nesterov=True)
    g = opt.param_groups[0]
    assert (g["lr"], g["momentum"], g["dampening"], g["weight_decay"], g["nesterov"], g["capturable"]) == (0.1, 0.9, 0, 1e-4, True, False)
    assert len(opt.state) == 0
    assert SGD([_param()]).defaults["momentum"] == 0 and SGD([_param()]).defaults["lr"] == 1e-3


@pytest.mark.parametrize("capturable", [False, True])
def test_schedulers_that_cycle_momentum_accept_the_class(capturable):
    opt = SGD([_param()], lr=0.1, momentum=0.9, capturable=capturable)
    assert "momentum" in opt.defaults
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=0.1, total_steps=8)          # cycle_momentum=True is the default
    assert opt.param_groups[0]["momentum"] == pytest.approx(0.95) and opt.param_groups[0]["lr"] == pytest.approx(0.1 / 25)
    assert sched.get_last_lr()[0] == opt.param_groups[0]["lr"]
    torch.optim.lr_scheduler.CyclicLR(SGD([_param()], lr=0.1, momentum=0.9), base_lr=0.01, max_lr=0.1)


def test_sgd_state_loads_from_torch_and_keeps_its_capturable_flag():
    p, q = _param(), _param()
    ref = torch.optim.SGD([q], lr=0.1, momentum=0.9, weight_decay=1e-4)
    q.grad = torch.ones_like(q)
    ref.step()
    a = SGD([p], lr=0.5, momentum=0.5, capturable=True)
    a._plans["stale"] = None
    a.load_state_dict(copy.deepcopy(ref.state_dict()))
    g = a.param_groups[0]
    assert g["capturable"] is True and g["lr"] == 0.1 and g["momentum"] == 0.9 and g["weight_decay"] == 1e-4
    assert a.state[p].keys() == {"momentum_buffer"} and torch.equal(a.state[p]["momentum_buffer"], ref.state[q]["momentum_buffer"])
    assert not a._plans
    # ... and back: torch.optim.SGD takes a state_dict of this class
    ref2 = torch.optim.SGD([_param()], lr=1.0)
    ref2.load_state_dict(copy.deepcopy(a.state_dict()))
    assert ref2.param_groups[0]["momentum"] == 0.9 and list(ref2.state_dict()["state"][0]) == ["momentum_buffer"]
    # a checkpoint written with maximize=True asks for another update: refused, not ignored
    mx = torch.optim.SGD([_param()], lr=0.1, maximize=True)
    with pytest.raises(ValueError):
        SGD([_param()], lr=0.1).load_state_dict(mx.state_dict())
