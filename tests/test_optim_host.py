"""CPU: the host mechanism that cellsegmentation_amd.optim.Adam and SGD share -- the pure launch planner against results worked out
from its rule, the bound of the plan cache, what Adam.load_state_dict decides for CPU tensors -- and the C ABI of the one-launch
Adam (include/cellseg_hip.h against the ctypes table of _lib.py)."""
import copy
import ctypes
import os
import re

import pytest
import torch

from cellsegmentation_amd import _lib
from cellsegmentation_amd.optim import SGD, Adam, plan_launches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NUMELS, CHUNK = [5, 16384, 16385, 1], 16384


def test_plan_launches_sorts_by_class_and_splits_at_the_cap():
    order, launches = plan_launches(NUMELS, (1, 0, 1, 0), CHUNK, 2)
    assert order == [1, 3, 0, 2]
    assert launches == [(0, [1, 3], [(0, 0), (1, 0)], 0), (2, [0, 2], [(2, 0), (3, 0), (3, 1)], 1)]
    order, launches = plan_launches(NUMELS, (1, 0, 1, 0), CHUNK, 1)
    assert order == [1, 3, 0, 2]
    assert [(t0, pairs) for t0, _, pairs, _ in launches] == [(0, [(0, 0)]), (1, [(1, 0)]), (2, [(2, 0)]), (3, [(3, 0), (3, 1)])]
    assert [(members, cls) for _, members, _, cls in launches] == [([1], 0), ([3], 0), ([0], 1), ([2], 1)]
    order, launches = plan_launches(NUMELS, (0, 0, 0, 0), CHUNK, 320)
    assert order == [0, 1, 2, 3]
    assert launches == [(0, [0, 1, 2, 3], [(0, 0), (1, 0), (2, 0), (2, 1), (3, 0)], 0)]


@pytest.mark.parametrize("classes,cap", [((1, 0, 1, 0), 2), ((1, 0, 1, 0), 1), ((0, 0, 0, 0), 320), ((2, 1, 0, 1), 3), ((0, 0, 0, 0), 3)])
def test_plan_launches_covers_every_row_and_every_element_once(classes, cap):
    order, launches = plan_launches(NUMELS, classes, CHUNK, cap)
    assert sorted(order) == list(range(len(NUMELS))) and [classes[i] for i in order] == sorted(classes)
    rows, covered = [], {i: [] for i in range(len(NUMELS))}
    for t0, members, pairs, cls in launches:
        assert 1 <= len(members) <= cap and members == order[t0:t0 + len(members)] and all(classes[i] == cls for i in members)
        rows += range(t0, t0 + len(members))
        for row, c in pairs:
            assert t0 <= row < t0 + len(members)                 # the kernel indexes its gradient table with row - t0
            i = order[row]
            covered[i] += range(c * CHUNK, min((c + 1) * CHUNK, NUMELS[i]))
    assert rows == list(range(len(NUMELS)))
    for i, n in enumerate(NUMELS):
        assert covered[i] == list(range(n)), i


def _param():
    return torch.arange(6, dtype=torch.float32).reshape(2, 3).requires_grad_()


@pytest.mark.parametrize("make", [lambda ps: Adam(ps, lr=1e-3), lambda ps: SGD(ps, lr=1e-3, momentum=0.9)], ids=["adam", "sgd"])
def test_plan_cache_is_bounded_and_drops_the_oldest(make):
    for groups in (1, 2):
        opt = make([{"params": [_param()]} for _ in range(groups)])
        bound = opt._MAX_PLANS * groups
        assert bound == 8 * groups
        for k in range(3 * bound):
            assert opt._remember(("stub", k), k) == k
            assert len(opt._plans) == min(k + 1, bound)
        assert list(opt._plans) == [("stub", k) for k in range(2 * bound, 3 * bound)]


@pytest.mark.parametrize("capturable", [False, True])
def test_adam_state_loads_from_torch_and_keeps_its_capturable_flag(capturable):
    p, q = _param(), _param()
    ref = torch.optim.Adam([q], lr=0.1, weight_decay=1e-4)
    q.grad = torch.ones_like(q)
    ref.step()
    ref.step()
    sd = copy.deepcopy(ref.state_dict())
    assert sd["param_groups"][0]["capturable"] is False and not sd["state"][0]["step"].is_cuda
    a = Adam([p], lr=0.5, capturable=capturable)
    a._plans["stale"] = None
    a._hsteps[id(p)] = [0, 7.0]
    a.load_state_dict(sd)
    g = a.param_groups[0]
    assert g["capturable"] is capturable and g["lr"] == 0.1 and g["weight_decay"] == 1e-4
    assert not a._plans and not a._hsteps
    st = a.state[p]
    assert st.keys() == {"step", "exp_avg", "exp_avg_sq"} and torch.equal(st["exp_avg_sq"], ref.state[q]["exp_avg_sq"])
    # an fp32 scalar of its own (the launches advance it), where the flag says: with the parameter, or on the host
    assert st["step"].dtype == torch.float32 and st["step"].shape == () and float(st["step"]) == 2.0
    assert st["step"].device == (p.device if capturable else torch.device("cpu"))
    assert st["step"].data_ptr() != sd["state"][0]["step"].data_ptr()
    # ... and the other way: a checkpoint that says capturable does not change the flag of a host-side optimizer either
    sd2 = copy.deepcopy(ref.state_dict())
    sd2["param_groups"][0]["capturable"] = not capturable
    a.load_state_dict(sd2)
    assert a.param_groups[0]["capturable"] is capturable and float(a.state[p]["step"]) == 2.0
    # torch.optim.Adam takes a state_dict of this class
    ref2 = torch.optim.Adam([_param()], lr=1.0)
    ref2.load_state_dict(copy.deepcopy(a.state_dict()))
    assert ref2.param_groups[0]["lr"] == 0.1 and float(ref2.state_dict()["state"][0]["step"]) == 2.0


def test_every_adam_entry_point_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "cellseg_hip.h")).read()
    declared = sorted(set(re.findall(r"\b(cs_adam_step[a-z0-9_]*)\s*\(", header)))
    assert declared == ["cs_adam_step", "cs_adam_step_dev"]
    assert sorted(n for n in _lib._SIGNATURES if n.startswith("cs_adam_step")) == declared
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
    assert re.search(r"typedef struct CsAdamTensor \{ float\* p; float\* m; float\* v; long long n; \} CsAdamTensor;", header)
    # the planner's two constants come from the library, which also sizes the kernels' by-value gradient table with them
    assert (lib.cs_adam_chunk_elems(), lib.cs_adam_max_tensors()) == (16384, 320)


def test_adam_entry_points_check_their_arguments_before_launching():
    lib = _lib.load()
    # NULL tables: refused by CS_CHECK_ARG, nothing is enqueued
    assert lib.cs_adam_step(None, None, 0, 1, None, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, None) == -1
    assert b"adam_step" in lib.cs_last_error() and b"adam_step_dev" not in lib.cs_last_error()
    assert lib.cs_adam_step_dev(None, None, 0, 1, None, 1, None, None, None, 1e-3, 0.9, 0.999, 1e-8, 0.0, None) == -1
    assert b"adam_step_dev" in lib.cs_last_error()
    # a NULL among the gradient pointers: found while they are packed, which all four entry points do before their first launch.
    # (The tables are never read on the host: any non-NULL address stands in for them.)
    tab = ctypes.create_string_buffer(64)
    grads = (ctypes.c_void_p * 2)(ctypes.addressof(tab), None)
    head = (tab, grads, 0, 2, tab, 1)
    assert lib.cs_adam_step(*head, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, None) == -1
    assert lib.cs_last_error() == b"adam_step: NULL gradient"
    assert lib.cs_adam_step_dev(*head, tab, tab, None, 1e-3, 0.9, 0.999, 1e-8, 0.0, None) == -1
    assert lib.cs_last_error() == b"adam_step_dev: NULL gradient"
    assert lib.cs_sgd_step(*head, 0.1, 0.9, 0.0, 0.0, 0, 0, None) == -1
    assert lib.cs_last_error() == b"sgd_step: NULL gradient"
    assert lib.cs_sgd_step_dev(*head, tab, 0.0, 0.0, 0, 0, None) == -1
    assert lib.cs_last_error() == b"sgd_step_dev: NULL gradient"
    # ... and more tensors than the by-value gradient table holds are refused before it is written
    assert lib.cs_adam_step(tab, grads, 0, 321, tab, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, None) == -1
    assert lib.cs_last_error().startswith(b"adam_step: 1..320 tensors")
