"""``Adam`` and ``SGD``: torch.optim's updates as ONE HIP launch per <= 320 tensors (csrc/optim.hip), on one host mechanism.

The reference's drivers construct ``optim.Adam(filter(requires_grad, model.parameters()), lr, weight_decay)`` (train_tile.py:282,
train_image.py:476, train_seg.py:309) or, whenever a scheduler is given, ``optim.SGD(lr, momentum=0.9, weight_decay=1e-4)``
(train_tile.py:280-303, train_seg.py:289-312, train_image.py:483-508).  Both classes keep torch's constructor, ``step`` / ``zero_grad`` /
``state_dict`` / ``load_state_dict``, ``param_groups`` (schedulers change ``lr`` / ``momentum`` there) and torch's state (``step``,
``exp_avg``, ``exp_avg_sq``; ``momentum_buffer``, none when momentum is 0), so a checkpoint written with torch's class loads into
ours and back; only the arithmetic runs in our kernels (Adam: one launch instead of torch's five, 2.9 TB/s on the ResNet-50 tile
step).  fp32 CUDA parameters only, no amsgrad / maximize.  Parameters without a gradient are skipped, like in torch.

The mechanism (``plan_launches``, ``_OneLaunch``), written once: the parameters that have a gradient get a CLASS each (whatever must
be a launch argument: Adam's step count, SGD's "this step creates the buffer"); a device table of tensor rows sorted by class, one
launch per (class, <= 320 rows) with a device table of 16 Ki-element chunks, the gradients' addresses by value.  A ``Plan`` holds
those tables AND the tensors whose addresses they contain; plans are cached per (group, parameter addresses, classes), a few per
group, and are never built while the stream is capturing (the tables are copied from the host): one eager step comes first.

``capturable=True`` (torch's flag, same state layout): what changes from step to step is read from device memory, so ``step()`` may
be captured into a HIP graph (graphed.GraphedStep) and every replay is the next step.  Adam (cs_adam_step_dev): ``step`` is an fp32
scalar ON THE DEVICE, a one-thread-per-tensor launch advances it and forms the bias corrections in double, so parameters at
different step counts share a launch; ``lr`` comes from a device double.  SGD (cs_sgd_step_dev): ``lr`` AND ``momentum`` come from a
device ``double[2]``, so a captured step follows ``OneCycleLR`` (which moves both at every iteration); ``torch.optim.SGD`` replays the
values of the capture for ever.  ``sync_hyper()`` (cheap; pass it as a ``pre_replay`` hook of GraphedStep) keeps those doubles equal
to ``param_groups``; every other hyper-parameter is a launch argument, fixed at capture.
"""
import collections
import ctypes

import torch

from . import _capture, _lib

# table: the device rows; launches: (first row, members as indices into the parameter list, device chunk table, number of chunks,
# class); extra: what else the class's launches read (Adam capturable: step pointers, coefficient scratch); keep: every tensor whose
# address the tables hold -- whoever holds the plan (the cache, a captured graph through _capture.keep) holds that memory
Plan = collections.namedtuple("Plan", "table launches extra keep")


def plan_launches(numels, classes, chunk, cap):
    """(order, launches): `order` is the tensor indices stably sorted by class (members of a class stay in parameter order) = the
    rows of the device table; consecutive rows go into one launch while they have the same class and the launch has fewer than
    `cap` rows.  A launch is (first row t0, members, [(row, chunk index)] over ceil(numel / chunk) chunks per member, class)."""
    order = sorted(range(len(numels)), key=lambda i: classes[i])
    launches, t0 = [], 0
    while t0 < len(order):
        t1 = t0
        while t1 < len(order) and t1 - t0 < cap and classes[order[t1]] == classes[order[t0]]:
            t1 += 1
        members = order[t0:t1]
        pairs = [(t0 + j, c) for j, i in enumerate(members) for c in range((numels[i] + chunk - 1) // chunk)]
        launches.append((t0, members, pairs, classes[order[t0]]))
        t0 = t1
    return order, launches


class _OneLaunch(torch.optim.Optimizer):
    """The host mechanism of both classes (module docstring).  A class gives `_HYPER`, `_EAGER_WHY`, `_rows` and `_step_group`."""
    _MAX_PLANS = 8
    _HYPER = ()             # the group entries a capturable group's launches read from device doubles, in the kernel's order
    _EAGER_WHY = ""         # why the non-capturable form cannot be captured

    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        self._name = "cellsegmentation_amd.optim." + type(self).__name__
        self._plans = {}            # (group index, tensor addresses, classes) -> Plan; a few entries (alternating parameter sets)
        self._hyper_dev = {}        # group index -> [device double[len(_HYPER)], the host values it holds or None]  (capturable groups)

    def _check_hyper(self, gi, want):
        """Refuse a change of the mirrored values that the launches cannot follow."""

    def sync_hyper(self):
        """Copy every capturable group's current `_HYPER` values into the device doubles its (possibly captured) launches read.  One
        tiny fill per CHANGED value: call before replaying a captured step whenever a scheduler moved them
        (GraphedStep(pre_replay=...))."""
        for gi, group in enumerate(self.param_groups):
            if not group.get("capturable", False):
                continue
            want = tuple([float(group[k]) for k in self._HYPER])
            slot = self._hyper_dev.get(gi)
            if slot is None:
                p0 = next((p for p in group["params"]), None)
                if p0 is None:
                    continue
                slot = self._hyper_dev[gi] = [torch.empty(len(want), dtype=torch.float64, device=p0.device), None]
            if slot[1] == want:
                continue
            self._check_hyper(gi, want)
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"{self._name}: {' or '.join(self._HYPER)} changed since the last sync_hyper(); call opt.sync_hyper() "
                                   "before capturing (a fill captured into the graph would reset the value at every replay)")
            for k, v in enumerate(want):
                if slot[1] is None or slot[1][k] != v:
                    slot[0][k].fill_(v)
            slot[1] = want

    def load_state_dict(self, state_dict):
        """torch's loader takes every hyper-parameter -- `capturable` included -- from the LOADED groups.  Where the values a launch
        reads live is a property of this optimizer object, not of the checkpoint: each group keeps the flag it was constructed with,
        so a checkpoint written by torch's class or by either form resumes in both."""
        want = [bool(g.get("capturable", False)) for g in self.param_groups]
        super().load_state_dict(state_dict)
        for g, capt in zip(self.param_groups, want):
            g["capturable"] = capt
        self._plans.clear()
        for slot in self._hyper_dev.values():
            slot[1] = None

    def _plan(self, gi, plist, classes, capturing):
        """The cached Plan of one set of parameters (`classes`: one per parameter, or None for a single class).  A parameter's
        storage can be replaced from outside (module.to(device) after the optimizer was built), so its address is part of the key;
        the state tensors are this class's own, and whatever replaces them (`_init_state`, load_state_dict) drops the plans."""
        key = (gi, tuple([p.data_ptr() for p in plist]), classes)
        plan = self._plans.get(key)
        if plan is None:
            if capturing:
                # (building the tables copies from the host, which a capture forbids)
                raise RuntimeError(f"{self._name}: run one eager step with this set of parameters before capturing (its device tables "
                                   "are built on the first step; GraphedStep's warm-up does)")
            for p in plist:
                if p.dtype != torch.float32 or not p.is_cuda or not p.is_contiguous() or p.is_sparse:
                    raise RuntimeError(f"{self._name}: contiguous fp32 CUDA parameters with dense fp32 gradients only")
            lib, dev = _lib.load(), plist[0].device
            order, launches = plan_launches([p.numel() for p in plist], classes or (0,) * len(plist), lib.cs_adam_chunk_elems(),
                                            lib.cs_adam_max_tensors())
            rows, extra, keep = self._rows(plist, classes, order)
            table = torch.tensor([rows[i] for i in order], dtype=torch.int64).to(dev)
            launches = [(t0, members, torch.tensor(pairs, dtype=torch.int32).to(dev), len(pairs), cls) for t0, members, pairs, cls in launches]
            plan = self._remember(key, Plan(table, launches, extra, list(plist) + keep))
        elif capturing:
            _capture.keep(plan)             # the plan cache is bounded: a captured launch keeps its tables alive itself
        return plan

    def _remember(self, key, plan):
        while len(self._plans) >= self._MAX_PLANS * max(1, len(self.param_groups)):
            self._plans.pop(next(iter(self._plans)))
        self._plans[key] = plan
        return plan

    @staticmethod
    def _grad_ptrs(plist, members):
        """(the gradients, alive until the launch is queued; the HOST array of their addresses)"""
        gts = [plist[i].grad for i in members]
        gts = [g if g.is_contiguous() else g.contiguous() for g in gts]
        return gts, (ctypes.c_void_p * len(gts))(*[g.data_ptr() for g in gts])

    @torch.no_grad()
    def step(self, closure=None):
        capturing = _capture.capturing()
        if capturing and not all(g.get("capturable", False) for g in self.param_groups):
            # a launch ARGUMENT captured into a graph is replayed for ever
            raise RuntimeError(f"{self._name}.step() cannot be captured into a HIP graph ({self._EAGER_WHY}); construct it with "
                               "capturable=True")
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.load()
        for gi, group in enumerate(self.param_groups):
            plist = [p for p in group["params"] if p.grad is not None]
            if not plist:
                continue
            for p in plist:
                g = p.grad
                if g.dtype != torch.float32 or g.is_sparse:
                    raise RuntimeError(f"{self._name}: contiguous fp32 CUDA parameters with dense fp32 gradients only")
            hyper = None
            if group.get("capturable", False):
                self.sync_hyper()              # (before any state is created: it may refuse the new values)
                hyper = self._hyper_dev[gi][0]
                if capturing:
                    _capture.keep(hyper)
            self._step_group(lib, gi, group, plist, hyper, capturing, torch.cuda.current_stream(plist[0].device).cuda_stream)
        return loss


class Adam(_OneLaunch):
    _HYPER = ("lr",)
    _EAGER_WHY = "the step count lives on the host"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, capturable=False):
        if amsgrad:
            raise ValueError("cellsegmentation_amd.optim.Adam: amsgrad is not implemented (the reference never enables it)")
        if lr < 0 or eps < 0 or weight_decay < 0 or not (0 <= betas[0] < 1 and 0 <= betas[1] < 1):
            raise ValueError("invalid Adam hyper-parameters")
        # (`capturable` in the defaults, as in torch: Optimizer.load_state_dict then keeps `step` on the parameter's device as fp32)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, capturable=bool(capturable)))
        self._hsteps = {}           # id(param) -> [address of its `step` tensor, host copy of the value]

    def _init_state(self, p, capturable=False):
        st = self.state[p]
        st["step"] = torch.zeros((), dtype=torch.float32, device=p.device) if capturable else torch.tensor(0.0)
        st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        # new moments / step tensors (first step, or the state was reset from outside: `opt.state.clear()`): no cached device table
        # or host step count may be used with them
        self._hsteps.pop(id(p), None)
        self._plans.clear()

    def _host_step(self, p):
        """Host copy of the parameter's step count: this class is the only writer of `step` (one foreach add per launch), so the
        tensor is read back only when it was replaced (load_state_dict) or never seen."""
        st = self.state[p]["step"]
        h = self._hsteps.get(id(p))
        if h is None or h[0] != st.data_ptr():
            h = self._hsteps[id(p)] = [st.data_ptr(), float(st)]
        return h

    def load_state_dict(self, state_dict):
        """(see _OneLaunch.)  The loaded step counts move to the device (fp32 scalars) or to the host, as each group's flag says."""
        super().load_state_dict(state_dict)
        for g in self.param_groups:
            for p in g["params"]:
                st = self.state.get(p)
                if st and "step" in st:
                    step = torch.as_tensor(st["step"], dtype=torch.float32)
                    st["step"] = step.to(p.device).reshape(()).clone() if g["capturable"] else step.cpu().reshape(()).clone()
        self._hsteps.clear()

    def _rows(self, plist, classes, order):
        """CsAdamTensor rows (p, m, v, n).  Capturable (`classes` None: the step counts are read on the device, one launch serves
        any mixture): also one `float*` per table row (the parameter's device step count) + 2 floats of coefficient scratch per row."""
        sts = [self.state[p] for p in plist]
        rows = [[p.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel()] for p, st in zip(plist, sts)]
        keep = [st[k] for st in sts for k in ("exp_avg", "exp_avg_sq")]
        if classes is not None:
            return rows, None, keep
        for st in sts:
            if not st["step"].is_cuda or st["step"].dtype != torch.float32 or st["step"].numel() != 1:
                raise RuntimeError("cellsegmentation_amd.optim.Adam(capturable=True): `step` must be an fp32 scalar on the GPU "
                                   "(state loaded from a non-capturable optimizer? load it through load_state_dict)")
        dev = plist[0].device
        steps = torch.tensor([sts[i]["step"].data_ptr() for i in order], dtype=torch.int64).to(dev)
        return rows, (steps, torch.empty((len(order), 2), dtype=torch.float32, device=dev)), keep + [st["step"] for st in sts]

    def _step_group(self, lib, gi, group, plist, lr_dev, capturing, stream):
        state = self.state
        for p in plist:
            if p not in state or len(state[p]) == 0:
                if capturing:
                    raise RuntimeError("cellsegmentation_amd.optim.Adam: run one eager step before capturing (the optimizer state is "
                                       "created on the first step; GraphedStep's warm-up does)")
                self._init_state(p, lr_dev is not None)
        scalars = (float(group["betas"][0]), float(group["betas"][1]), float(group["eps"]), float(group["weight_decay"]))
        if lr_dev is not None:
            plan = self._plan(gi, plist, None, capturing)
            steps, coef = plan.extra
            for t0, members, chunks, n_chunks, _ in plan.launches:
                gts, grads = self._grad_ptrs(plist, members)
                _lib.check(lib.cs_adam_step_dev(plan.table.data_ptr(), grads, t0, len(members), chunks.data_ptr(), n_chunks, steps.data_ptr(),
                                                coef.data_ptr(), lr_dev.data_ptr(), float(group["lr"]), *scalars, stream), "adam_step_dev")
            return
        # the bias corrections are per-launch arguments, so parameters at different step counts (one optimizer over parameter sets that
        # skip steps; the reference's train_alternative, train/train.py:240-268, alternates two sets) go to different launches, as
        # torch.optim.Adam's per-parameter step allows: the class of a parameter numbers its step count in order of first appearance
        hs = [self._host_step(p) for p in plist]
        seen = {}
        plan = self._plan(gi, plist, tuple(seen.setdefault(h[1], len(seen)) for h in hs), capturing)
        for t0, members, chunks, n_chunks, _ in plan.launches:
            t = hs[members[0]][1] + 1.0
            gts, grads = self._grad_ptrs(plist, members)
            _lib.check(lib.cs_adam_step(plan.table.data_ptr(), grads, t0, len(members), chunks.data_ptr(), n_chunks, float(group["lr"]), *scalars,
                                        t, stream), "adam_step")
            for i in members:
                hs[i][1] = t
            torch._foreach_add_([state[plist[i]]["step"] for i in members], 1.0)


class SGD(_OneLaunch):
    _PLAIN, _FIRST, _LATER = 0, 1, 2          # class of a tensor in one step: no buffer used / buffer created by this step / has history
    _HYPER = ("lr", "momentum")
    _EAGER_WHY = "lr and momentum are launch arguments"

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, capturable=False, *, maximize=False, foreach=None,
                 fused=None):
        if maximize or foreach or fused:
            raise ValueError("cellsegmentation_amd.optim.SGD: maximize / foreach / fused are not implemented (the reference never enables "
                             "them; the update is one launch as it is)")
        if lr < 0 or momentum < 0 or weight_decay < 0:
            raise ValueError("invalid SGD hyper-parameters: lr, momentum and weight_decay must not be negative")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        # (`momentum` in the defaults is what OneCycleLR(cycle_momentum=True) / CyclicLR look for)
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=bool(nesterov),
                                      maximize=False, capturable=bool(capturable)))
        self._uses_buf = {}         # group index -> momentum != 0 at the first step  (capturable groups)

    def _init_state(self, p):
        """The buffer of a parameter's first momentum step: the launch WRITES it (buf = g'), so it starts uninitialised."""
        self.state[p]["momentum_buffer"] = torch.empty_like(p, memory_format=torch.contiguous_format)
        self._plans.clear()         # a new buffer: no cached device table may be used with it

    def _check_hyper(self, gi, want):
        if self._uses_buf.get(gi) is not None and (want[1] != 0) != self._uses_buf[gi]:
            raise ValueError("cellsegmentation_amd.optim.SGD(capturable=True): momentum may not change between 0 and non-zero after "
                             "the first step (whether the launches use momentum buffers is fixed)")

    def load_state_dict(self, state_dict):
        """(see _OneLaunch.)  A checkpoint written with maximize=True asks for another update: refused, not ignored."""
        super().load_state_dict(state_dict)
        self._uses_buf.clear()
        if any(g.get("maximize", False) for g in self.param_groups):
            raise ValueError("cellsegmentation_amd.optim.SGD: maximize is not implemented (the reference never enables it)")

    def _rows(self, plist, classes, order):
        """CsSgdTensor rows (p, buf, n); buf is NULL in the _PLAIN class."""
        rows, keep = [], []
        for p, c in zip(plist, classes):
            buf = 0
            if c != self._PLAIN:
                b = self.state[p]["momentum_buffer"]
                if b.dtype != torch.float32 or b.device != p.device or not b.is_contiguous() or b.numel() != p.numel():
                    raise RuntimeError("cellsegmentation_amd.optim.SGD: `momentum_buffer` must be a contiguous fp32 tensor of the "
                                       "parameter's size on its device (load foreign state through load_state_dict)")
                buf = b.data_ptr()
                keep.append(b)
            rows.append([p.data_ptr(), buf, p.numel()])
        return rows, None, keep

    def _step_group(self, lib, gi, group, plist, hyper, capturing, stream):
        lr, momentum, dampening = float(group["lr"]), float(group["momentum"]), float(group["dampening"])
        if momentum == 0:
            classes = (self._PLAIN,) * len(plist)          # as in torch: no buffer is created, read or written
        else:
            # the `first` flag is a launch argument, so the tensors whose buffer this step creates and those with history (one
            # optimizer over parameter sets that start at different steps: train_alternative) go to different launches
            state, classes = self.state, []
            for p in plist:
                if (state[p].get("momentum_buffer") if p in state else None) is not None:
                    classes.append(self._LATER)
                    continue
                if capturing:
                    raise RuntimeError("cellsegmentation_amd.optim.SGD: run one eager step before capturing (the momentum buffers "
                                       "are created on the first step; GraphedStep's warm-up does)")
                self._init_state(p)
                classes.append(self._FIRST)
            classes = tuple(classes)
        if hyper is not None and self._uses_buf.get(gi) is None:
            self._uses_buf[gi] = momentum != 0
        plan = self._plan(gi, plist, classes, capturing)
        tail = (dampening, float(group["weight_decay"]), int(bool(group["nesterov"])))
        for t0, members, chunks, n_chunks, cls in plan.launches:
            gts, grads = self._grad_ptrs(plist, members)
            head = (plan.table.data_ptr(), grads, t0, len(members), chunks.data_ptr(), n_chunks)
            if hyper is not None:
                _lib.check(lib.cs_sgd_step_dev(*head, hyper.data_ptr(), *tail, int(cls == self._FIRST), stream), "sgd_step_dev")
            else:
                _lib.check(lib.cs_sgd_step(*head, lr, momentum, *tail, int(cls == self._FIRST), stream), "sgd_step")
        if self._FIRST in classes:
            # the next step of this set finds every buffer in place: build its tables now, so that a capture may follow one
            # eager step (a cache miss inside a capture cannot be served)
            self._plan(gi, plist, (self._LATER,) * len(plist), False)
