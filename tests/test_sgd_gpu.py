"""cellsegmentation_amd.optim.SGD (one HIP launch, csrc/optim.hip: cs_sgd_step / cs_sgd_step_dev) against torch.optim.SGD on the same
parameters and gradients: the optimizer the reference's drivers train with whenever a scheduler is given (train_tile.py:280-303:
momentum 0.9, weight_decay 1e-4), eagerly, with lr AND momentum moved by OneCycleLR between replays of a captured step, and as part of
one whole training step under graphed.GraphedStep."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

from cellsegmentation_amd import functional as HF  # noqa: E402
from cellsegmentation_amd import optim as O  # noqa: E402
from cellsegmentation_amd import synth  # noqa: E402
from cellsegmentation_amd.graphed import GraphedStep  # noqa: E402
from cellsegmentation_amd.model import resnet as R  # noqa: E402

# small tensors, the 16 Ki-element chunk boundary, several chunks with a ragged tail, > 320 tensors (two launches); _params adds a
# 4-byte-aligned view (the scalar path of the kernel)
SHAPES = [(64, 3, 7, 7), (64,), (2, 2048), (2,), (1,), (3,), (17,), (16383,), (16384,), (16385,), (100003,)] + [(33, 5)] * 330


def _draw(shape, gen, integer):
    return torch.randint(-8, 9, shape, generator=gen).float() if integer else torch.randn(shape, generator=gen)


def _params(dev, shapes, seed, integer=False, view=False):
    g = torch.Generator().manual_seed(seed)
    ps = [_draw(s, g, integer).to(dev).requires_grad_() for s in shapes]
    if view:
        base = _draw((5000,), g, integer).to(dev)
        ps.insert(3, base[1:4098].detach().requires_grad_())
        assert ps[3].data_ptr() % 16 == 4
    return ps


def _feed(gen, dev, integer, *param_lists):
    """One fresh gradient per parameter, a private copy of it for every optimizer."""
    for ps in zip(*param_lists):
        gr = _draw(ps[0].shape, gen, integer).to(dev)
        for p in ps:
            p.grad = gr.clone()


def _close(p, q):
    """The project's bound for a one-launch optimizer against torch's (tests/test_optim_gpu.py)."""
    p, q = p.detach(), q.detach()
    return float((p - q).abs().max()) <= 2e-6 * max(1.0, float(q.abs().max()))


def _buf_close(a, b):
    return float((a - b).abs().max()) <= 1e-6 * float(b.abs().max())


@pytest.mark.parametrize("capturable", [False, True])
@pytest.mark.parametrize("dampening,nesterov", [(0, False), (0.5, False), (0, True)])
def test_sgd_is_exact_on_small_integers(dampening, nesterov, capturable, dev):
    """Integer parameters and gradients in [-8, 8], lr / momentum / weight_decay / dampening powers of two: every intermediate is a
    small dyadic rational (|p| stays below 14), so fp32 is exact with or without FMA contraction and torch.optim.SGD must be met bit
    for bit -- any error in the chunk table, the tail, the gradient pointer table, the first-step flag or the launch split shows."""
    ours, ref = _params(dev, SHAPES, 1, True, True), _params(dev, SHAPES, 1, True, True)
    kw = dict(lr=0.25, momentum=0.5, weight_decay=0.5, dampening=dampening, nesterov=nesterov)
    a = O.SGD(ours, capturable=capturable, **kw)
    b = torch.optim.SGD(ref, **kw)
    g = torch.Generator().manual_seed(7)
    for step in range(4):
        _feed(g, dev, True, ours, ref)
        if step == 2:
            for o in (a, b):
                o.param_groups[0]["lr"], o.param_groups[0]["momentum"] = 0.5, 0.25
        a.step()
        b.step()
    torch.cuda.synchronize()
    for i, (p, q) in enumerate(zip(ours, ref)):
        assert torch.equal(p, q), (i, tuple(p.shape))
        assert torch.equal(a.state[p]["momentum_buffer"], b.state[q]["momentum_buffer"]), (i, tuple(p.shape))


@pytest.mark.parametrize("capturable", [False, True])
@pytest.mark.parametrize("momentum,dampening,nesterov,wd", [(0, 0, False, 0), (0.9, 0, False, 1e-4), (0.9, 0, True, 1e-4), (0.9, 0.1, False, 0)])
def test_sgd_matches_torch_over_several_steps(momentum, dampening, nesterov, wd, capturable, dev):
    """Real values; lr and (where there is one) momentum change at step 3, as a scheduler does; then the state goes to torch and back.
    With momentum 0 the momentum stays 0: torch creates no state then, and neither does this class."""
    ours, ref = _params(dev, SHAPES, 1, view=True), _params(dev, SHAPES, 1, view=True)
    kw = dict(lr=5e-4, momentum=momentum, dampening=dampening, nesterov=nesterov, weight_decay=wd)
    a = O.SGD(ours, capturable=capturable, **kw)
    b = torch.optim.SGD(ref, **kw)
    g = torch.Generator().manual_seed(7)
    for step in range(5):
        _feed(g, dev, False, ours, ref)
        if step == 3:
            for o in (a, b):
                o.param_groups[0]["lr"] = 1e-3
                if momentum:
                    o.param_groups[0]["momentum"] = 0.85
        a.step()
        b.step()
    torch.cuda.synchronize()
    for i, (p, q) in enumerate(zip(ours, ref)):
        assert _close(p, q), (i, tuple(p.shape), float((p - q).abs().max()))
    sa, sb = a.state_dict(), b.state_dict()
    assert sa["state"].keys() == sb["state"].keys()
    if momentum == 0:
        assert len(sa["state"]) == 0 and len(a.state) == 0
    else:
        assert len(sa["state"]) == len(ours)
    for k in sa["state"]:
        assert sa["state"][k].keys() == sb["state"][k].keys() == {"momentum_buffer"}
        assert _buf_close(sa["state"][k]["momentum_buffer"], sb["state"][k]["momentum_buffer"]), k
    # state interchange: torch's into a fresh one of ours, ours into a fresh torch.optim.SGD, one more identical step each way
    a2 = O.SGD(ours, capturable=capturable, **kw)
    a2.load_state_dict(copy.deepcopy(sb))       # (load_state_dict may alias same-device tensors: the optimizers must not share buffers)
    b2 = torch.optim.SGD(ref, **kw)
    b2.load_state_dict(copy.deepcopy(sa))
    assert a2.param_groups[0]["capturable"] is capturable and a2.param_groups[0]["lr"] == b2.param_groups[0]["lr"] == 1e-3
    for p, q in zip(ours, ref):
        p.grad, q.grad = torch.ones_like(p), torch.ones_like(q)
    a2.step()
    b2.step()
    torch.cuda.synchronize()
    for i, (p, q) in enumerate(zip(ours, ref)):
        assert _close(p, q), (i, tuple(p.shape), float((p - q).abs().max()))
        if momentum:
            assert _buf_close(a2.state[p]["momentum_buffer"], b2.state[q]["momentum_buffer"]), i


@pytest.mark.parametrize("capturable", [False, True])
def test_sgd_alternating_parameter_sets_mix_first_and_later_steps(capturable, dev):
    """The reference's train_alternative (train/train.py:240-268): ONE optimizer, tile steps (encoder + tile head have gradients) and
    image steps (encoder + image heads) in turn.  The image heads get their first gradient one step after the encoder, so that step()
    holds tensors whose buffer is created (buf = g') next to tensors with history: one launch per class.  `never` gets no gradient."""
    shapes = {"enc": [(64, 3, 7, 7), (64,), (128, 64, 3, 3)], "tile": [(2, 128), (2,)], "img": [(7, 128), (7,), (1, 128)], "never": [(10,)]}
    g = torch.Generator().manual_seed(3)
    mk = lambda: {k: [torch.randn(s, generator=torch.Generator().manual_seed(11 + i)).to(dev).requires_grad_() for i, s in enumerate(v)]
                  for k, v in shapes.items()}
    ours, ref = mk(), mk()
    flat = lambda d: d["enc"] + d["tile"] + d["img"] + d["never"]
    a = O.SGD(flat(ours), lr=5e-4, momentum=0.9, weight_decay=1e-4, capturable=capturable)
    b = torch.optim.SGD(flat(ref), lr=5e-4, momentum=0.9, weight_decay=1e-4)
    plans = []
    for step in range(7):
        active = ("enc", "tile") if step % 2 == 0 else ("enc", "img")
        for grp in shapes:
            for p, q in zip(ours[grp], ref[grp]):
                if grp in active:
                    gr = torch.randn(p.shape, generator=g).to(dev)
                    p.grad, q.grad = gr, gr.clone()
                else:
                    p.grad = q.grad = None
        a.step()
        b.step()
        plans.append(len(a._plans))
    torch.cuda.synchronize()
    for p, q in zip(flat(ours)[:-1], flat(ref)[:-1]):
        assert _close(p, q), (tuple(p.shape), float((p - q).abs().max()))
        assert _buf_close(a.state[p]["momentum_buffer"], b.state[q]["momentum_buffer"])
    assert len(a.state[ours["never"][0]]) == 0 and torch.equal(ours["never"][0], ref["never"][0])
    assert plans[-1] == plans[3] <= 3, plans          # steady state: the tile set and the image set, no new plan per step


def test_sgd_refusals(dev):
    """All raised on the host before any launch."""
    p = torch.randn(1000, device=dev, requires_grad=True)
    with pytest.raises(ValueError):
        O.SGD([p], lr=1e-3, maximize=True)
    with pytest.raises(ValueError):
        O.SGD([p], lr=1e-3, nesterov=True, momentum=0)
    with pytest.raises(ValueError):
        O.SGD([p], lr=1e-3, nesterov=True, momentum=0.9, dampening=0.1)
    with pytest.raises(ValueError):
        O.SGD([p], lr=-1e-3)
    a = O.SGD([p], lr=1e-3, momentum=0.9)
    p.grad = torch.ones_like(p)
    a.step()                                  # warm: the plan exists
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with pytest.raises(RuntimeError, match="cannot be captured"):
            with torch.cuda.graph(torch.cuda.CUDAGraph(), stream=side):
                a.step()
    torch.cuda.synchronize()
    # the capturable form needs the momentum buffers of an eager step before it can be captured
    q = torch.randn(1000, device=dev, requires_grad=True)
    c = O.SGD([q], lr=1e-3, momentum=0.9, capturable=True)
    q.grad = torch.ones_like(q)
    c.sync_hyper()
    before = q.detach().clone()
    with torch.cuda.stream(side):
        with pytest.raises(RuntimeError, match="one eager step"):
            with torch.cuda.graph(torch.cuda.CUDAGraph(), stream=side):
                c.step()
    torch.cuda.synchronize()
    assert torch.equal(q, before) and len(c.state[q]) == 0
    # ... and its momentum may not cross zero once it has stepped
    c.step()
    c.param_groups[0]["momentum"] = 0.0
    with pytest.raises(ValueError, match="momentum"):
        c.sync_hyper()
    torch.cuda.synchronize()


def test_sgd_capturable_follows_onecycle_between_graph_replays(dev):
    """step() of the capturable form captured into a HIP graph, driven by a real OneCycleLR (cycle_momentum=True, its default: lr and
    momentum both move at every iteration): every replay takes the values sync_hyper() left on the device, equals the same optimizer
    stepped eagerly BIT FOR BIT, and torch.optim.SGD under the same schedule within the bound."""
    shapes = [(128, 64, 3, 3), (128,), (2, 2048), (4099,)]
    ours, eag, ref = _params(dev, shapes, 5), _params(dev, shapes, 5), _params(dev, shapes, 5)
    a = O.SGD(ours, lr=0.1, momentum=0.9, weight_decay=1e-4, capturable=True)
    e = O.SGD(eag, lr=0.1, momentum=0.9, weight_decay=1e-4, capturable=True)
    b = torch.optim.SGD(ref, lr=0.1, momentum=0.9, weight_decay=1e-4)
    scheds = [torch.optim.lr_scheduler.OneCycleLR(o, max_lr=0.1, total_steps=8) for o in (a, e, b)]
    gen = torch.Generator().manual_seed(9)
    static = [torch.zeros_like(p) for p in ours]
    for p, s in zip(ours, static):
        p.grad = s

    def feed():
        for s, q, r in zip(static, eag, ref):
            gr = torch.randn(s.shape, generator=gen).to(dev)
            s.copy_(gr)
            q.grad, r.grad = gr.clone(), gr.clone()

    feed()
    a.step(); e.step(); b.step()              # eager first step: buffers and device tables exist
    for s in scheds:
        s.step()
    torch.cuda.synchronize()
    a.sync_hyper()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            a.step()                           # captured, not executed
    torch.cuda.current_stream().wait_stream(side)
    seen = []
    for _ in range(5):
        feed()
        a.sync_hyper()
        graph.replay()
        e.step(); b.step()
        seen.append((a.param_groups[0]["lr"], a.param_groups[0]["momentum"]))
        for s in scheds:
            s.step()
    torch.cuda.synchronize()
    assert len(set(seen)) == 5 and all(o.param_groups[0]["lr"] == a.param_groups[0]["lr"] for o in (e, b))
    assert a.param_groups[0]["momentum"] != 0.9 and a.param_groups[0]["momentum"] == b.param_groups[0]["momentum"]
    for p, q, r in zip(ours, eag, ref):
        assert torch.equal(p, q)                                        # graph replay == eager, same kernels
        assert torch.equal(a.state[p]["momentum_buffer"], e.state[q]["momentum_buffer"])
        assert _close(p, r), float((p - r).abs().max())
        assert _buf_close(a.state[p]["momentum_buffer"], b.state[r]["momentum_buffer"])
    # a changed lr without sync_hyper() is refused inside a capture (the fill would be baked into the graph)
    a.param_groups[0]["lr"] = 3e-3
    with torch.cuda.stream(side):
        with pytest.raises(RuntimeError, match="sync_hyper"):
            with torch.cuda.graph(torch.cuda.CUDAGraph(), stream=side):
                a.step()
    torch.cuda.synchronize()


def _build(dev):
    m = R.MILresnet18()
    sd = m.state_dict()
    synth.fill_state_dict(sd)
    m.load_state_dict(sd)
    m = m.to(dev).set_compute_dtype(torch.bfloat16)
    m.setmode("tile")
    m.set_encoder_grads(True)
    m.train()
    opt = O.SGD([p for p in m.parameters() if p.requires_grad], lr=1e-3, momentum=0.9, weight_decay=1e-4, capturable=True)
    return m, opt, torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=1e-3, total_steps=12)


def _make_step(m, opt, sched):
    def step(xb, yb):
        opt.zero_grad(set_to_none=True)
        loss = HF.cross_entropy(m(xb, freeze_bn=True), yb, 1.0)
        loss.backward()
        opt.step()
        # host code: it runs after every eagerly enqueued step -- GraphedStep's warm-up steps included -- and neither at the capture
        # (the captured step is not executed) nor at a replay, after which the caller steps the scheduler
        if not torch.cuda.is_current_stream_capturing():
            sched.step()
        return loss.detach()
    return step


def test_graphed_resnet18_tile_step_under_onecycle_sgd_equals_eager_steps_bit_for_bit(dev):
    """The loop body train/train.py:29-42 with the scheduler-run optimizer, ResNet-18 on a bag of 8 tiles of 32 x 32 (spatial
    extents 16, 8, 8, 4, 2, 1: every layer runs): eager steps against graphed.GraphedStep with pre_replay=(opt.sync_hyper,).
    Schedule bookkeeping: GraphedStep's 2 warm-up steps are REAL steps on the example batch, so the eager model takes 2 steps on that
    batch first; each of them is followed by scheduler.step() (inside the step function, see _make_step) on both models, the capture
    advances nothing, and every later step -- eager or replayed -- is followed by one scheduler.step().  Both models therefore take
    their k-th update at the k-th point of the schedule."""
    bag, size = 8, 32
    batches = [(synth.normalise(synth.ihc_tiles(bag, size, 100 + i)).to(dev), torch.tensor([(j * 7 + i) % 2 for j in range(bag)], device=dev))
               for i in range(3)]
    m1, o1, s1 = _build(dev)
    eager = _make_step(m1, o1, s1)
    for _ in range(2):
        eager(*batches[0])
    losses1 = [eager(*batches[k % 3]).clone() for k in range(4)]
    m2, o2, s2 = _build(dev)
    graphed = GraphedStep(_make_step(m2, o2, s2), batches[0], warmup=2, pre_replay=(o2.sync_hyper,))
    losses2 = []
    for k in range(4):
        losses2.append(graphed(*batches[k % 3]).clone())
        s2.step()
    torch.cuda.synchronize()
    assert o1.param_groups[0]["lr"] == o2.param_groups[0]["lr"] and o1.param_groups[0]["momentum"] == o2.param_groups[0]["momentum"] != 0.9
    assert all(torch.equal(x, y) for x, y in zip(losses1, losses2)), (losses1, losses2)
    assert all(bool(torch.isfinite(x)) for x in losses1)
    for (k, x), (_, y) in zip(m1.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(x, y), k
    stepped = 0
    for p, q in zip(o1.param_groups[0]["params"], o2.param_groups[0]["params"]):
        if not o1.state.get(p):                      # upconv5-8 stay trainable in every mode but get no gradient here
            assert not o2.state.get(q)
            continue
        stepped += 1
        assert torch.equal(o1.state[p]["momentum_buffer"], o2.state[q]["momentum_buffer"])
    assert stepped > 50


def test_sgd_plans_keep_the_buffers_their_tables_point_at_alive(dev):
    """A plan's device table holds raw addresses of the momentum buffers, and a captured graph holds the plan (_capture.keep): the
    plan must own that memory, or `opt.state.clear()` frees what a replay reads and writes."""
    import gc
    import weakref
    ps = _params(dev, [(5,), (16385,)], 3)
    a = O.SGD(ps, lr=5e-4, momentum=0.9)
    for p in ps:
        p.grad = torch.ones_like(p)
    a.step()
    torch.cuda.synchronize()
    refs = [weakref.ref(a.state[p]["momentum_buffer"]) for p in ps]
    plans = list(a._plans.values())           # this step's (buffers created) and the next one's, built ahead
    assert len(plans) == 2
    a.state.clear()
    gc.collect()
    assert all(r() is not None for r in refs)
    del plans
    a._plans.clear()
    gc.collect()
    assert all(r() is None for r in refs)
