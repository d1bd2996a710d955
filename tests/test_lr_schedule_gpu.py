"""The device-side learning-rate schedule (set_lr_schedule) on the GPU, against the fp64 formula of _lr_ref:
the lr itself, the update it produces, every optimizer, skipped steps, state_dict, a captured step, overlap."""
import copy

import numpy as np
import pytest
import torch

import _lr_ref

pytestmark = pytest.mark.gpu
dev = "cuda"

SIZES = [1, 7, 16385, 33 * 5]
BASE = (0.1, 0.03)  # two groups


def _params(seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    return [torch.randn(n, device=dev, generator=g).requires_grad_(True) for n in SIZES]


def _groups(ps, base=BASE, **kw):
    return [{"params": ps[:2], "lr": base[0], **kw}, {"params": ps[2:], "lr": base[1], **kw}]


def _grads(seed):
    g = torch.Generator(device=dev).manual_seed(1000 + seed)
    return [torch.randn(n, device=dev, generator=g) for n in SIZES]


def _set(ps, gs):
    for p, g in zip(ps, gs):
        if p.grad is None:
            p.grad = g.clone()
        else:
            p.grad.copy_(g)


def _ulps(a, b):
    """|a - b| in units of b's fp32 ulp (0 where both are 0)."""
    a, b = np.float32(a), np.float32(b)
    return abs(float(a) - float(b)) / float(np.spacing(np.abs(b)) if b != 0 else np.float32(1e-45))


def _assert_lrs(cur, want64):
    """current_lr against the fp64 values rounded to fp32, to within one fp32 ulp."""
    for got, w in zip(cur.tolist(), want64):
        assert _ulps(got, np.float32(w)) <= 1.0, (got, w)


@pytest.mark.parametrize("r", [0.0, 0.1])
@pytest.mark.parametrize("kind", _lr_ref.KINDS)
def test_formula_and_update(C, kind, r):
    """13 steps of SGD (momentum 0, weight decay 0: dp = -lr * g) with W = 3, T = 10: current_lr is the fp64
    formula rounded to fp32 to within one ulp, the update is that lr times the gradient, steps 10..12 hold."""
    from distributed_pytorch_example_amd.optim import SGD

    W, T, power = 3, 10, 2.0 if kind == "poly" else 1.0
    ps = _params(1)
    opt = SGD(_groups(ps), lr=1.0, momentum=0.0, weight_decay=0.0)
    opt.set_lr_schedule(kind, warmup_steps=W, total_steps=T, min_ratio=r, power=power)
    assert opt.current_lr is None
    worst = 0.0
    for s in range(13):
        gs = _grads(s)
        before = [p.detach().clone() for p in ps]
        _set(ps, gs)
        opt.step()
        cur = opt.current_lr
        assert cur.dtype == torch.float32 and cur.shape == (2,) and cur.is_cuda
        cur = cur.tolist()
        for gi, b in enumerate(BASE):
            want = np.float32(_lr_ref.lr(b, s, kind, W, T, r, power))
            u = _ulps(cur[gi], want)
            worst = max(worst, u)
            assert u <= 1.0, (kind, r, s, gi, cur[gi], float(want))
            if s >= T:  # past T the decays hold at min_ratio (the constant schedule, by its formula, at 1)
                assert _ulps(cur[gi], np.float32((1.0 if kind == "constant" else r) * b)) <= 1.0
        for i, (p, p0, g) in enumerate(zip(ps, before, gs)):
            lr = torch.tensor(cur[0 if i < 2 else 1], dtype=torch.float32, device=dev)
            # p - lr * g in fp32, contracted or not: two roundings of magnitudes <= |p| + |lr g|
            want = p0.double() - lr.double() * g.double()
            tol = 2.0 ** -23 * (p0.abs().double() + (lr * g).abs().double()) + 1e-30
            assert bool(((p.detach().double() - want).abs() <= tol).all()), (kind, s, i)
        assert all(g["lr"] == b for g, b in zip(opt.param_groups, BASE))  # the base lr is never mutated
    assert float(opt.schedule_step) == 13.0
    print(f"\n{kind} r={r}: worst current_lr error {worst:.2f} ulp")


@pytest.mark.parametrize("name", ["adam", "adamw", "lars", "lamb"])
def test_every_optimizer_takes_the_scheduled_lr(C, name):
    """One scheduled step (s = 1 of a 4-step warm-up, and s = 6 of a linear decay: factors that fp64 evaluates
    with the same operations on host and device) is bitwise the same optimizer stepping with the constant
    lr = base * f(s) and no schedule."""
    from distributed_pytorch_example_amd import optim

    cls = {"adam": optim.Adam, "adamw": optim.AdamW, "lars": optim.LARS, "lamb": optim.LAMB}[name]
    kw = dict(weight_decay=1e-2)
    for kind, W, T, r, s in (("cosine", 4, 10, 0.0, 1), ("linear", 2, 10, 0.25, 6)):
        a_p, b_p = _params(2), _params(2)
        a = cls(_groups(a_p), lr=1.0, **kw)
        a.set_lr_schedule(kind, warmup_steps=W, total_steps=T, min_ratio=r)
        sd = a.state_dict()
        sd["lr_schedule"]["last_step"] = s  # start the counter at s
        a.load_state_dict(sd)
        consts = tuple(_lr_ref.lr(b, s, kind, W, T, r) for b in BASE)
        b = cls(_groups(b_p, consts), lr=1.0, **kw)
        gs = _grads(40)
        _set(a_p, gs); a.step()
        _set(b_p, gs); b.step()
        torch.cuda.synchronize()
        assert a.current_lr.tolist() == [float(np.float32(c)) for c in consts]
        for x, y in zip(a_p, b_p):
            assert torch.equal(x, y), (name, kind)
        assert float(a.schedule_step) == s + 1


def test_skipped_step_consumes_no_schedule_step(C):
    from distributed_pytorch_example_amd.optim import SGD

    W, T = 3, 10
    ps = _params(3)
    opt = SGD(_groups(ps), lr=1.0, momentum=0.0)
    opt.set_grad_clip(1e9, skip_nonfinite=True)
    opt.set_lr_schedule("linear", warmup_steps=W, total_steps=T)
    _set(ps, _grads(1)); opt.step()
    assert float(opt.schedule_step) == 1.0
    bad = _grads(2)
    bad[2][5] = float("inf")
    before = [p.detach().clone() for p in ps]
    _set(ps, bad); opt.step()
    assert float(opt.schedule_step) == 1.0 and float(opt.skipped_steps) == 1.0
    lr_skipped = opt.current_lr.clone()
    for p, p0 in zip(ps, before):
        assert torch.equal(p, p0)
    _set(ps, _grads(3)); opt.step()  # the next real step uses the lr the skipped one would have
    assert torch.equal(opt.current_lr, lr_skipped)
    _assert_lrs(opt.current_lr, [_lr_ref.lr(b, 1, "linear", W, T) for b in BASE])
    assert float(opt.schedule_step) == 2.0


def test_state_dict_round_trip(C):
    """Saved after 4 steps and loaded into a fresh optimizer: the next 5 lrs and parameters are bitwise those
    of the uninterrupted run."""
    from distributed_pytorch_example_amd.optim import AdamW

    sched = dict(warmup_steps=3, total_steps=10, min_ratio=0.1)
    a_p = _params(4)
    a = AdamW(_groups(a_p), lr=1.0)
    a.set_lr_schedule("cosine", **sched)
    for s in range(4):
        _set(a_p, _grads(s)); a.step()
    sd = copy.deepcopy(a.state_dict())
    assert sd["lr_schedule"] == {"kind": "cosine", "warmup_steps": 3, "total_steps": 10, "min_ratio": 0.1, "power": 1.0,
                                 "last_step": 4}
    assert all(type(v) in (str, int, float) for v in sd["lr_schedule"].values())
    b_p = [p.detach().clone().requires_grad_(True) for p in a_p]
    b = AdamW(_groups(b_p), lr=1.0)
    b.load_state_dict(sd)
    for s in range(4, 9):
        gs = _grads(s)
        _set(a_p, gs); a.step()
        _set(b_p, gs); b.step()
        assert torch.equal(a.current_lr, b.current_lr)
        _assert_lrs(a.current_lr, [_lr_ref.lr(x, s, "cosine", 3, 10, 0.1) for x in BASE])
        for x, y in zip(a_p, b_p):
            assert torch.equal(x, y)
    assert float(b.schedule_step) == 9.0
    # without a schedule the entry is absent, and such a state dict leaves a set schedule alone
    c = AdamW(_groups(_params(4)), lr=1.0)
    assert "lr_schedule" not in c.state_dict()


def test_scheduled_step_replays_in_a_graph(C):
    """graph_safe: one scheduled step captured after a warm-up step on a side stream and replayed 4 times: the lr
    advances per replay and equals the eager twin's bitwise, min_ratio changed between replays included."""
    from distributed_pytorch_example_amd.optim import AdamW

    kw = dict(warmup_steps=2, total_steps=6)
    ratios = [0.0, 0.0, 0.0, 0.5, 0.5]  # min_ratio in force at steps 0..4
    eager_p, graph_p = _params(5), _params(5)
    eager, graphed = AdamW(_groups(eager_p), lr=1.0), AdamW(_groups(graph_p), lr=1.0)
    eager_lrs = []
    for s, r in enumerate(ratios):
        eager.set_lr_schedule("linear", min_ratio=r, **kw)
        _set(eager_p, _grads(s)); eager.step()
        eager_lrs.append(eager.current_lr.clone())
    torch.cuda.synchronize()

    graphed.set_lr_schedule("linear", min_ratio=ratios[0], **kw)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _set(graph_p, _grads(0)); graphed.step()  # warm-up: builds the table and the schedule block
    torch.cuda.current_stream().wait_stream(side)
    graphed.graph_safe = True
    g = torch.cuda.CUDAGraph()
    _set(graph_p, _grads(1))
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        graphed.step()  # (capture does not run it)
    for s in range(1, 5):
        if ratios[s] != ratios[s - 1]:
            graphed.set_lr_schedule("linear", min_ratio=ratios[s], **kw)
        _set(graph_p, _grads(s))
        g.replay()
        assert torch.equal(graphed.current_lr, eager_lrs[s]), s
    torch.cuda.synchronize()
    # the lr did advance per replay (the warm-up's last step and the decay's first both use the base lr)
    assert len({tuple(t.tolist()) for t in eager_lrs[1:]}) == 3
    _assert_lrs(eager_lrs[4], [_lr_ref.lr(b, 4, "linear", 2, 6, 0.5) for b in BASE])
    for a, b in zip(graph_p, eager_p):
        assert torch.equal(a, b)
    assert float(graphed.schedule_step) == 5.0


def test_schedule_off_gives_the_base_lr_again(C):
    from distributed_pytorch_example_amd.optim import SGD

    a_p, b_p = _params(6), _params(6)
    a, b = SGD(_groups(a_p), lr=1.0, momentum=0.9), SGD(_groups(b_p), lr=1.0, momentum=0.9)
    a.set_lr_schedule("poly", warmup_steps=1, total_steps=4, power=2.0)
    _set(a_p, _grads(0)); a.step()
    a.set_lr_schedule(None)
    assert a.current_lr is None and "lr_schedule" not in a.state_dict()
    with torch.no_grad():
        for x, y in zip(a_p, b_p):
            y.copy_(x)
    b.load_state_dict(copy.deepcopy(a.state_dict()))
    for s in range(1, 3):
        _set(a_p, _grads(s)); a.step()
        _set(b_p, _grads(s)); b.step()
    torch.cuda.synchronize()
    for x, y in zip(a_p, b_p):
        assert torch.equal(x, y)


def test_argument_checks(C):
    from distributed_pytorch_example_amd.optim import SGD

    opt = SGD(_groups(_params(7)), lr=1.0)
    for bad in (dict(kind="step", total_steps=10), dict(kind="linear", warmup_steps=-1, total_steps=10),
                dict(kind="linear", warmup_steps=10, total_steps=10), dict(kind="linear", total_steps=10, min_ratio=1.5),
                dict(kind="poly", total_steps=10, power=0.0), dict(kind="cosine")):
        with pytest.raises(ValueError):
            opt.set_lr_schedule(bad.pop("kind"), **bad)


def test_overlap_optimizer_takes_the_schedule(C):
    """DDP.overlap_optimizer (one process: the per-bucket steps during backward) with a schedule: not refused, the
    lrs are the schedule's, and the parameters match stepping after backward as closely as two such runs do."""
    from distributed_pytorch_example_amd.models import get_model
    from distributed_pytorch_example_amd.ops import functional as Fx
    from distributed_pytorch_example_amd.optim import build_optimizer
    from distributed_pytorch_example_amd.parallel import DDP

    torch.manual_seed(0)
    base = get_model("resnet_tiny", num_classes=10).to(dev)
    sched = dict(kind="cosine", warmup_steps=2, total_steps=4, min_ratio=0.1)
    runs, lrs = {}, {}
    for overlap in (False, "again", True):
        m = copy.deepcopy(base)
        ddp = DDP(m, bucket_cap_mb=0.25, first_bucket_mb=0.05)
        opt = build_optimizer("sgd", m.parameters(), lr=1e-2, weight_decay=1e-2, lr_schedule=sched)
        if overlap is True:
            ddp.overlap_optimizer(opt)
        g = torch.Generator(device=dev).manual_seed(1)
        lrs[overlap] = []
        for step in range(4):
            x = torch.randn(8, 3, 32, 32, device=dev, generator=g)
            y = torch.randint(0, 10, (8,), device=dev, generator=g)
            Fx.cross_entropy(ddp(x), y, 10).backward()
            opt.step()
            lrs[overlap].append(opt.current_lr.tolist())
            for p in m.parameters():
                p.grad = None
        torch.cuda.synchronize()
        assert ddp.num_buckets() > 2 and float(opt.schedule_step) == 4.0
        runs[overlap] = [p.detach().clone() for p in m.parameters()]
    assert lrs[True] == lrs[False]
    for s, row in enumerate(lrs[True]):
        assert _ulps(row[0], np.float32(_lr_ref.lr(1e-2, s, "cosine", 2, 4, 0.1))) <= 1.0

    def dev_(x, y):
        return max(((a - b).abs().max() / (b.abs().max() + 1e-30)).item() for a, b in zip(x, y))

    noise = dev_(runs["again"], runs[False])
    d = dev_(runs[True], runs[False])
    print(f"\noverlap vs after {d:.3e}; after vs after {noise:.3e}")
    if noise == 0.0:
        assert d == 0.0
    else:
        assert d <= 10 * noise + 1e-6, (d, noise)
