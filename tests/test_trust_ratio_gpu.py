"""LARS / LAMB with fused per-tensor trust ratios (csrc/kernels/optim.hip lars_sqnorm_kernel / lamb_phase1_kernel /
trust_ratio_kernel / lars_kernel / lamb_phase2_kernel, optim.LARS, optim.LAMB) against the fp64 reference
tests/_trust_ref.py.

The parameter set is test_grad_clip_gpu.py's (< 100 k elements): one element, around one 1024-element step,
exactly one chunk, one chunk plus one element, several chunks with a ragged end, a 2-D tensor, and a tensor
whose gradient is only 4-B aligned.  A 1-element tensor sits directly before multi-chunk tensors and a
multi-chunk one directly before a small one, which is where a wrong per-tensor segment shows.  Two param
groups: group 0 with the trust ratio and weight decay, group 1 with neither.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
try:
    from _trust_ref import TrustRef, assert_matches, assert_stats
finally:
    sys.path.pop(0)

pytestmark = pytest.mark.gpu
dev = "cuda"

CHUNK = 16384
SHAPES = [(1,), (1023,), (1024,), (1025,), (CHUNK,), (CHUNK + 1,), (3 * CHUNK + 1031,), (257, 33), (2051,)]
OFFSET_VIEW = len(SHAPES) - 1  # this tensor's .grad starts at element 1 of a flat buffer
SPLIT = 5  # tensors [0, SPLIT) form group 0, the rest group 1
KINDS = ["lars", "lars_nesterov", "lamb"]


def _params(seed=0):
    """Parameters with zeroed .grad storage (the last one a 4-B aligned view)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    ps = [torch.randn(s, device=dev, generator=g).requires_grad_(True) for s in SHAPES]
    for i, p in enumerate(ps):
        if i == OFFSET_VIEW:
            flat = torch.zeros(p.numel() + 5, device=dev)
            p.grad = flat[1:1 + p.numel()].view_as(p)
            assert p.grad.data_ptr() % 16 == 4
        else:
            p.grad = torch.zeros_like(p)
    return ps


def _grads(seed, scale=1.0):
    g = torch.Generator(device=dev).manual_seed(1000 + seed)
    return [torch.randn(s, device=dev, generator=g) * scale for s in SHAPES]


def _set(ps, gs):
    with torch.no_grad():
        for p, g in zip(ps, gs):
            p.grad.copy_(g)


def _ref_norm(gs):
    return torch.sqrt(sum((g.double() ** 2).sum() for g in gs)).item()


def _groups(ps, kind, lr, all_on=False, wd=1e-2):
    off = {} if all_on else ({"trust_ratio": False} if kind == "lamb" else {"trust_coefficient": 0.0})
    return [{"params": ps[:SPLIT], "lr": lr, "weight_decay": wd},
            {"params": ps[SPLIT:], "lr": lr * 0.5, "weight_decay": wd if all_on else 0.0, **off}]


def _kw(kind):
    if kind == "lamb":
        return dict(lr=1e-2)
    return dict(lr=0.05, momentum=0.9, nesterov=kind == "lars_nesterov", trust_coefficient=0.02)


def _pair(kind, ps, **gkw):
    """The fused optimizer on ``ps`` and the fp64 reference started from the same values."""
    from distributed_pytorch_example_amd import optim

    kw = _kw(kind)
    cls, name = (optim.LAMB, "lamb") if kind == "lamb" else (optim.LARS, "lars")
    return cls(_groups(ps, kind, kw["lr"], **gkw), **kw), TrustRef(name, _groups(ps, kind, kw["lr"], **gkw), **kw)


def _positions(n):
    """First and last element and both sides of every chunk boundary."""
    return sorted({0, n - 1} | {q for c in range(1, (n + CHUNK - 1) // CHUNK + 1) for q in (c * CHUNK - 1, c * CHUNK) if q < n})


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.uint8)


# ------------------------------------------------------------------------- per-tensor segments
def test_lars_segments_exact(C):
    """One 2^a_i in every weight tensor and one 2^b_i in every gradient, everything else 0, exponents distinct per
    tensor: each tensor's norms are exactly its own powers of two and ratio == 2^(a_i - b_i - 10), for all
    tensors in one step.  A wrong first_chunk (or a lost tail) leaks a neighbour's power of two or loses its
    own.  lr = 0 keeps the weights, so the rounds walk the positions on the same optimizer."""
    from distributed_pytorch_example_amd.optim import LARS

    ps = _params()
    opt = LARS(_groups(ps, "lars", 0.0, all_on=True, wd=0.0), lr=0.0, momentum=0.0, trust_coefficient=2.0 ** -10, trust_eps=0.0)
    assert opt.trust_stats is None
    a = [i - 4 for i in range(len(ps))]
    b = [3 - 2 * (i % 5) + i // 5 for i in range(len(ps))]
    assert len(set(a)) == len(a) and len({x - y for x, y in zip(a, b)}) > 4
    pos = [_positions(p.numel()) for p in ps]
    rounds = max(len(q) for q in pos)
    print("rounds:", rounds)
    want = torch.tensor([[2.0 ** x, 2.0 ** y, 2.0 ** (x - y - 10)] for x, y in zip(a, b)])
    for r in range(rounds):
        with torch.no_grad():
            for i, p in enumerate(ps):
                p.zero_()
                p.grad.zero_()
                p.view(-1)[pos[i][r % len(pos[i])]] = 2.0 ** a[i]
                p.grad.view(-1)[pos[i][(r + 1) % len(pos[i])]] = 2.0 ** b[i]
        opt.step()
        got = opt.trust_stats.cpu()
        assert got.shape == (len(ps), 3) and got.dtype == torch.float32
        assert torch.equal(got, want), (r, got, want)


def test_lamb_segments_count_elements(C):
    """LAMB's first step with weight_decay 0 has u = g / (|g| + eps) elementwise, so a tensor with k_i non-zero
    gradient elements (|g| >= 1, eps 1e-6: each |u| within 1e-6 of 1) has un = sqrt(k_i) within 1e-5; k_i is
    distinct per tensor and the elements sit on the segment and chunk edges first."""
    from distributed_pytorch_example_amd.optim import LAMB

    ps = _params(1)
    opt = LAMB(_groups(ps, "lamb", 1e-3, all_on=True, wd=0.0), lr=1e-3)
    ks = []
    with torch.no_grad():
        for i, p in enumerate(ps):
            n = p.numel()
            k = min(i + 1, n) if i else 1
            where = (_positions(n) + [q for q in range(7, n, max(1, n // 11)) if q not in _positions(n)])[:k]
            assert len(where) == k
            ks.append(k)
            for j, q in enumerate(where):
                p.grad.view(-1)[q] = (-1.0) ** j * 2.0 ** (j % 5)
    assert len(set(ks)) == len(ks)
    wn = [p.detach().double().norm().item() for p in ps]
    opt.step()
    got = opt.trust_stats.cpu().double()
    for i, k in enumerate(ks):
        assert abs(got[i, 1].item() - k ** 0.5) <= 1e-5 * k ** 0.5, (i, k, got[i])
        assert abs(got[i, 0].item() - wn[i]) <= 1e-5 * wn[i], (i, got[i], wn[i])


# ------------------------------------------------------------------------- parity with the fp64 reference
@pytest.mark.parametrize("kind", KINDS)
def test_parity_with_fp64_reference(C, kind):
    from distributed_pytorch_example_amd.ops import _state

    ps = _params(3)
    ours, ref = _pair(kind, ps)
    shadows = [_state.shadow(p) for p in ps]
    for s in range(4):
        gs = _grads(10 + s)
        _set(ps, gs)
        ours.step()
        for p, g in zip(ps, gs):
            assert torch.equal(p.grad, g)  # not modified by step()
        ref.step(gs)
        assert_stats(ours.trust_stats, ref)
    torch.cuda.synchronize()
    assert_matches(ours, ps, ref)
    for p, sh in zip(ps, shadows):
        assert torch.equal(sh.view(-1)[:p.numel()], p.detach().view(-1).bfloat16())
    st = ours.trust_stats.cpu()
    assert (st[SPLIT:, 2] == 1.0).all() and (st[:SPLIT, 2] != 1.0).all()
    assert ours.trust_on().tolist() == [True] * SPLIT + [False] * (len(ps) - SPLIT)


@pytest.mark.parametrize("nesterov", [False, True])
def test_zero_trust_coefficient_is_the_fused_sgd_bitwise(C, nesterov):
    from distributed_pytorch_example_amd.optim import LARS, SGD

    a_p, b_p = _params(4), _params(4)
    groups = lambda ps: [{"params": ps[:SPLIT], "lr": 0.05, "weight_decay": 1e-2}, {"params": ps[SPLIT:], "lr": 0.02}]
    lars = LARS(groups(a_p), lr=0.05, momentum=0.9, nesterov=nesterov, trust_coefficient=0.0)
    sgd = SGD(groups(b_p), lr=0.05, momentum=0.9, nesterov=nesterov)
    for s in range(3):
        gs = _grads(20 + s)
        _set(a_p, gs); lars.step()
        _set(b_p, gs); sgd.step()
    for p, q in zip(a_p, b_p):
        assert torch.equal(_bits(p.detach()), _bits(q.detach()))
        assert torch.equal(_bits(lars.state[p]["momentum_buffer"]), _bits(sgd.state[q]["momentum_buffer"]))
    assert (lars.trust_stats[:, 2] == 1.0).all()


@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_zero_norms_give_ratio_one(C, kind):
    """An all-zero weight tensor and an all-zero gradient tensor (LAMB: with weight_decay 0, so that u is 0 too)
    take ratio exactly 1.0, in a group with the ratio on; the update equals the reference."""
    ps = _params(5)
    with torch.no_grad():
        ps[1].zero_()
        ps[6].zero_()
    ours, ref = _pair(kind, ps, all_on=True, wd=0.0 if kind == "lamb" else 1e-2)
    for s in range(2):
        gs = _grads(30 + s)
        gs[3].zero_()
        gs[5].zero_()
        _set(ps, gs)
        ours.step()
        ref.step(gs)
        st = ours.trust_stats.cpu()
        if s == 0:
            assert st[1, 0] == 0.0 and st[6, 0] == 0.0 and st[1, 2] == 1.0 and st[6, 2] == 1.0
            assert st[3, 1] == 0.0 and st[5, 1] == 0.0 and st[3, 2] == 1.0 and st[5, 2] == 1.0
            assert all(st[i, 2] != 1.0 for i in (0, 2, 4, 7, 8))
        assert_stats(ours.trust_stats, ref)
    assert_matches(ours, ps, ref)


# ------------------------------------------------------------------------------------- clipping
@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_with_clipping(C, kind):
    """max_norm at half the smallest step norm (it clips on every step): parity with the reference, whose
    clipping is torch's clip_grad_norm_ on fp64; under LARS the reported norm is bitwise the one a clip-only
    fused SGD reports for the same gradients (same partials, same finishing kernel)."""
    from distributed_pytorch_example_amd.optim import SGD

    ps = _params(6)
    ours, ref = _pair(kind, ps)
    steps = [_grads(40 + s) for s in range(4)]
    m = 0.5 * min(_ref_norm(gs) for gs in steps)
    ours.set_grad_clip(m)
    if kind == "lars":
        sgd_p = _params(6)
        sgd = SGD([{"params": sgd_p[:SPLIT]}, {"params": sgd_p[SPLIT:]}], lr=0.01)
        sgd.set_grad_clip(m)
    for gs in steps:
        _set(ps, gs)
        ours.step()
        n = ref.step(gs, m)
        assert ours.grad_norm.item() > m
        assert abs(ours.grad_norm.item() - n.item()) <= 1e-5 * n.item()
        for p, g in zip(ps, gs):
            assert torch.equal(p.grad, g)
        if kind == "lars":
            _set(sgd_p, gs)
            sgd.step()
            assert torch.equal(_bits(ours.grad_norm), _bits(sgd.grad_norm))
        assert_stats(ours.trust_stats, ref)
    assert_matches(ours, ps, ref)


@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_skip_nonfinite_leaves_everything_untouched(C, kind):
    from distributed_pytorch_example_amd.ops import _state

    ps = _params(7)
    ours, ref = _pair(kind, ps)
    shadows = [_state.shadow(p) for p in ps]
    ours.set_grad_clip(1.0, skip_nonfinite=True)
    gs = _grads(50)
    _set(ps, gs); ours.step()  # a finite step first: states exist, step == 1
    ref.step(gs, 1.0)
    assert float(ours.skipped_steps) == 0.0

    def snap():
        out = [p.detach().clone() for p in ps] + [sh.clone() for sh in shadows] + [ours.trust_stats.clone()]
        for p in ps:
            st = ours.state[p]
            assert set(st) == ({"exp_avg", "exp_avg_sq", "step"} if kind == "lamb" else {"momentum_buffer", "step"})
            out += [v.clone() for k, v in sorted(st.items())]
        return out

    before = snap()
    bad = [g.clone() for g in _grads(51)]
    bad[-1].view(-1)[-1] = float("inf")
    _set(ps, bad); ours.step()
    after = snap()
    assert len(before) == len(after)
    for x, y in zip(before, after):
        assert torch.equal(_bits(x), _bits(y))
    assert all(float(ours.state[p]["step"]) == 1.0 for p in ps)
    assert float(ours.skipped_steps) == 1.0
    assert torch.isinf(ours.grad_norm).item()
    gs = _grads(52)  # the next finite step equals the reference's step from the unchanged state
    _set(ps, gs); ours.step()
    ref.step(gs, 1.0)
    assert_matches(ours, ps, ref)
    assert_stats(ours.trust_stats, ref)
    assert float(ours.skipped_steps) == 1.0


# ------------------------------------------------------------------------- determinism, graph
@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_same_gradients_twice_are_bitwise_equal(C, kind):
    a_p, b_p = _params(8), _params(8)
    a, _ = _pair(kind, a_p)
    b, _ = _pair(kind, b_p)
    for s in range(2):
        gs = _grads(60 + s)
        _set(a_p, gs); a.step()
        _set(b_p, gs); b.step()
        assert torch.equal(_bits(a.trust_stats), _bits(b.trust_stats))
    for p, q in zip(a_p, b_p):
        assert torch.equal(_bits(p.detach()), _bits(q.detach()))


@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_step_replays_in_a_graph(C, kind):
    """graph_safe: one step() captured on a single stream after warm-up on a side stream; three replays with new
    gradient values in the same .grad storage: parameters and trust_stats bitwise equal to the eager run."""
    eager_p, graph_p = _params(9), _params(9)
    eager, _ = _pair(kind, eager_p)
    graphed, _ = _pair(kind, graph_p)
    seq = [_grads(70 + s) for s in range(4)]
    for gs in seq:
        _set(eager_p, gs); eager.step()
    torch.cuda.synchronize()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _set(graph_p, seq[0]); graphed.step()  # warm-up: builds the table and the scratch
    torch.cuda.current_stream().wait_stream(side)
    graphed.graph_safe = True
    g = torch.cuda.CUDAGraph()
    _set(graph_p, seq[1])
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        graphed.step()  # (capture does not run it)
    g.replay()
    _set(graph_p, seq[2])
    g.replay()
    _set(graph_p, seq[3])
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(graph_p, eager_p):
        assert torch.equal(_bits(a.detach()), _bits(b.detach()))
    assert torch.equal(_bits(graphed.trust_stats), _bits(eager.trust_stats))
    assert all(float(graphed.state[p]["step"]) == 4.0 for p in graph_p)


# ------------------------------------------------------------------------------------- DDP
@pytest.mark.parametrize("name", ["lars", "lamb"])
def test_overlap_optimizer_is_refused(C, name):
    """Both sides refuse: DDP.overlap_optimizer checks the optimizer, and the optimizer refuses to be attached
    (the ratio kernel is a grid-wide step between backward and the update)."""
    from distributed_pytorch_example_amd.optim import build_optimizer
    from distributed_pytorch_example_amd.parallel import DDP

    mlp = torch.nn.Sequential(torch.nn.Linear(16, 32), torch.nn.ReLU(), torch.nn.Linear(32, 4)).to(dev)
    ddp = DDP(mlp)  # world 1
    opt = build_optimizer(name, mlp.parameters(), lr=0.1)
    with pytest.raises(RuntimeError, match="trust ratio"):
        ddp.overlap_optimizer(opt)
    with pytest.raises(RuntimeError, match="trust ratio"):
        opt._ov_attach(torch.cuda.Stream())
    assert opt._ov_stream is None and ddp._ov_opt is None
