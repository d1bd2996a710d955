"""Global-norm gradient clipping fused into the optimizer step (csrc/kernels/optim.hip
grad_sqnorm_kernel / grad_clip_coef_kernel / grad_scale_kernel, optim.set_grad_clip, optim.clip_grad_norm_).

The parameter set (< 100 k elements) holds the sizes at which the (tensor, chunk) walk can go wrong: one
element, around one 1024-element step, exactly one chunk, one chunk plus one element, several chunks with
a ragged end, a 2-D tensor, and a tensor whose gradient is only 4-B aligned (scalar path).  Two param
groups with different lr.
"""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
dev = "cuda"

CHUNK = 16384
SHAPES = [(1,), (1023,), (1024,), (1025,), (CHUNK,), (CHUNK + 1,), (3 * CHUNK + 1031,), (257, 33), (2051,)]
OFFSET_VIEW = len(SHAPES) - 1  # this tensor's .grad starts at element 1 of a flat buffer
SPLIT = 5  # tensors [0, SPLIT) form group 0, the rest group 1


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


def _groups(ps, lr):
    return [{"params": ps[:SPLIT], "lr": lr}, {"params": ps[SPLIT:], "lr": lr * 0.5}]


def _grads(seed, scale=1.0):
    g = torch.Generator(device=dev).manual_seed(1000 + seed)
    return [torch.randn(s, device=dev, generator=g) * scale for s in SHAPES]


def _set(ps, gs):
    with torch.no_grad():
        for p, g in zip(ps, gs):
            p.grad.copy_(g)


def _ref_norm(gs):
    return torch.sqrt(sum((g.double() ** 2).sum() for g in gs)).item()


def _make(kind, ps, lr=1e-2):
    from distributed_pytorch_example_amd import optim

    if kind == "adam":
        return optim.Adam(_groups(ps, lr))
    if kind == "adamw":
        return optim.AdamW(_groups(ps, lr), weight_decay=1e-2)
    nesterov = kind == "sgd_nesterov"
    return optim.SGD(_groups(ps, lr), momentum=0.9, nesterov=nesterov)


def _twin(kind, ps, lr=1e-2):
    if kind == "adam":
        return torch.optim.Adam(_groups(ps, lr))
    if kind == "adamw":
        return torch.optim.AdamW(_groups(ps, lr), weight_decay=1e-2)
    return torch.optim.SGD(_groups(ps, lr), momentum=0.9, nesterov=kind == "sgd_nesterov")


KINDS = ["adam", "adamw", "sgd", "sgd_nesterov"]
STATE_KEYS = ("exp_avg", "exp_avg_sq", "momentum_buffer")


def _assert_close_to_twin(ours, ref, ours_p, ref_p):
    for a, b in zip(ours_p, ref_p):
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-6)
    for a, b in zip(ours_p, ref_p):
        sa, sb = ours.state[a], ref.state[b]
        for k in STATE_KEYS:
            if k in sb:
                assert torch.allclose(sa[k], sb[k], rtol=1e-5, atol=1e-6), k
        if "step" in sb:
            assert float(sa["step"]) == float(sb["step"])


# --------------------------------------------------------------------------- the norm itself
def test_single_element_positions_exact(C):
    """All gradients 0 except one 3.0 at the first / last element of each tensor and on both sides of every
    chunk boundary: the norm is exactly 3.0 (9.0 and its root are exact in fp32).  A lost tail or a
    double-counted overlap gives 0 or sqrt(18)."""
    from distributed_pytorch_example_amd.optim import SGD

    ps = _params()
    opt = SGD(_groups(ps, 0.1))
    opt.set_grad_clip(1.0)
    assert opt.grad_norm is None
    norms, where = [], []
    for ti, p in enumerate(ps):
        n = p.numel()
        pos = sorted({0, n - 1} | {q for c in range(1, (n + CHUNK - 1) // CHUNK + 1) for q in (c * CHUNK - 1, c * CHUNK)
                                   if q < n})
        for q in pos:
            p.grad.view(-1)[q] = 3.0
            opt.step()
            norms.append(opt.grad_norm.clone())
            where.append((ti, q))
            p.grad.view(-1)[q] = 0.0
    got = torch.stack(norms).cpu()
    print("positions probed:", len(where))
    bad = [(w, v) for w, v in zip(where, got.tolist()) if v != 3.0]
    assert not bad, bad


def test_norm_accuracy_and_determinism(C):
    """|norm - ref| / ref <= 1e-5 against the fp64 sum.  Bound: a lane adds at most 64 squares in fp32
    (sequential worst case 64 x 2^-24 ~ 4e-6), the wave / block / fp64 tree adds < 12 roundings, the root
    halves the relative error: 1e-5 leaves more than 2x.  The same gradients twice: bitwise equal."""
    from distributed_pytorch_example_amd.optim import Adam

    ps = _params()
    opt = Adam(_groups(ps, 1e-3))
    opt.set_grad_clip(1.0)
    for seed, scale in ((0, 1.0), (1, 1e-3), (2, 37.0)):
        gs = _grads(seed, scale)
        ref = _ref_norm(gs)
        _set(ps, gs)
        opt.step()
        a = opt.grad_norm.clone()
        opt.step()
        b = opt.grad_norm.clone()
        rel = abs(a.item() - ref) / ref
        print(f"seed {seed} scale {scale}: norm {a.item():.7g} ref {ref:.7g} rel err {rel:.2e}")
        assert rel <= 1e-5
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------- parity with torch
@pytest.mark.parametrize("kind", KINDS)
def test_parity_with_torch_clipping(C, kind):
    """set_grad_clip(m) + step == torch clip_grad_norm_(ps, m) + the torch.optim twin, 4 steps, with m below
    every step's norm (it clips on every step).  The gradients are left untouched."""
    ours_p, ref_p = _params(3), _params(3)
    ours = _make(kind, ours_p)
    ref = _twin(kind, ref_p)
    steps = [_grads(10 + s) for s in range(4)]
    m = 0.5 * min(_ref_norm(gs) for gs in steps)
    ours.set_grad_clip(m)
    for gs in steps:
        _set(ours_p, gs)
        ours.step()
        assert ours.grad_norm.item() > m
        for p, g in zip(ours_p, gs):
            assert torch.equal(p.grad, g)  # not modified by step()
        _set(ref_p, gs)
        torch.nn.utils.clip_grad_norm_(ref_p, m)
        ref.step()
    torch.cuda.synchronize()
    _assert_close_to_twin(ours, ref, ours_p, ref_p)


@pytest.mark.parametrize("kind", KINDS)
def test_no_clip_when_norm_below_max_is_bitwise(C, kind):
    """max_norm 10x above the norm: coef == 1.0 and the parameters equal, bitwise, those of the same
    optimizer without any clip (and the torch sequence within the kernels' tolerance)."""
    ours_p, plain_p, ref_p = _params(4), _params(4), _params(4)
    ours = _make(kind, ours_p)
    plain = _make(kind, plain_p)
    ref = _twin(kind, ref_p)
    steps = [_grads(20 + s) for s in range(4)]
    m = 10.0 * max(_ref_norm(gs) for gs in steps)
    ours.set_grad_clip(m)
    for gs in steps:
        _set(ours_p, gs); ours.step()
        _set(plain_p, gs); plain.step()
        _set(ref_p, gs); torch.nn.utils.clip_grad_norm_(ref_p, m); ref.step()
    torch.cuda.synchronize()
    for a, b in zip(ours_p, plain_p):
        assert torch.equal(a, b)
    _assert_close_to_twin(ours, ref, ours_p, ref_p)


def test_clip_off_again_is_plain_step(C):
    """set_grad_clip(None) after clipped steps: the following steps are bitwise the unclipped ones (the
    coef slot of the hyper-parameter rows is back at 1.0)."""
    from distributed_pytorch_example_amd.optim import SGD

    ours_p, plain_p = _params(5), _params(5)
    ours, plain = SGD(_groups(ours_p, 0.05), momentum=0.9), SGD(_groups(plain_p, 0.05), momentum=0.9)
    gs = _grads(30)
    ours.set_grad_clip(0.25)
    _set(ours_p, gs); ours.step()
    ours.set_grad_clip(None)
    plain.load_state_dict(copy.deepcopy(ours.state_dict()))  # continue from the same point, never clipped
    with torch.no_grad():
        for a, b in zip(ours_p, plain_p):
            b.copy_(a)
    for s in range(2):
        gs = _grads(31 + s)
        _set(ours_p, gs); ours.step()
        _set(plain_p, gs); plain.step()
    for a, b in zip(ours_p, plain_p):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------ non-finite gradients
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_nonfinite_default_matches_torch(C, kind):
    """One inf in the last element of the last tensor, default mode: as the torch sequence (coef 0, the inf
    becomes NaN), same NaN pattern and same finite values."""
    ours_p, ref_p = _params(6), _params(6)
    ours = _make(kind, ours_p)
    ref = _twin(kind, ref_p)
    ours.set_grad_clip(1.0)
    gs = _grads(40)
    gs[-1].view(-1)[-1] = float("inf")
    _set(ours_p, gs); ours.step()
    _set(ref_p, gs); torch.nn.utils.clip_grad_norm_(ref_p, 1.0); ref.step()
    assert torch.isinf(ours.grad_norm).item()
    assert float(ours.skipped_steps) == 0.0
    for a, b in zip(ours_p, ref_p):
        assert torch.equal(torch.isnan(a), torch.isnan(b))
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-6, equal_nan=True)
    assert torch.isnan(ours_p[-1].view(-1)[-1]).item()


@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_skip_nonfinite_leaves_everything_untouched(C, kind):
    from distributed_pytorch_example_amd.ops import _state

    ours_p, ref_p = _params(7), _params(7)
    ours = _make(kind, ours_p)
    ref = _twin(kind, ref_p)
    shadows = [_state.shadow(p) for p in ours_p]
    ours.set_grad_clip(1.0, skip_nonfinite=True)
    gs = _grads(50)
    _set(ours_p, gs); ours.step()  # a finite step first: states exist, step == 1
    _set(ref_p, gs); torch.nn.utils.clip_grad_norm_(ref_p, 1.0); ref.step()
    assert float(ours.skipped_steps) == 0.0
    for p, sh in zip(ours_p, shadows):  # the step kept the bf16 shadows current
        assert torch.equal(sh.view(-1)[:p.numel()], p.detach().view(-1).bfloat16())

    def snap():
        out = [p.detach().clone() for p in ours_p] + [sh.clone() for sh in shadows]
        for p in ours_p:
            out += [v.clone() for k, v in sorted(ours.state[p].items()) if torch.is_tensor(v)]
        return out

    before = snap()
    bad = [g.clone() for g in _grads(51)]
    bad[-1].view(-1)[-1] = float("inf")
    _set(ours_p, bad); ours.step()
    after = snap()
    assert len(before) == len(after)
    for a, b in zip(before, after):
        assert torch.equal(a.view(torch.uint8) if a.dtype != torch.float32 else a.view(torch.int32),
                           b.view(torch.uint8) if b.dtype != torch.float32 else b.view(torch.int32))
    assert all(float(ours.state[p]["step"]) == 1.0 for p in ours_p)
    assert float(ours.skipped_steps) == 1.0
    assert torch.isinf(ours.grad_norm).item()
    # the next finite step equals torch's step from the unchanged state
    gs = _grads(52)
    _set(ours_p, gs); ours.step()
    _set(ref_p, gs); torch.nn.utils.clip_grad_norm_(ref_p, 1.0); ref.step()
    _assert_close_to_twin(ours, ref, ours_p, ref_p)
    assert float(ours.skipped_steps) == 1.0


# ---------------------------------------------------------------------------------- HIP graph
def test_clipped_step_replays_in_a_graph(C):
    """graph_safe: one clipped step() captured on a single stream after warm-up on a side stream; two replays
    with new gradient values in the same .grad storage and max_norm changed through the device scalar in
    between: parameters bitwise equal to the eager run."""
    from distributed_pytorch_example_amd.optim import AdamW

    eager_p, graph_p = _params(8), _params(8)
    eager, graphed = AdamW(_groups(eager_p, 1e-2)), AdamW(_groups(graph_p, 1e-2))
    seq = [(_grads(60), 3.0), (_grads(61), 3.0), (_grads(62), 3.0), (_grads(63), 0.5)]
    for gs, m in seq:
        eager.set_grad_clip(m)
        _set(eager_p, gs); eager.step()
    torch.cuda.synchronize()

    graphed.set_grad_clip(seq[0][1])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _set(graph_p, seq[0][0]); graphed.step()  # warm-up: builds the table and the scratch
    torch.cuda.current_stream().wait_stream(side)
    graphed.graph_safe = True
    g = torch.cuda.CUDAGraph()
    _set(graph_p, seq[1][0])
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        graphed.step()  # (capture does not run it)
    g.replay()
    _set(graph_p, seq[2][0])
    g.replay()
    graphed.set_grad_clip(seq[3][1])
    _set(graph_p, seq[3][0])
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(graph_p, eager_p):
        assert torch.equal(a, b)
    assert torch.equal(graphed.grad_norm, eager.grad_norm)
    assert all(float(graphed.state[p]["step"]) == 4.0 for p in graph_p)


# ------------------------------------------------------------------------------ free function
def test_free_function_matches_torch(C):
    from distributed_pytorch_example_amd import optim

    ours_p, ref_p = _params(9), _params(9)
    gs = _grads(70)
    ref = _ref_norm(gs)
    for m in (0.5 * ref, 10.0 * ref):
        _set(ours_p, gs); _set(ref_p, gs)
        n_ours = optim.clip_grad_norm_(ours_p, m)
        n_ref = torch.nn.utils.clip_grad_norm_(ref_p, m)
        assert n_ours.shape == n_ref.shape and n_ours.is_cuda
        assert abs(n_ours.item() - ref) / ref <= 1e-5
        for a, b in zip(ours_p, ref_p):
            assert torch.allclose(a.grad, b.grad, rtol=1e-6, atol=0.0)
    # the same norm as the optimizer reports for these gradients
    opt = optim.SGD(_groups(ours_p, 0.1))
    opt.set_grad_clip(1.0)
    _set(ours_p, gs)
    opt.step()
    _set(ours_p, gs)
    assert torch.equal(optim.clip_grad_norm_(ours_p, 1.0), opt.grad_norm)
    # other norm types go to torch
    _set(ours_p, gs); _set(ref_p, gs)
    a = optim.clip_grad_norm_(ours_p, 0.1, norm_type=float("inf"))
    b = torch.nn.utils.clip_grad_norm_(ref_p, 0.1, norm_type=float("inf"))
    assert torch.equal(a, b)
    for p, q in zip(ours_p, ref_p):
        assert torch.equal(p.grad, q.grad)
    # error_if_nonfinite raises before scaling, as torch
    _set(ours_p, gs)
    ours_p[-1].grad.view(-1)[-1] = float("nan")
    with pytest.raises(RuntimeError, match="non-finite"):
        optim.clip_grad_norm_(ours_p, 1.0, error_if_nonfinite=True)
    assert torch.equal(ours_p[0].grad, gs[0])


# ------------------------------------------------------------------------------------- DDP
def test_overlap_optimizer_with_clipping_is_refused(C):
    """Both orders raise: a bucket stepped during backward would be updated before the global norm exists."""
    from distributed_pytorch_example_amd.optim import SGD
    from distributed_pytorch_example_amd.parallel import DDP

    mlp = torch.nn.Sequential(torch.nn.Linear(16, 32), torch.nn.ReLU(), torch.nn.Linear(32, 4)).to(dev)
    ddp = DDP(mlp)  # world 1
    opt = SGD(mlp.parameters(), lr=0.1)
    opt.set_grad_clip(1.0)
    with pytest.raises(RuntimeError, match="clip"):
        ddp.overlap_optimizer(opt)
    opt.set_grad_clip(None)
    ddp.overlap_optimizer(opt)
    with pytest.raises(RuntimeError, match="overlap_optimizer"):
        opt.set_grad_clip(1.0)
    ddp.overlap_optimizer(opt, enable=False)
    opt.set_grad_clip(1.0)  # detached again: allowed
