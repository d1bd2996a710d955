"""The plain fused update rules (csrc/kernels/optim.hip adam_kernel / sgd_kernel: AdamRule, SgdRule, optim_chunk)
through optim.Adam / optim.AdamW / optim.SGD, element by element against the fp64 reference tests/_optim_ref.py
(itself checked against torch.optim on fp64 tensors in test_optim_ref_cpu.py).

  a  exact cases: every element of p, the states and the bf16 shadow equals fp64 bit for bit
  b  one step from the device's own fp32 state against fp64, within the derived per-element budget: the
     hyper-parameter grid as the param groups of one optimizer, t = 1, 2, 3 by stepping and 10, 1000, 100000 from a
     loaded state dict; the geometry list under two rows
  c  6 steps against the fp64 trajectory with double hyper-parameters, at the project's optimizer tolerance
  d  zero and non-finite gradients     e  lr = 0 and lr as a tensor     f  add_param_group mid-run
  g  guard regions around every operand   h  state dict into stock torch.optim

The geometry list is test_trust_ratio_gpu.py's SHAPES (the last tensor's .grad is a view at a 4-byte offset) plus
one tensor whose parameter is itself such a view (its states are aligned, p is not): both take the one-element path.
"""
import copy
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
try:
    import _optim_ref as R
    from _trust_ref import assert_matches
finally:
    sys.path.pop(0)

pytestmark = pytest.mark.gpu
dev = "cuda"

CHUNK = 16384
SHAPES = [(1,), (1023,), (1024,), (1025,), (CHUNK,), (CHUNK + 1,), (3 * CHUNK + 1031,), (257, 33), (2051,), (2051,)]
GRAD_VIEW, PARAM_VIEW = 8, 9  # .grad 4 bytes into its buffer / the parameter 4 bytes into its buffer
SHADOWED = (1, 4, 6, 7, 9)  # tensors with a bf16 shadow
NG = 2051  # a grid tensor: two 1024-element vector steps and a 3-element tail
WORST = {}  # (test, quantity) -> worst error / budget, printed by every budget test


def _numel(s):
    n = 1
    for x in s:
        n *= x
    return n


def _bits(t):
    return t.detach().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same_bits(a, b):
    return torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


def _shadow_is_bf16_of(sh, p):
    """The shadow is p.bfloat16() bit for bit (a NaN is a NaN: its payload is the converting instruction's)."""
    want = p.detach().to(torch.bfloat16).reshape(-1)
    sh = sh.reshape(-1)
    nan = want.isnan()
    return torch.equal(sh.isnan(), nan) and _same_bits(torch.where(nan, torch.zeros_like(sh), sh), torch.where(nan, torch.zeros_like(want), want))


def _leaf(x, offset=False):
    """A leaf parameter holding the CPU tensor ``x``; ``offset``: a view one element into a flat buffer."""
    if offset:
        flat = torch.zeros(x.numel() + 5, device=dev)
        p = flat[1:1 + x.numel()].view(x.shape)
        p.copy_(x)
        p = p.detach().requires_grad_(True)
        assert p.data_ptr() % 16 == 4 and p.is_contiguous()
        return p
    return x.clone().to(dev).requires_grad_(True)


def _grad_storage(p, offset=False):
    if offset:
        flat = torch.zeros(p.numel() + 5, device=dev)
        p.grad = flat[1:1 + p.numel()].view_as(p)
        assert p.grad.data_ptr() % 16 == 4
    else:
        p.grad = torch.zeros_like(p, memory_format=torch.contiguous_format)


def _shadow(p):
    """A bf16 shadow by a torch cast (the layers' cast kernel is for whole, aligned parameters)."""
    p._dpe_shadow, p._dpe_shadow_ver = p.detach().to(torch.bfloat16).contiguous(), p._version


def _geometry(values):
    """The geometry list holding ``values`` (one CPU tensor per SHAPES entry)."""
    ps = [_leaf(x.reshape(s), offset=i == PARAM_VIEW) for i, (x, s) in enumerate(zip(values, SHAPES))]
    for i, p in enumerate(ps):
        _grad_storage(p, offset=i == GRAD_VIEW)
        if i in SHADOWED:
            _shadow(p)
    return ps


def _set(ps, gs):
    with torch.no_grad():
        for p, g in zip(ps, gs):
            p.grad.copy_(g.reshape(p.shape))


def _adam_kw(hp):
    kw = {k: v for k, v in hp.items() if k != "decoupled"}
    if hp.get("decoupled"):
        kw["decoupled_weight_decay"] = True
    return kw


def _make(kind, groups):
    """kind "adam" (decoupled rows as Adam's group flag), "adamw" (the class; every row decoupled) or "sgd";
    groups: [(params, hp)] with hp in the reference's format."""
    from distributed_pytorch_example_amd import optim

    if kind == "sgd":
        return optim.SGD([{"params": ps, **hp} for ps, hp in groups])
    if kind == "adamw":
        assert all(hp.get("decoupled") for _, hp in groups)
        return optim.AdamW([{"params": ps, **{k: v for k, v in hp.items() if k != "decoupled"}} for ps, hp in groups])
    return optim.Adam([{"params": ps, **_adam_kw(hp)} for ps, hp in groups])


def _state(opt, p, kind):
    """(t, s1, s2) as the device holds them: fp32 CPU copies (None where the state has none)."""
    st = opt.state.get(p, {})
    t = int(float(st["step"])) if "step" in st else 0
    keys = ("momentum_buffer", None) if kind == "sgd" else ("exp_avg", "exp_avg_sq")
    return (t,) + tuple(st[k].detach().cpu().clone() if k and st.get(k) is not None else None for k in keys)


def _step_and_check(name, kind, opt, ps, hps, gs):
    """One fused step with gradients ``gs`` and, per tensor, step64 from the fp32 state read back before it: every
    element of p and of the states within its budget (non-finite exactly where the reference is), .grad bitwise
    unchanged, the counter exact, the shadow the bf16 rounding of the new p."""
    sgd = kind == "sgd"
    before = [(p.detach().cpu().clone(),) + _state(opt, p, kind) for p in ps]
    _set(ps, gs)
    gbits = [_bits(p.grad).clone() for p in ps]
    opt.step()
    for i, (p, hp, g) in enumerate(zip(ps, hps, gs)):
        p0, t0, s1, s2 = before[i]
        t = t0 + 1
        g = g.reshape(p.shape)
        assert torch.equal(_bits(p.grad), gbits[i]), (name, i, "grad changed")
        assert float(opt.state[p]["step"]) == float(t), (name, i, "step counter")
        tag = f"{name} tensor {i} t={t}"
        if sgd:
            has_b = float(hp.get("momentum", 0.0)) != 0.0
            want = R.sgd_step64(p0, g, s1, hp, t)
            bud = R.sgd_budget(p0, g, s1, hp, t)
            got = {"p": p, "b": opt.state[p].get("momentum_buffer")}
            assert (got["b"] is not None) == has_b, (tag, "momentum buffer")
            pairs = [("p", want[0])] + ([("b", want[1])] if has_b else [])
        else:
            z = torch.zeros_like(p0)
            want = R.adam_step64(p0, g, z if s1 is None else s1, z if s2 is None else s2, hp, t)
            bud = R.adam_budget(p0, g, z if s1 is None else s1, z if s2 is None else s2, hp, t)
            got = {"p": p, "m": opt.state[p]["exp_avg"], "v": opt.state[p]["exp_avg_sq"]}
            pairs = [("p", want[0]), ("m", want[1]), ("v", want[2])]
        for k, w in pairs:
            r = R.check(got[k], w, bud[k], f"{tag} {k}")
            WORST[(name, k)] = max(WORST.get((name, k), 0.0), r)
        for j, r in enumerate(R.term_ratios(p, want[0], bud["terms"])):
            WORST[(name, f"p/term{j + 1}")] = max(WORST.get((name, f"p/term{j + 1}"), 0.0), r)
        sh = getattr(p, "_dpe_shadow", None)
        if sh is not None:
            assert p._dpe_shadow_ver == p._version and _shadow_is_bf16_of(sh, p), (tag, "shadow")


def _report(name):
    print(f"\n{name}: worst error / budget " + ", ".join(f"{k} {v:.3f}" for (n, k), v in sorted(WORST.items()) if n == name))


# ------------------------------------------------------------------------------------------- the device's pow
def test_device_pow_error():
    """P of adam_budget: the ulp error of fp32 pow on the device over the (b, t) pairs of the grid, by torch.pow on
    fp32 device tensors against fp64 (the math library, not the kernels under test).  The budget takes the
    measured maximum plus 1 ulp.  Also: pow(b, 1) == b, which the exact Adam cases at t = 1 rely on."""
    b = torch.tensor([x for x, _ in R.POW_PAIRS], dtype=torch.float32)
    t = torch.tensor([float(y) for _, y in R.POW_PAIRS], dtype=torch.float32)
    got = torch.pow(b.to(dev), t.to(dev)).cpu()
    err = R.pow_ulp_error(b, t, got)
    for (x, y), e, r in zip(R.POW_PAIRS, err.tolist(), got.tolist()):
        print(f"pow({x!r}, {y}) = {r!r}: {e:.3f} ulp")
    one = torch.tensor([0.5, 0.75, 0.9, 0.95, 0.999, 1.0 - 2.0 ** -10, 0.0], dtype=torch.float32)
    assert torch.equal(torch.pow(one.to(dev), torch.ones(7, device=dev)).cpu(), one)
    print(f"worst {float(err.max()):.3f} ulp; P_DEVICE = {R.P_DEVICE}")
    assert float(err.max()) + 1.0 <= R.P_DEVICE


# ------------------------------------------------------------------------------------------- a: exact cases
@pytest.mark.parametrize("case", range(len(R.TIER_A_SGD)))
def test_a_sgd_exact(C, case):
    """Multiples of 2^-6, lr 2^-3, momentum 1/2, dampening 1/4 or Nesterov: every intermediate is an fp32 value
    (test_optim_ref_cpu.py asserts it), so p, the buffer and the shadow are fp64's bit for bit, at every element
    of the geometry list, for 2 steps with wd = 2^-4 and 4 without."""
    hp, steps = R.TIER_A_SGD[case]
    data = [R.tier_a_sgd(_numel(s), 10 * case + i, steps) for i, s in enumerate(SHAPES)]
    ps = _geometry([d[0] for d in data])
    opt = _make("sgd", [(ps[:4], hp), (ps[4:], hp)])
    ref = [(d[0], None) for d in data]
    for t in range(1, steps + 1):
        _set(ps, [d[1][t - 1] for d in data])
        opt.step()
        for i, p in enumerate(ps):
            wp, wb, _ = R.sgd_step64(ref[i][0], data[i][1][t - 1], ref[i][1], hp, t)
            assert torch.equal(wp.float().double(), wp) and torch.equal(wb.float().double(), wb)
            ref[i] = (wp.float(), wb.float())
            assert _same_bits(p.detach().cpu().reshape(-1), ref[i][0]), (case, t, i, "p")
            assert _same_bits(opt.state[p]["momentum_buffer"].cpu().reshape(-1), ref[i][1]), (case, t, i, "b")
            assert float(opt.state[p]["step"]) == t
            if i in SHADOWED:
                assert _same_bits(p._dpe_shadow.cpu().reshape(-1), ref[i][0].to(torch.bfloat16)), (case, t, i, "shadow")


@pytest.mark.parametrize("name,hp,c", R.TIER_A_ADAM, ids=[x[0] for x in R.TIER_A_ADAM])
def test_a_adam_exact(C, name, hp, c):
    """Adam / AdamW at t = 1 with b1 = 1/2, b2 = 3/4, lr = 2^-5 on dyadic p: g = +-2^k with eps = 0 moves p by
    exactly lr sign(g); |g| = 1 with eps = 1 by exactly lr / 2 sign(g), which pins where eps enters; AdamW first
    multiplies by 1 - 2^-8.  p, m, v and the shadow are fp64's bit for bit.  (Relies on the device's
    powf(b, 1) == b: test_device_pow_error checks it with torch.pow.)"""
    data = [R.tier_a_adam(name, _numel(s), 20 + i) for i, s in enumerate(SHAPES)]
    ps = _geometry([d[0] for d in data])
    opt = _make("adamw" if hp.get("decoupled") else "adam", [(ps[:4], hp), (ps[4:], hp)])
    _set(ps, [d[1] for d in data])
    opt.step()
    decay = 1.0 - 2.0 ** -8 if hp.get("weight_decay") else 1.0
    sg = -1.0 if hp.get("maximize") else 1.0
    for i, p in enumerate(ps):
        p0, g = data[i]
        z = torch.zeros_like(p0)
        wp, wm, wv, _ = R.adam_step64(p0, g, z, z, hp, 1)
        assert torch.equal(wp, p0.double() * decay - c * g.double().sign())
        assert torch.equal(wm, sg * g.double() / 2) and torch.equal(wv, g.double() ** 2 / 4)
        assert _same_bits(p.detach().cpu().reshape(-1), wp.float()), (name, i, "p")
        assert _same_bits(opt.state[p]["exp_avg"].cpu().reshape(-1), wm.float()), (name, i, "m")
        assert _same_bits(opt.state[p]["exp_avg_sq"].cpu().reshape(-1), wv.float()), (name, i, "v")
        if i in SHADOWED:
            assert _same_bits(p._dpe_shadow.cpu().reshape(-1), wp.float().to(torch.bfloat16)), (name, i, "shadow")


# ------------------------------------------------------------------------------------------- b: one step, budget
def _load_state(opt, ps, kind, step, seed):
    """A state dict with ``step`` set and random states (v >= 0), loaded into the optimizer."""
    sd = copy.deepcopy(opt.state_dict())
    gen = torch.Generator().manual_seed(seed)
    for i, p in enumerate(ps):
        st = sd["state"][i]
        st["step"] = torch.tensor(float(step))
        if kind == "sgd":
            if st.get("momentum_buffer") is not None:
                st["momentum_buffer"] = R.wide(p.numel(), gen).reshape(p.shape).to(dev)
        else:
            st["exp_avg"] = R.wide(p.numel(), gen).reshape(p.shape).to(dev)
            st["exp_avg_sq"] = R.wide(p.numel(), gen, square=True).reshape(p.shape).to(dev)
    opt.load_state_dict(sd)


def test_b_adam_grid(C):
    """The 60 rows of the Adam grid as the param groups of ONE optimizer (mixed rows in one launch, hp + group * HP),
    one 2051-element tensor each; t = 1, 2, 3 by stepping, then t = 10, 1000, 100000 from a loaded state dict
    with random exp_avg and exp_avg_sq >= 0."""
    name = "adam grid"
    gen = torch.Generator().manual_seed(1)
    ps = [_leaf(R.wide(NG, gen)) for _ in R.ADAM_GRID]
    for p in ps:
        _grad_storage(p)
    opt = _make("adam", [([p], hp) for p, hp in zip(ps, R.ADAM_GRID)])
    for t in (1, 2, 3):
        _step_and_check(name, "adam", opt, ps, R.ADAM_GRID, [R.wide(NG, gen, zeros=0.05) for _ in ps])
    for t in (10, 1000, 100000):
        _load_state(opt, ps, "adam", t - 1, t)
        _step_and_check(name, "adam", opt, ps, R.ADAM_GRID, [R.wide(NG, gen, zeros=0.05) for _ in ps])
        assert all(float(opt.state[p]["step"]) == t for p in ps)
    _report(name)


def test_b_sgd_grid(C):
    """The 54 rows of the SGD grid as the groups of one optimizer: groups with momentum 0 (no buffer, a null state
    pointer) sit next to groups with momentum; t = 1, 2, 3 by stepping, then one step from a loaded state dict with a
    random momentum_buffer."""
    name = "sgd grid"
    gen = torch.Generator().manual_seed(2)
    ps = [_leaf(R.wide(NG, gen)) for _ in R.SGD_GRID]
    for p in ps:
        _grad_storage(p)
    opt = _make("sgd", [([p], hp) for p, hp in zip(ps, R.SGD_GRID)])
    for t in (1, 2, 3):
        _step_and_check(name, "sgd", opt, ps, R.SGD_GRID, [R.wide(NG, gen, zeros=0.05) for _ in ps])
    _load_state(opt, ps, "sgd", 7, 3)
    _step_and_check(name, "sgd", opt, ps, R.SGD_GRID, [R.wide(NG, gen, zeros=0.05) for _ in ps])
    assert all(float(opt.state[p]["step"]) == 8 for p in ps)
    assert sum(opt.state[p].get("momentum_buffer") is None for p in ps) == 6
    _report(name)


GEOMETRY_ROWS = [
    ("adamw", dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.1, decoupled=True)),
    ("adam", dict(lr=1e-3, betas=(0.5, 1.0 - 2.0 ** -10), eps=1e-3, weight_decay=0.1, maximize=True)),
    ("sgd", dict(lr=0.05, momentum=0.9, dampening=0.25, weight_decay=1e-4)),
    ("sgd", dict(lr=0.05, momentum=0.5, nesterov=True, weight_decay=2.0 ** -4, maximize=True)),
]


@pytest.mark.parametrize("row", range(len(GEOMETRY_ROWS)))
def test_b_geometry(C, row):
    """The geometry list (scalar tail only, around one vector step, one chunk, a chunk and one element, several
    chunks with a ragged end, 2-D, a .grad view and a parameter view at 4-byte offsets; half with bf16 shadows)
    under one hyper-parameter row, 3 steps."""
    kind, hp = GEOMETRY_ROWS[row]
    name = f"geometry {kind} {row}"
    gen = torch.Generator().manual_seed(30 + row)
    ps = _geometry([R.wide(_numel(s), gen) for s in SHAPES])
    opt = _make(kind, [(ps[:5], hp), (ps[5:], hp)])
    for t in (1, 2, 3):
        _step_and_check(name, "sgd" if kind == "sgd" else "adam", opt, ps, [hp] * len(ps),
                        [R.wide(_numel(s), gen, zeros=0.05) for s in SHAPES])
    _report(name)


# ------------------------------------------------------------------------------------------- c: trajectory
@pytest.mark.parametrize("kind", ["adam", "adamw", "sgd"])
def test_c_trajectory(C, kind):
    """6 steps against OptimRef (double hyper-parameters, as torch.optim) at the project's optimizer tolerance."""
    gen = torch.Generator().manual_seed(40)
    ps = _geometry([torch.randn(_numel(s), generator=gen) for s in SHAPES])
    if kind == "sgd":
        hps = [dict(lr=1e-2, momentum=0.9, dampening=0.1, weight_decay=1e-2), dict(lr=5e-3, momentum=0.5, nesterov=True)]
    else:
        hps = [dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, decoupled=kind == "adamw"),
               dict(lr=5e-3, betas=(0.8, 0.95), eps=1e-6, weight_decay=0.1, decoupled=True, maximize=True)]
    opt = _make(kind, [(ps[:5], hps[0]), (ps[5:], hps[1])])
    ref = R.OptimRef("sgd" if kind == "sgd" else "adam", [{"params": ps[:5], **hps[0]}, {"params": ps[5:], **hps[1]}])
    for s in range(6):
        gs = [torch.randn(_numel(sh), generator=gen).reshape(sh) for sh in SHAPES]
        _set(ps, gs)
        opt.step()
        ref.step(gs)
        assert_matches(opt, ps, ref)


# ------------------------------------------------------------------------------------------- d: zero / non-finite
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_d_zero_gradient_changes_nothing(C, kind):
    """Rows that are never hit: zero gradient, wd = 0, fresh state -- p bitwise unchanged and m, v, b exactly 0 over
    3 steps (eps > 0: 0 / (0 + eps) = 0)."""
    gen = torch.Generator().manual_seed(50)
    vals = [R.wide(_numel(s), gen) for s in SHAPES]
    ps = _geometry(vals)
    hp = dict(lr=1e-2, momentum=0.9, dampening=0.25) if kind == "sgd" else dict(lr=1e-2, eps=1e-8)
    opt = _make(kind, [(ps, hp)])
    for t in range(3):
        opt.step()
        for i, p in enumerate(ps):
            assert _same_bits(p.detach().cpu().reshape(-1), vals[i]), (t, i)
            for k in ("exp_avg", "exp_avg_sq", "momentum_buffer"):
                if k in opt.state[p]:
                    assert int(_bits(opt.state[p][k]).abs().max()) == 0, (t, i, k)  # +0.0, bit for bit
            assert float(opt.state[p]["step"]) == t + 1


def test_d_adamw_decay_alone(C):
    """Zero gradient under AdamW: p is exactly fl(p * fl(1 - lr wd)) per step.  (lr and wd as fp32; the factor is
    the same whether lr wd is rounded before the subtraction or, contracted into an FMA, not: asserted.)"""
    gen = torch.Generator().manual_seed(51)
    vals = [R.wide(_numel(s), gen) for s in SHAPES]
    ps = _geometry(vals)
    opt = _make("adamw", [(ps, dict(lr=1e-3, weight_decay=0.1, decoupled=True))])
    lr, wd = np.float32(1e-3), np.float32(0.1)
    f = float(np.float32(1.0) - lr * wd)
    assert f == float(np.float32(1.0 - float(lr) * float(wd))) and f < 1.0
    want = [v.clone() for v in vals]
    for t in range(3):
        opt.step()
        want = [w * f for w in want]
        for i, p in enumerate(ps):
            assert _same_bits(p.detach().cpu().reshape(-1), want[i]), (t, i)
            assert int(_bits(opt.state[p]["exp_avg"]).abs().max()) == 0 and int(_bits(opt.state[p]["exp_avg_sq"]).abs().max()) == 0


def test_d_adam_eps0_nan_where_the_reference_has_it(C):
    """eps = 0 and g = 0 on a fresh state: 0 / 0.  NaN in p exactly at the zero-gradient elements, as in fp64, the
    other elements within budget; m and v stay finite everywhere."""
    gen = torch.Generator().manual_seed(52)
    ps = _geometry([R.wide(_numel(s), gen) for s in SHAPES])
    hp = dict(lr=1e-3, eps=0.0)
    opt = _make("adam", [(ps, hp)])
    gs = [R.wide(_numel(s), gen, zeros=0.05) for s in SHAPES]
    for g in gs:
        g[-1] = 0.0  # the last element of every tensor (a tail element where there is a tail)
    _step_and_check("eps0", "adam", opt, ps, [hp] * len(ps), gs)
    for p, g in zip(ps, gs):
        assert torch.equal(p.detach().isnan().cpu().reshape(-1), g == 0) and bool((g == 0).any())
        assert bool(opt.state[p]["exp_avg"].isfinite().all()) and bool(opt.state[p]["exp_avg_sq"].isfinite().all())


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_d_nonfinite_gradient_elements(C, kind):
    """One inf and one NaN gradient element on both sides of a chunk boundary and in a tail, no clipping: the
    non-finite values appear in p and the states at exactly those elements, with the reference's values; every
    other element stays within budget."""
    gen = torch.Generator().manual_seed(53)
    ps = _geometry([R.wide(_numel(s), gen) for s in SHAPES])
    hp = dict(lr=0.05, momentum=0.9, dampening=0.25) if kind == "sgd" else dict(lr=1e-3, eps=1e-8)
    opt = _make(kind, [(ps, hp)])
    gs = [R.wide(_numel(s), gen, zeros=0.05) for s in SHAPES]
    where = {5: [(CHUNK - 1, "inf"), (CHUNK, "nan")], 6: [(CHUNK - 1, "nan"), (CHUNK, "inf"), (2 * CHUNK - 1, "inf"),
                                                          (2 * CHUNK, "nan"), (3 * CHUNK + 1030, "inf"), (3 * CHUNK + 1025, "nan")],
             3: [(1024, "inf")], 8: [(2049, "nan"), (5, "inf")], 9: [(2050, "inf"), (1024, "nan")]}
    for i, spots in where.items():
        for q, what in spots:
            gs[i][q] = float(what)
    _step_and_check(f"nonfinite {kind}", kind, opt, ps, [hp] * len(ps), gs)
    for i, p in enumerate(ps):
        bad = torch.zeros(p.numel(), dtype=torch.bool)
        for q, _ in where.get(i, []):
            bad[q] = True
        tensors = [p.detach()] + [opt.state[p][k] for k in ("exp_avg", "exp_avg_sq", "momentum_buffer") if k in opt.state[p]]
        for x in tensors:
            assert torch.equal(~x.isfinite().cpu().reshape(-1), bad), (kind, i)
    _report(f"nonfinite {kind}")


# ------------------------------------------------------------------------------------------- e: lr
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_e_lr_zero(C, kind):
    """lr = 0, wd = 0: p bitwise unchanged while the states advance within budget."""
    gen = torch.Generator().manual_seed(60)
    vals = [R.wide(_numel(s), gen) for s in SHAPES]
    ps = _geometry(vals)
    hp = dict(lr=0.0, momentum=0.9, dampening=0.25) if kind == "sgd" else dict(lr=0.0, eps=1e-8)
    opt = _make(kind, [(ps, hp)])
    for t in range(3):
        _step_and_check(f"lr0 {kind}", kind, opt, ps, [hp] * len(ps), [R.wide(_numel(s), gen, zeros=0.05) for s in SHAPES])
        for i, p in enumerate(ps):
            assert _same_bits(p.detach().cpu().reshape(-1), vals[i]), (t, i)
    for p in ps:
        s1 = opt.state[p]["momentum_buffer" if kind == "sgd" else "exp_avg"]
        assert bool((s1 != 0).any())


@pytest.mark.parametrize("kind", ["adam", "adamw", "sgd"])
def test_e_lr_tensor_is_the_float(C, kind):
    """lr given as a 0-dimensional tensor: bitwise the run with the float."""
    hp = dict(lr=0.05, momentum=0.9, weight_decay=1e-4) if kind == "sgd" else \
        dict(lr=3e-3, eps=1e-8, weight_decay=0.1, decoupled=kind == "adamw")
    gen = torch.Generator().manual_seed(61)
    vals = [R.wide(_numel(s), gen) for s in SHAPES]
    gs = [[R.wide(_numel(s), gen, zeros=0.05) for s in SHAPES] for _ in range(3)]
    runs = []
    for lr in (hp["lr"], torch.tensor(hp["lr"])):
        ps = _geometry(vals)
        opt = _make(kind, [(ps, dict(hp, lr=lr))])
        for g in gs:
            _set(ps, g)
            opt.step()
        runs.append((ps, opt))
    (a_p, a), (b_p, b) = runs
    for x, y in zip(a_p, b_p):
        assert _same_bits(x, y)
        for k in ("exp_avg", "exp_avg_sq", "momentum_buffer"):
            if k in a.state[x]:
                assert _same_bits(a.state[x][k], b.state[y][k])
    assert not _same_bits(a_p[6].detach().cpu().reshape(-1), vals[6])


# ------------------------------------------------------------------------------------------- f: add_param_group
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_f_add_param_group_mid_run(C, kind):
    """3 steps, then a group with other hyper-parameters, then 3 more: per-parameter counters that differ inside
    one launch.  The old tensors are bitwise those of a twin that never got the group; the new tensors follow the
    fp64 one-step reference with their own t = 1..3; the counters read 6 and 3."""
    gen = torch.Generator().manual_seed(70)
    vals = [R.wide(_numel(s), gen) for s in SHAPES]
    new_shapes = [(NG,), (CHUNK + 5,)]
    new_vals = [R.wide(_numel(s), gen) for s in new_shapes]
    if kind == "sgd":
        hp, hp2 = dict(lr=0.05, momentum=0.9, dampening=0.25, weight_decay=1e-4), dict(lr=0.01, momentum=0.5, nesterov=True)
    else:
        hp = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
        hp2 = dict(lr=3e-3, betas=(0.5, 0.95), eps=1e-3, weight_decay=0.1, decoupled=True)
    a_p, b_p = _geometry(vals), _geometry(vals)
    a, b = _make(kind, [(a_p, hp)]), _make(kind, [(b_p, hp)])
    gs = [[R.wide(_numel(s), gen, zeros=0.05) for s in SHAPES] for _ in range(6)]
    for s in range(3):
        _set(a_p, gs[s]); a.step()
        _set(b_p, gs[s]); b.step()
    new = [_leaf(x) for x in new_vals]
    for p in new:
        _grad_storage(p)
    a.add_param_group({"params": new, **(hp2 if kind == "sgd" else _adam_kw(hp2))})
    for s in range(3, 6):
        _set(b_p, gs[s]); b.step()
        _set(a_p, gs[s])
        _step_and_check(f"add group {kind}", kind, a, a_p + new, [hp] * len(a_p) + [hp2] * len(new),
                        gs[s] + [R.wide(_numel(sh), gen, zeros=0.05) for sh in new_shapes])
        assert all(float(a.state[p]["step"]) == s - 2 for p in new)
    for x, y in zip(a_p, b_p):
        assert _same_bits(x, y)
        for k in ("exp_avg", "exp_avg_sq", "momentum_buffer"):
            if k in b.state[y]:
                assert _same_bits(a.state[x][k], b.state[y][k])
        assert float(a.state[x]["step"]) == float(b.state[y]["step"]) == 6.0
    assert all(float(a.state[p]["step"]) == 3.0 for p in new)
    _report(f"add group {kind}")


# ------------------------------------------------------------------------------------------- g: guard regions
GUARD_SIZES = [1, 3, 1023, 1024, 1025, CHUNK, CHUNK + 1, CHUNK + 1027]
PAD = 1088  # elements of NaN pattern on each side (16-byte multiple in fp32 and bf16); all of it is checked
NAN32, NAN16 = 0x7FC0BEEF, 0x7FC5  # + 0x10000 * tag in fp32: every operand's pattern is its own NaN payload


def _guarded(n, offset, dtype, fill, tag=0):
    """(buffer bits, interior view, pattern): ``n`` elements inside a buffer of a NaN bit pattern, PAD (+ ``offset``)
    elements from its start."""
    it, pat = (torch.int32, NAN32 + 0x10000 * tag) if dtype == torch.float32 else (torch.int16, NAN16)
    raw = torch.full((2 * PAD + n + 8,), pat, dtype=it, device=dev)
    view = raw.view(dtype)[PAD + offset:PAD + offset + n]
    view.copy_(fill)
    return raw, view, pat


def _guards_intact(raw, n, offset, pat):
    lo, hi = raw[:PAD + offset], raw[PAD + offset + n:]
    return bool((lo == pat).all()) and bool((hi == pat).all())


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_g_guard_regions(C, kind, offset):
    """Every operand -- p, the gradient, each state and the bf16 shadow -- is a view into the interior of a larger
    buffer of a NaN bit pattern, once with 16-byte aligned interiors and once 4 bytes (the shadow 2 bytes) off.
    After 2 steps the pattern around every operand is bitwise untouched (all 1088 elements on each side, the 64
    nearest included), and the interior is within budget: the 16-byte stores and the half-width shadow store
    stay inside their tensors."""
    gen = torch.Generator().manual_seed(80 + offset)
    hp = dict(lr=0.05, momentum=0.9, dampening=0.25, weight_decay=1e-4) if kind == "sgd" else \
        dict(lr=1e-3, eps=1e-8, weight_decay=0.1, decoupled=True)
    ps, raws = [], []
    for n in GUARD_SIZES:
        val = R.wide(n, gen)
        praw, pv, ppat = _guarded(n, offset, torch.float32, val)
        p = pv.detach().requires_grad_(True)
        graw, p.grad, gpat = _guarded(n, offset, torch.float32, torch.zeros(n), 1)
        sraw, sh, spat = _guarded(n, offset, torch.bfloat16, val.to(torch.bfloat16))
        p._dpe_shadow, p._dpe_shadow_ver = sh, p._version
        assert p.data_ptr() % 16 == 4 * offset and p.grad.data_ptr() % 16 == 4 * offset and sh.data_ptr() % 8 == 2 * offset
        ps.append(p)
        raws.append([(praw, ppat), (graw, gpat), (sraw, spat)])
    opt = _make(kind, [(ps[:3], hp), (ps[3:], hp)])
    for p, rr in zip(ps, raws):
        n = p.numel()
        st = {"step": torch.tensor(0.0)}
        for j, k in enumerate(("momentum_buffer",) if kind == "sgd" else ("exp_avg", "exp_avg_sq")):
            raw, st[k], pat = _guarded(n, offset, torch.float32, torch.zeros(n), 2 + j)
            assert st[k].data_ptr() % 16 == 4 * offset
            rr.append((raw, pat))
        opt.state[p] = st
    for t in range(2):
        _step_and_check(f"guard {kind} {offset}", kind, opt, ps, [hp] * len(ps), [R.wide(n, gen, zeros=0.05) for n in GUARD_SIZES])
    for p, rr in zip(ps, raws):
        ptrs = {p.data_ptr(), p.grad.data_ptr(), p._dpe_shadow.data_ptr()} | {x.data_ptr() for x in opt.state[p].values()}
        n = p.numel()
        for raw, pat in rr:
            assert _guards_intact(raw, n, offset, pat), (kind, offset, n, hex(pat))
            assert raw.data_ptr() + (PAD + offset) * raw.element_size() in ptrs  # the optimizer stepped these views
    _report(f"guard {kind} {offset}")


# ------------------------------------------------------------------------------------------- h: into stock torch
@pytest.mark.parametrize("kind", ["adam", "adamw", "sgd", "sgd_plain"])
def test_h_state_dict_into_stock_torch(C, kind):
    """After 3 fused steps, state_dict() loads into the stock torch optimizer holding the same weights on the GPU;
    2 more steps of both agree at the project's optimizer tolerance.  Plain SGD (momentum 0) carries no buffer."""
    gen = torch.Generator().manual_seed(90)
    shapes = SHAPES[:GRAD_VIEW]  # stock torch allocates its own gradients and states: whole tensors
    ps = [_leaf(torch.randn(_numel(s), generator=gen).reshape(s)) for s in shapes]
    for p in ps:
        _grad_storage(p)
    if kind.startswith("sgd"):
        hp = dict(lr=1e-2, momentum=0.9 if kind == "sgd" else 0.0, dampening=0.1 if kind == "sgd" else 0.0, weight_decay=1e-2)
        stock_cls, stock_kw = torch.optim.SGD, hp
    else:
        hp = dict(lr=1e-2, betas=(0.8, 0.95), eps=1e-6, weight_decay=0.1, decoupled=kind == "adamw")
        stock_cls = torch.optim.AdamW if kind == "adamw" else torch.optim.Adam
        stock_kw = {k: v for k, v in hp.items() if k != "decoupled"}
    opt = _make("sgd" if kind.startswith("sgd") else kind, [(ps[:4], hp), (ps[4:], dict(hp, lr=5e-3))])
    for s in range(3):
        _set(ps, [torch.randn(_numel(sh), generator=gen) for sh in shapes])
        opt.step()
    sd = copy.deepcopy(opt.state_dict())
    if kind == "sgd_plain":
        assert all(st.get("momentum_buffer") is None for st in sd["state"].values())
        assert all(opt.state[p].get("momentum_buffer") is None for p in ps)
    qs = [p.detach().clone().requires_grad_(True) for p in ps]
    stock = stock_cls([{"params": qs[:4]}, {"params": qs[4:], "lr": 5e-3}], **stock_kw)
    stock.load_state_dict(sd)
    for s in range(2):
        gs = [torch.randn(_numel(sh), generator=gen).reshape(sh).to(dev) for sh in shapes]
        _set(ps, gs)
        for q, g in zip(qs, gs):
            q.grad = g.clone()
        opt.step()
        stock.step()
    for p, q in zip(ps, qs):
        assert torch.allclose(p.detach(), q.detach(), rtol=1e-5, atol=1e-6), float((p - q).abs().max())
        for k in ("exp_avg", "exp_avg_sq", "momentum_buffer"):
            if opt.state[p].get(k) is not None:
                assert torch.allclose(opt.state[p][k], stock.state[q][k], rtol=1e-5, atol=1e-6), k
        assert float(opt.state[p]["step"]) == 5.0
        if not kind.startswith("sgd"):
            assert float(stock.state[q]["step"]) == 5.0
