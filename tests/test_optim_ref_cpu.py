"""tests/_optim_ref.py checked without a GPU: the fp64 reference against torch.optim on fp64 tensors (which makes
it independent of the project), the fp32 emulation of AdamRule / SgdRule inside the derived budgets over the whole
hyper-parameter grid with no element left out, and the preconditions of the exact (tier A) cases that
test_optim_kernels_gpu.py runs bitwise."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
try:
    import _optim_ref as R
finally:
    sys.path.pop(0)

N = 257


U64 = 1e-13  # the budgets' shape with this unit roundoff: 6 to 10 counted roundings, so about 1e-12 relative


def _worst(got, want, tol, what):
    """``|got - want| <= tol`` everywhere.  The allowance is the one-step budget's shape with u = 1e-13: 1e-12
    relative to the magnitudes that enter the element's update, not to a result that may be a difference of two
    near-equal values (torch's lerp and addcdiv order their operations differently from the reference)."""
    err = (got - want).abs()
    assert bool((err <= tol).all()), (what, float((err / tol.clamp_min(1e-300)).max()))
    return float((err / tol.clamp_min(1e-300)).max())


def _torch_adam(hp, p):
    h = dict(R.ADAM_DEFAULTS)
    h.update(hp)
    q = p.double().clone().requires_grad_(True)
    cls = torch.optim.AdamW if h["decoupled"] and hp.get("_class") == "adamw" else torch.optim.Adam
    kw = dict(lr=h["lr"], betas=h["betas"], eps=h["eps"], weight_decay=h["weight_decay"], maximize=h["maximize"])
    if cls is torch.optim.Adam:
        kw["decoupled_weight_decay"] = h["decoupled"]
    return q, cls([q], **kw)


@pytest.mark.parametrize("t0", [t - 1 for t in R.ADAM_T])
def test_adam_reference_is_torch_fp64(t0):
    """OptimRef (and with it adam_step64) against torch.optim.Adam / AdamW on fp64 CPU tensors: every grid row, 4
    steps from a state at step t0 (fresh at 0, random exp_avg / exp_avg_sq >= 0 later).  torch keeps its own step
    counter and state tensors over the 4 steps; their values are set to the reference's after each comparison."""
    worst = 0.0
    for r, hp in enumerate(R.ADAM_GRID):
        hp = dict(hp, _class="adamw" if r % 2 else "adam")  # decoupled rows alternate AdamW and Adam's group flag
        p, g, m, v = R.wide_case(N, 100 + r, t0 + 1)
        q, opt = _torch_adam(hp, p)
        ref = R.OptimRef("adam", [{"params": [p], **{k: x for k, x in hp.items() if k != "_class"}}])
        if t0:
            opt.state[q] = {"step": torch.tensor(float(t0)), "exp_avg": m.double().clone(), "exp_avg_sq": v.double().clone()}
            ref.load_state(0, t0, exp_avg=m, exp_avg_sq=v)
        gen = torch.Generator().manual_seed(r)
        for s in range(4):
            g = R.wide(N, gen, zeros=0.05)
            z = torch.zeros(N, dtype=torch.float64)
            bud = R.adam_budget(ref.params[0], g, ref.state[0].get("exp_avg", z), ref.state[0].get("exp_avg_sq", z),
                                hp, t0 + s + 1, P=1.0, u=U64)
            q.grad = g.double().clone()
            opt.step()
            ref.step([g])
            got = [q.detach(), opt.state[q]["exp_avg"], opt.state[q]["exp_avg_sq"]]
            new = [ref.params[0], ref.state[0]["exp_avg"], ref.state[0]["exp_avg_sq"]]
            for a, b, what in zip(got, new, "pmv"):
                worst = max(worst, _worst(a, b, bud[what], (r, hp, s, what)))
            assert float(opt.state[q]["step"]) == ref.state[0]["step"] == t0 + s + 1
            with torch.no_grad():  # the next step starts from the reference's state: its allowance is for one step
                for a, b in zip(got, new):
                    a.copy_(b)
    print(f"\nadam t0={t0}: worst difference {worst:.3e} of the allowance")


def test_sgd_reference_is_torch_fp64():
    worst = 0.0
    for r, hp in enumerate(R.SGD_GRID):
        p, g, _, _ = R.wide_case(N, 200 + r, 1)
        q = p.double().clone().requires_grad_(True)
        opt = torch.optim.SGD([q], **hp)
        ref = R.OptimRef("sgd", [{"params": [p], **hp}])
        gen = torch.Generator().manual_seed(r)
        for s in range(4):
            g = R.wide(N, gen, zeros=0.05)
            bud = R.sgd_budget(ref.params[0], g, ref.state[0].get("momentum_buffer"), hp, s + 1, u=U64)
            q.grad = g.double().clone()
            opt.step()
            ref.step([g])
            got, new = [q.detach()], [ref.params[0]]
            if hp["momentum"] != 0:
                got.append(opt.state[q]["momentum_buffer"])
                new.append(ref.state[0]["momentum_buffer"])
            else:
                assert "momentum_buffer" not in ref.state[0] and opt.state[q].get("momentum_buffer") is None
            for a, b, what in zip(got, new, "pb"):
                worst = max(worst, _worst(a, b, bud[what] if s or what == "p" else U64 * b.abs(), (r, hp, s, what)))
            with torch.no_grad():
                for a, b in zip(got, new):
                    a.copy_(b)
    print(f"\nsgd: worst difference {worst:.3e} of the allowance")


def test_one_step_functions_round_the_hyperparameters_to_fp32():
    """step64 with its default rounding is step64 without it on hyper-parameters rounded beforehand, bitwise; and the
    rounding matters (0.1, 0.999 and 1e-3 are no fp32 values)."""
    p, g, m, v = R.wide_case(N, 7, 5)
    hp = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-3, weight_decay=0.1)
    hp32 = dict(lr=R._r32(1e-3), betas=(R._r32(0.9), R._r32(0.999)), eps=R._r32(1e-3), weight_decay=R._r32(0.1))
    a, b, c = R.adam_step64(p, g, m, v, hp, 5), R.adam_step64(p, g, m, v, hp32, 5, round32=False), \
        R.adam_step64(p, g, m, v, hp, 5, round32=False)
    assert all(torch.equal(x, y) for x, y in zip(a[:3], b[:3])) and not torch.equal(a[0], c[0])
    hp = dict(lr=0.05, momentum=0.9, dampening=0.1, weight_decay=1e-4)
    hp32 = {k: R._r32(x) for k, x in hp.items()}
    a, b, c = R.sgd_step64(p, g, m, hp, 2), R.sgd_step64(p, g, m, hp32, 2, round32=False), \
        R.sgd_step64(p, g, m, hp, 2, round32=False)
    assert all(torch.equal(x, y) for x, y in zip(a[:2], b[:2])) and not torch.equal(a[0], c[0])


def test_adam_emulation_within_budget():
    """|emulate32 - step64| <= budget at every element, every grid row, every t, on the wide data (P = 1 for the
    CPU's pow)."""
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    terms = [0.0] * 5
    n = 0
    for r, hp in enumerate(R.ADAM_GRID):
        for t in R.ADAM_T:
            p, g, m, v = R.wide_case(1024, 1000 * r + t, t)
            want = R.adam_step64(p, g, m, v, hp, t)
            got = R.adam_emulate32(p, g, m, v, hp, t)
            bud = R.adam_budget(p, g, m, v, hp, t, P=R.P_CPU)
            assert not any(bool(x.isnan().any()) for x in want[:3])
            for k, a, b in zip("pmv", got, want):
                worst[k] = max(worst[k], R.check(a, b, bud[k], f"row {r} {hp} t={t} {k}"))
            terms = [max(x, y) for x, y in zip(terms, R.term_ratios(got[0], want[0], bud["terms"]))]
            n += p.numel()
    print(f"\nadam emulation, {n} elements: worst error / budget p {worst['p']:.3f} m {worst['m']:.3f} v {worst['v']:.3f}; "
          "p where term 1..5 dominates " + " ".join(f"{x:.3f}" for x in terms))
    assert worst["p"] > 0.5  # term 1 is a single rounding: the emulation comes close to it


def test_sgd_emulation_within_budget():
    worst = {"p": 0.0, "b": 0.0}
    terms = [0.0] * 3
    for r, hp in enumerate(R.SGD_GRID):
        for t in R.SGD_T:
            p, g, b, _ = R.wide_case(1024, 5000 + 10 * r + t, t)
            b = b if hp["momentum"] != 0 else None
            want = R.sgd_step64(p, g, b, hp, t)
            got = R.sgd_emulate32(p, g, b, hp, t)
            bud = R.sgd_budget(p, g, b, hp, t)
            worst["p"] = max(worst["p"], R.check(got[0], want[0], bud["p"], f"row {r} {hp} t={t} p"))
            if hp["momentum"] != 0:
                worst["b"] = max(worst["b"], R.check(got[1], want[1], bud["b"], f"row {r} {hp} t={t} b"))
            else:
                assert got[1] is None and want[1] is None and bud["b"] is None
            terms = [max(x, y) for x, y in zip(terms, R.term_ratios(got[0], want[0], bud["terms"]))]
    print(f"\nsgd emulation: worst error / budget p {worst['p']:.3f} b {worst['b']:.3f}; "
          "p where term 1..3 dominates " + " ".join(f"{x:.3f}" for x in terms))
    assert worst["p"] > 0.5


def test_budget_tells_a_wrong_rule_from_a_right_one():
    """The budgets are tight enough for the faults the GPU file is there to catch: each of these wrong rules, run
    in fp64, leaves its budget somewhere on the grid."""
    def over(got, want, tol):
        return bool(((got - want).abs() > tol).any())

    hp = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-3)
    p, g, m, v = R.wide_case(1024, 1, 1000)
    lr, b1, b2, eps = R._r32(1e-3), R._r32(0.9), R._r32(0.999), R._r32(1e-3)
    want = R.adam_step64(p, g, m, v, hp, 1000)
    bud = R.adam_budget(p, g, m, v, hp, 1000)
    pd, m2, v2 = p.double(), want[1], want[2]
    eps_inside = pd - lr / (1 - b1 ** 1000) * m2 / ((v2.sqrt() + eps) / (1 - b2 ** 1000) ** 0.5)
    step_less = pd - lr / (1 - b1 ** 1000) * m2 / (v2.sqrt() / (1 - b2 ** 999) ** 0.5 + eps)
    assert over(eps_inside, want[0], bud["p"]) and over(step_less, want[0], bud["p"])
    # dropped (1 - lr wd) at lr wd = 1e-5, and the negation under maximize after the coupled decay at wd = 1e-4
    hp = dict(lr=1e-3, weight_decay=1e-2, decoupled=True)
    want, bud = R.adam_step64(p, g, m, v, hp, 10), R.adam_budget(p, g, m, v, hp, 10)
    assert over(R.adam_step64(p, g, m, v, dict(hp, weight_decay=0.0), 10)[0], want[0], bud["p"])
    hp = dict(lr=0.05, momentum=0.9, dampening=0.25, weight_decay=1e-4, maximize=True)
    want, bud = R.sgd_step64(p, g, m, hp, 2), R.sgd_budget(p, g, m, hp, 2)
    wrong = R.sgd_step64(p, -(g.double() + R._r32(1e-4) * pd), m, dict(hp, weight_decay=0.0, maximize=False), 2)
    assert over(wrong[0], want[0], bud["p"]) and over(wrong[1], want[1], bud["b"])
    # dampening on the first momentum step
    want, bud = R.sgd_step64(p, g, None, hp, 1), R.sgd_budget(p, g, None, hp, 1)
    assert over(0.75 * want[1], want[1], bud["b"])


@pytest.mark.parametrize("case", range(len(R.TIER_A_SGD)))
def test_tier_a_sgd_is_exact_in_fp32(case):
    """The precondition of the bitwise SGD cases: on multiples of 2^-6 with lr = 2^-3, momentum 1/2 and dampening
    1/4 (or Nesterov), the fp32 emulation equals fp64 bit for bit for 2 steps with wd = 2^-4 and 4 steps without,
    each step from the previous fp64 result (so every intermediate is an fp32 value)."""
    hp, steps = R.TIER_A_SGD[case]
    p, gs = R.tier_a_sgd(4096, case, steps)
    b = None
    for t, g in enumerate(gs, 1):
        want = R.sgd_step64(p, g, b, hp, t)
        got = R.sgd_emulate32(p, g, b, hp, t)
        assert torch.equal(got[0].double(), want[0]) and torch.equal(got[1].double(), want[1]), (hp, t)
        p, b = got
    assert not torch.equal(p, R.tier_a_sgd(4096, case, steps)[0])


@pytest.mark.parametrize("name,hp,c", R.TIER_A_ADAM, ids=[x[0] for x in R.TIER_A_ADAM])
def test_tier_a_adam_closed_form(name, hp, c):
    """The precondition of the bitwise Adam / AdamW cases at t = 1: emulation == fp64 bit for bit, and fp64 is
    the closed form p (1 - lr wd) - c sign(g); m = g / 2, v = g^2 / 4."""
    p, g = R.tier_a_adam(name, 4096, 3)
    z = torch.zeros_like(p)
    want = R.adam_step64(p, g, z, z, hp, 1)
    got = R.adam_emulate32(p, g, z, z, hp, 1)
    for a, b in zip(got, want[:3]):
        assert torch.equal(a.double(), b)
    decay = 1.0 - 2.0 ** -8 if hp.get("weight_decay") else 1.0
    assert torch.equal(want[0], p.double() * decay - c * g.double().sign())
    sg = -1.0 if hp.get("maximize") else 1.0
    assert torch.equal(want[1], sg * g.double() / 2) and torch.equal(want[2], g.double() ** 2 / 4)
    if name.startswith("pow2"):
        assert g.abs().min() == 2.0 ** -10 and g.abs().max() == 2.0 ** 10
    # where eps enters: added before the division by sqrt(1 - b2^t) the eps = 1 cases would move by lr / 3
    if name.startswith("eps1"):
        wrong = p.double() * decay - 2.0 ** -4 * (g.double() / 2) / ((g.double().abs() / 2 + 1.0) / 0.5)
        assert bool(((wrong - want[0]).abs() > 2.0 ** -8).all())  # lr / 2 - lr / 3 = 2^-5 / 6


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_optimref_add_param_group(kind):
    """A group added after 3 steps starts its own counters: 3 more steps agree with torch.optim on fp64 tensors
    (free-running trajectories on N(0, 1) data, 1e-10 of the largest magnitude), counters 6 and 3."""
    gen = torch.Generator().manual_seed(11)
    ps = [torch.randn(n, generator=gen) for n in (5, 300)]
    new = [torch.randn(n, generator=gen) for n in (7, 129)]
    if kind == "adam":
        hp, hp2 = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8), dict(lr=3e-3, betas=(0.5, 0.95), eps=1e-3, weight_decay=0.1)
        mk = lambda qs: torch.optim.Adam(qs, **hp)  # noqa: E731
    else:
        hp, hp2 = dict(lr=0.05, momentum=0.9, dampening=0.25, weight_decay=1e-4), dict(lr=0.01, momentum=0.5, dampening=0.0, nesterov=True)
        mk = lambda qs: torch.optim.SGD(qs, **hp)  # noqa: E731
    qs = [p.double().clone().requires_grad_(True) for p in ps]
    opt, ref = mk(qs), R.OptimRef(kind, [{"params": ps}], **hp)  # hp as the defaults: the new group inherits them
    for s in range(6):
        if s == 3:
            qs += [p.double().clone().requires_grad_(True) for p in new]
            opt.add_param_group({"params": qs[2:], **hp2})
            ref.add_param_group({"params": new, **hp2})
        gs = [torch.randn(q.shape, generator=gen) for q in qs]
        for q, g in zip(qs, gs):
            q.grad = g.double()
        opt.step()
        ref.step(gs)
        for i, q in enumerate(qs):
            assert float((q.detach() - ref.params[i]).abs().max()) <= 1e-10 * float(ref.params[i].abs().max()), (s, i)
    assert [st["step"] for st in ref.state] == [6, 6, 3, 3]
    if kind == "adam":
        assert [float(opt.state[q]["step"]) for q in qs] == [6.0, 6.0, 3.0, 3.0]
