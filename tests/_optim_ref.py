"""Independent references of the plain update rules of optim.Adam / optim.AdamW / optim.SGD (imported by
test_optim_ref_cpu.py and test_optim_kernels_gpu.py): plain torch on the CPU, nothing from the extension.

    adam_step64 / sgd_step64        one step in fp64 from fp32 inputs, straight from the torch.optim definitions
    OptimRef                        a multi-step fp64 trajectory with its own state, groups and per-parameter t
    adam_emulate32 / sgd_emulate32  the same rule with every operation rounded to fp32 once, in AdamRule's /
                                    SgdRule's order (csrc/kernels/optim.hip), without contraction
    adam_budget / sgd_budget        per-element error allowance of one fp32 step against step64
    wide / tier_a_*                 the test data
    ADAM_GRID / SGD_GRID            the hyper-parameter grid both test files walk

``hp`` is a dict: Adam ``lr, betas, eps, weight_decay, maximize, decoupled``; SGD ``lr, momentum, dampening,
weight_decay, nesterov, maximize``.
"""
import itertools

import numpy as np
import torch

U = 2.0 ** -24  # unit roundoff of fp32
# ulp error of the device's fp32 pow over the (b, t) pairs of ADAM_GRID, measured with torch.pow on fp32 device
# tensors against fp64 (test_optim_kernels_gpu.py test_device_pow_error: 0.508 ulp on an MI355X), plus 1 ulp.
P_DEVICE = 1.51
P_CPU = 1.0  # what the CPU tests take for the emulation's torch.pow

ADAM_DEFAULTS = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, maximize=False, decoupled=False)
SGD_DEFAULTS = dict(lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, maximize=False)

f32 = np.float32


def _r32(x):
    """A Python float rounded to fp32 (as a Python float)."""
    return float(f32(x))


def adam_hp(hp, round32):
    h = dict(ADAM_DEFAULTS)
    h.update(hp)
    lr = h["lr"]
    lr = float(lr.item() if torch.is_tensor(lr) else lr)
    b1, b2 = (float(b) for b in h["betas"])
    eps, wd = float(h["eps"]), float(h["weight_decay"])
    if round32:
        lr, b1, b2, eps, wd = (_r32(x) for x in (lr, b1, b2, eps, wd))
    return lr, b1, b2, eps, wd, bool(h["maximize"]), bool(h["decoupled"])


def sgd_hp(hp, round32):
    h = dict(SGD_DEFAULTS)
    h.update(hp)
    lr = h["lr"]
    lr = float(lr.item() if torch.is_tensor(lr) else lr)
    mom, damp, wd = float(h["momentum"]), float(h["dampening"]), float(h["weight_decay"])
    if round32:
        lr, mom, damp, wd = (_r32(x) for x in (lr, mom, damp, wd))
    return lr, mom, damp, wd, bool(h["nesterov"]), bool(h["maximize"])


def _d(x):
    return x.detach().double().cpu()


# ------------------------------------------------------------------------------------------- fp64 steps
def adam_step64(p, g, m, v, hp, t, round32=True):
    """Step ``t`` (the counter after its increment) of torch.optim.Adam / AdamW in fp64: maximize, then the coupled
    ``g += wd p`` or the decoupled ``p *= 1 - lr wd``, ``m`` by lerp, ``v``, ``denom = sqrt(v) / sqrt(1 - b2^t) + eps``,
    ``p -= lr / (1 - b1^t) * m / denom``.  The hyper-parameters are taken as the device holds them: each one
    rounded to fp32 first (the hp row of csrc/kernels/optim.hip is ``float[12]``), then used in fp64;
    ``round32=False`` (OptimRef) keeps them double, as torch.optim does.

    Returns ``(p, m, v, mag)``; ``mag`` holds what adam_budget needs: S = |g| + wd |p| (coupled) or |g|, the
    decayed weight p1, step_size, denom and the update delta = step_size m / denom."""
    lr, b1, b2, eps, wd, maximize, decoupled = adam_hp(hp, round32)
    p, g, m, v = _d(p), _d(g), _d(m), _d(v)
    S = g.abs()
    if maximize:
        g = -g
    if wd != 0.0:
        if decoupled:
            p = p * (1.0 - lr * wd)
        else:
            S = S + wd * p.abs()
            g = g + wd * p
    m = m + (1.0 - b1) * (g - m)
    v = b2 * v + (1.0 - b2) * g * g
    step_size = lr / (1.0 - b1 ** t)
    denom = v.sqrt() / (1.0 - b2 ** t) ** 0.5 + eps
    delta = step_size * (m / denom)
    return p - delta, m, v, dict(S=S, p1=p, step_size=step_size, denom=denom, delta=delta)


def sgd_step64(p, g, b, hp, t, round32=True):
    """Step ``t`` of torch.optim.SGD in fp64: maximize, then ``g += wd p``; with momentum the first step sets
    ``b = g`` (no dampening), later ones ``b = mom b + (1 - damp) g``; then ``g + mom b`` (Nesterov) or ``b``;
    ``p -= lr d``.  ``b`` is ``None`` without momentum (and may be on the first step).  Hyper-parameters as in
    adam_step64: rounded to fp32 first unless ``round32=False``.

    Returns ``(p, b, mag)`` with mag = S, the direction d and b_old."""
    lr, mom, damp, wd, nesterov, maximize = sgd_hp(hp, round32)
    p, g = _d(p), _d(g)
    S = g.abs()
    if maximize:
        g = -g
    if wd != 0.0:
        S = S + wd * p.abs()
        g = g + wd * p
    b_old = torch.zeros_like(p) if b is None else _d(b)
    d = g
    if mom != 0.0:
        b = g.clone() if t <= 1 else mom * b_old + (1.0 - damp) * g
        d = g + mom * b if nesterov else b
    else:
        b = None
    return p - lr * d, b, dict(S=S, d=d, b_old=b_old)


class OptimRef:
    """fp64 trajectory of torch.optim.{Adam, AdamW, SGD} with double hyper-parameters (as torch.optim uses them).

        ref = OptimRef("adam" | "sgd", groups, **defaults)   # groups: [{"params": [tensors], <hp>}, ...]
        ref.add_param_group({"params": [...], <hp>})          # its tensors start at t = 0
        ref.step(grads)                                       # one tensor per parameter, in group order
        ref.params[i] / ref.state[i]                          # fp64; state keys as torch's, "step" an int
    """

    def __init__(self, kind, groups, **defaults):
        assert kind in ("adam", "sgd")
        self.kind = kind
        self.defaults = dict(ADAM_DEFAULTS if kind == "adam" else SGD_DEFAULTS)
        self.defaults.update(defaults)
        self.groups, self.params, self.state = [], [], []
        for g in groups:
            self.add_param_group(g)

    def add_param_group(self, g):
        hp = dict(self.defaults)
        hp.update({k: v for k, v in g.items() if k != "params"})
        idx = []
        for p in g["params"]:
            idx.append(len(self.params))
            self.params.append(_d(p).clone())
            self.state.append({})
        self.groups.append((hp, idx))

    def load_state(self, i, step, **tensors):
        self.state[i] = {"step": int(step), **{k: _d(x).clone() for k, x in tensors.items()}}

    def step(self, grads):
        for hp, idx in self.groups:
            for i in idx:
                st = self.state[i]
                t = st["step"] = st.get("step", 0) + 1
                if self.kind == "adam":
                    z = torch.zeros_like(self.params[i])
                    self.params[i], st["exp_avg"], st["exp_avg_sq"], _ = adam_step64(
                        self.params[i], grads[i], st.get("exp_avg", z), st.get("exp_avg_sq", z), hp, t, round32=False)
                else:
                    # a loaded torch.optim.SGD state has a buffer and no counter: t only tells first from later
                    first = "momentum_buffer" not in st
                    self.params[i], b, _ = sgd_step64(self.params[i], grads[i], st.get("momentum_buffer"), hp,
                                                      1 if first else 2, round32=False)
                    if b is not None:
                        st["momentum_buffer"] = b


# ------------------------------------------------------------------------------------------- fp32 emulation
def _pow32(b, t):
    return f32(torch.pow(torch.tensor(b, dtype=torch.float32), torch.tensor(float(t), dtype=torch.float32)).item())


def _f(x):
    return x.detach().float().cpu().clone()


def adam_emulate32(p, g, m, v, hp, t):
    """AdamRule on fp32 CPU tensors, one rounding per operation, in the kernel's order; the per-block scalars
    as its constructor computes them: ``lr / (1 - powf(b1, t))`` and ``sqrtf(1 - powf(b2, t))`` in fp32.  (The
    device contracts some multiply-adds into FMAs, which round once where this rounds twice.)"""
    lr, b1, b2, eps, wd, maximize, decoupled = (f32(x) if isinstance(x, float) else x for x in adam_hp(hp, True))
    one = f32(1.0)
    step_size = lr / (one - _pow32(b1, t))
    bc2_sqrt = np.sqrt(one - _pow32(b2, t))
    assert step_size.dtype == np.float32 and bc2_sqrt.dtype == np.float32
    p, g, m, v = _f(p), _f(g), _f(m), _f(v)
    if maximize:
        g = -g
    if wd != 0:
        if decoupled:
            p = p * float(one - lr * wd)
        else:
            g = g + float(wd) * p
    m = m + float(one - b1) * (g - m)
    v = float(b2) * v + (float(one - b2) * g) * g
    denom = v.sqrt() / float(bc2_sqrt) + float(eps)
    p = p - float(step_size) * (m / denom)
    assert p.dtype == m.dtype == v.dtype == torch.float32
    return p, m, v


def sgd_emulate32(p, g, b, hp, t):
    """SgdRule on fp32 CPU tensors, one rounding per operation, in the kernel's order."""
    lr, mom, damp, wd, nesterov, maximize = (f32(x) if isinstance(x, float) else x for x in sgd_hp(hp, True))
    p, g = _f(p), _f(g)
    if maximize:
        g = -g
    if wd != 0:
        g = g + float(wd) * p
    if mom != 0:
        b = g.clone() if t <= 1 else float(mom) * _f(b) + float(f32(1.0) - damp) * g
        g = g + float(mom) * b if nesterov else b
    else:
        b = None
    p = p - float(lr) * g
    assert p.dtype == torch.float32
    return p, b


# ------------------------------------------------------------------------------------------- budgets
def pow_err(b, t, P, u=U):
    """e(b, t): relative error of fp32 ``1 - powf(b, t)`` with a pow that is ``P`` ulp off.  pow's value b^t is
    wrong by at most P ulp <= P 2^-23 b^t; one more u absolute covers a pow result that lands on the coarser grid
    just below 1; dividing by 1 - b^t makes both relative to the difference, whose own rounding and that of the
    operation consuming it are the 2u."""
    bt = b ** t
    return (P * 2.0 * u * bt + u) / (1.0 - bt) + 2.0 * u


def adam_budget(p, g, m, v, hp, t, P=P_DEVICE, u=U):
    """Per-element absolute allowance for one fp32 AdamRule step from the fp32 state (p, g, m, v) against
    adam_step64 of the same state.  u = 2^-24; every constant is a count of fp32 roundings (first order; each
    count carries the slack noted, which covers the products of two errors).  An FMA contraction removes
    roundings, never adds one.

    g' is the gradient after maximize (exact) and the coupled decay ``g + wd p``: the product and the sum round,
    both on quantities <= S = |g| + wd |p|: e_g = 2 u S (0 when there is no coupled decay).

    m = m + (1 - b1)(g' - m): (1 - b1) times [e_g + the difference + fl(1 - b1) + the product: 3 roundings on
    <= S + |m|], plus the final sum's u |m_new| <= u (|m| + S):
        tol_m = 6 u (|m_old| + S)                  c_m = 2 + 3 + 1

    v = b2 v + ((1 - b2) g') g': the final sum and b2 v round on <= v_new: 2 u v_new.  The other product is
    (1 - b2) g'^2 with three roundings (fl(1 - b2) and two products) and twice the relative error of g', on
    <= (1 - b2) S^2:
        tol_v = 2 u v_new + 7 u (1 - b2) S^2       c_v = 2, c_v' = 3 + 2 * 2

    p is the sum of five terms:
      1. u |p_new|: the final subtraction's rounding.
      2. the decoupled decay p (1 - lr wd): lr wd, the subtraction and the product round,
         u |p| (lr wd + 2 |1 - lr wd|).
      3. (step_size / denom) tol_m: m's error through the quotient.
      4. |delta| tol_v / (2 v_new): v's error through the root (relative to sqrt(v) / bc2 <= denom).
      5. |delta| (K u + e(b1, t) + e(b2, t) / 2), delta the fp64 update: step_size = lr / (1 - powf(b1, t)) carries
         e(b1, t), bc2_sqrt = sqrtf(1 - powf(b2, t)) half of e(b2, t), and K = 8 counts the roundings of
         lr / ., sqrtf(1 - .), sqrtf(v), / bc2_sqrt, + eps, m / denom, step_size * . (7) plus 1 for second order.
    Terms 3 and 4 are scaled by 1 + e(b1, t) + e(b2, t) / 2 + K u, the factor by which the fp32 step_size / denom
    may exceed the fp64 one.

    P is the ulp error of the device's fp32 pow: measured 0.508 ulp at most over the (b, t) pairs of ADAM_GRID on an
    MI355X (torch.pow on fp32 device tensors against fp64; pow(b, 1) == b exactly), so P_DEVICE = 0.508 + 1 = 1.51
    rounded up; the CPU emulation is held to P = 1.

    Returns {"p", "m", "v": allowances, "terms": the five terms of p}."""
    lr, b1, b2, eps, wd, maximize, decoupled = adam_hp(hp, True)
    p_new, m_new, v_new, mag = adam_step64(p, g, m, v, hp, t)
    S, delta = mag["S"], mag["delta"].abs()
    coupled = wd != 0.0 and not decoupled
    tol_m = 6.0 * u * (_d(m).abs() + S)
    tol_v = 2.0 * u * v_new + 7.0 * u * (1.0 - b2) * S * S
    if not coupled:  # no e_g: 4 and 3 roundings where the docstring counts 6 and 7
        tol_m = 4.0 * u * (_d(m).abs() + S)
        tol_v = 2.0 * u * v_new + 3.0 * u * (1.0 - b2) * S * S
    K = 8.0
    e = pow_err(b1, t, P, u) + 0.5 * pow_err(b2, t, P, u)
    amp = 1.0 + e + K * u
    t1 = u * p_new.abs()
    t2 = u * _d(p).abs() * (lr * wd + 2.0 * abs(1.0 - lr * wd)) if (decoupled and wd != 0.0) else torch.zeros_like(t1)
    t3 = amp * (mag["step_size"] / mag["denom"]).abs() * tol_m
    rel_v = torch.where(v_new > 0, tol_v / (2.0 * v_new.clamp_min(1e-300)), torch.zeros_like(v_new))
    t4 = amp * delta * rel_v
    t5 = delta * (K * u + e)
    return {"p": t1 + t2 + t3 + t4 + t5, "m": tol_m, "v": tol_v, "terms": [t1, t2, t3, t4, t5]}


def sgd_budget(p, g, b, hp, t, u=U):
    """The same for SgdRule against sgd_step64.  e_g = 2 u S as in adam_budget (0 without weight decay).

    b: the first step copies g', tol_b = e_g.  Later b = mom b + (1 - damp) g': mom b rounds and the sum rounds
    (on <= mom |b| + S), and (1 - damp) times [e_g + fl(1 - damp) + the product on S]:
        tol_b = 5 u (mom |b_old| + S)              c = 2 + 2 + 1
    d: b (plain), g' (no momentum) or g' + mom b (Nesterov: e_g + mom tol_b + two roundings on <= |d| + mom |b|).
    p = p - lr d: lr tol_d + u lr |d| (the product) + u |p_new| (the subtraction)."""
    lr, mom, damp, wd, nesterov, maximize = sgd_hp(hp, True)
    p_new, b_new, mag = sgd_step64(p, g, b, hp, t)
    S, d = mag["S"], mag["d"].abs()
    e_g = 2.0 * u * S if wd != 0.0 else torch.zeros_like(S)
    tol_b = None
    tol_d = e_g
    if mom != 0.0:
        tol_b = e_g if t <= 1 else 5.0 * u * (mom * mag["b_old"].abs() + S)
        tol_d = tol_b
        if nesterov:
            tol_d = e_g + mom * tol_b + u * (mom * b_new.abs() + d)
    t1 = u * p_new.abs()
    t2 = lr * tol_d
    t3 = u * lr * d
    return {"p": t1 + t2 + t3, "b": tol_b, "terms": [t1, t2, t3]}


def check(got, want, tol, what=""):
    """``|got - want| <= tol`` at every element; where the fp64 reference is NaN or infinite the result must be
    the same NaN or infinity, and non-finite nowhere else.  Returns the worst error / allowance (0 / 0 counts as 0)."""
    got, want, tol = _d(got).reshape(-1), _d(want).reshape(-1), _d(tol).reshape(-1)
    nan = ~want.isfinite()
    same = (got == want) | (got.isnan() & want.isnan())
    assert torch.equal(~got.isfinite(), nan) and bool(same[nan].all()), \
        f"{what}: non-finite values differ from the reference's at {int((~same & (nan | ~got.isfinite())).sum())} elements"
    err = torch.where(nan, torch.zeros_like(got), (got - want).abs())
    tol = torch.where(nan, torch.zeros_like(tol), tol)
    bad = err > tol
    ratio = torch.where(err > 0, err / tol.clamp_min(1e-300), torch.zeros_like(err))
    if bool(bad.any()):
        i = int(ratio.argmax())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements over budget, worst at {i}: got "
                             f"{got[i].item():.9e} want {want[i].item():.9e} err {err[i].item():.3e} budget {tol[i].item():.3e}")
    return float(ratio.max()) if ratio.numel() else 0.0


def term_ratios(got, want, terms):
    """Worst error / allowance of p among the elements where each term is the largest one (0 where none is)."""
    got, want = _d(got).reshape(-1), _d(want).reshape(-1)
    ts = torch.stack([_d(x).reshape(-1) for x in terms])
    tot = ts.sum(0)
    ok = want.isfinite() & (tot > 0)
    ratio = torch.where(ok, (got - want).abs() / tot.clamp_min(1e-300), torch.zeros_like(tot))
    top = ts.argmax(0)
    return [float(ratio[ok & (top == k)].max()) if bool((ok & (top == k)).any()) else 0.0 for k in range(len(terms))]


# ------------------------------------------------------------------------------------------- data
def wide(n, gen, zeros=0.0, square=False):
    """``randn * 2^e`` with e uniform in [-20, 10] per element (so a square stays a normal fp32), ``zeros`` of
    them exact zeros; ``square``: the square of such values (a second moment)."""
    x = torch.randn(n, generator=gen) * torch.exp2(torch.rand(n, generator=gen) * 30.0 - 20.0)
    if zeros:
        x[torch.rand(n, generator=gen) < zeros] = 0.0
    x = x.float()
    return x * x if square else x


def wide_case(n, seed, t, momentum=True):
    """(p, g, m, v) for Adam / (p, g, b) for SGD use the first three: fresh zero state at t = 1, random state
    (v >= 0) later; 5 % of the gradient are exact zeros."""
    gen = torch.Generator().manual_seed(seed)
    p, g = wide(n, gen), wide(n, gen, zeros=0.05)
    if t > 1:
        return p, g, wide(n, gen), wide(n, gen, square=True)
    return p, g, torch.zeros(n), torch.zeros(n)


def dyadic(n, gen):
    """Integer multiples of 2^-6 in [-1, 1]."""
    return torch.randint(-64, 65, (n,), generator=gen).float() / 64.0


TIER_A_SGD = [  # (hp, steps that stay exact)
    (dict(lr=2.0 ** -3, momentum=0.5, dampening=0.25, weight_decay=2.0 ** -4), 2),
    (dict(lr=2.0 ** -3, momentum=0.5, dampening=0.0, nesterov=True, weight_decay=2.0 ** -4), 2),
    (dict(lr=2.0 ** -3, momentum=0.5, dampening=0.25, weight_decay=0.0), 4),
    (dict(lr=2.0 ** -3, momentum=0.5, dampening=0.0, nesterov=True, weight_decay=0.0), 4),
    (dict(lr=2.0 ** -3, momentum=0.5, dampening=0.25, weight_decay=0.0, maximize=True), 4),
]


def tier_a_sgd(n, seed, steps):
    """p and one gradient per step: multiples of 2^-6 in [-1, 1]."""
    gen = torch.Generator().manual_seed(seed)
    return dyadic(n, gen), [dyadic(n, gen) for _ in range(steps)]


_TA = dict(lr=2.0 ** -5, betas=(0.5, 0.75))
TIER_A_ADAM = [  # (name, hp, update as a multiple of sign(g))
    ("pow2", dict(_TA, eps=0.0), 2.0 ** -5),
    ("pow2_max", dict(_TA, eps=0.0, maximize=True), -2.0 ** -5),
    ("eps1", dict(_TA, eps=1.0), 2.0 ** -6),
    ("pow2_w", dict(_TA, eps=0.0, weight_decay=2.0 ** -3, decoupled=True), 2.0 ** -5),
    ("eps1_w", dict(_TA, eps=1.0, weight_decay=2.0 ** -3, decoupled=True), 2.0 ** -6),
]


def tier_a_adam(name, n, seed):
    """Adam / AdamW at t = 1 with b1 = 1/2, b2 = 3/4, lr = 2^-5, p dyadic: m = g / 2 and v = g^2 / 4 with bias
    corrections 1/2 and sqrt(1/4), so sqrt(v) / bc2 = |g| and step_size = 2^-4.  g = +-2^k (k in [-10, 10]) with
    eps = 0: the update is lr sign(g).  |g| = 1 with eps = 1: denom = 2 and the update is lr / 2 sign(g) (eps
    added before the division by bc2 would give denom = 3 and lr / 3).  AdamW with wd = 2^-3 first multiplies
    p by 1 - 2^-8, exact on multiples of 2^-6 in [-1, 1]."""
    gen = torch.Generator().manual_seed(seed)
    p = dyadic(n, gen)
    sign = torch.randint(0, 2, (n,), generator=gen).float() * 2.0 - 1.0
    k = torch.randint(-10, 11, (n,), generator=gen).float() if name.startswith("pow2") else torch.zeros(n)
    return p, sign * torch.exp2(k)


# ------------------------------------------------------------------------------------------- the grid
BETAS = [(0.9, 0.999), (0.9, 0.95), (0.0, 0.999), (0.5, 1.0 - 2.0 ** -10), (0.9, 0.0)]
ADAM_T = [1, 2, 3, 10, 1000, 100000]
SGD_T = [1, 2, 3]


def adam_grid():
    """betas x eps x (no decay, coupled 0.1, decoupled 0.1) x maximize: 60 rows."""
    rows = []
    for betas, eps, (wd, dec), mx in itertools.product(BETAS, [1e-8, 1e-3], [(0.0, False), (0.1, False), (0.1, True)],
                                                       [False, True]):
        rows.append(dict(lr=1e-3, betas=betas, eps=eps, weight_decay=wd, decoupled=dec, maximize=mx))
    return rows


def sgd_grid():
    """(momentum 0 | momentum x dampening | Nesterov) x wd x maximize: 54 rows."""
    kinds = [dict(momentum=0.0)]
    for mom in (0.5, 0.9):
        kinds += [dict(momentum=mom, dampening=d) for d in (0.0, 0.25, 0.5)] + [dict(momentum=mom, nesterov=True)]
    rows = []
    for kind, wd, mx in itertools.product(kinds, [0.0, 1e-4, 2.0 ** -4], [False, True]):
        rows.append(dict(SGD_DEFAULTS, lr=0.05, weight_decay=wd, maximize=mx, **kind))
    return rows


ADAM_GRID = adam_grid()
SGD_GRID = sgd_grid()
POW_PAIRS = sorted({(_r32(b), t) for betas in BETAS for b in betas for t in ADAM_T})


def pow_ulp_error(b32, t32, got32):
    """ulp error of fp32 pow results ``got32`` for fp32 inputs (tensors) against fp64."""
    want = b32.double().cpu() ** t32.double().cpu()
    ulp = torch.from_numpy(np.spacing(want.float().numpy().astype(np.float32))).double().abs()
    return ((got32.double().cpu() - want).abs() / ulp)
