"""Independent fp64 reference of optim.LARS and optim.LAMB (imported by the trust-ratio tests): a plain
per-tensor loop over fp64 copies, straight from the definitions.  Clipping is
``torch.nn.utils.clip_grad_norm_`` on the fp64 gradients.

    ref = TrustRef("lars" | "lamb", groups)      # groups: [{"params": [fp32 tensors], <hyper-parameters>}, ...]
    ref.step(grads, max_norm=None)               # grads: one tensor per parameter, in group order
    ref.params / ref.state[i] / ref.stats        # fp64; stats rows (wn, gn or un, ratio) of the last step
"""
import math

import torch

LARS_DEFAULTS = dict(momentum=0.9, dampening=0.0, weight_decay=0.0, nesterov=False, trust_coefficient=1e-3,
                     trust_eps=1e-8, maximize=False)
LAMB_DEFAULTS = dict(betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, trust_ratio=True, maximize=False)


class TrustRef:
    def __init__(self, kind, groups, **defaults):
        assert kind in ("lars", "lamb")
        self.kind = kind
        base = dict(LARS_DEFAULTS if kind == "lars" else LAMB_DEFAULTS)
        base.update(defaults)
        self.groups = []
        self.params = []
        for g in groups:
            hp = dict(base)
            hp.update({k: v for k, v in g.items() if k != "params"})
            idx = []
            for p in g["params"]:
                idx.append(len(self.params))
                self.params.append(p.detach().double().cpu().clone())
            self.groups.append((hp, idx))
        self.state = [dict() for _ in self.params]
        self.stats = None

    def step(self, grads, max_norm=None):
        """One step; returns the total gradient norm (before clipping) when ``max_norm`` is given."""
        gs = [g.detach().double().cpu().clone() for g in grads]
        norm = None
        if max_norm is not None:
            holders = [torch.zeros_like(g).requires_grad_(True) for g in gs]
            for h, g in zip(holders, gs):
                h.grad = g
            norm = torch.nn.utils.clip_grad_norm_(holders, max_norm)
            gs = [h.grad for h in holders]
        stats = [None] * len(self.params)
        for hp, idx in self.groups:
            for i in idx:
                w, st = self.params[i], self.state[i]
                g = -gs[i] if hp["maximize"] else gs[i]
                stats[i] = self._lars(w, g, st, hp) if self.kind == "lars" else self._lamb(w, g, st, hp)
        self.stats = torch.tensor(stats, dtype=torch.float64)
        return norm

    @staticmethod
    def _lars(w, g, st, hp):
        wn, gn = w.norm().item(), g.norm().item()
        wd, tc = hp["weight_decay"], hp["trust_coefficient"]
        ratio = tc * wn / (gn + wd * wn + hp["trust_eps"]) if (tc > 0 and wn > 0 and gn > 0) else 1.0
        d = ratio * (g + wd * w)
        mom = hp["momentum"]
        if mom != 0:
            if "momentum_buffer" not in st:
                st["momentum_buffer"] = d.clone()
            else:
                st["momentum_buffer"] = mom * st["momentum_buffer"] + (1.0 - hp["dampening"]) * d
            b = st["momentum_buffer"]
            d = d + mom * b if hp["nesterov"] else b
        st["step"] = st.get("step", 0) + 1
        w -= hp["lr"] * d
        return [wn, gn, ratio]

    @staticmethod
    def _lamb(w, g, st, hp):
        if "exp_avg" not in st:
            st["exp_avg"], st["exp_avg_sq"], st["step"] = torch.zeros_like(w), torch.zeros_like(w), 0
        st["step"] += 1
        t = st["step"]
        b1, b2 = hp["betas"]
        st["exp_avg"] = st["exp_avg"] + (1.0 - b1) * (g - st["exp_avg"])
        st["exp_avg_sq"] = b2 * st["exp_avg_sq"] + (1.0 - b2) * g * g
        u = (st["exp_avg"] / (1.0 - b1 ** t)) / (torch.sqrt(st["exp_avg_sq"] / (1.0 - b2 ** t)) + hp["eps"])
        u = u + hp["weight_decay"] * w
        wn, un = w.norm().item(), u.norm().item()
        ratio = wn / un if (hp["trust_ratio"] and wn > 0 and un > 0) else 1.0
        w -= hp["lr"] * ratio * u
        return [wn, un, ratio]


def assert_matches(ours, ours_params, ref, rtol=1e-5, atol=1e-6, equal_nan=False):
    """Parameters and every state tensor of ``ours`` against the fp64 reference, at the project's optimizer
    tolerance; the step counters exactly."""
    for i, p in enumerate(ours_params):
        a, b = p.detach().double().cpu(), ref.params[i]
        assert torch.allclose(a, b, rtol=rtol, atol=atol, equal_nan=equal_nan), \
            f"param {i}: max abs diff {(a - b).abs().max().item():.3e}"
        st = ours.state[p]
        for k in ("momentum_buffer", "exp_avg", "exp_avg_sq"):
            if k in ref.state[i]:
                a, b = st[k].detach().double().cpu(), ref.state[i][k]
                assert torch.allclose(a, b, rtol=rtol, atol=atol, equal_nan=equal_nan), \
                    f"{k} of param {i}: max abs diff {(a - b).abs().max().item():.3e}"
        if "step" in ref.state[i]:
            assert float(st["step"]) == float(ref.state[i]["step"]), f"step of param {i}"


def assert_stats(stats, ref, rel=1e-5):
    """trust_stats norms within ``rel`` of fp64 (the bound derived in test_grad_clip_gpu.py
    test_norm_accuracy_and_determinism: the same summation shape), the ratio with them."""
    got = stats.detach().double().cpu()
    for i in range(got.shape[0]):
        for c in range(3):
            a, b = got[i, c].item(), ref.stats[i, c].item()
            if b == 0.0 or not math.isfinite(b):
                assert a == b or (math.isnan(a) and math.isnan(b)), (i, c, a, b)
            else:
                # the ratio is a quotient of two such norms (plus an fp32 rounding or two)
                assert abs(a - b) <= (rel if c < 2 else 3 * rel) * abs(b), (i, c, a, b)
