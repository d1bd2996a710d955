"""fp64 references of Muon (imported by test_muon_cpu.py and test_muon_gpu.py): plain torch in float64, straight
from the definition.  No kernel code and nothing of optim.Muon.

    ns_ref64(u)        the Newton-Schulz chain in fp64, no rounding
    ns_emulated(u)     the same chain with a bf16 rounding after the normalisation and after each of the three
                       products, the products themselves in fp64
    MuonRef            the optimizer in fp64, taking O from either of the two

For a wide block (rows <= cols): A = X X^T, B = b A + c A A, X = a X + B X.  A tall block takes the Gram matrix
of its short side: A = X^T X, X = a X + X B.  X0 = u / (|u|_F + 1e-7).
"""
import math

import torch

NS_COEFFICIENTS = (3.4445, -4.7750, 2.0315)


def _bf(x):
    """One rounding to bf16 (through fp32, whose 24 bits hold every tie of the 8-bit rounding), back in fp64."""
    return x.float().bfloat16().double()


def _ns(u, steps, coefficients, rnd):
    a, b, c = coefficients
    u = u.double()
    X = rnd(u / (u.norm() + 1e-7))
    tall = X.shape[0] > X.shape[1]
    for _ in range(steps):
        A = rnd(X.T @ X if tall else X @ X.T)
        B = rnd(b * A + c * (A @ A))
        X = rnd(a * X + (X @ B if tall else B @ X))
    return X


def ns_ref64(u, steps=5, coefficients=NS_COEFFICIENTS):
    return _ns(u, steps, coefficients, lambda x: x)


def ns_emulated(u, steps=5, coefficients=NS_COEFFICIENTS):
    return _ns(u, steps, coefficients, _bf)


def ns_blocks(fn, u, split=1, steps=5, coefficients=NS_COEFFICIENTS):
    """``fn`` on each of the ``split`` equal row blocks of u."""
    rows = u.shape[0] // split
    return torch.cat([fn(u[i * rows:(i + 1) * rows], steps, coefficients) for i in range(split)])


def gamma(scale, rows, cols):
    return 0.2 * math.sqrt(max(rows, cols)) if scale == "match_rms" else math.sqrt(max(1.0, rows / cols))


class MuonRef:
    """Muon on fp64 copies of ``params`` (2-D tensors): ``step(grads)`` takes this step's gradients and returns, per
    parameter, (u, O) in fp64.  ``w`` and ``buf`` are the fp64 weights and momentum buffers."""

    def __init__(self, params, lr, weight_decay=0.0, momentum=0.95, nesterov=True, ns_steps=5,
                 ns_coefficients=NS_COEFFICIENTS, scale="match_rms", splits=None, ns=ns_ref64, maximize=False):
        self.w = [p.detach().double().cpu().clone() for p in params]
        self.buf = [torch.zeros_like(w) for w in self.w]
        self.lr, self.wd, self.mu, self.nesterov = lr, weight_decay, momentum, nesterov
        self.k, self.abc, self.scale, self.ns, self.maximize = ns_steps, ns_coefficients, scale, ns, maximize
        self.splits = list(splits) if splits is not None else [1] * len(self.w)

    def step(self, grads, lr=None, coef=1.0):
        lr = self.lr if lr is None else lr
        out = []
        for i, g in enumerate(grads):
            g = g.detach().double().cpu() * coef
            if self.maximize:
                g = -g
            self.buf[i] = self.buf[i] + (1.0 - self.mu) * (g - self.buf[i])
            u = g + self.mu * (self.buf[i] - g) if self.nesterov else self.buf[i]
            s = self.splits[i]
            O = ns_blocks(self.ns, u, s, self.k, self.abc)
            gm = gamma(self.scale, u.shape[0] // s, u.shape[1])
            self.w[i] = self.w[i] * (1.0 - lr * self.wd) - lr * gm * O
            out.append((u, O))
        return out
