"""fp64 references for the depthwise 7x7 kernels, computed from the bf16-rounded operands, with the absolute-value
sums their rounding budgets need.  One case per (shape, kind), computed once and shared."""
import functools

import torch
import torch.nn.functional as F

SHAPES = [(1, 7, 7, 8), (2, 5, 9, 16), (1, 9, 70, 8), (2, 30, 14, 40), (3, 16, 20, 96), (1, 14, 14, 384), (2, 56, 56, 96)]


def _bf(t):
    return t.to(torch.bfloat16).float()


def _conv(x, w, b=None):  # NHWC x, [C, 1, 7, 7] w, all fp64
    return F.conv2d(x.permute(0, 3, 1, 2), w, b, padding=3, groups=w.shape[0]).permute(0, 2, 3, 1)


@functools.lru_cache(maxsize=None)
def case(shape, exact: bool):
    """x is fp32 (full mantissa in the randn case: the fp32 arm rounds it, the bf16 arm gets ``_bf(x)``); w, b, dy are
    bf16-representable / fp32.  Every reference is of ``_bf(x)``."""
    N, H, W, C = shape
    g = torch.Generator().manual_seed(1000 + sum(shape))
    if exact:
        x = torch.randint(-2, 3, shape, generator=g).float()
        w = torch.randint(-1, 2, (C, 1, 7, 7), generator=g).float()
        b = torch.randint(-3, 4, (C,), generator=g).float()
        dy = torch.randint(-2, 3, shape, generator=g).float()
    else:
        x = torch.randn(shape, generator=g)
        w = _bf(torch.randn((C, 1, 7, 7), generator=g) * 0.2)
        b = torch.randn((C,), generator=g)
        dy = _bf(torch.randn(shape, generator=g))
    xd = _bf(x).double().requires_grad_()
    wd, bd = w.double().requires_grad_(), b.double().requires_grad_()
    y = _conv(xd, wd, bd)
    dx, dw, db = torch.autograd.grad(y, (xd, wd, bd), dy.double())
    xa, wa, dya = xd.detach().abs().requires_grad_(), wd.detach().abs().requires_grad_(), dy.double().abs()
    ya = _conv(xa, wa)
    s_dx, s_dw = torch.autograd.grad(ya, (xa, wa), dya)
    return dict(x=x, w=w, b=b, dy=dy, y=y.detach(), dx=dx, dw=dw, db=db, s_y=ya.detach() + b.double().abs(), s_dx=s_dx,
                s_dw=s_dw, s_db=dya.sum(dim=(0, 1, 2)))


def rows_bound(r, s):  # one bf16 RNE of the result + 50 fp32 roundings of the FMA chain and the bias add
    return 2.0 ** -8 * r.abs() + 50 * 2.0 ** -24 * s + 1e-30


def wgrad_bound(shape, s):  # any-order fp32 summation of exact products
    N, H, W, _ = shape
    return (N * H * W + 8) * 2.0 ** -24 * s
