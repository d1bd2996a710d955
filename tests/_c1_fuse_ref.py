"""CPU fp64 references and error budgets for tests/test_c1_fuse_gpu.py (the next block's conv1 formed inside
conv3's streaming pass, pwconv.hip's C1 variant).

h1 = out W1^T over bf16 operands (products exact in fp32), K = 256 fp32 additions in some order, one rounding to
bf16: |h1 - exact| <= U |exact| + (K + 5) u32 sum_k |out||W1|, the budget tests/_gemm_ref.py gives a bf16 GEMM
output with one split (U = 2^-8: one bf16 rounding; the fp32 term counts K additions and the slack of 5 roundings
that file uses).

BatchNorm-forward sums of the stored h1 over M rows, fp32 partial sums in some order:
|sum - exact| <= (M + 1) u32 sum |terms| (the form the fused-BN tests use), with terms h1 and h1^2.
"""
import torch

U = 2.0 ** -8
u32 = 2.0 ** -24
FLOOR = 1e-30  # added to every bound: exact zeros compare cleanly


def h1_ref(out, w1):
    """(exact h1, per-element bound) from the STORED bf16 block output [M, 256] and the bf16 W1 [C1, 256]."""
    o, w = out.detach().cpu().double(), w1.detach().cpu().double()
    K = o.shape[1]
    y = o @ w.t()
    mag = o.abs() @ w.abs().t()
    return y, U * y.abs() + (K + 5) * u32 * mag + FLOOR


def stats_ref(h1):
    """(sums [2, C1], bounds [2, C1]) of the stored bf16 h1 [M, C1]: sum and sum of squares per channel."""
    h = h1.detach().cpu().double()
    M = h.shape[0]
    s, ss = h.sum(0), (h * h).sum(0)
    return torch.stack([s, ss]), torch.stack([(M + 1) * u32 * h.abs().sum(0) + FLOOR, (M + 1) * u32 * ss + FLOOR])
