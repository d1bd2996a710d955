#!/usr/bin/env python3
"""The junction between two layer-1 bottlenecks at ResNet-50's shape (batch 512, 56 x 56): today's conv3 pass
(conv1x1_apply, 64 -> 256, writes the block output) + the next block's conv1 (conv_fwd, 256 -> 64 or 128, reads it
back) against the one pass that forms both (DPE_C1_FUSE: conv1x1_apply_next), with the share of the 6 TB/s byte
bound (operands read once, results written once) each pass reaches.  HIP events around 20 back-to-back calls after
3 warm-ups."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from distributed_pytorch_example_amd.ops._ext import ext

X = ext()
DEV = "cuda"
N, H, C, Cout = 512, 56, 64, 256
M = N * H * H
g = torch.Generator(device=DEV).manual_seed(0)
x = torch.randn(N, H, H, Cout, device=DEV, generator=g).abs().bfloat16()
h2 = torch.randn(N, H, H, C, device=DEV, generator=g).bfloat16()
w3 = (torch.randn(Cout, 1, 1, C, device=DEV, generator=g) * C ** -0.5).bfloat16()
gamma = torch.ones(Cout, device=DEV); beta = torch.zeros(Cout, device=DEV)
c2 = torch.stack([torch.ones(C, device=DEV), torch.zeros(C, device=DEV), torch.zeros(C, device=DEV), torch.ones(C, device=DEV)])
CONF = ([1, 1], [0, 0], [1, 1])

def t(name, fn, nbytes=None):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20): fn()
    e1.record(); torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1000 / 20
    extra = f"  {nbytes / us / 1e6:.2f} TB/s = {100 * nbytes / 6.0e12 / (us * 1e-6):.0f} % of the 6 TB/s byte bound" if nbytes else ""
    print(f"{name:58s} {us:8.1f} us{extra}", flush=True)
    return us

T = lambda m, c: m * c * 2
G, sv = X.bn_gram(h2, c2, c2)
c3, _ = X.bn_gram_coef(G, sv, w3, M, gamma, beta, None, None, 0.1, 1e-5)
apply_bytes = T(M, C) + 2 * T(M, Cout) + M * Cout // 8
for c1 in (64, 128):
    w1 = (torch.randn(c1, 1, 1, Cout, device=DEV, generator=g) * Cout ** -0.5).bfloat16()
    print(f"--- 256 -> {c1}: today's two calls")
    out, bits = X.conv1x1_apply(h2, w3, c2, c3, x, None)
    old = t("conv1x1_apply(h2, W3, c2, c3, x)", lambda: X.conv1x1_apply(h2, w3, c2, c3, x, None), apply_bytes)
    old += t(f"conv_fwd(out, W1) + stats (256 -> {c1})", lambda: X.conv_fwd(out, w1, *CONF, True, None), T(M, Cout) + T(M, c1))
    print(f"{'sum':58s} {old:8.1f} us")
    print(f"--- 256 -> {c1}: one pass")
    if not X.c1_fuse_ok([N, H, H, C], Cout, c1):
        print("outside c1_fuse_ok's envelope")
        continue
    new = t("conv1x1_apply_next(h2, W3, c2, c3, x, W1)", lambda: X.conv1x1_apply_next(h2, w3, c2, c3, x, None, w1),
            apply_bytes + T(M, c1))
    print(f"{'sum':58s} {new:8.1f} us   ({new - old:+.1f} us)")
