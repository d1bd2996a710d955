#!/usr/bin/env python3
"""The downsample branch's forward at ResNet-50 layer1.0's shape (batch 512, 56 x 56, 64 -> 256): today's downsample
conv + bn_coef + conv3 (conv1x1_apply reading hd) against the coefficient kernels + the fused concatenated-K pass
(DPE_DOWN_CAT: bn_gram_coef + conv1x1_apply_cat), with the share of the 6 TB/s byte bound (operands read once,
result written once) each streaming pass reaches.  HIP events around 20 back-to-back calls after 3 warm-ups."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from distributed_pytorch_example_amd.ops._ext import ext

X = ext()
DEV = "cuda"
N, H, C, Cout = 512, 56, 64, 256
M = N * H * H
g = torch.Generator(device=DEV).manual_seed(0)
x = torch.randn(N, H, H, C, device=DEV, generator=g).abs().bfloat16()
h2 = torch.randn(N, H, H, C, device=DEV, generator=g).bfloat16()
w3 = (torch.randn(Cout, 1, 1, C, device=DEV, generator=g) * C ** -0.5).bfloat16()
wd = (torch.randn(Cout, 1, 1, C, device=DEV, generator=g) * C ** -0.5).bfloat16()
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
pil = X.bn_gram_pilot(x)
Gx, sx = X.bn_gram(x, None, pil)
print("--- today's path")
hd, st = X.conv_fwd(x, wd, *CONF, True, None)
cd = X.bn_coef(st, M, gamma, beta, None, None, 0.1, 1e-5)
old = t("downsample conv_fwd(x, W_d) + stats", lambda: X.conv_fwd(x, wd, *CONF, True, None), T(M, C) + T(M, Cout))
old += t("bn_coef (bn_finalize)", lambda: X.bn_coef(st, M, gamma, beta, None, None, 0.1, 1e-5))
old += t("conv1x1_apply(h2, W3, c2, c3, hd, cd)", lambda: X.conv1x1_apply(h2, w3, c2, c3, hd, cd),
         T(M, C) + 2 * T(M, Cout) + M * Cout // 8)
old += t("bn_gram_u(G_x, W_d)", lambda: X.bn_gram_u(Gx, wd))
print(f"{'sum':58s} {old:8.1f} us")
print("--- fused path")
cdn, ud = X.bn_gram_coef(Gx, sx, wd, M, gamma, beta, None, None, 0.1, 1e-5)
new = t("bn_gram_coef(G_x, s_x, W_d) (u_d + coefficients)", lambda: X.bn_gram_coef(Gx, sx, wd, M, gamma, beta, None, None, 0.1, 1e-5))
new += t("conv1x1_apply_cat(h2, W3, c2, c3, x, W_d, cd)", lambda: X.conv1x1_apply_cat(h2, w3, c2, c3, x, wd, cdn),
         2 * T(M, C) + T(M, Cout) + M * Cout // 8)
print(f"{'sum':58s} {new:8.1f} us   ({new - old:+.1f} us)")
