#!/usr/bin/env python3
"""The downsample BN's backward at ResNet-50 layer1.0's shape (batch 512, 56 x 56, 64 -> 256): every op of the
Gram-algebra chain (DPE_BND_GRAM) and of the bn_bwd_partials + weight grad + accumulating data grad chain it
replaces, with the share of the 6 TB/s byte bound (scripts/sol_table.py's: operands read once, result written
once) each reaches.  HIP events around 20 back-to-back calls after 3 warm-ups."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from distributed_pytorch_example_amd.ops._ext import ext

X = ext()
DEV = "cuda"
N, H, Cin, Cout = 512, 56, 64, 256
M = N * H * H
g = torch.Generator(device=DEV).manual_seed(0)
x = torch.randn(N, H, H, Cin, device=DEV, generator=g).abs().bfloat16()
dz = torch.randn(N, H, H, Cout, device=DEV, generator=g).bfloat16()
w = (torch.randn(Cout, 1, 1, Cin, device=DEV, generator=g) * Cin ** -0.5).bfloat16()
gamma = torch.ones(Cout, device=DEV); beta = torch.zeros(Cout, device=DEV)
CONF = ([1, 1], [0, 0], [1, 1])
hd, st = X.conv_fwd(x, w, *CONF, True, None)
cd = X.bn_coef(st, M, gamma, beta, None, None, 0.1, 1e-5)
part = torch.zeros(2, Cout, 1, device=DEV)
part[0, :, 0] = dz.float().sum((0, 1, 2))
dg = torch.zeros(Cout, device=DEV); db = torch.zeros(Cout, device=DEV)
dw = torch.zeros(w.shape, dtype=torch.float32, device=DEV)
P = torch.empty(w.shape, dtype=torch.float32, device=DEV)
dh1 = torch.randn(N, H, H, 64, device=DEV, generator=g).bfloat16()
w1 = (torch.randn(64, 1, 1, Cin, device=DEV, generator=g) * 0.1).bfloat16()

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
pil = X.bn_gram_pilot(x)
G, s = X.bn_gram(x, None, pil)
u = X.bn_gram_u(G, w)
print("--- new path (forward additions)")
t("bn_gram_pilot(x)", lambda: X.bn_gram_pilot(x))
t("bn_gram(x) Gram pass + reduce", lambda: X.bn_gram(x, None, pil), T(M, Cin))
t("bn_gram_u", lambda: X.bn_gram_u(G, w))
print("--- new path (backward)")
t("P_d = conv_wgrad(dz3, x) deterministic", lambda: X.conv_wgrad(dz, x, P, *CONF, 1.0, None, deterministic=True, overwrite=True), T(M, Cout) + T(M, Cin))
bcat, e = X.bn_gram_bwd(part, P, w, u, s, cd, gamma, M, dg, db, dw)
t("bn_gram_bwd (3 small kernels)", lambda: X.bn_gram_bwd(part, P, w, u, s, cd, gamma, M, dg, db, dw))
t("conv1x1_dgrad_cat_plain [dz3 | x] -> dxd", lambda: X.conv1x1_dgrad_cat_plain(dz, x, bcat, e), T(M, Cout) + 2 * T(M, Cin))
dxd = X.conv1x1_dgrad_cat_plain(dz, x, bcat, e)
t("conv1 dgrad 64->64 + residual dxd", lambda: X.conv_dgrad(dh1, w1, list(x.shape), *CONF, dxd), 3 * T(M, Cin))
print("--- today's path (backward)")
part2 = torch.zeros(2, Cout, 1, device=DEV); part2[0] = part[0]
t("bn_bwd_partials(dz3, hd) apply pass", lambda: X.bn_bwd_partials(dz, hd, gamma, cd, part2, dg, db, relu_mask=False), 3 * T(M, Cout))
dhd = X.bn_bwd_partials(dz, hd, gamma, cd, part2, dg, db, relu_mask=False)
t("conv_wgrad(dhd, x)", lambda: X.conv_wgrad(dhd, x, dw, *CONF, 1.0, None), T(M, Cout) + T(M, Cin))
t("conv1 dgrad 64->64", lambda: X.conv_dgrad(dh1, w1, list(x.shape), *CONF), 2 * T(M, Cin))
dx = X.conv_dgrad(dh1, w1, list(x.shape), *CONF)
t("conv_dgrad_acc(dhd, W_d, dx)", lambda: X.conv_dgrad_acc(dhd, w, dx, *CONF), T(M, Cout) + 2 * T(M, Cin))
