#!/usr/bin/env python3
"""P = dz3^T a2 formed by the conv1 data grad's epilogue (DPE_PW_FUSED_P) against the same data grad followed by
the deterministic weight grad over the stored dz3, at the ResNet-50 shapes that take it (batch 512): layer1.0/1.1
(64 -> 256 at 56 x 56, 64 columns), layer1.2 (128 -> 256 at 56 x 56 with the stride-2 compact residual, 64 columns)
and layer2.1/2.2 (128 -> 512 at 28 x 28, 128 columns).  HIP events around 20 back-to-back calls after 3 warm-ups."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from distributed_pytorch_example_amd.ops._ext import ext

X = ext()
DEV = "cuda"
Z = ([1, 1], [0, 0], [1, 1])


def t(fn):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000 / 20


for name, K, N, K2, H, s2 in (("layer1.0/1.1", 64, 256, 64, 56, False), ("layer1.2", 128, 256, 64, 56, True),
                              ("layer2.1/2.2", 128, 512, 128, 28, False)):
    B = 512
    g = torch.Generator(device=DEV).manual_seed(0)
    dy = torch.randn(B, H, H, K, device=DEV, generator=g).bfloat16()
    w = (torch.randn(K, 1, 1, N, device=DEV, generator=g) * K ** -0.5).bfloat16()
    res = torch.randn(B, H // 2 if s2 else H, H // 2 if s2 else H, N, device=DEV, generator=g).bfloat16()
    bits = torch.randint(0, 256, (B, H, H, N // 8), device=DEV, generator=g, dtype=torch.uint8)
    h2 = torch.randn(B, H, H, K2, device=DEV, generator=g).bfloat16()
    c2 = torch.stack([torch.ones(K2, device=DEV), 0.1 * torch.ones(K2, device=DEV), torch.zeros(K2, device=DEV),
                      torch.ones(K2, device=DEV)]).contiguous()
    P = torch.empty(N, 1, 1, K2, device=DEV)
    xs = [B, H, H, N]
    dg = lambda **kw: X.conv_dgrad_bn(dy, w, xs, *Z, res, None, None, None, None, s2, bits, **kw)
    dx = dg()[0]
    t_dg = t(dg)
    t_wg = t(lambda: X.conv_wgrad(dx, h2, P, *Z, 1.0, c2, deterministic=True, overwrite=True))
    t_f = t(lambda: dg(p_src=h2, p_coef=c2))
    print(f"{name:14s} K={K:3d} N={N:3d} K2={K2:3d}: data grad {t_dg:7.1f} us + weight grad {t_wg:7.1f} us = "
          f"{t_dg + t_wg:7.1f} us;  fused (data grad with P + slab sum) {t_f:7.1f} us;  saved {t_dg + t_wg - t_f:7.1f} us",
          flush=True)
