"""ConvNeXt (Liu et al. 2022, the torchvision parameterisation): ConvNeXt-T has 28,589,128 parameters.

NHWC throughout, an fp32 residual stream [N, H, W, C]:

* stem: ``Fx.to_nhwc_input`` (channels padded to 8), a torch view into 4 x 4 patch rows, ``Fx.linear`` with the
  conv-layout filter [D, 3, 4, 4] re-laid as [D, (py, px, c)], then LayerNorm;
* block: ``Fx.depthwise_conv2d_nhwc`` (the 7x7 row-walking kernels, fp32 in, bf16 out), LayerNorm(eps 1e-6),
  ``Linear(C, 4C)`` + GELU, ``Linear(4C, C)`` with fp32 output, per-channel layer scale, residual;
* downsample: LayerNorm, a 2 x 2 space-to-depth view, ``Fx.linear`` with the filter [Dout, Din, 2, 2] re-laid alike;
* head: ``Fx.global_avg_pool_nhwc``, LayerNorm, Linear.

Layer scale, the residual add and the space-to-depth copies are torch ops (as the class-token assembly in vit.py);
there is no stochastic depth.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..ops import functional as Fx
from ..ops.layers import DepthwiseConv2d, LayerNorm, Linear


@dataclass
class ConvNeXtConfig:
    depths: Tuple[int, ...] = (3, 3, 9, 3)
    dims: Tuple[int, ...] = (96, 192, 384, 768)
    image_size: int = 224
    in_chans: int = 3
    num_classes: int = 1000
    layer_scale_init: float = 1e-6

    @classmethod
    def tiny_test(cls, **kw):
        base = dict(depths=(1, 1, 2, 1), dims=(8, 16, 32, 64), image_size=32, num_classes=10)
        base.update(kw)
        return cls(**base)


def _ln_rows(ln: LayerNorm, x):
    return ln(x.reshape(-1, x.shape[-1])).reshape(x.shape)


class PatchConv(nn.Module):
    """A k x k / stride k convolution (+ bias) as a GEMM over space-to-depth rows; filter in conv layout [D, C, k, k]."""

    def __init__(self, cin: int, cout: int, k: int):
        super().__init__()
        self.k = k
        self.weight = nn.Parameter(torch.empty(cout, cin, k, k))
        self.bias = nn.Parameter(torch.zeros(cout))

    def forward(self, x):
        """x [N, H, W, C'] with C' >= cin (zero-padded channels) -> [N, H/k, W/k, cout] fp32."""
        N, H, W, Cp = x.shape
        k, D = self.k, self.weight.shape[0]
        rows = x.reshape(N, H // k, k, W // k, k, Cp).permute(0, 1, 3, 2, 4, 5).reshape(-1, k * k * Cp)
        w = F.pad(self.weight.permute(0, 2, 3, 1), (0, Cp - self.weight.shape[1])).reshape(D, -1)
        return Fx.linear(rows, w, self.bias, out_f32=True).reshape(N, H // k, W // k, D)


class Block(nn.Module):
    def __init__(self, dim: int, layer_scale_init: float):
        super().__init__()
        self.dwconv = DepthwiseConv2d(dim)
        self.norm = LayerNorm(dim, eps=1e-6)
        self.fc1 = Linear(dim, 4 * dim, act=Fx.ACT_GELU)
        self.fc2 = Linear(4 * dim, dim, out_f32=True)
        self.gamma = nn.Parameter(torch.full((dim,), float(layer_scale_init)))

    def forward(self, x):
        h = self.dwconv(x)
        h = self.norm(h.reshape(-1, h.shape[-1]))
        h = self.fc2(self.fc1(h))
        return x + (self.gamma * h).reshape(x.shape)


class ConvNeXt(nn.Module):
    def __init__(self, cfg: ConvNeXtConfig = ConvNeXtConfig()):
        super().__init__()
        if len(cfg.depths) != len(cfg.dims):
            raise ValueError("depths and dims must have one entry per stage")
        if any(d % 8 for d in cfg.dims):
            raise ValueError("every stage width must be a multiple of 8 (the depthwise kernels' channel chunks)")
        down = 4 * 2 ** (len(cfg.dims) - 1)
        if cfg.image_size % down:
            raise ValueError(f"image_size {cfg.image_size} must be a multiple of {down}")
        self.cfg = cfg
        self.stem = PatchConv(cfg.in_chans, cfg.dims[0], 4)
        self.stem_norm = LayerNorm(cfg.dims[0], eps=1e-6)
        self.down_norms = nn.ModuleList([LayerNorm(d, eps=1e-6) for d in cfg.dims[:-1]])
        self.downs = nn.ModuleList([PatchConv(a, b, 2) for a, b in zip(cfg.dims[:-1], cfg.dims[1:])])
        self.stages = nn.ModuleList([nn.ModuleList([Block(d, cfg.layer_scale_init) for _ in range(n)])
                                     for d, n in zip(cfg.dims, cfg.depths)])
        self.head_norm = LayerNorm(cfg.dims[-1], eps=1e-6)
        self.head = Linear(cfg.dims[-1], cfg.num_classes)
        self.head.weight._dpe_muon = False  # build_optimizer("muon"): the classifier stays on AdamW
        self._init()

    def _init(self):
        # trunc-normal(0.02) weights, zero biases (the depthwise filters are initialised by their layer)
        with torch.no_grad():
            for m in self.modules():
                if isinstance(m, (Linear, PatchConv)):
                    nn.init.trunc_normal_(m.weight, std=0.02)
                    m.bias.zero_()

    def forward(self, x):
        """fp32 NCHW images [B, 3, S, S] -> logits [B, num_classes]."""
        cfg = self.cfg
        assert x.shape[1:] == (cfg.in_chans, cfg.image_size, cfg.image_size), "input must be [B, C, image_size, image_size]"
        h = _ln_rows(self.stem_norm, self.stem(Fx.to_nhwc_input(x))).float()
        for i, stage in enumerate(self.stages):
            if i:
                h = self.downs[i - 1](_ln_rows(self.down_norms[i - 1], h))
            for blk in stage:
                h = blk(h)
        h = Fx.global_avg_pool_nhwc(h.to(torch.bfloat16) if h.is_cuda else h)
        return self.head(self.head_norm(h))

    def num_params(self) -> int:
        return sum(p.numel() for p in self.parameters())
