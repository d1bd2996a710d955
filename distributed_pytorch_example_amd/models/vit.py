"""Vision Transformer (ViT / DeiT, the timm parameterisation): ViT-B/16 86,567,656 and ViT-S/16 22,050,664 parameters.

Pre-LN encoder on the GPT-2 blocks (models/gpt2.py ``Block``, fused or per-op) in their bidirectional attention mode:

* ``Fx.patchify`` packs the fp32 NCHW batch into bf16 patch rows ordered (c, py, px) in one kernel, so the
  patch-embedding filter [D, C, p, p] flattened is an ``Fx.linear`` weight;
* the fp32 residual stream is [B, Tp, D] with Tp = the N + 1 tokens (class token first) rounded up to whole 64-key
  tiles; the rows from N + 1 on are padding.  The attention kernels bound the visible keys by ``seq_len = N + 1`` and
  write zeros into the padding rows of their output and gradient; the GEMMs and LayerNorms compute the padding rows
  (23 % more rows at 197 tokens) and nothing reads them: the head sees row 0 only;
* ``ln_f`` and the classifier head run on the class-token row.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch
import torch.nn as nn

from ..ops import functional as Fx
from ..ops.layers import LayerNorm, Linear
from . import gpt2 as _gpt2


@dataclass
class ViTConfig:
    image_size: int = 224
    patch_size: int = 16
    in_chans: int = 3
    num_classes: int = 1000
    n_layer: int = 12
    n_head: int = 12
    n_embd: int = 768
    bias: bool = True  # (what Block reads; the timm models have every bias)

    @classmethod
    def tiny(cls, **kw):
        base = dict(image_size=32, patch_size=8, num_classes=10, n_layer=2, n_head=2, n_embd=128)
        base.update(kw)
        return cls(**base)

    @property
    def num_patches(self) -> int:
        return (self.image_size // self.patch_size) ** 2

    @property
    def seq_len(self) -> int:  # class token + patches
        return self.num_patches + 1

    @property
    def padded_len(self) -> int:  # whole 64-key tiles
        return (self.seq_len + 63) // 64 * 64


class PatchEmbed(nn.Module):
    """The patch-embedding filter in conv layout [D, C, p, p] (+ bias), applied as a GEMM over Fx.patchify's rows."""

    def __init__(self, cfg: ViTConfig):
        super().__init__()
        self.patch = cfg.patch_size
        self.weight = nn.Parameter(torch.empty(cfg.n_embd, cfg.in_chans, cfg.patch_size, cfg.patch_size))
        self.bias = nn.Parameter(torch.zeros(cfg.n_embd))

    def forward(self, x):
        # a fresh 2-D view every call: its bf16 shadow is cast from the master as it is now
        return Fx.linear(Fx.patchify(x, self.patch), self.weight.view(self.weight.shape[0], -1), self.bias)


class ViT(nn.Module):
    def __init__(self, cfg: ViTConfig = ViTConfig()):
        super().__init__()
        if cfg.image_size % cfg.patch_size:
            raise ValueError(f"patch_size {cfg.patch_size} must divide image_size {cfg.image_size}")
        self.cfg = cfg
        D = cfg.n_embd
        self.patch_embed = PatchEmbed(cfg)
        self.cls_token = nn.Parameter(torch.empty(1, 1, D))
        self.pos_embed = nn.Parameter(torch.empty(1, cfg.seq_len, D))
        self.blocks = nn.ModuleList([_gpt2.Block(cfg, seq_len=cfg.seq_len) for _ in range(cfg.n_layer)])
        for i, blk in enumerate(self.blocks):
            blk._dpe_layer = i  # the fused backward flushes deferred weight grads at layer 0 (end of backward)
        self.ln_f = LayerNorm(D)
        self.head = Linear(D, cfg.num_classes)
        # build_optimizer("muon") keeps these on AdamW (the 4-D patch filter stays there by its shape)
        self.pos_embed._dpe_muon = self.cls_token._dpe_muon = self.head.weight._dpe_muon = False
        self._init()

    def _init(self):
        # timm / DeiT: trunc-normal(0.02) for the weights, the class token and the positions; zero biases
        with torch.no_grad():
            for w in (self.patch_embed.weight, self.cls_token, self.pos_embed, self.head.weight):
                nn.init.trunc_normal_(w, std=0.02)
            self.patch_embed.bias.zero_()
            self.head.bias.zero_()
            for blk in self.blocks:
                for lin in (blk.c_attn, blk.attn_proj, blk.c_fc, blk.mlp_proj):
                    nn.init.trunc_normal_(lin.weight, std=0.02)
                    lin.bias.zero_()

    def forward(self, x):
        """fp32 NCHW images [B, C, S, S] -> logits [B, num_classes]."""
        cfg = self.cfg
        B = x.shape[0]
        assert x.shape[1:] == (cfg.in_chans, cfg.image_size, cfg.image_size), "input must be [B, C, image_size, image_size]"
        if _gpt2._FUSED and x.is_cuda:
            from ._gpt2_fused import reset_wgrad_queue

            reset_wgrad_queue()
        tok = self.patch_embed(x)  # [B, N, D]
        pos = self.pos_embed
        rows = [(self.cls_token + pos[:, :1]).expand(B, -1, -1), tok.float() + pos[:, 1:]]
        if cfg.padded_len > cfg.seq_len:
            rows.append(torch.zeros(B, cfg.padded_len - cfg.seq_len, cfg.n_embd, dtype=torch.float32, device=x.device))
        h = torch.cat(rows, dim=1)  # the fp32 residual stream [B, Tp, D]
        for blk in self.blocks:
            h = blk(h)
        h = self.ln_f(h)[:, 0]
        return self.head(h)

    def num_params(self) -> int:
        return sum(p.numel() for p in self.parameters())
