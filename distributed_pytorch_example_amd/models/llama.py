"""Llama-style decoder (TinyLlama-1.1B: 1,100,048,384 parameters; Llama-3.2-1B has the same 32 x 64 head shape).

Pre-norm transformer with RMSNorm, rotary position embedding on grouped-query attention (head dim 64) and a SwiGLU
MLP, no biases, untied LM head by default.  On the GPU every step of a block is a gfx950 kernel:

* residual stream in fp32; RMSNorm (csrc/kernels/llama.hip) reads it and emits bf16 for the GEMMs;
* ``c_attn`` writes [B, T, Hq + 2 Hkv, 64] -- the query heads, then the key heads, then the value heads -- which the
  RoPE kernel rotates in place and the GQA flash-attention kernels (attn.hip) read as it lies;
* ``c_fc`` is the row-concatenated [gate_proj; up_proj]: one GEMM, then the SwiGLU kernel;
* both out-projections add into the residual stream in the GEMM epilogue (Fx.linear_residual);
* packed documents: Fx.doc_bounds once per batch gives the attention its bounds and RoPE its positions, which
  restart at every document.

Per-op autograd; there is no hand-scheduled fused block.

Generation (``generate``, the host loop of models/_generation.py): the prefill runs the padded prompts through the ops
above and writes each layer's rotated K heads and its V heads into a KVCache of n_kv_head heads; a decode step is
RMSNorm -> Fx.linear_skinny(c_attn) -> Fx.attn_decode_gqa (csrc/kernels/decode_gqa.hip: the G query heads of a KV head
in one workgroup on the matrix unit, the rotation of the step's q and k and the cache store fused in) ->
linear_skinny(attn_proj, residual) -> RMSNorm -> linear_skinny(c_fc) -> Fx.swiglu -> linear_skinny(mlp_proj,
residual), then ln_f and the LM head; nothing syncs per token and the step replays from a HIP graph.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch
import torch.nn as nn

from ..ops import functional as Fx
from ..ops.layers import Linear, RMSNorm
from ._generation import GenerationMixin

HEAD_DIM = 64


@dataclass
class LlamaConfig:
    n_layer: int
    n_head: int
    n_kv_head: int
    n_embd: int
    ffn_dim: int
    vocab_size: int = 32000
    block_size: int = 2048
    rope_theta: float = 10000.0
    rms_eps: float = 1e-5
    tie_embeddings: bool = False
    label_smoothing: float = 0.0  # training-loss regularisers, inside the fused LM-head CE (Fx.lm_head_ce)
    z_loss: float = 0.0
    sliding_window: int = 0  # W >= 1: every layer's query i attends the keys i - W + 1 .. i only (0 = all of 0 .. i)

    @classmethod
    def tiny(cls, **kw):
        base = dict(vocab_size=512, block_size=128, n_layer=2, n_head=4, n_kv_head=2, n_embd=256, ffn_dim=704)
        base.update(kw)
        return cls(**base)

    @classmethod
    def tinyllama_1_1b(cls, **kw):
        base = dict(n_layer=22, n_head=32, n_kv_head=4, n_embd=2048, ffn_dim=5632)
        base.update(kw)
        return cls(**base)


class LlamaBlock(nn.Module):
    def __init__(self, cfg: LlamaConfig):
        super().__init__()
        d = cfg.n_embd
        self.n_head, self.n_kv_head = cfg.n_head, cfg.n_kv_head
        self.window = cfg.sliding_window or None
        self.ln_1 = RMSNorm(d, cfg.rms_eps)
        self.c_attn = Linear(d, (cfg.n_head + 2 * cfg.n_kv_head) * HEAD_DIM, bias=False)  # rows: Q heads, K heads, V heads
        self.attn_proj = Linear(cfg.n_head * HEAD_DIM, d, bias=False)
        self.ln_2 = RMSNorm(d, cfg.rms_eps)
        self.c_fc = Linear(d, 2 * cfg.ffn_dim, bias=False)  # rows: gate_proj, then up_proj
        self.mlp_proj = Linear(cfg.ffn_dim, d, bias=False)
        # each is written by one weight-grad GEMM that honours grad_fresh (ops/_state.py)
        for lin in (self.c_attn, self.attn_proj, self.c_fc, self.mlp_proj):
            lin.weight._dpe_overwrite_ok = True
        # optim.Muon orthogonalises gate_proj and up_proj separately; c_attn's Q / K / V blocks are unequal, it stays whole
        self.c_fc.weight._dpe_muon_split = 2

    def forward(self, x, table, doc=None):
        """``table``: Fx.rope_table's (cos, sin); ``doc``: Fx.doc_bounds' (doc_start, doc_end, pos) or None."""
        qkv = self.c_attn(self.ln_1(x))
        qkv = Fx.rope(qkv, self.n_head, self.n_kv_head, table, None if doc is None else doc[2], inplace=True)
        a = Fx.causal_attention(qkv, self.n_head, doc, n_kv_head=self.n_kv_head, window=self.window)
        x = Fx.linear_residual(a, self.attn_proj.weight, None, x)
        u = Fx.swiglu(self.c_fc(self.ln_2(x)))
        return Fx.linear_residual(u, self.mlp_proj.weight, None, x)


class Llama(GenerationMixin, nn.Module):
    def __init__(self, cfg: LlamaConfig):
        super().__init__()
        if cfg.n_kv_head < 1 or cfg.n_head % cfg.n_kv_head:
            raise ValueError(f"n_head ({cfg.n_head}) must be a multiple of n_kv_head ({cfg.n_kv_head})")
        if cfg.sliding_window < 0:
            raise ValueError(f"sliding_window must be >= 1 (0 = none), got {cfg.sliding_window}")
        if cfg.n_embd != cfg.n_head * HEAD_DIM:
            raise ValueError(f"n_embd ({cfg.n_embd}) must be n_head * {HEAD_DIM}")
        self.cfg = cfg
        self.wte = nn.Parameter(torch.empty(cfg.vocab_size, cfg.n_embd))
        self.h = nn.ModuleList([LlamaBlock(cfg) for _ in range(cfg.n_layer)])
        self.ln_f = RMSNorm(cfg.n_embd, cfg.rms_eps)
        self.lm_head = None if cfg.tie_embeddings else Linear(cfg.n_embd, cfg.vocab_size, bias=False)
        head = self.head_weight()
        head._dpe_overwrite_ok = True  # the LM-head weight grad is its first writer (a tied wte: the embedding adds after it)
        self.wte._dpe_muon = head._dpe_muon = False  # build_optimizer("muon") keeps the embedding and the head on AdamW
        cos, sin = Fx.rope_table(cfg.block_size, cfg.rope_theta)
        self.register_buffer("rope_cos", cos, persistent=False)
        self.register_buffer("rope_sin", sin, persistent=False)
        self._init()

    def head_weight(self):
        return self.wte if self.lm_head is None else self.lm_head.weight

    def _init(self):
        # N(0, 0.02); the residual projections scaled by 1/sqrt(2 * n_layer), as models/gpt2.py
        std = 0.02
        with torch.no_grad():
            self.wte.normal_(0, std)
            if self.lm_head is not None:
                self.lm_head.weight.normal_(0, std)
            for blk in self.h:
                for lin in (blk.c_attn, blk.c_fc):
                    lin.weight.normal_(0, std)
                for lin in (blk.attn_proj, blk.mlp_proj):
                    lin.weight.normal_(0, std / math.sqrt(2 * self.cfg.n_layer))

    def forward(self, idx, targets=None, doc_start=None):
        """Logits [B, T, V(p)], or -- with ``targets`` -- the mean next-token cross-entropy through the fused LM-head +
        CE op.  ``doc_start`` [B, T] (see Fx.doc_bounds): the rows hold packed documents; attention stays inside
        each and the rotary positions restart at its first token."""
        B, T = idx.shape
        assert T <= self.cfg.block_size, "sequence longer than block_size"
        doc = None
        if doc_start is not None:
            assert doc_start.shape == idx.shape, "doc_start must have idx's shape"
            doc = Fx.doc_bounds(doc_start)  # once per batch, shared by every layer
        table = (self.rope_cos, self.rope_sin)
        x = Fx.embedding(idx, self.wte, None)
        for blk in self.h:
            x = blk(x, table, doc)
        x = self.ln_f(x)
        if targets is not None:
            return Fx.lm_head_ce(x, self.head_weight(), targets, label_smoothing=self.cfg.label_smoothing,
                                 z_loss=self.cfg.z_loss)
        return Fx.lm_head(x, self.head_weight())

    def num_params(self) -> int:
        return sum(p.numel() for p in self.parameters())

    # ------------------------------------------------------------ generation
    # generate(), its host loop and the HIP-graph replay: _generation.GenerationMixin
    def _cache_heads(self) -> int:
        return self.cfg.n_kv_head

    def _head(self, h):
        """Logits [B, V(p)] of the LM head for h [B, D] (after ln_f)."""
        V = self.cfg.vocab_size
        if self.decode_skinny:
            return Fx.linear_skinny(h, self.head_weight(), pad_rows=((V + 63) // 64 * 64 - V) if h.is_cuda else 0)
        return Fx.lm_head(h, self.head_weight())

    def _prefill(self, idx, lens, cache):
        """The padded prompts [B, T] through the training ops; every layer's rotated K heads and its V heads go into
        the cache head-major, and the LM head runs on row lens[b] - 1 of every sequence only.  Returns logits [B, V(p)]."""
        B, T = idx.shape
        Hq, Hkv = self.cfg.n_head, self.cfg.n_kv_head
        table = (self.rope_cos, self.rope_sin)
        x = Fx.embedding(idx, self.wte, None)
        for l, blk in enumerate(self.h):
            qkv = Fx.rope(blk.c_attn(blk.ln_1(x)), Hq, Hkv, table, inplace=True)
            kv = qkv.view(B, T, Hq + 2 * Hkv, -1)
            cache.buf[l, 0, :, :, :T] = kv[:, :, Hq:Hq + Hkv].transpose(1, 2)
            cache.buf[l, 1, :, :, :T] = kv[:, :, Hq + Hkv:].transpose(1, 2)
            a = Fx.causal_attention(qkv, Hq, n_kv_head=Hkv, window=blk.window)
            x = Fx.linear_residual(a, blk.attn_proj.weight, None, x)
            x = Fx.linear_residual(Fx.swiglu(blk.c_fc(blk.ln_2(x))), blk.mlp_proj.weight, None, x)
        last = x[torch.arange(B, device=x.device), lens.long() - 1]  # [B, D]
        return self._head(self.ln_f(last.unsqueeze(1)).squeeze(1))

    def _decode_step(self, tok, cache):
        """One token per row through the cache: tok int64 [B] at position cache.len -> logits [B, V(p)].  The position
        (the table row of the rotation, the cache row) is read from cache.len on the device by Fx.attn_decode_gqa;
        cache.len is not advanced here and nothing syncs."""
        B = tok.shape[0]
        Hq, Hkv = self.cfg.n_head, self.cfg.n_kv_head
        table = (self.rope_cos, self.rope_sin)
        x = Fx.embedding(tok.view(B, 1), self.wte, None).view(B, -1)  # fp32 [B, D]
        for l, blk in enumerate(self.h):
            qkv = self._proj(blk.ln_1(x), blk.c_attn)
            a = Fx.attn_decode_gqa(qkv, cache.buf[l, 0], cache.buf[l, 1], cache.len, Hq, Hkv, table, window=blk.window or 0)
            x = self._proj(a, blk.attn_proj, residual=x)
            u = Fx.swiglu(self._proj(blk.ln_2(x), blk.c_fc))
            x = self._proj(u, blk.mlp_proj, residual=x)
        return self._head(self.ln_f(x))
