"""GPT-2 (BASELINE.json config 4: GPT-2-small, 124,439,808 parameters, T=1024).

Pre-LN transformer with tied token embedding / LM head, GELU(tanh) MLP, causal
self-attention, LayerNorm with bias -- the standard GPT-2 definition (same
parameterisation as HF/nanoGPT ``GPT2``), executed on gfx950 kernels:

* residual stream kept in fp32; LayerNorm reads it and emits bf16 for the GEMMs;
* QKV projection writes [B, T, 3, H, 64] which the flash-attention kernel reads
  in place (no split / transpose copies); attention output feeds the
  out-projection directly;
* the out-projections add into the fp32 residual stream inside the GEMM
  epilogue (one launch for ``x + proj(a)``);
* the LM head is the tied wte (bf16 shadow padded to a multiple of 64 rows),
  bf16 logits feed the fused cross-entropy kernel which writes bf16 dlogits.
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass

import torch
import torch.nn as nn

from ..ops import functional as Fx
from ..ops.layers import LayerNorm, Linear

# DPE_GPT2_FUSED=0: per-op autograd graph for the blocks (A/B reference)
_FUSED = os.environ.get("DPE_GPT2_FUSED", "1") != "0"


@dataclass
class GPT2Config:
    vocab_size: int = 50257
    block_size: int = 1024
    n_layer: int = 12
    n_head: int = 12
    n_embd: int = 768
    dropout: float = 0.0
    bias: bool = True
    label_smoothing: float = 0.0  # training-loss regularisers, inside the fused LM-head CE (Fx.lm_head_ce)
    z_loss: float = 0.0

    @classmethod
    def tiny(cls, **kw):
        base = dict(vocab_size=512, block_size=128, n_layer=2, n_head=2, n_embd=128)
        base.update(kw)
        return cls(**base)


class Block(nn.Module):
    """``seq_len``: the attention mode.  None (the default) is causal attention; an integer L is bidirectional
    attention over the first L rows of a sequence padded to whole 64-key tiles (models/vit.py) -- the rows from L on
    are padding, and no dropout or packed documents go with it."""

    def __init__(self, cfg, seq_len=None):
        super().__init__()
        d = cfg.n_embd
        self.n_head = cfg.n_head
        self.seq_len = None if seq_len is None else int(seq_len)
        self.ln_1 = LayerNorm(d, bias=cfg.bias)
        self.c_attn = Linear(d, 3 * d, bias=cfg.bias)
        self.attn_proj = Linear(d, d, bias=cfg.bias)
        self.ln_2 = LayerNorm(d, bias=cfg.bias)
        self.c_fc = Linear(d, 4 * d, bias=cfg.bias)
        self.mlp_proj = Linear(4 * d, d, bias=cfg.bias)
        self.fused = _FUSED
        # every backward writes these through one weight-grad GEMM that honours grad_fresh (fused
        # and per-op paths alike): DDP may leave them out of the gradient re-zero (ops/_state.py)
        for lin in (self.c_attn, self.attn_proj, self.c_fc, self.mlp_proj):
            lin.weight._dpe_overwrite_ok = True
        self.c_attn.weight._dpe_muon_split = 3  # optim.Muon orthogonalises the Q, K and V row blocks separately

    def forward(self, x, doc=None, drop=None):
        """``doc``: the (doc_start, doc_end, pos) of Fx.doc_bounds for packed documents, None for one per row.
        ``drop``: None, or (p, rng, stream) for a training forward with dropout -- p the rate, rng the forward's
        DropoutState snapshot (None off the GPU), stream the layer's first call-site id (attention; + 1 the
        attention residual, + 2 the MLP residual)."""
        if self.seq_len is not None and (drop is not None or doc is not None):
            raise ValueError("the bidirectional block takes neither dropout nor packed documents")
        # (the fused block calls the attention kernels directly: only for the shapes they take)
        if (x.is_cuda and self.fused and torch.is_grad_enabled()
                and Fx.attn_kernel_ok(x.shape[1], x.shape[2] // self.n_head)):
            from ._gpt2_fused import block_forward  # hand-scheduled fwd/bwd, one autograd node

            return block_forward(self, x, doc) if drop is None else block_forward(self, x, doc, drop)
        if drop is not None:
            # dropout on P and on both projections' outputs: the projection GEMMs write bf16 (no fp32-residual
            # epilogue) and dropout_add forms x + dropout(proj)
            p, rng, stream = drop
            h = self.ln_1(x)
            a = Fx.causal_attention(self.c_attn(h), self.n_head, doc, dropout_p=p, rng=rng, stream=stream)
            x = Fx.dropout_add(x, self.attn_proj(a), p, rng, stream + 1)
            h = self.ln_2(x)
            u = Fx.gelu(self.c_fc(h))
            return Fx.dropout_add(x, self.mlp_proj(u), p, rng, stream + 2)
        h = self.ln_1(x)
        qkv = self.c_attn(h)
        if self.seq_len is not None:
            a = Fx.attention(qkv, self.n_head, self.seq_len)
        else:
            a = Fx.causal_attention(qkv, self.n_head) if doc is None else Fx.causal_attention(qkv, self.n_head, doc)
        x = Fx.linear_residual(a, self.attn_proj.weight, self.attn_proj.bias, x)
        h = self.ln_2(x)
        u = Fx.gelu(self.c_fc(h))
        return Fx.linear_residual(u, self.mlp_proj.weight, self.mlp_proj.bias, x)


class GPT2(nn.Module):
    def __init__(self, cfg: GPT2Config = GPT2Config()):
        super().__init__()
        self.cfg = cfg
        self.wte = nn.Parameter(torch.empty(cfg.vocab_size, cfg.n_embd))
        self.wpe = nn.Parameter(torch.empty(cfg.block_size, cfg.n_embd))
        self.h = nn.ModuleList([Block(cfg) for _ in range(cfg.n_layer)])
        for i, blk in enumerate(self.h):
            blk._dpe_layer = i  # the fused backward flushes deferred weight grads at layer 0 (end of backward)
        self.ln_f = LayerNorm(cfg.n_embd, bias=cfg.bias)
        # tied LM head / embedding: the LM-head weight grad (first writer) overwrites when fresh, the
        # embedding scatter-add accumulates after it
        self.wte._dpe_overwrite_ok = True
        self.wte._dpe_muon = self.wpe._dpe_muon = False  # embeddings / LM head: build_optimizer("muon") keeps them on AdamW
        self._init()

    def _init(self):
        # GPT-2 init: N(0, 0.02); residual projections scaled by 1/sqrt(2*n_layer)
        std = 0.02
        with torch.no_grad():
            self.wte.normal_(0, std)
            self.wpe.normal_(0, std)
            for blk in self.h:
                for lin in (blk.c_attn, blk.c_fc):
                    lin.weight.normal_(0, std)
                    if lin.bias is not None:
                        lin.bias.zero_()
                for lin in (blk.attn_proj, blk.mlp_proj):
                    lin.weight.normal_(0, std / math.sqrt(2 * self.cfg.n_layer))
                    if lin.bias is not None:
                        lin.bias.zero_()

    def forward(self, idx, targets=None, doc_start=None):
        """Logits [B, T, V(p)], or -- with ``targets`` -- the mean next-token
        cross-entropy through the fused LM-head + CE op (logits never materialise
        outside it).  ``doc_start`` [B, T] (see Fx.doc_bounds): the rows hold packed documents; attention
        stays inside each and positions restart at its first token."""
        B, T = idx.shape
        assert T <= self.cfg.block_size, "sequence longer than block_size"
        if _FUSED and idx.is_cuda:
            from ._gpt2_fused import reset_wgrad_queue

            reset_wgrad_queue()
        if self.training and self.cfg.dropout > 0.0:
            x = self._forward_dropout(idx, doc_start)
        elif doc_start is None:
            x = Fx.embedding(idx, self.wte, self.wpe[:T] if not idx.is_cuda else self.wpe)
            for blk in self.h:
                x = blk(x)
        else:
            assert doc_start.shape == idx.shape, "doc_start must have idx's shape"
            doc = Fx.doc_bounds(doc_start)  # once per batch, shared by every layer
            x = Fx.embedding(idx, self.wte, self.wpe, doc[2])
            for blk in self.h:
                x = blk(x, doc)
        x = self.ln_f(x)
        if targets is not None:
            return Fx.lm_head_ce(x, self.wte, targets, label_smoothing=self.cfg.label_smoothing, z_loss=self.cfg.z_loss)
        return Fx.lm_head(x, self.wte)

    def _forward_dropout(self, idx, doc_start):
        """The blocks' input and output in training mode with cfg.dropout > 0: dropout on the embedding sum, on the
        attention probabilities and on both projections' outputs before the residual add.  One snapshot of the
        device-side RNG state serves the whole forward and its backward; the live state then advances once, by
        the largest counter range any call of the step uses.  Call sites differ in their stream: embedding 0,
        layer l attention 1 + 3l, attention residual 2 + 3l, MLP residual 3 + 3l."""
        B, T = idx.shape
        p = float(self.cfg.dropout)
        assert 0.0 < p < 1.0, "dropout must be in [0, 1)"
        rng = None
        if idx.is_cuda:
            st = Fx.dropout_state(idx.device)
            rng = st.snapshot()
            st.advance(max(B * self.cfg.n_head * ((T + 3) // 4) ** 2, (B * T * self.cfg.n_embd + 3) // 4))
        doc = None
        if doc_start is None:
            x = Fx.embedding(idx, self.wte, self.wpe[:T] if not idx.is_cuda else self.wpe)
        else:
            assert doc_start.shape == idx.shape, "doc_start must have idx's shape"
            doc = Fx.doc_bounds(doc_start)
            x = Fx.embedding(idx, self.wte, self.wpe, doc[2])
        x = Fx.dropout_rng(x, p, rng, 0)
        for l, blk in enumerate(self.h):
            x = blk(x, doc, (p, rng, 1 + 3 * l))
        return x

    def num_params(self) -> int:
        return sum(p.numel() for p in self.parameters())

    # ------------------------------------------------------------ generation
    decode_skinny = True  # the decode step's projections on Fx.linear_skinny (False: Fx.linear, the A/B arm)

    def _proj(self, x, lin, act=Fx.ACT_NONE, residual=None):
        """One decode-step projection of x [B, K]: bf16 out (bias, GELU) or, with ``residual``, the fp32 residual
        stream updated in place."""
        if self.decode_skinny:
            return Fx.linear_skinny(x, lin.weight, lin.bias, act, residual)
        if residual is not None:
            return Fx.linear_residual(x, lin.weight, lin.bias, residual)
        return Fx.linear(x, lin.weight, lin.bias, act)

    def _head(self, h):
        """Logits [B, V(p)] of the tied LM head for h [B, D] (after ln_f)."""
        V = self.cfg.vocab_size
        if self.decode_skinny:
            return Fx.linear_skinny(h, self.wte, pad_rows=((V + 63) // 64 * 64 - V) if h.is_cuda else 0)
        return Fx.lm_head(h, self.wte)

    def _prefill(self, idx, lens, cache):
        """The padded prompts [B, T] through the existing ops; every layer's K/V go into the cache, and the LM head
        runs on row lens[b] - 1 of every sequence only.  Returns logits [B, V(p)]."""
        B, T = idx.shape
        H = self.cfg.n_head
        x = Fx.embedding(idx, self.wte, self.wpe[:T] if not idx.is_cuda else self.wpe)
        for l, blk in enumerate(self.h):
            qkv = blk.c_attn(blk.ln_1(x))
            kv = qkv.view(B, T, 3, H, -1)
            cache.buf[l, 0, :, :, :T] = kv[:, :, 1].transpose(1, 2)
            cache.buf[l, 1, :, :, :T] = kv[:, :, 2].transpose(1, 2)
            x = Fx.linear_residual(Fx.causal_attention(qkv, H), blk.attn_proj.weight, blk.attn_proj.bias, x)
            x = Fx.linear_residual(Fx.gelu(blk.c_fc(blk.ln_2(x))), blk.mlp_proj.weight, blk.mlp_proj.bias, x)
        last = x[torch.arange(B, device=x.device), lens.long() - 1]  # [B, D]
        return self._head(self.ln_f(last.unsqueeze(1)).squeeze(1))

    def _decode_step(self, tok, cache):
        """One token per row through the cache: tok int64 [B] at position cache.len -> logits [B, V(p)].  Every
        per-step value (the position, the cache row) is read from device tensors; cache.len is not advanced here."""
        B = tok.shape[0]
        H = self.cfg.n_head
        x = Fx.embedding(tok.view(B, 1), self.wte, self.wpe, cache.len.view(B, 1)).view(B, -1)  # fp32 [B, D]
        for l, blk in enumerate(self.h):
            qkv = self._proj(blk.ln_1(x), blk.c_attn)
            a = Fx.attn_decode(qkv, cache.buf[l, 0], cache.buf[l, 1], cache.len, H)
            x = self._proj(a, blk.attn_proj, residual=x)
            u = self._proj(blk.ln_2(x), blk.c_fc, Fx.ACT_GELU)
            x = self._proj(u, blk.mlp_proj, residual=x)
        return self._head(self.ln_f(x))

    @torch.no_grad()
    def generate(self, idx, max_new_tokens: int, *, prompt_lens=None, temperature: float = 1.0, top_k: int = 0,
                 top_p: float = 1.0, eos_id=None, seed=None, return_logits: bool = False, graph: bool = False):
        """Continue the prompts ``idx`` [B, T] (right-padded; ``prompt_lens`` [B] gives the ragged lengths) by
        ``max_new_tokens`` tokens -> int64 [B, max_new_tokens]; with ``return_logits`` also the fp32
        [B, max_new_tokens, V] logits each token was drawn from.

        One prefill pass over the padded prompts fills a KVCache; every further token is one decode step on the
        single-token kernels (Fx.linear_skinny, Fx.attn_decode) and one Fx.sample_logits.  The sampler's rules:
        temperature 0 is the argmax (lowest index on ties); otherwise s = z / temperature, top-k keeps the values >=
        the k-th largest (ties stay), top-p then keeps a token iff the softmax mass of the strictly larger kept values
        is < top_p, and the token is the arg max of s + Gumbel noise.  A row that has emitted ``eos_id`` repeats it.
        ``seed`` restarts the sampler's RNG for this call.  The host checks the lengths once; after that nothing
        syncs per token.  ``graph``: the decode step is captured in a HIP graph after one eager step and replayed."""
        if idx.dim() != 2 or idx.dtype != torch.int64:
            raise ValueError("generate: idx must be int64 [B, T]")
        B, T = idx.shape
        dev = idx.device
        if prompt_lens is None:
            lens_host = [T] * B
        else:
            lens_host = [int(v) for v in (prompt_lens.tolist() if torch.is_tensor(prompt_lens) else prompt_lens)]
        if len(lens_host) != B or min(lens_host) < 1 or max(lens_host) > T:
            raise ValueError("generate: prompt_lens must hold one length in [1, T] per row")
        if max_new_tokens < 1:
            raise ValueError("generate: max_new_tokens must be >= 1")
        if max(lens_host) + max_new_tokens > self.cfg.block_size:
            raise ValueError(f"generate: max(prompt_lens) + max_new_tokens = {max(lens_host) + max_new_tokens} exceeds "
                             f"block_size = {self.cfg.block_size}")
        if graph and not idx.is_cuda:
            raise ValueError("generate: graph=True needs the GPU")
        was_training = self.training
        self.eval()
        try:
            V = self.cfg.vocab_size
            Tp = max(lens_host)
            if Tp % 64 and (Tp + 63) // 64 * 64 <= self.cfg.block_size:
                Tp = (Tp + 63) // 64 * 64  # whole 64-key tiles: the flash forward serves the prefill
            prompt = torch.zeros(B, Tp, dtype=torch.int64, device=dev)
            prompt[:, :min(T, Tp)] = idx[:, :min(T, Tp)]
            cache = KVCache(self, B, self.cfg.block_size)
            cache.len.copy_(torch.tensor(lens_host, dtype=torch.int32))
            state = gen = None
            if idx.is_cuda:
                state = Fx.sampler_state(dev) if seed is None else Fx.DropoutState(dev).manual_seed(seed)
            elif seed is not None:
                gen = torch.Generator().manual_seed(int(seed))
            out = torch.empty(B, max_new_tokens, dtype=torch.int64, device=dev)
            lgs = torch.empty(B, max_new_tokens, V, dtype=torch.float32, device=dev) if return_logits else None

            def draw(logits):
                return Fx.sample_logits(logits, V, temperature, top_k, top_p, state, eos_id, cache.done, gen)

            logits = self._prefill(prompt, cache.len, cache)
            tok = draw(logits)
            out[:, 0] = tok
            if return_logits:
                lgs[:, 0] = logits[:, :V]
            if graph and max_new_tokens > 2:
                self._generate_graph(tok, cache, draw, out, lgs)
            else:
                for i in range(1, max_new_tokens):
                    logits = self._decode_step(tok, cache)
                    cache.len.add_(1)
                    tok = draw(logits)
                    out[:, i] = tok
                    if return_logits:
                        lgs[:, i] = logits[:, :V]
            return (out, lgs) if return_logits else out
        finally:
            self.train(was_training)

    def _generate_graph(self, tok, cache, draw, out, lgs):
        """Tokens 1 .. of ``out``: one eager decode step (it also refreshes every weight shadow and sizes the
        allocator), then the same step captured once and replayed.  The current token, cache.len, cache.done and the
        RNG state are device tensors the captured kernels read and update in place; the copy of the token into its
        result column is the one eager op per token."""
        V = self.cfg.vocab_size
        cur = tok.clone()

        def step():
            logits = self._decode_step(cur, cache)
            cache.len.add_(1)
            cur.copy_(draw(logits))
            return logits

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            logits = step()
        torch.cuda.current_stream().wait_stream(side)
        out[:, 1] = cur
        if lgs is not None:
            lgs[:, 1] = logits[:, :V]
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            logits = step()
        for i in range(2, out.shape[1]):
            g.replay()
            out[:, i] = cur
            if lgs is not None:
                lgs[:, i] = logits[:, :V]


class KVCache:
    """The keys and values of every layer for ``batch`` sequences of up to ``max_len`` tokens: one
    [L, 2, B, H, Tmax, 64] buffer (bf16 on the GPU, fp32 on the CPU), head-major so one (row, head) streams one
    contiguous run; ``len`` int32 [B] = tokens cached per row; ``done`` int32 [B] = the row has emitted eos."""

    def __init__(self, model: GPT2, batch: int, max_len: int):
        cfg = model.cfg
        dev = model.wte.device
        self.buf = torch.zeros(cfg.n_layer, 2, batch, cfg.n_head, max_len, cfg.n_embd // cfg.n_head,
                               dtype=torch.bfloat16 if dev.type == "cuda" else torch.float32, device=dev)
        self.len = torch.zeros(batch, dtype=torch.int32, device=dev)
        self.done = torch.zeros(batch, dtype=torch.int32, device=dev)
