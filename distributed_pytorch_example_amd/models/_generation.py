"""The model-independent half of generation, shared by GPT2 and Llama: the KV cache, the host loop of ``generate``
(length checks, prompt padding to whole 64-key tiles, sampler state, eager loop) and the HIP-graph replay of the decode
step.  A model supplies ``_prefill(idx, lens, cache)`` and ``_decode_step(tok, cache)``, both -> logits [B, V(p)], and,
where its cache holds fewer heads than it has query heads, ``_cache_heads()``."""
from __future__ import annotations

import torch

from ..ops import functional as Fx


class KVCache:
    """The keys and values of every layer for ``batch`` sequences of up to ``max_len`` tokens: one
    [L, 2, B, H, Tmax, 64] buffer (bf16 on the GPU, fp32 on the CPU), head-major so one (row, head) streams one
    contiguous run; H is the model's ``_cache_heads()`` (n_head for GPT-2, n_kv_head for Llama); ``len`` int32 [B] =
    tokens cached per row; ``done`` int32 [B] = the row has emitted eos."""

    def __init__(self, model, batch: int, max_len: int):
        cfg = model.cfg
        dev = model.wte.device
        self.buf = torch.zeros(cfg.n_layer, 2, batch, model._cache_heads(), max_len, cfg.n_embd // cfg.n_head,
                               dtype=torch.bfloat16 if dev.type == "cuda" else torch.float32, device=dev)
        self.len = torch.zeros(batch, dtype=torch.int32, device=dev)
        self.done = torch.zeros(batch, dtype=torch.int32, device=dev)


class GenerationMixin:
    decode_skinny = True  # the decode step's projections on Fx.linear_skinny (False: Fx.linear, the A/B arm)

    def _cache_heads(self) -> int:
        return self.cfg.n_head

    def _proj(self, x, lin, act=Fx.ACT_NONE, residual=None):
        """One decode-step projection of x [B, K]: bf16 out (bias, GELU) or, with ``residual``, the fp32 residual
        stream updated in place."""
        if self.decode_skinny:
            return Fx.linear_skinny(x, lin.weight, lin.bias, act, residual)
        if residual is not None:
            return Fx.linear_residual(x, lin.weight, lin.bias, residual)
        return Fx.linear(x, lin.weight, lin.bias, act)

    @torch.no_grad()
    def generate(self, idx, max_new_tokens: int, *, prompt_lens=None, temperature: float = 1.0, top_k: int = 0,
                 top_p: float = 1.0, eos_id=None, seed=None, return_logits: bool = False, graph: bool = False):
        """Continue the prompts ``idx`` [B, T] (right-padded; ``prompt_lens`` [B] gives the ragged lengths) by
        ``max_new_tokens`` tokens -> int64 [B, max_new_tokens]; with ``return_logits`` also the fp32
        [B, max_new_tokens, V] logits each token was drawn from.

        One prefill pass over the padded prompts fills a KVCache; every further token is one decode step on the
        single-token kernels (Fx.linear_skinny, Fx.attn_decode / Fx.attn_decode_gqa) and one Fx.sample_logits.  The
        sampler's rules: temperature 0 is the argmax (lowest index on ties); otherwise s = z / temperature, top-k keeps
        the values >= the k-th largest (ties stay), top-p then keeps a token iff the softmax mass of the strictly larger
        kept values is < top_p, and the token is the arg max of s + Gumbel noise.  A row that has emitted ``eos_id``
        repeats it.  ``seed`` restarts the sampler's RNG for this call.  The host checks the lengths once; after that
        nothing syncs per token.  ``graph``: the decode step is captured in a HIP graph after one eager step and
        replayed."""
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
