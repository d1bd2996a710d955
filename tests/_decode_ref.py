"""References of the generation kernels (imported by test_decode_attn_gpu.py, test_linear_skinny_gpu.py,
test_sample_gpu.py, test_generate_gpu.py and test_generate_cpu.py).  Nothing here calls the extension.

    philox(seed, ctr, stream, c3)         Philox-4x32-10 in numpy; c3 = SAMPLE_C3 is the sampler's counter word
    attn_decode_ref(qkv, kc, vc, lens)    fp64 single-query attention from _gpt2_ref.attn_ref, with its b_out budget
    keep_ref(s, top_k, top_p)             the sampler's kept set on fp64 values, and its distance from ambiguity
    gumbel_ref(seed, offset, stream, B, V)   g = -log(-log u) in fp64 from the sampler's Philox words
    head_tail_row(V, ...)                 constructed logits: geometric head tokens at permuted positions over a flat tail
    naive_generate(model, ...)            greedy decoding by full forwards
"""
import math

import numpy as np
import torch

from _gpt2_ref import attn_ref

SAMPLE_C3 = 0x5A3C91E7
M32 = np.uint64(0xFFFFFFFF)


def philox(seed, ctr, stream, c3=SAMPLE_C3):
    """key = (seed lo, seed hi), counter = (stream, ctr lo, ctr hi, c3); ``ctr`` uint64 array -> uint32 [..., 4]."""
    ch = np.asarray(ctr, dtype=np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    c0 = np.full(ch.shape, int(stream) & 0xFFFFFFFF, dtype=np.uint64)
    c1, c2, c3 = ch & M32, ch >> np.uint64(32), np.full(ch.shape, c3, dtype=np.uint64)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


# ------------------------------------------------------------------ attention
def attn_decode_ref(qkv_step, kc, vc, lens, scale):
    """qkv_step [B, 3, H, 64], kc / vc [B, H, Tmax, 64] (bf16, before the step), lens list -> (out, b_out) fp64
    [B, H * 64]: _gpt2_ref.attn_ref on the first lens[b] + 1 tokens (the cached rows, then the step's), its last
    query row, with its budget 2^-7 (P |v|)."""
    B, _, H, D = qkv_step.shape
    outs, bounds = [], []
    for b in range(B):
        n = int(lens[b])
        qkv = torch.zeros(1, n + 1, 3, H, D, dtype=torch.float64)
        qkv[0, :n, 1] = kc[b, :, :n].double().transpose(0, 1)
        qkv[0, :n, 2] = vc[b, :, :n].double().transpose(0, 1)
        qkv[0, n] = qkv_step[b].double()
        r = attn_ref(qkv, torch.zeros(1, n + 1, H, D, dtype=torch.float64), scale)
        outs.append(r["out"][0, n].reshape(-1))
        bounds.append(r["b_out"][0, n].reshape(-1))
    return torch.stack(outs), torch.stack(bounds)


# -------------------------------------------------------------------- sampler
def keep_ref(s, top_k=0, top_p=1.0):
    """s [R, V] (the fp32 values z / temperature) -> (keep bool [R, V], margin [R]): top-k keeps s >= the k-th
    largest value (multiplicity counted, ties stay); top-p keeps j iff the fp64 softmax mass, over what top-k kept,
    of the strictly larger values is < top_p.  margin = min_j |M_>(j) - top_p| over the top-k survivors: a kernel
    summing fp32 probabilities may disagree only where that is below its summation error."""
    s = s.double()
    R, V = s.shape
    keep = torch.ones(R, V, dtype=torch.bool)
    if 0 < top_k < V:
        keep = s >= torch.topk(s, top_k, dim=-1).values[:, -1:]
    margin = torch.full((R,), float("inf"), dtype=torch.float64)
    if top_p < 1.0:
        sm = torch.where(keep, s, torch.full_like(s, float("-inf")))
        p = torch.softmax(sm, dim=-1)
        sv, order = torch.sort(sm, dim=-1, descending=True)
        ps = torch.gather(p, -1, order)
        above_sorted = torch.cumsum(ps, -1) - ps
        new = torch.cat([torch.ones(R, 1, dtype=torch.bool), sv[:, 1:] != sv[:, :-1]], dim=-1)
        i = torch.arange(V).expand(R, V)
        first = torch.cummax(torch.where(new, i, torch.zeros_like(i)), dim=-1).values
        above_sorted = torch.gather(above_sorted, -1, first)
        above = torch.zeros_like(above_sorted).scatter(-1, order, above_sorted)
        margin = torch.where(keep, (above - top_p).abs(), torch.full_like(above, float("inf"))).min(-1).values
        keep = keep & (above < top_p)
    return keep, margin


def gumbel_ref(seed, offset, stream, B, V):
    """fp64 [B, V]: g_j = -log(-log u_j), u_j = (2 n + 1) 2^-24 with n the top 23 bits of word j % 4 of
    philox(seed, offset + row * ceil(V / 4) + j / 4, stream)."""
    V4 = (V + 3) // 4
    ctr = (np.arange(B, dtype=np.uint64)[:, None] * np.uint64(V4) + np.arange(V4, dtype=np.uint64)[None, :]
           + np.uint64(int(offset) & 0xFFFFFFFFFFFFFFFF))
    w = philox(seed, ctr, stream).reshape(B, V4 * 4)[:, :V]
    u = (2.0 * (w >> np.uint32(9)).astype(np.float64) + 1.0) * 2.0 ** -24
    return torch.from_numpy(-np.log(-np.log(u)))


def head_tail_row(V, n_head, ratio=0.5, tail_mass=2.0 ** -11, seed=0, ties=0):
    """fp32 logits [V]: ``n_head`` head tokens at permuted positions with probabilities ~ ratio^i (the last ``ties``
    of them share one value) over a flat tail of total mass < 2^-10.  Every value is a bf16 number, so bf16 and
    fp32 kernels see the same row.  Returns (z, head positions in descending order of probability)."""
    g = torch.Generator().manual_seed(seed)
    pos = torch.randperm(V, generator=g)[:n_head]
    lp = torch.arange(n_head, dtype=torch.float64) * math.log(ratio)
    if ties:
        lp[n_head - ties:] = lp[n_head - ties]
    z = torch.full((V,), 0.0, dtype=torch.float64)
    if V > n_head:
        tail = math.log(tail_mass / (V - n_head))  # relative to the first head token (probability ~ 1 - ratio)
        z[:] = tail
    z[pos] = lp
    z = z.to(torch.bfloat16).float()
    return z, pos


# ------------------------------------------------------------------- generate
@torch.no_grad()
def naive_generate(model, idx, lens, n_new):
    """Greedy tokens [B, n_new] and fp32 logits [B, n_new, V] by a full forward of the whole prefix per token."""
    V = model.cfg.vocab_size
    toks, lgs = [], []
    for b in range(idx.shape[0]):
        seq = idx[b:b + 1, :lens[b]]
        row, lrow = [], []
        for _ in range(n_new):
            z = model(seq)[0, -1, :V].float()
            t = int(torch.where(z == z.max())[0][0])
            row.append(t)
            lrow.append(z)
            seq = torch.cat([seq, torch.tensor([[t]], dtype=seq.dtype, device=seq.device)], dim=1)
        toks.append(row)
        lgs.append(torch.stack(lrow))
    return torch.tensor(toks), torch.stack(lgs)
