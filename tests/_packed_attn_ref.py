"""fp64 reference of packed-document causal attention (imported by test_packed_attn_cpu.py and
test_packed_attn_gpu.py): attn_ref of _gpt2_ref.py with the mask doc_start[b, i] <= j <= i in place of j <= i,
the same closed-form gradients and the same rounding-budget formulas (C_LSE / C_DV imported, not restated).

    packed_attn_ref(qkv, dout, scale, doc_start)       like attn_ref
    packed_attn_autograd(qkv, dout, scale, doc_start)  the same gradients from fp64 autograd
    doc_start_of(T, boundaries)                        doc_start row with documents starting at the boundaries
    geometric_doc_start(B, T, mean, seed)              seeded geometric document lengths (minimum 1), per row
"""
import math

import torch

from _gpt2_ref import C_DV, C_LSE, FLOOR


def doc_mask(doc_start, T, device):
    """[B, 1, T, T] bool, True where query i must NOT see key j."""
    i = torch.arange(T, device=device)
    ds = doc_start.to(device).long()
    return ((i[None, None, :] > i[None, :, None]) | (i[None, None, :] < ds[:, :, None])).unsqueeze(1)


def packed_attn_ref(qkv, dout, scale, doc_start):
    """qkv [B, T, 3, H, D], dout [B, T, H, D], doc_start [B, T] -> the dict of attn_ref (fp64, kernels' layouts)."""
    q, k, v = qkv.double().permute(2, 0, 3, 1, 4)  # [B, H, T, D]
    do = dout.double().permute(0, 2, 1, 3)
    T = q.shape[-2]
    S = scale * (q @ k.transpose(-1, -2))
    S = S.masked_fill(doc_mask(doc_start, T, S.device), float("-inf"))
    lse = torch.logsumexp(S, dim=-1)
    P = torch.exp(S - lse.unsqueeze(-1))
    O = P @ v
    dV = P.transpose(-1, -2) @ do
    dP = do @ v.transpose(-1, -2)
    delta = (do * O).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    dQ = scale * (dS @ k)
    dK = scale * (dS.transpose(-1, -2) @ q)
    # budgets (attn_ref's)
    A = P @ v.abs()
    b_out = 2.0 ** -7 * A
    b_dv = C_DV * 2.0 ** -7 * (P.transpose(-1, -2) @ do.abs())
    E = 2.0 ** -7 * (do.abs() * A).sum(-1, keepdim=True)
    W = 2.0 ** -7 * P * (dP.abs() + delta.abs()) + P * E
    b_dq = scale * (W @ k.abs()) + 2.0 ** -9 * dQ.abs()
    b_dk = scale * (W.transpose(-1, -2) @ q.abs()) + 2.0 ** -9 * dK.abs()

    def lay(a):  # [B, H, T, D] -> [B, T, H, D]
        return a.permute(0, 2, 1, 3).contiguous()

    return {
        "out": lay(O), "lse2": lse / math.log(2.0),
        "dqkv": torch.stack([lay(dQ), lay(dK), lay(dV)], dim=2),
        "b_out": lay(b_out) + FLOOR, "b_lse2": C_LSE * 2.0 ** -8,
        "b_dqkv": torch.stack([lay(b_dq), lay(b_dk), lay(b_dv)], dim=2) + FLOOR,
    }


def packed_attn_autograd(qkv, dout, scale, doc_start):
    """(O, dqkv) from fp64 autograd through the explicit masked softmax (checks the closed forms above)."""
    x = qkv.double().clone().requires_grad_(True)
    q, k, v = x.permute(2, 0, 3, 1, 4)
    T = q.shape[-2]
    S = scale * (q @ k.transpose(-1, -2))
    S = S.masked_fill(doc_mask(doc_start, T, S.device), float("-inf"))
    O = (torch.softmax(S, dim=-1) @ v).permute(0, 2, 1, 3)
    O.backward(dout.double())
    return O.detach(), x.grad


def doc_start_of(T, boundaries):
    """int32 [T]: documents start at 0 and at every index of ``boundaries``."""
    ds = torch.zeros(T, dtype=torch.int32)
    for b in sorted(boundaries):
        ds[b:] = b
    return ds


def geometric_doc_start(B, T, mean, seed):
    """int32 [B, T]: per row, document lengths 1 + Geometric(1 / mean) from a seeded generator."""
    g = torch.Generator().manual_seed(seed)
    first = torch.rand(B, T, generator=g) < 1.0 / mean
    first[:, 0] = True
    t = torch.arange(T).expand(B, -1)
    return torch.cummax(torch.where(first, t, torch.zeros_like(t)), dim=1).values.to(torch.int32)
