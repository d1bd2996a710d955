"""fp64 reference of the bidirectional attention with a key-length bound (imported by test_bidir_attn_gpu.py and
test_vit_cpu.py): _gpt2_ref.attn_ref with the mask "query i < L sees the keys j < L" in place of the causal one.

    bidir_attn_ref(qkv, dout, scale, L)        out, lse2, dqkv and attn_ref's budgets, evaluated on this reference
    bidir_attn_autograd(qkv, dout, scale, L)   the same gradients from fp64 autograd (checks the closed forms)
    bidir_tile_row_max(qkv, scale, L)          per (row, 64-key tile) maximum of S * log2(e) over the keys < L

Rows >= L are padding: out and dqkv are zeros there and lse2 is 0.0 (the value the kernels write).  Nothing at or past
row L of qkv or dout enters any value: the padding queries' P rows and the padding keys' P columns are exact zeros,
so the budgets (the project's own: bf16 P / dS, l built from the rounded P, a bf16 O inside delta, bf16 outputs,
C_LSE and C_DV of _gpt2_ref.py) do not depend on the mask beyond P itself.
"""
import math

import torch

from _gpt2_ref import C_DV, C_LSE, FLOOR, LOG2E


def _masked_p(q, k, scale, L):
    """(P, lse) of the bidirectional softmax: P [B, H, T, T] with zero rows and columns from L on; lse [B, H, T] with
    0 from L on."""
    T = q.shape[-2]
    live = torch.arange(T, device=q.device) < L
    S = scale * (q @ k.transpose(-1, -2))
    S = S.masked_fill(~live[None, None, None, :], float("-inf"))
    lse = torch.logsumexp(S, dim=-1)
    P = torch.exp(S - lse.unsqueeze(-1)) * live[None, None, :, None].to(S.dtype)
    return P, lse * live.to(S.dtype), live


def bidir_attn_ref(qkv, dout, scale, L):
    """qkv [B, T, 3, H, D], dout [B, T, H, D] (any float dtype), 1 <= L <= T -> dict of fp64 tensors in the kernels'
    layouts, as _gpt2_ref.attn_ref: out, lse2 (log2 units; 0 for rows >= L), dqkv, b_out, b_lse2, b_dqkv."""
    q, k, v = qkv.double().permute(2, 0, 3, 1, 4)  # [B, H, T, D]
    P, lse, live = _masked_p(q, k, scale, L)
    rows = live[None, None, :, None].to(q.dtype)
    # the padding rows hold finite values that P's zeros multiply away; they are zeroed here so that a reference on
    # inputs with huge padding stays exact
    q, k, v = q * rows, k * rows, v * rows
    do = dout.double().permute(0, 2, 1, 3) * rows
    O = P @ v
    dV = P.transpose(-1, -2) @ do
    dP = do @ v.transpose(-1, -2)
    delta = (do * O).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    dQ = scale * (dS @ k)
    dK = scale * (dS.transpose(-1, -2) @ q)
    # budgets (attn_ref's formulas)
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


def bidir_attn_autograd(qkv, dout, scale, L):
    """(out, dqkv) from fp64 autograd through an explicit softmax over the first L rows only (the padding rows never
    enter the graph: their output and gradient are zeros)."""
    x = qkv.double().clone().requires_grad_(True)
    q, k, v = x[:, :L].permute(2, 0, 3, 1, 4)  # [B, H, L, D]
    O = (torch.softmax(scale * (q @ k.transpose(-1, -2)), dim=-1) @ v).permute(0, 2, 1, 3)
    O.backward(dout.double()[:, :L])
    out = torch.zeros(dout.shape, dtype=torch.float64, device=qkv.device)
    out[:, :L] = O.detach()
    return out, x.grad


def bidir_tile_row_max(qkv, scale, L, tile=64):
    """[B, H, T, T / tile]: max over the keys j < L of each 64-key tile of S_ij * log2(e); -inf where the whole tile
    lies at or past L (those tiles are never visited)."""
    q, k, _ = qkv.double().permute(2, 0, 3, 1, 4)
    T = q.shape[-2]
    S = scale * LOG2E * (q @ k.transpose(-1, -2))
    S = S.masked_fill((torch.arange(T, device=S.device) >= L)[None, None, None, :], float("-inf"))
    return S.view(*S.shape[:-1], T // tile, tile).amax(-1)
