"""Reference of the attention-dropout mask and of dropped attention (imported by test_attn_dropout_cpu.py and
test_attn_dropout_gpu.py).  Nothing here calls the extension: the mask is recomputed in numpy from its contract.

Contract.  rng = (seed, offset) (64-bit each), stream a 32-bit call-site id.
  attention: P is covered by 4-query x 4-key granules; with bh = b*H + h and n4 = T/4, granule (bh, i/4, j/4) has
    counter G = (bh*n4 + i/4)*n4 + j/4 and r = philox4x32(seed, offset + G, stream) (64-bit sum).  Element (i, j)
    takes byte j%4 (little-endian) of word r[i%4] and is KEPT iff byte >= thr, thr = clamp(round(256 p), 1, 255);
    kept probabilities are scaled by s = 256 / (256 - thr).  The softmax denominator and lse2 are the undropped ones.
  elementwise: element n of the flat tensor keeps iff philox4x32(seed, offset + n/4, stream)[n%4] >= p * 2^32
    (dropout_kernel's rule; its threshold is the float product, clamped to 2^32 - 1), scale 1 / (1 - p).

    philox4x32(seed, counter_hi, counter_lo)       numpy, vectorised over counter_hi; common.h's variant
    keep_mask(seed, offset, stream, B, H, T, thr)  bool [B, H, T, T]
    eltwise_keep(seed, offset, stream, n, p)       bool [n]
    attn_dropout_ref(qkv, dout, scale, doc_start, keep, thr)   fp64 outputs, gradients and rounding budgets
    attn_dropout_autograd(...)                     the same gradients from fp64 autograd
"""
import math

import numpy as np
import torch

from _gpt2_ref import C_DV, C_LSE, FLOOR
from _packed_attn_ref import doc_mask

M32 = np.uint64(0xFFFFFFFF)


def philox4x32(seed, counter_hi, counter_lo):
    """Philox-4x32-10 exactly as csrc/kernels/common.h: key = (seed lo, seed hi), counter = (counter_lo,
    counter_hi lo, counter_hi hi, 0x9E3779B9), its round function and key schedule.  ``counter_hi``: uint64 array
    (any shape); returns uint32 [..., 4]."""
    ch = np.asarray(counter_hi, dtype=np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    c0 = np.full(ch.shape, int(counter_lo) & 0xFFFFFFFF, dtype=np.uint64)
    c1 = ch & M32
    c2 = ch >> np.uint64(32)
    c3 = np.full(ch.shape, 0x9E3779B9, dtype=np.uint64)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0  # < 2^64: both factors < 2^32
        p1 = np.uint64(0xCD9E8D57) * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)
        c1 = p1 & M32
        c3 = p0 & M32
        c0, c2 = n0, n2
        k0 = (k0 + 0x9E3779B9) & 0xFFFFFFFF
        k1 = (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def attn_threshold(p):
    return min(255, max(1, int(math.floor(256.0 * p + 0.5))))


def keep_mask(seed, offset, stream, B, H, T, thr):
    """bool torch tensor [B, H, T, T]: True where P[b, h, i, j] is kept."""
    assert T % 4 == 0
    n4 = T // 4
    bh = np.arange(B * H, dtype=np.uint64)[:, None, None]
    i4 = np.arange(n4, dtype=np.uint64)[None, :, None]
    j4 = np.arange(n4, dtype=np.uint64)[None, None, :]
    G = (bh * np.uint64(n4) + i4) * np.uint64(n4) + j4
    ctr = (G + np.uint64(int(offset) & 0xFFFFFFFFFFFFFFFF))  # wraps mod 2^64 like the kernel's add
    r = philox4x32(seed, ctr, stream)  # [BH, n4, n4, 4 (word = i % 4)]
    sh = (np.arange(4, dtype=np.uint32) * 8)[None, None, None, None, :]
    byte = (r[..., None] >> sh) & np.uint32(0xFF)  # [BH, n4, n4, i%4, j%4]
    keep = byte >= np.uint32(thr)
    keep = keep.transpose(0, 1, 3, 2, 4).reshape(B, H, T, T)  # i = 4*i4 + word, j = 4*j4 + byte
    return torch.from_numpy(np.ascontiguousarray(keep))


def eltwise_keep(seed, offset, stream, n, p):
    """bool torch tensor [n]: the keep set of dropout_add / dropout_cast / dropout."""
    n4 = (n + 3) // 4
    ctr = np.arange(n4, dtype=np.uint64) + np.uint64(int(offset) & 0xFFFFFFFFFFFFFFFF)
    r = philox4x32(seed, ctr, stream).reshape(-1)[:n]
    thr = np.uint32(min(float(np.float32(p) * np.float32(4294967296.0)), 4294967295.0))
    return torch.from_numpy(r >= thr)


def _masks(doc_start, B, T, device):
    if doc_start is None:
        doc_start = torch.zeros(B, T, dtype=torch.int32)
    return doc_mask(doc_start, T, device)


def attn_dropout_ref(qkv, dout, scale, doc_start, keep, thr):
    """qkv [B, T, 3, H, D], dout [B, T, H, D], doc_start [B, T] or None, keep bool [B, H, T, T] -> the dict of
    packed_attn_ref with dropout on P: Pt = P o M s (s = 256 / (256 - thr)) wherever P multiplies V or dO,

        O = Pt V,  dV = Pt^T dO,  dP = dO V^T,  delta = rowsum(dO o O),  dS = P o (M s dP - delta),
        dQ = scale dS K,  dK = scale dS^T Q;  lse2 from the undropped P.

    Budgets: packed_attn_ref's formulas with Pt for P where it multiplies V or dO (A = Pt |v|, b_dv from Pt^T |dO|,
    W = 2^-7 P (|M s dP| + |delta|) + P E).  "dead" marks the rows whose every visible key is dropped."""
    q, k, v = qkv.double().permute(2, 0, 3, 1, 4)  # [B, H, T, D]
    do = dout.double().permute(0, 2, 1, 3)
    B, _, T, _ = q.shape
    s = 256.0 / (256.0 - thr)
    Ms = keep.to(q.device).double() * s
    masked = _masks(doc_start, B, T, q.device)
    S = scale * (q @ k.transpose(-1, -2))
    S = S.masked_fill(masked, float("-inf"))
    lse = torch.logsumexp(S, dim=-1)
    P = torch.exp(S - lse.unsqueeze(-1))
    Pt = P * Ms
    O = Pt @ v
    dV = Pt.transpose(-1, -2) @ do
    dP = do @ v.transpose(-1, -2)
    delta = (do * O).sum(-1, keepdim=True)
    dS = P * (Ms * dP - delta)
    dQ = scale * (dS @ k)
    dK = scale * (dS.transpose(-1, -2) @ q)
    A = Pt @ v.abs()
    b_out = 2.0 ** -7 * A
    b_dv = C_DV * 2.0 ** -7 * (Pt.transpose(-1, -2) @ do.abs())
    E = 2.0 ** -7 * (do.abs() * A).sum(-1, keepdim=True)
    W = 2.0 ** -7 * P * ((Ms * dP).abs() + delta.abs()) + P * E
    b_dq = scale * (W @ k.abs()) + 2.0 ** -9 * dQ.abs()
    b_dk = scale * (W.transpose(-1, -2) @ q.abs()) + 2.0 ** -9 * dK.abs()
    dead = ~((keep.to(q.device) & ~masked).any(-1))  # [B, H, T]

    def lay(a):  # [B, H, T, D] -> [B, T, H, D]
        return a.permute(0, 2, 1, 3).contiguous()

    return {
        "out": lay(O), "lse2": lse / math.log(2.0),
        "dqkv": torch.stack([lay(dQ), lay(dK), lay(dV)], dim=2),
        "b_out": lay(b_out) + FLOOR, "b_lse2": C_LSE * 2.0 ** -8,
        "b_dqkv": torch.stack([lay(b_dq), lay(b_dk), lay(b_dv)], dim=2) + FLOOR,
        "dead": dead,
    }


def attn_dropout_autograd(qkv, dout, scale, doc_start, keep, thr):
    """(O, dqkv) from fp64 autograd through the explicit masked softmax with the mask applied to P."""
    x = qkv.double().clone().requires_grad_(True)
    q, k, v = x.permute(2, 0, 3, 1, 4)
    B, _, T, _ = q.shape
    S = scale * (q @ k.transpose(-1, -2))
    S = S.masked_fill(_masks(doc_start, B, T, S.device), float("-inf"))
    Pt = torch.softmax(S, dim=-1) * (keep.to(S.device).double() * (256.0 / (256.0 - thr)))
    O = (Pt @ v).permute(0, 2, 1, 3)
    O.backward(dout.double())
    return O.detach(), x.grad
