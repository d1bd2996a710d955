"""fp64 references of the Llama kernels (csrc/kernels/llama.hip) on the values the kernel reads, and an independent
plain-torch Llama with Hugging Face semantics (rotate_half, repeat_interleave of K / V, F.silu(gate) * up)."""
import math

import torch
import torch.nn.functional as F

FLOOR = 1e-30  # added to every bound: exact zeros compare cleanly


def rope_ref(x, cos, sin, rows, n_rot, inverse=False):
    """x [B, T, W, 64], table rows [B, T] -> (the rotated heads, their bound: one bf16 rounding + fp32 arithmetic)."""
    xd = x.double()
    c = cos.double()[rows].unsqueeze(2)
    s = sin.double()[rows].unsqueeze(2) * (-1.0 if inverse else 1.0)
    x1, x2 = xd[:, :, :n_rot, :32], xd[:, :, :n_rot, 32:]
    ref = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)
    mag = torch.cat([(x1 * c).abs() + (x2 * s).abs(), (x2 * c).abs() + (x1 * s).abs()], -1)
    return ref, 2.0 ** -8 * ref.abs() + 1e-6 * mag + FLOOR


def rms_ref(x, w, dy, eps=1e-5):
    """-> y, rstd [rows], xhat, dx, dw (fp64)."""
    xd, g = x.double(), dy.double() * w.double()
    rstd = (xd.pow(2).mean(-1) + eps).rsqrt()
    xh = xd * rstd.unsqueeze(-1)
    dx = rstd.unsqueeze(-1) * (g - xh * (g * xh).mean(-1, keepdim=True))
    return xh * w.double(), rstd, xh, dx, (dy.double() * xh).sum(0)


def swiglu_ref(gu, du):
    """-> u, dg, dv (fp64)."""
    g, v = gu.double().chunk(2, dim=-1)
    sg = torch.sigmoid(g)
    d = du.double()
    return g * sg * v, d * v * sg * (1.0 + g * (1.0 - sg)), d * g * sg


def llama_ref(m, idx, doc_start=None):
    """Logits of the models.llama.Llama ``m`` in its parameters' dtype, written the Hugging Face way."""
    cfg = m.cfg
    B, T = idx.shape
    Hq, Hkv, D = cfg.n_head, cfg.n_kv_head, cfg.n_embd // cfg.n_head
    dt = m.wte.dtype
    t = torch.arange(T)
    ds = torch.zeros(B, T, dtype=torch.long) if doc_start is None else doc_start.long()
    inv_freq = 1.0 / (cfg.rope_theta ** (torch.arange(0, D, 2, dtype=torch.float64) / D))
    ang = ((t - ds).double()[..., None] * inv_freq).repeat(1, 1, 2)  # [B, T, D]
    cos, sin = ang.cos().to(dt).unsqueeze(2), ang.sin().to(dt).unsqueeze(2)
    mask = (t[None, :, None] >= t[None, None, :]) & (t[None, None, :] >= ds[:, :, None])  # [B, i, j]

    def rotate_half(x):
        return torch.cat([-x[..., D // 2:], x[..., :D // 2]], dim=-1)

    def norm(x, w):
        return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + cfg.rms_eps) * w

    x = F.embedding(idx, m.wte)
    for blk in m.h:
        q, k, v = F.linear(norm(x, blk.ln_1.weight), blk.c_attn.weight).view(B, T, -1, D).split([Hq, Hkv, Hkv], dim=2)
        q, k = q * cos + rotate_half(q) * sin, k * cos + rotate_half(k) * sin
        k, v = k.repeat_interleave(Hq // Hkv, dim=2), v.repeat_interleave(Hq // Hkv, dim=2)
        s = torch.einsum("bihd,bjhd->bhij", q, k) / math.sqrt(D)
        p = torch.softmax(s.masked_fill(~mask.unsqueeze(1), float("-inf")), dim=-1)
        x = x + F.linear(torch.einsum("bhij,bjhd->bihd", p, v).reshape(B, T, -1), blk.attn_proj.weight)
        gate, up = F.linear(norm(x, blk.ln_2.weight), blk.c_fc.weight).chunk(2, dim=-1)
        x = x + F.linear(F.silu(gate) * up, blk.mlp_proj.weight)
    return F.linear(norm(x, m.ln_f.weight), m.head_weight())
