"""Independent fp64 references of the GPT-2 kernels (imported by test_gpt2_kernels_gpu.py and
test_gpt2_ref_cpu.py): plain torch in float64, straight from the definitions, computed on whatever device
the inputs live on.  Every reference takes the values the kernel sees (the bf16-rounded tensors, widened).

    attn_ref(qkv, dout, scale)        causal attention, closed-form gradients, per-element rounding budgets
    staircase_qkv(...)                inputs that move the forward's running row max tile by tile
    tile_row_max(qkv, scale)          per (row, 64-key tile) maximum of S * log2(e), from the fp64 scores
    ce_ref(z, labels, V, ...)         cross-entropy rows, gradient, argmax
    ln_ref(x, w, b, eps) / ln_bwd_ref(dy, x, w, eps)
    gelu_ref(x) / gelu_grad_ref(x)    tanh-GELU and its derivative
"""
import math

import torch

LOG2E = 1.4426950408889634
FLOOR = 1e-30  # added to every bound: exact zeros compare cleanly

# Two of the attention budgets carry a constant above the 1.0 they started with (2^-8 for lse2, 2^-7 for dV,
# counting each bf16 rounding as 2^-9).  bf16 keeps 8 significant bits, so one rounding is off by up to 2^-8,
# and where one key carries a row's softmax nothing averages that out (the causal-leak case: keys 16x larger):
#  * lse2: l is the sum of the rounded P, so it is off by up to 2^-8 and log2(l) by 2^-8 log2(e) = 1.443 * 2^-8.
#  * dV_jd = sum_i P_ij dO_id with one dominant i: the backward's P = exp2(s - lse2) inherits l's 2^-8, is
#    rounded to bf16 (2^-8), and so is dV (2^-8): 3 * 2^-8 = 1.5 * 2^-7.
# attn_emulate (the algorithm's roundings in torch, no kernel) measures 1.074 and 1.015 against the original
# budgets on that case -- the kernels measured 1.076 and 1.015 -- so the constants may rise to 2.15 and 2.03
# at most; they are set to the worst cases derived above, 1.5 each (1.443 plus fp32 slack for lse2).
C_LSE = 1.5
C_DV = 1.5


# ------------------------------------------------------------------ attention
def attn_ref(qkv, dout, scale):
    """qkv [B, T, 3, H, D], dout [B, T, H, D] (any float dtype) -> dict of fp64 tensors in the kernels' layouts:
    out [B, T, H, D], lse2 [B, H, T] (log2 units), dqkv [B, T, 3, H, D], and the bounds b_out, b_dqkv (the
    rounding budgets of the issue: bf16 P / dS, l built from the rounded P, a bf16 O inside delta, bf16
    outputs), each evaluated on the reference itself."""
    q, k, v = qkv.double().permute(2, 0, 3, 1, 4)  # [B, H, T, D]
    do = dout.double().permute(0, 2, 1, 3)
    T = q.shape[-2]
    S = scale * (q @ k.transpose(-1, -2))
    S = S.masked_fill(torch.ones(T, T, dtype=torch.bool, device=S.device).triu(1), float("-inf"))
    lse = torch.logsumexp(S, dim=-1)
    P = torch.exp(S - lse.unsqueeze(-1))
    O = P @ v
    dV = P.transpose(-1, -2) @ do
    dP = do @ v.transpose(-1, -2)
    delta = (do * O).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    dQ = scale * (dS @ k)
    dK = scale * (dS.transpose(-1, -2) @ q)
    # budgets
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


def attn_autograd(qkv, dout, scale):
    """The same gradients from fp64 autograd through the explicit softmax (checks attn_ref's closed forms)."""
    x = qkv.double().clone().requires_grad_(True)
    q, k, v = x.permute(2, 0, 3, 1, 4)
    T = q.shape[-2]
    S = scale * (q @ k.transpose(-1, -2))
    S = S.masked_fill(torch.ones(T, T, dtype=torch.bool, device=S.device).triu(1), float("-inf"))
    O = (torch.softmax(S, dim=-1) @ v).permute(0, 2, 1, 3)
    O.backward(dout.double())
    return O.detach(), x.grad


def tile_row_max(qkv, scale, tile=64):
    """[B, H, T, T / tile]: max over the visible (j <= i) keys of each 64-key tile of S_ij * log2(e); -inf
    where the whole tile is above the diagonal."""
    q, k, _ = qkv.double().permute(2, 0, 3, 1, 4)
    T = q.shape[-2]
    S = scale * LOG2E * (q @ k.transpose(-1, -2))
    S = S.masked_fill(torch.ones(T, T, dtype=torch.bool, device=S.device).triu(1), float("-inf"))
    return S.view(*S.shape[:-1], T // tile, tile).amax(-1)


def deferred_max_trace(tmax, th=8.0):
    """The forward's deferred running max replayed on tile_row_max's output: the max moves only when a tile's
    row max exceeds it by more than ``th``.  Returns (rescales on a tile after the row's first, largest
    deferred excess, smallest distance of any decision from the threshold), per row: [B, H, T] each."""
    m = torch.full_like(tmax[..., 0], float("-inf"))
    later = torch.zeros_like(m)
    defer = torch.zeros_like(m)
    dist = torch.full_like(m, float("inf"))
    started = torch.zeros_like(m, dtype=torch.bool)
    for t in range(tmax.shape[-1]):
        mc = tmax[..., t]
        vis = torch.isfinite(mc)
        need = vis & (mc > m + th)
        later += (need & started).double()
        ex = torch.where(vis & started & ~need, mc - m, torch.zeros_like(m))
        defer = torch.maximum(defer, ex)
        d = torch.where(vis & started, (mc - m - th).abs(), torch.full_like(m, float("inf")))
        dist = torch.minimum(dist, d)
        m = torch.where(need, mc, m)
        started |= vis
    return later, defer, dist


def staircase_qkv(T, jumps, a_hi=8.0, reverse=False, seed=0, D=64, tile=64, block=16):
    """[1, T, 3, H, D] bf16 (H = len(jumps)) with q_i = a_i u + 0.5 n_i, k_j = b_j u + 0.5 n'_j, u a unit
    vector and the noise orthogonal to it: a_i alternates a_hi / 0 in blocks of ``block`` rows, b_j steps once
    per key tile by the amount that moves an a_hi row's scaled score by jumps[h] log2 units (``reverse``:
    falling with j instead of rising).  v is randn."""
    g = torch.Generator().manual_seed(seed)
    H = len(jumps)
    scale = 1.0 / math.sqrt(D)
    u = torch.randn(D, generator=g, dtype=torch.float64)
    u /= u.norm()

    def noise():
        n = torch.randn(T, H, D, generator=g, dtype=torch.float64)
        return n - (n @ u).unsqueeze(-1) * u

    i = torch.arange(T)
    a = torch.where((i // block) % 2 == 0, torch.tensor(a_hi, dtype=torch.float64), torch.tensor(0.0, dtype=torch.float64))
    step = i // tile
    if reverse:
        step = step.max() - step
    qkv = torch.empty(1, T, 3, H, D, dtype=torch.float64)
    nq, nk = noise(), noise()
    for h, J in enumerate(jumps):
        db = J / (a_hi * scale * LOG2E)
        b = step.double() * db
        qkv[0, :, 0, h] = a.unsqueeze(-1) * u + 0.5 * nq[:, h]
        qkv[0, :, 1, h] = b.unsqueeze(-1) * u + 0.5 * nk[:, h]
    qkv[0, :, 2] = torch.randn(T, H, D, generator=g, dtype=torch.float64)
    return qkv.to(torch.bfloat16), a


def attn_emulate(qkv, dout, scale, tile=64, th=8.0):
    """Torch emulation of the kernels' roundings (measures what the algorithm itself costs against attn_ref):
    per 64-key tile a deferred running max, P rounded to bf16 before it meets V and before it is summed into
    l, fp32 accumulation, a bf16 O; backward with P = exp2(s - lse2) from the forward's fp32 lse2, delta from
    the bf16 O, dS rounded to bf16, fp32 accumulation, bf16 outputs.  Returns (out, lse2, dqkv) like the
    kernels (bf16, fp32, bf16)."""
    bf = torch.bfloat16
    q, k, v = qkv.float().permute(2, 0, 3, 1, 4)
    do = dout.float().permute(0, 2, 1, 3)
    B, H, T, D = q.shape
    sl2 = scale * LOG2E
    s2 = (q @ k.transpose(-1, -2)) * sl2
    mask = torch.ones(T, T, dtype=torch.bool, device=q.device).triu(1)
    s2 = s2.masked_fill(mask, float("-inf"))
    m = torch.full((B, H, T), float("-inf"), device=q.device)
    l = torch.zeros(B, H, T, device=q.device)
    acc = torch.zeros(B, H, T, D, device=q.device)
    for t in range(T // tile):
        st = s2[..., t * tile:(t + 1) * tile]
        mc = st.amax(-1)
        vis = torch.isfinite(mc)
        need = vis & (mc > m + th)
        alpha = torch.where(need, torch.exp2(m - mc), torch.ones_like(m))
        m = torch.where(need, mc, m)
        l, acc = l * alpha, acc * alpha.unsqueeze(-1)
        p = torch.where(vis.unsqueeze(-1), torch.exp2(st - m.unsqueeze(-1)), torch.zeros_like(st)).to(bf).float()
        l = l + p.sum(-1)
        acc = acc + p @ v[..., t * tile:(t + 1) * tile, :]
    out = (acc / l.unsqueeze(-1)).to(bf)
    lse2 = m + torch.log2(l)
    P = torch.exp2(s2 - lse2.unsqueeze(-1)).masked_fill(mask, 0.0)
    delta = (do * out.float()).sum(-1, keepdim=True)
    dS = (P * (do @ v.transpose(-1, -2) - delta)).to(bf).float()
    Pb = P.to(bf).float()
    dV = (Pb.transpose(-1, -2) @ do).to(bf)
    dQ = ((dS @ k) * scale).to(bf)
    dK = ((dS.transpose(-1, -2) @ q) * scale).to(bf)

    def lay(a):
        return a.permute(0, 2, 1, 3).contiguous()

    return lay(out), lse2, torch.stack([lay(dQ), lay(dK), lay(dV)], dim=2)


# -------------------------------------------------------------- cross-entropy
def ce_ref(z, labels, V, grad_scale=1.0, ignore_index=-100):
    """z [B, ld] (the kernel's input values), labels [B] -> fp64 (loss rows [B] with 0 on ignored rows,
    gradient [B, ld] = (softmax - onehot) * grad_scale with ignored rows and padding columns 0, argmax [B],
    valid [B] bool)."""
    zz = z.double()[:, :V]
    logp = torch.log_softmax(zz, dim=-1)
    valid = labels != ignore_index
    safe = torch.where(valid, labels, torch.zeros_like(labels))
    loss = torch.where(valid, -logp.gather(1, safe.unsqueeze(1)).squeeze(1), torch.zeros_like(logp[:, 0]))
    g = torch.exp(logp)
    g.scatter_add_(1, safe.unsqueeze(1), -torch.ones_like(g[:, :1]))
    g = g * grad_scale * valid.unsqueeze(1).double()
    full = torch.zeros(z.shape, dtype=torch.float64, device=z.device)
    full[:, :V] = g
    return loss, full, zz.argmax(1), valid


# ------------------------------------------------------------------ LayerNorm
def ln_ref(x, w, b=None, eps=1e-5):
    """fp64 (y, mean, rstd, xhat) of LayerNorm over the last dim (biased variance)."""
    xd = x.double()
    mean = xd.mean(-1, keepdim=True)
    var = ((xd - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = (xd - mean) * rstd
    y = xh * w.double()
    if b is not None:
        y = y + b.double()
    return y, mean.squeeze(-1), rstd.squeeze(-1), xh


def ln_bwd_ref(dy, x, w, eps=1e-5):
    """fp64 (dx, dw, db) of LayerNorm's backward, from the definition dx = rstd (g - mean(g) - xhat mean(g xhat))."""
    _, _, rstd, xh = ln_ref(x, w, None, eps)
    dyd = dy.double()
    g = dyd * w.double()
    dx = rstd.unsqueeze(-1) * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    return dx, (dyd * xh).sum(0), dyd.sum(0)


# ----------------------------------------------------------------------- GELU
_K0, _K1 = math.sqrt(2.0 / math.pi), 0.044715


def gelu_ref(x):
    xd = x.double()
    return 0.5 * xd * (1.0 + torch.tanh(_K0 * (xd + _K1 * xd ** 3)))


def gelu_grad_ref(x):
    xd = x.double()
    t = torch.tanh(_K0 * (xd + _K1 * xd ** 3))
    return 0.5 * (1.0 + t) + 0.5 * xd * (1.0 - t * t) * _K0 * (1.0 + 3.0 * _K1 * xd * xd)
