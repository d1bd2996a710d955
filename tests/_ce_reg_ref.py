"""fp64 references of the label-smoothed / z-loss cross-entropy, shared by the CPU and the GPU tests.

Per non-ignored row, V classes, eps = label_smoothing, lam = z_loss:
    loss_i = (1 - eps)(lse - z_y) + eps (lse - mean_j z_j) + lam lse^2
    d/dz_j = p_j (1 + 2 lam lse) - (1 - eps)[j = y] - eps / V
The loss is the mean over the non-ignored rows; the gradients here are those of the rows' SUM (what the kernel
writes: the 1 / count goes in afterwards).  Columns >= V and ignored rows have gradient 0.
"""
import torch
import torch.nn.functional as F

DROPS = ("eps_over_V", "label_weight", "z_factor")


def autograd_ref(z64, y, V, eps, lam, ign=-100):
    """(mean loss, gradient of the rows' sum [B, ld]) by torch autograd in fp64: F.cross_entropy with
    label_smoothing plus lam * mean(logsumexp^2) over the non-ignored rows."""
    zz = z64[:, :V].detach().clone().requires_grad_(True)
    keep = y != ign
    n = int(keep.sum())
    full = torch.zeros_like(z64)
    if n == 0:
        return 0.0, full
    loss = F.cross_entropy(zz, y, label_smoothing=eps, ignore_index=ign)
    loss = loss + lam * (torch.logsumexp(zz, dim=1).square() * keep).sum() / n
    (g,) = torch.autograd.grad(loss * n, zz)
    full[:, :V] = g
    return loss.item(), full


def formula_ref(z64, y, V, eps, lam, ign=-100, drop=None):
    """The same by the closed formula; ``drop`` leaves one term out (a reference crippled on purpose)."""
    assert drop is None or drop in DROPS
    zz = z64[:, :V]
    keep = y != ign
    n = max(int(keep.sum()), 1)
    lse = torch.logsumexp(zz, dim=1)
    p = torch.softmax(zz, dim=1)
    yy = y.clamp(min=0)
    zy = zz.gather(1, yy[:, None])[:, 0]
    on = 1.0 if drop == "label_weight" else 1.0 - eps
    off = 0.0 if drop == "eps_over_V" else eps / V
    zl = 0.0 if drop == "z_factor" else lam
    g = p * (1.0 + 2.0 * zl * lse)[:, None] - off
    g[torch.arange(len(y)), yy] -= on
    g[~keep] = 0.0
    rows = on * (lse - zy) + (V * off) * (lse - zz.mean(dim=1)) + zl * lse.square()
    full = torch.zeros_like(z64)
    full[:, :V] = g
    return (rows * keep).sum().item() / n, full


def f32_bound(E0):
    """Max-abs bound of the fp32 gradients: twice the plain kernel's own error on the same logits (the new arm
    adds one subtraction and one multiply per element) plus one fp32 ulp of 1."""
    return 2.0 * E0 + 2.0 ** -23


def sensitivity(z64, y, V, eps, lam, grad_bound, loss_rel_bound=1e-4):
    """How far each crippled reference is from the true one, in units of the bound the kernel is held to:
    {drop: (gradient max-abs distance / grad_bound, loss relative distance / loss_rel_bound)} for the terms
    that (eps, lam) switch on.  A bound that could not see a missing term would give ratios below 1."""
    loss, g = formula_ref(z64, y, V, eps, lam)
    out = {}
    for drop in DROPS:
        if (drop == "z_factor" and lam == 0.0) or (drop != "z_factor" and eps == 0.0):
            continue
        l2, g2 = formula_ref(z64, y, V, eps, lam, drop=drop)
        out[drop] = ((g2 - g).abs().max().item() / grad_bound, abs(l2 - loss) / abs(loss) / loss_rel_bound)
    return out
