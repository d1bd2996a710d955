"""fp64 references of mixup / cutmix, shared by the CPU and the GPU tests.

The decision row (fp32[8]):  [w_pix, w_lab, x1, y1, x2, y2, mode, lam_raw], mode 0 none / 1 mixup / 2 cutmix.

Pixel rule (partner of image n: image (n - 1) mod N, i.e. x.roll(1, 0)):
    inside the box [y1:y2, x1:x2] (clamped into the image)   out = x_partner
    outside                                                  out = w_pix x + (1 - w_pix) x_partner
then one round-to-nearest-even rounding to bf16.

Box rule (torchvision's): centre (r_x, r_y), half sizes int(0.5 sqrt(1 - lam) W) and int(0.5 sqrt(1 - lam) H),
clamped to the image; w_lab = 1 - (x2 - x1)(y2 - y1) / (H W).

Two-label cross-entropy per non-ignored row (V classes, eps = label_smoothing, zl = z_loss, w = the weight of y):
    zmix   = w z_y + (1 - w) z_y2
    loss_i = (1 - eps)(lse - zmix) + eps (lse - mean_j z_j) + zl lse^2
    d/dz_j = p_j (1 + 2 zl lse) - eps / V - (1 - eps) w [j = y] - (1 - eps)(1 - w) [j = y2]
A row is ignored iff labels[row] == ignore_index; labels2[row] == ignore_index means no partner (w = 1).

Which Philox-4x32-10 words feed which decision (mix_draw_kernel, csrc/kernels/mix.hip).  Row i of a launch uses
key = seed and counter = (stream, offset + i, k), k being the fourth counter word:
    k = 0               word 0: mix at all (u < prob)     word 1: cutmix over mixup (u < switch_prob)
                        word 2: r_x = (word * W) >> 32    word 3: r_y = (word * H) >> 32
    k = 1 + 13 g + t    trip t < 12 of Gamma draw g in {0, 1}: words 0, 1 the Box-Muller normal, word 2 the
                        acceptance uniform of Marsaglia-Tsang
    k = 1 + 13 g + 12   word 0: the boost uniform U^(1 / alpha) of Gamma draw g when alpha < 1
with u = ((word >> 8) + 0.5) / 2^24 and lam = G0 / (G0 + G1).
"""
import numpy as np
import torch
import torch.nn.functional as F


# ------------------------------------------------------------------ pixels
def clamp_box(row, H, W):
    """(x1, y1, x2, y2) of a row as the kernels use it: each value clamped into the image, then truncated."""
    r = [float(v) for v in row]
    cl = lambda v, hi: 0 if v != v else int(min(max(v, 0.0), float(hi)))  # noqa: E731  (a NaN clamps to 0)
    return cl(r[2], W), cl(r[3], H), cl(r[4], W), cl(r[5], H)


def box_mask(row, H, W):
    x1, y1, x2, y2 = clamp_box(row, H, W)
    m = torch.zeros(H, W, dtype=torch.bool)
    if x2 > x1 and y2 > y1:
        m[y1:y2, x1:x2] = True
    return m


def mix_pixels(x, row):
    """The pixel rule in fp64 on an NCHW batch (any float dtype), before the bf16 rounding."""
    x64 = x.double().cpu()
    xp = x64.roll(1, 0)
    w = float(row[0])
    out = w * x64 + (1.0 - w) * xp
    m = box_mask(row, x.shape[-2], x.shape[-1])
    return torch.where(m, xp, out)


def pack_s2d(v):
    """NCHW [N,C<=4,H,W] -> [N,H/2,W/2,16], channel (ay * 2 + ax) * 4 + c, zeros for c >= C (same dtype)."""
    N, C, H, W = v.shape
    out = torch.zeros(N, H // 2, W // 2, 16, dtype=v.dtype)
    for ay in range(2):
        for ax in range(2):
            for c in range(C):
                out[..., (ay * 2 + ax) * 4 + c] = v[:, c, ay::2, ax::2]
    return out


def pack_nhwc(v, cpad):
    N, C, H, W = v.shape
    out = torch.zeros(N, H, W, max(C, cpad), dtype=v.dtype)
    out[..., :C] = v.permute(0, 2, 3, 1)
    return out


def bf16_round(v64):
    """fp64 -> the nearest bf16 (ties to even), as fp64; straight from fp64 (through fp32 it would round twice)."""
    a = v64.detach().cpu().numpy().astype(np.float64)
    m, e = np.frexp(a)  # a = m 2^e, 0.5 <= |m| < 1: bf16 keeps 8 significant bits
    q = np.rint(m * 256.0) / 256.0  # np.rint: ties to even
    return torch.from_numpy(np.ldexp(q, e))


# --------------------------------------------------------------------- box
def cutmix_box(lam, r_x, r_y, H, W):
    r = 0.5 * np.sqrt(max(0.0, 1.0 - float(lam)))
    hw, hh = int(r * W), int(r * H)
    return max(r_x - hw, 0), max(r_y - hh, 0), min(r_x + hw, W), min(r_y + hh, H)


def half_sizes(lam, H, W):
    r = 0.5 * np.sqrt(np.maximum(0.0, 1.0 - np.asarray(lam, dtype=np.float64)))
    return np.floor(r * W), np.floor(r * H)


# ---------------------------------------------------------------------- CE
def _second(y, y2, w, ign):
    B = len(y)
    w = torch.as_tensor(w, dtype=torch.float64).reshape(-1).cpu()
    w = w.expand(B).clone() if w.numel() == 1 else w.clone()
    none = y2 == ign
    w[none.cpu()] = 1.0
    return torch.where(none, y, y2), w.to(y.device)


def ce_autograd_ref(z64, y, y2, w, V, eps, zl, ign=-100):
    """(mean loss, gradient of the rows' sum [B, ld]) by torch autograd in fp64 on the soft target
    w onehot(y) + (1 - w) onehot(y2): F.cross_entropy with label_smoothing, plus zl * lse^2."""
    zz = z64[:, :V].detach().clone().requires_grad_(True)
    keep = y != ign
    n = int(keep.sum())
    full = torch.zeros_like(z64)
    if n == 0:
        return 0.0, full
    yy2, ww = _second(y, y2, w, ign)
    tgt = ww[:, None] * F.one_hot(y.clamp(min=0), V).double() + (1.0 - ww)[:, None] * F.one_hot(yy2.clamp(min=0), V).double()
    rows = F.cross_entropy(zz, tgt, reduction="none", label_smoothing=eps) + zl * torch.logsumexp(zz, dim=1).square()
    tot = (rows * keep).sum()
    (g,) = torch.autograd.grad(tot, zz)
    full[:, :V] = g
    return tot.item() / n, full


def ce_formula_ref(z64, y, y2, w, V, eps, zl, ign=-100, drop=None):
    """The same by the closed formula; ``drop="partner"`` leaves the y2 term out of loss and gradient (a reference
    crippled on purpose: the kernel's bound must not pass against it)."""
    assert drop in (None, "partner")
    zz = z64[:, :V]
    keep = y != ign
    n = max(int(keep.sum()), 1)
    yy2, ww = _second(y, y2, w, ign)
    lse = torch.logsumexp(zz, dim=1)
    p = torch.softmax(zz, dim=1)
    yy = y.clamp(min=0)
    zy = zz.gather(1, yy[:, None])[:, 0]
    zy2 = zz.gather(1, yy2.clamp(min=0)[:, None])[:, 0]
    w2 = torch.zeros_like(ww) if drop == "partner" else 1.0 - ww
    g = p * (1.0 + 2.0 * zl * lse)[:, None] - eps / V
    ar = torch.arange(len(y), device=z64.device)
    g[ar, yy] -= (1.0 - eps) * ww
    g[ar, yy2.clamp(min=0)] -= (1.0 - eps) * w2
    g[~keep] = 0.0
    rows = (1.0 - eps) * (lse - ww * zy - w2 * zy2) + eps * (lse - zz.mean(dim=1)) + zl * lse.square()
    full = torch.zeros_like(z64)
    full[:, :V] = g
    return (rows * keep).sum().item() / n, full


def mix_bound(E0):
    """Max-abs bound of the fp32 gradients of the two-label kernels: _ce_reg_ref.f32_bound (2 E0 + 2^-23) plus one more
    2^-23 for the extra multiply and subtraction at the two label columns."""
    return 2.0 * E0 + 2.0 ** -22


# ------------------------------------------------------------ distributions
def betainc_quad(alpha, x, n=4001):
    """Regularised incomplete beta I_x(alpha, alpha) by composite Simpson in t with u = t^(1/alpha): the integrand
    u^(alpha-1) (1-u)^(alpha-1) du becomes (1/alpha)(1 - t^(1/alpha))^(alpha-1) dt, without the singularity at 0.
    x > 1/2 goes through the symmetry I_x = 1 - I_(1-x), so the one at u = 1 is never approached."""
    x = np.atleast_1d(np.asarray(x, dtype=np.float64))

    def half(xx):  # integral over u in [0, xx], xx <= 1/2
        T = xx ** alpha
        t = np.linspace(0.0, 1.0, n)[None, :] * T[:, None]
        f = (1.0 - t ** (1.0 / alpha)) ** (alpha - 1.0) / alpha
        wts = np.ones(n)
        wts[1:-1:2], wts[2:-1:2] = 4.0, 2.0
        return (f * wts).sum(axis=1) * (T / (n - 1)) / 3.0

    total = 2.0 * half(np.array([0.5]))[0]
    lo = half(np.minimum(x, 1.0 - x)) / total
    return np.clip(np.where(x <= 0.5, lo, 1.0 - lo), 0.0, 1.0)


def ks_sup(sample, cdf):
    """sup |F_n - F| of a sample against a CDF given as a function, both one-sided gaps at every sample point."""
    s = np.sort(np.asarray(sample, dtype=np.float64))
    n = len(s)
    F_ = cdf(s)
    return max(np.max(np.arange(1, n + 1) / n - F_), np.max(F_ - np.arange(0, n) / n))


def ks_sup_discrete(values, K):
    """sup |F_n - F| for integer values against the uniform distribution on 0..K-1."""
    cnt = np.bincount(np.asarray(values, dtype=np.int64), minlength=K)[:K]
    Fn = np.cumsum(cnt) / len(values)
    return float(np.max(np.abs(Fn - np.arange(1, K + 1) / K)))


def check_lam_sample(lam, alpha, tol=0.03):
    """The distribution check the GPU draw is held to, as a function so a torch fp64 Beta sample can go through the
    same code: returns sup |F_n - F| against the exact Beta(alpha, alpha) CDF and asserts it is within tol."""
    lam = np.asarray(lam, dtype=np.float64)
    assert np.all((lam >= 0.0) & (lam <= 1.0))
    d = ks_sup(lam, lambda v: betainc_quad(alpha, v))
    assert d <= tol, (alpha, d)
    return d
