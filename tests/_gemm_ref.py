"""Independent fp64 references of the dense GEMM kernels (imported by test_gemm_kernels_gpu.py and
test_gemm_ref_cpu.py): plain torch in float64, straight from the definitions, from the values the kernel sees
(bf16 operands widened).  No kernel code.

    gemm_ref(A, B, layout, ...)        y, its magnitude sum (for the budgets) and, for TN, the bias gradient
    int_case(M, N, K, layout, out)     Tier A: integer operands whose every fp32 partial sum is exact
    randn_case(M, N, K, layout)        Tier B: randn operands, bias, residual, accumulator, pre-activation
    b_f32 / b_bf16 / b_gelu / b_gelu_bwd / b_db    Tier B budgets, evaluated on the reference
    emulate(...)                       the kernels' roundings in fp32 torch (no kernel)
    gelu_fast32 / gelu_grad_fast32     hgemm.hip's exp-based GELU formulas in fp32 torch

Layouts (operand shapes as the kernels take them): "nt" A [M, K], B [N, K] (y = x w^T); "nn" A [M, K], B [K, N]
(dx = dy w); "tn" A [K, M], B [K, N] (dw = dy^T x).

Rounding constants: U = 2^-8 (one rounding to bf16) and u32 = 2^-24 (one fp32 rounding), as derived in
_resnet_ref.py; none is tuned to a kernel.  A sum of K exact products accumulated in fp32 in any order is off by
at most (K - 1) u32 sum|terms|; a K split adds one addition per slab, and the epilogue multiplies by alpha, adds
the bias and the residual or the old contents (<= 4 more roundings): (K + splits + 4) u32 mag.

GELU.  hgemm.hip evaluates g = x / (1 + e), e = exp(a), a = -2 sqrt(2 / pi) (x + 0.044715 x^3), and
t = 1 - 2 / (1 + exp(-a)) with the hardware's exp (exp2 of a rounded product) and reciprocal.  The terms
G_C u32 max(1, |x|) and GP_C u32 w(x), w = 1 + |x| k0 (1 + 3 k1 x^2), are the error of those formulas in fp32 torch
against fp64 over [-12, 12] as test_gemm_ref_cpu.py measures it (1.98 and 2.45; the constants are those figures
rounded up, not multiples of them).  An error dt of t enters gelu' = (1 + t) / 2 + x (1 - t^2) k0 (1 + 3 k1 x^2) / 2
as dt (1 / 2 + |x t| k0 (1 + 3 k1 x^2)) <= dt w.  On top of the measured terms the hardware's part is derived, not
measured: its reciprocal is good to 1 ulp (torch's division to 1/2), and its exp to 1 ulp of a result whose argument
was rounded once more, a relative error eps <= (|a| + 1) u32 of e.
  g:  the reciprocal adds u32 |g|; eps enters g as eps e / (1 + e) |g|, which is <= u32 |g| for a <= 0 ((|a| + 1)
      e^-|a| <= 1) and, for a > 0 (x < 0, where |x| <= a / 1.6), <= u32 a (a + 1) / (1.6 (1 + e^a)) <= 0.5 u32:
      G_HW = (2 |g| + 0.5) u32.
  t:  the reciprocal r <= 1 adds 2 u32 r <= 2 u32; eps enters t as 2 e / (1 + e)^2 eps <= 0.75 u32 (the maximum of
      2 (|a| + 1) e^a / (1 + e^a)^2, at |a| = 1.5): GP_HW = 3 u32 w.

bf16 residual on the implicit GEMM (igemm.hip finish_row): the tile is packed to bf16 first, then unpacked, the bf16
residual added in fp32 and the sum packed again -- two bf16 roundings, of y0 = alpha acc + bias and of y0 + res.  The
one-rounding budget U |y| + f32 term is therefore exceeded by the algorithm itself (emulate(res_bf16=...) is at
70 - 130 times it in fp32 torch where y0 and the residual cancel, test_gemm_ref_cpu.py::test_bf16_residual_rounds_twice); b_bf16_res counts both:
U (|y0| + f) + f + U |y0 + res| with f the fp32 term (the fp32 add of two bf16 values of magnitude <= 2^8 apart in
exponent is within u32, inside f's slack of 4 roundings).

gemm_f32.hip (fp32 operands: the products are not exact): a k-ordered fma chain, K roundings, then alpha, the
bias and, for the weight grad, the add into dw, one rounding each: (K + extra) u32 mag with extra = 0 for the
plain product.  The K u32 mag this started from misses by 1.49 at K = 1 with a bias in plain fp32 torch
(test_gemm_ref_cpu.py::test_f32_cases prints it): u32 |a b| + u32 |a b + bias| against u32 (|a b| + |bias|).
"""
import functools

import torch

from _gpt2_ref import gelu_grad_ref, gelu_ref
from _resnet_ref import FLOOR, INT_MAX, U, u32

BF = torch.bfloat16
LAYOUTS = {"nt": (True, True), "nn": (True, False), "tn": (False, False)}  # (a_k, b_k) of the raw entry
CFGS = {"nt": [0, 1, 2, 3], "nn": [0, 1], "tn": [0]}                       # gemm.cpp layout_ok
TILE = {0: (256, 256), 1: (128, 256), 2: (256, 128), 3: (128, 128)}
ALPHA_T = 0.25            # the device scalar multiplied into alpha (a power of two, as every Tier A alpha)
G_C = 2.0                 # measured 1.98 (u32 per max(1, |x|)): the formula in fp32 torch against fp64
GP_C = 2.5                # measured 2.45 (u32 per w(x))
GP_HW = 3.0               # derived: the hardware reciprocal and exp inside t (u32 per w(x))
_K0, _K1 = 0.7978845608028654, 0.044715


# ================================================================== reference
def _mats(A, B, layout):
    """(A as [M, K], B as [K, N]) in float64."""
    Ad, Bd = A.double(), B.double()
    return (Ad.t() if layout == "tn" else Ad), (Bd.t() if layout == "nt" else Bd)


def gemm_ref(A, B, layout, alpha=1, bias=None, residual=None, acc=None):
    """fp64 y = alpha A B (+ bias per column) (+ residual) (+ acc) -> dict(y, mag) with
    mag = |alpha| sum_k |a||b| + |bias| + |residual| + |acc|; for "tn" also db = alpha sum_k A[k][m] and
    db_mag = |alpha| sum_k |A[k][m]| (the fused bias gradient: row sums of A^T)."""
    Am, Bm = _mats(A, B, layout)
    y = alpha * (Am @ Bm)
    mag = abs(alpha) * (Am.abs() @ Bm.abs())
    for t in (bias, residual, acc):
        if t is not None:
            y = y + t.double()
            mag = mag + t.double().abs()
    out = {"y": y, "mag": mag}
    if layout == "tn":
        out["db"] = alpha * Am.sum(1)
        out["db_mag"] = abs(alpha) * Am.abs().sum(1)
    return out


# ==================================================================== budgets
def b_f32(mag, K, splits=1):
    return (K + splits + 4) * u32 * mag + FLOOR


def b_f32_plain(mag, K, extra=0):
    """gemm_f32.hip: K roundings of the fma chain + ``extra`` epilogue roundings (alpha, bias, the add into dw)."""
    return (K + extra) * u32 * mag + FLOOR


def gp_weight(x):
    xd = x.double()
    return 1.0 + xd.abs() * _K0 * (1.0 + 3.0 * _K1 * xd * xd)


def b_bf16(y, mag, K, splits=1):
    return U * y.abs() + b_f32(mag, K, splits)


def b_bf16_res(y0, mag, res, K, splits=1):
    """A bf16 output rounded, a bf16 residual added in fp32, the sum rounded again (the module docstring)."""
    f = b_f32(mag, K, splits)
    return U * (y0.abs() + f) + f + U * (y0 + res.double()).abs()


def b_db(db, db_mag, K, splits=1, db0=None):
    """The fused bias gradient: K additions, the slab sums, alpha, and the add into the buffer."""
    tot = db if db0 is None else db + db0.double()
    return (K + splits + 4) * u32 * (db_mag + tot.abs()) + FLOOR


def b_gelu(v, mag, K, splits=1):
    """(gelu(v), bound) of bf16(gelu(v')) where v' is the fp32 pre-activation (v within b_f32 of it): one bf16
    rounding of the output, the function's change over the pre-activation's budget (both ends; |gelu'| <= 1.13
    and gelu is monotone outside [-0.76, 0], so the ends and 1.13 b bound it), and the fp32 evaluation."""
    b = b_f32(mag, K, splits)
    g = gelu_ref(v)
    dg = torch.maximum((gelu_ref(v + b) - g).abs(), (gelu_ref(v - b) - g).abs())
    dg = torch.maximum(dg, torch.where(v.abs() < 1.0, 1.13 * b, torch.zeros_like(b)))
    return g, U * g.abs() + dg + (G_C * v.abs().clamp(min=1.0) + 2.0 * g.abs() + 0.5) * u32 + FLOOR


def b_gelu_bwd(s, mag, aux, K, splits=1):
    """(s gelu'(aux), bound) of bf16(s' gelu'(aux)) with s' the fp32 alpha * acc: one bf16 rounding, s's budget
    times |gelu'|, the derivative's fp32 evaluation times |s|, and the fp32 product."""
    gp = gelu_grad_ref(aux)
    y = s * gp
    return y, U * y.abs() + b_f32(mag, K, splits) * gp.abs() + (GP_C + GP_HW) * u32 * gp_weight(aux) * s.abs() + u32 * y.abs() + FLOOR


def gelu_fast32(x):
    """hgemm.hip gelu_fwd in fp32 torch: x / (1 + exp(-2 u)), u = sqrt(2 / pi) (x + 0.044715 x^3)."""
    x = x.float()
    return x / (1.0 + torch.exp(-1.5957691216057308 * (x + 0.044715 * x * x * x)))


def gelu_grad_fast32(x):
    """hgemm.hip gelu_grad in fp32 torch: t = 1 - 2 / (1 + exp(2 u))."""
    x = x.float()
    k0, k1 = 0.7978845608028654, 0.044715
    t = 1.0 - 2.0 / (1.0 + torch.exp(2.0 * k0 * (x + k1 * x * x * x)))
    return 0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * k0 * (1.0 + 3.0 * k1 * x * x)


# ================================================================== emulation
def split_bounds(K, splits):
    """The planner's K ranges: kt = ceil(K-tiles / splits) tiles of 64 per split, the last one shorter."""
    kt = (K // 64 + splits - 1) // splits if K % 64 == 0 else -(-K // splits)
    step = kt * 64 if K % 64 == 0 else kt
    return [(k, min(K, k + step)) for k in range(0, K, step)]


def emulate(A, B, layout, alpha=1.0, bias=None, residual=None, acc=None, splits=1, out="f32", act=None, aux=None,
            res_bf16=None):
    """The kernels' roundings in fp32 torch: fp32 accumulate per K split, the partials summed in split order,
    v = alpha s + bias (+ residual | + acc) in fp32, one output rounding.  act "gelu": returns (bf16 gelu(v),
    bf16 v); "gelu_bwd": bf16(alpha s * gelu'(aux)); "relu".  ``res_bf16``: the implicit GEMM's bf16 residual,
    bf16(bf16(v) + res) with the add in fp32."""
    Am, Bm = _mats(A, B, layout)
    Am, Bm = Am.float(), Bm.float()
    K = Am.shape[1]
    s = None
    for k0, k1 in split_bounds(K, splits):
        part = Am[:, k0:k1] @ Bm[k0:k1]
        s = part if s is None else s + part
    v = s * float(alpha)
    if bias is not None:
        v = v + bias.float()
    if residual is not None:
        v = v + residual.float()
    if acc is not None:
        v = v + acc.float()
    if act == "gelu":
        return gelu_fast32(v).to(BF), v.to(BF)
    if act == "gelu_bwd":
        return (v * gelu_grad_fast32(aux)).to(BF)
    if act == "relu":
        v = v.clamp(min=0)
    if res_bf16 is not None:
        return (v.to(BF).float() + res_bf16.float()).to(BF)
    return v.to(BF) if out == "bf16" else v


def emulate_db(A, alpha=1.0, db0=None, splits=1):
    Am = A.float().t()
    s = None
    for k0, k1 in split_bounds(Am.shape[1], splits):
        part = Am[:, k0:k1].sum(1)
        s = part if s is None else s + part
    s = s * float(alpha)
    return s if db0 is None else s + db0.float()


# ========================================================================= cases
def _shapes(M, N, K, layout):
    return ((K, M) if layout == "tn" else (M, K)), ((N, K) if layout == "nt" else (K, N))


def _pattern(shape, gen, lo, hi, dens, phase=1):
    """Integers in [lo, hi] (sparse with density ``dens``), then made distinct per row and per column: element
    (i, j) with (i + j) % 7 == 0 is set to 1 + (i % 3) - (j % 2) * 3 in {-2 .. 3} clipped to the range -- a term
    that depends on both indices -- and the last row and last column are made nonzero."""
    v = torch.randint(lo, hi + 1, shape, generator=gen).double()
    if dens < 1.0:
        v = v * (torch.rand(shape, generator=gen) < dens)
    i = torch.arange(shape[0]).view(-1, 1)
    j = torch.arange(shape[1]).view(1, -1)
    if dens >= 1.0:
        t = (1 + (i % 3) - (j % 2) * 3).double().clamp(lo, hi)
        v = torch.where((i + j) % 7 == 0, t, v)
    # (fill-ins +-1, +-2 whose sign follows bit ``phase`` of the index: A uses bit 1 and B bit 2, so the products
    # of two filled lines cancel over every 8 indices instead of adding up to a large corner element)
    sgn = lambda n: (((n >> phase) & 1) * 2 - 1).double()
    v[-1, :] = torch.where(v[-1, :] == 0, (1 + j[0] % 2) * sgn(j[0]), v[-1, :])
    v[:, -1] = torch.where(v[:, -1] == 0, (1 + i[:, 0] % 2) * sgn(i[:, 0]), v[:, -1])
    return v + 0.0


def _distinct(t):
    """Every row of t differs from every other row, and every column from every other column (a dimension whose
    vectors are shorter than 16 values -- M = 1, N = 8 -- cannot promise that and is left out)."""
    rows = t.shape[1] < 16 or torch.unique(t, dim=0).shape[0] == t.shape[0]
    cols = t.shape[0] < 16 or torch.unique(t, dim=1).shape[1] == t.shape[1]
    return rows and cols


def check_int_case(c):
    """The builder's claims (asserted by int_case itself and, for every case, by test_gemm_ref_cpu.py)."""
    A, B = c["A"].double(), c["B"].double()
    for name in ("A", "B", "bias", "res", "acc", "db0"):
        assert torch.equal(c[name].double(), c[name].double().round()), (c["key"], name)
    for name, t in (("A", A), ("B", B)):
        assert (t[-1] != 0).all() and (t[:, -1] != 0).all(), (c["key"], name, "last row / column")
        assert _distinct(t), (c["key"], name, "rows / columns not distinct")
    Am, Bm = _mats(A, B, c["layout"])
    s = Am @ Bm
    if s.numel() <= 2 ** 20:  # (the workload-wide outputs of the two-launch plans: the operands' check suffices)
        assert _distinct(s), (c["key"], "product rows / columns not distinct")
    assert (Am.abs() @ Bm.abs()).max().item() < 2 ** 24 / 4  # every partial sum, times any alpha <= 2, below 2^24
    if c["out"] == "bf16":
        worst = 2 * s.abs().max().item() + c["bias"].abs().max().item() + c["res"].abs().max().item()
        assert worst <= INT_MAX, (c["key"], worst)


@functools.lru_cache(maxsize=None)
def int_case(M, N, K, layout, out="f32", seed=0):
    """Tier A case: bf16 A, B in ``layout`` and fp32 bias [N], res / acc [M, N], db0 [M], all integers.
    out "f32": dense integers in [-4, 4] (|sum_k| <= 16 K, |bias|, |res|, |acc| <= 64: below 2^24 for every K
    here, with alpha <= 2).  out "bf16": sparse integers in [-2, 2] whose density shrinks until
    2 |sum_k| + |bias| + |res| <= 256 (= _resnet_ref.INT_MAX) everywhere, so every output under alpha in
    {0.25, 0.5, 1, 2} with integer bias is exact in bf16 (alpha < 1: multiples of 1/4 below 2^6).  Every fp32
    partial sum in any order is then exact, and a kernel must reproduce the fp64 reference bit for bit whatever
    tile, K split, slab order, atomics or schedule it uses.  Cached: shared between tests, never modified."""
    gen = torch.Generator().manual_seed(7000 + seed)
    sa, sb = _shapes(M, N, K, layout)
    if out == "f32":
        A, B = _pattern(sa, gen, -4, 4, 1.0, 1), _pattern(sb, gen, -4, 4, 1.0, 2)
        lim = 64
    else:
        dens = 0.5
        for _ in range(24):
            A, B = _pattern(sa, gen, -2, 2, dens, 1), _pattern(sb, gen, -2, 2, dens, 2)
            Am, Bm = _mats(A, B, layout)
            if 2 * (Am @ Bm).abs().max().item() + 8 <= INT_MAX:
                break
            dens *= 0.8
        lim = 4
    c = dict(key=(M, N, K, layout, out, seed), layout=layout, out=out, M=M, N=N, K=K, A=A.to(BF), B=B.to(BF),
             bias=torch.randint(-lim, lim + 1, (N,), generator=gen).float(),
             res=torch.randint(-lim, lim + 1, (M, N), generator=gen).float(),
             acc=torch.randint(-lim, lim + 1, (M, N), generator=gen).float(),
             db0=torch.randint(-lim, lim + 1, (M,), generator=gen).float())
    check_int_case(c)
    return c


@functools.lru_cache(maxsize=None)
def randn_case(M, N, K, layout, seed=0):
    """Tier B case: randn bf16 A, B (B scaled by 1 / sqrt(K)), fp32 randn bias / res / acc / db0 and a bf16
    randn pre-activation ``aux`` (scaled by 1.5: both tails of gelu')."""
    gen = torch.Generator().manual_seed(8000 + seed)
    sa, sb = _shapes(M, N, K, layout)
    return dict(layout=layout, M=M, N=N, K=K, A=torch.randn(sa, generator=gen).to(BF),
                B=(torch.randn(sb, generator=gen) / K ** 0.5).to(BF), bias=torch.randn(N, generator=gen),
                res=torch.randn(M, N, generator=gen), acc=torch.randn(M, N, generator=gen),
                db0=torch.randn(M, generator=gen), aux=(1.5 * torch.randn(M, N, generator=gen)).to(BF))


# ---- (a) raw hgemm: (M, N, K, splits) per layout.  Every M of {1, 255, 257, 520} (tn: {8, 264, 520}), N of
# {8, 264, 520} and K of {64, 128, 192, 832} appears with every layout (and so, the test looping over CFGS[layout],
# with every tile configuration the layout accepts); K = 832 is 13 K-tiles (3 uneven splits of 5, 5, 3), K = 576 is
# 9 (2 splits of 5, 4): the planner takes a split only with >= 4 K-tiles in it.
RAW = {
    "nt": [(1, 8, 64, 1), (255, 264, 128, 1), (257, 520, 192, 1), (520, 264, 832, 3), (257, 8, 576, 2), (520, 520, 64, 1)],
    "nn": [(1, 8, 64, 1), (255, 264, 128, 1), (257, 520, 192, 1), (520, 264, 832, 3), (257, 8, 576, 2), (520, 520, 64, 1)],
    "tn": [(8, 8, 64, 1), (264, 264, 128, 1), (520, 520, 192, 1), (520, 264, 832, 3), (264, 8, 576, 2), (8, 520, 64, 1)],
}
RAW_B = {"nt": [(257, 520, 192, 1), (520, 264, 832, 3), (255, 264, 576, 2)],
         "nn": [(257, 520, 192, 1), (520, 264, 832, 3)],
         "tn": [(264, 520, 192, 1), (520, 264, 832, 3)]}
# ---- (b) TN with the fused bias gradient: N = 776 spans four tile columns, M tails of 8 and 264
DBIAS = [(520, 776, 832), (264, 264, 128), (8, 520, 64)]
# ---- (c) several units per block: 520 x 776, 13 K-tiles
MULTI = (520, 776, 832)
# ---- (d) two-launch plans: (M, N, K) of the GEMM per layout, walked under no reserve and under a reserve of all but
# 16 CUs until C.hgemm_plan2 reports each cut axis.  With one tile configuration TN's tail only pays off K-split,
# hence K = 1024; the NN cut along N likewise needs K >= 512 (72 x 4168 x 1024: the tail in 4 K splits).
CUT_CANDIDATES = {
    "nt": [(3080, 5128, 256), (5128, 3080, 256)],
    "nn": [(72, 4168, 1024), (520, 3080, 512), (584, 5640, 256), (1096, 4872, 128)],
    "tn": [(264, 4168, 1024), (4168, 264, 1024)],
}
CUT_OUT = {"nt": ("bf16", "f32"), "nn": ("bf16",), "tn": ("f32",)}
# ---- (e) weight grads: (tokens, out_features, in_features, ldy, seed)
WGRAD_HGEMM = [(128, 264, 520, None, 0), (128, 10, 72, 16, 0), (64, 259, 136, 320, 0), (192, 8, 8, None, 0)]
WGRAD_ATOMIC = [(100, 264, 136, None, 1), (36, 10, 72, 16, 1), (1000, 72, 264, None, 1)]
GROUP_SHAPES = [(264, 520), (136, 72), (8, 8), (520, 776), (264, 264), (72, 136), (8, 520), (520, 8), (256, 256),
                (264, 520), (136, 72), (16, 24)]
GROUP_T = [64, 128]
# ---- (f) the implicit-GEMM fallbacks: linear_fwd (M, N, K, what), linear_dgrad (M, in, out, with residual)
FWD_FALLBACK = [(65, 24, 40, "k"), (130, 72, 784, "k"), (65, 72, 64, "res"), (65, 72, 128, "f32relu")]
DGRAD_FALLBACK = [(65, 72, 64, True), (130, 136, 40, False), (65, 264, 40, True)]


def wgrad_int_case(T, n_out, n_in, seed=0):
    """The Tier A case behind one weight-grad problem: dy^T as the TN A operand, out_features rounded up to 8."""
    return int_case((n_out + 7) // 8 * 8, n_in, T, "tn", "f32", seed)


def extra_tier_a():
    """(M, N, K, layout, out, seed) of every Tier A case of (d), (e) and (f)."""
    c = [(M, N, K, lay, out, 0) for lay, lst in CUT_CANDIDATES.items() for M, N, K in lst for out in CUT_OUT[lay]]
    c += [((no + 7) // 8 * 8, ni, T, "tn", "f32", seed) for T, no, ni, _, seed in WGRAD_HGEMM + WGRAD_ATOMIC]
    c += [((no + 7) // 8 * 8, ni, T, "tn", "f32", 10 + i) for T in GROUP_T for i, (no, ni) in enumerate(GROUP_SHAPES)]
    c += [(M, N, K, "nt", "f32" if what == "f32relu" else "bf16", 0) for M, N, K, what in FWD_FALLBACK]
    c += [(M, ni, no, "nn", "bf16", 0) for M, ni, no, _ in DGRAD_FALLBACK]
    return c


# ---- (g) gemm_f32.hip
F32_M, F32_N, F32_K = [1, 63, 65], [1, 10, 66], [1, 15, 17, 784]
F32_CASES = [(1, 1, 1), (63, 10, 15), (65, 66, 17), (65, 10, 784), (1, 66, 784), (63, 1, 17), (65, 66, 1), (1, 10, 15)]


@functools.lru_cache(maxsize=None)
def f32_case(M, N, K, tier, seed=0):
    """fp32 x [M, K], w [N, K], dy [M, N], bias [N], dw0 [N, K]: Tier "A" dense integers in [-4, 4] (every
    sum below 2^24: exact), Tier "B" randn.  The last row / column of each operand is nonzero in Tier A."""
    gen = torch.Generator().manual_seed(9000 + seed)
    if tier == "A":
        mk = lambda *s: _pattern(s, gen, -4, 4, 1.0).float() if len(s) == 2 else torch.randint(-4, 5, s, generator=gen).float()
    else:
        mk = lambda *s: torch.randn(*s, generator=gen)
    return dict(x=mk(M, K), w=mk(N, K), dy=mk(M, N), bias=mk(N), dw0=mk(N, K))
