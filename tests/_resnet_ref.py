"""Independent fp64 references of the ResNet-50 kernels (imported by test_resnet_kernels_gpu.py and
test_resnet_ref_cpu.py): plain torch in float64, straight from the definitions.  Every reference takes the
values the kernel sees (the bf16-rounded tensors, widened), in the kernels' layouts (NHWC activations,
[K, R, S, C] filters).

    Geom / GEOMS / ..._CASES          conv geometries and the shared case lists
    conv_ref(x, w, dy, g)             y, dx, dw by fp64 autograd (+ the rounding budgets, on request)
    int_case(g, seed)                 Tier A: sparse small-integer x, w, dy whose y, dx, dw are integers <= 256
    dyadic_bn(shape, C, seed)         Tier A: pre-BN tensor and BN coefficients on the 1/8 grid, >= 5 % at the
                                      ReLU threshold
    pack_bits(mask)                   ReLU-mask bytes as bn_apply packs them
    conv_emulate(...)                 the kernels' roundings in fp32 torch (no kernel)
    bn_case / bn_fwd_ref / bn_fwd_budgets / bn_bwd_ref / bn_emulate
    pool_case / maxpool_ref / gavg_ref

Rounding constants (none is tuned to a kernel):
  U = 2^-8: one rounding to bf16.  bf16 keeps 8 significant bits, so the spacing in [2^e, 2^(e+1)) is 2^(e-7)
            and round-to-nearest is off by at most half of it, 2^(e-8) <= 2^-8 |v| (the per-rounding figure
            _gpt2_ref.py states: "one rounding is off by up to 2^-8").
  u = 2^-24: one fp32 rounding (24 significant bits, half a spacing).  A sum of n products accumulated in
            fp32 in ANY order is off by at most (n - 1) u sum |terms| to first order; the products of two
            bf16 values are exact in fp32 (16 significant bits).  The budgets use n u sum |terms|.
No constant here is above 1: every budget is a plain count of roundings, so there is no emulation ratio to
justify a raised one (the emulations below stay at ratio <= 1 against all of them: test_resnet_ref_cpu.py).
"""
import collections
import functools

import torch
import torch.nn.functional as F

BF = torch.bfloat16
U = 2.0 ** -8
u32 = 2.0 ** -24
FLOOR = 1e-30  # added to every bound: exact zeros compare cleanly
INT_MAX = 256  # Tier A: integers of magnitude <= 256 are exact in bf16 (8 significant bits)


# =================================================================== geometry
class Geom(collections.namedtuple("Geom", "name N H W C K R S stride pad dil")):
    """x [N, H, W, C], w [K, R, S, C]; stride (sh, sw); pad [ph, pw] or [top, left, bottom, right];
    dil (dh, dw)."""
    __slots__ = ()

    @property
    def pad4(self):
        p = self.pad
        return (p[0], p[1], p[2], p[3]) if len(p) == 4 else (p[0], p[1], p[0], p[1])

    @property
    def out_hw(self):
        t, l, b, r = self.pad4
        oh = (self.H + t + b - self.dil[0] * (self.R - 1) - 1) // self.stride[0] + 1
        ow = (self.W + l + r - self.dil[1] * (self.S - 1) - 1) // self.stride[1] + 1
        return oh, ow

    @property
    def M(self):
        oh, ow = self.out_hw
        return self.N * oh * ow

    @property
    def xshape(self):
        return [self.N, self.H, self.W, self.C]

    @property
    def args(self):  # (stride, pad, dil) as the bindings take them
        return [list(self.stride), list(self.pad), list(self.dil)]


def G(name, N, H, W, C, K, k, stride=(1, 1), pad=(0, 0), dil=(1, 1)):
    R, S = (k, k) if isinstance(k, int) else k
    g = Geom(name, N, H, W, C, K, R, S, tuple(stride), tuple(pad), tuple(dil))
    oh, ow = g.out_hw
    assert oh >= 1 and ow >= 1, name
    return g


# ----- the general implicit GEMM (igemm.hip).  None of these is pointwise + write-heavy (streaming kernel),
# 64 -> 64 3x3 (row-walking kernel), the s2d stem, or has >= 256 output columns over a power-of-two >= 64
# channels (hconv_ok: persistent GEMM), so conv_fwd / conv_dgrad / conv_wgrad end in run_igemm.  There:
#   forward      A_CONV_FWD x B_DENSE_K (1x1 stride 1 pad 0: A_DENSE_K): the LDS-DMA kernel when C % 32 == 0
#                (dpe_igemm_dma_launch's envelope), else the register-staged kernel;
#   data grad    stride 1, dilation 1, not pointwise: a forward conv of dy with the flipped filter and pad
#                R-1-p (LDS-DMA kernel when K % 32 == 0); stride 1 with dilation: A_CONV_DGRAD x B_CONV_DGRAD
#                (register-staged); strided: one sub-GEMM per output parity, forward-form;
#   weight grad  A_DENSE_M x B_CONV_WGRAD: the LDS-DMA weight-grad kernel when the pixel count is a multiple
#                of 32 and 32 / OW + 1 <= OH, else the register-staged kernel with fp32 atomics.
GENERAL = [
    # H != W both ways (C = 32: LDS-DMA forward; K = 40: register-staged data grad, N tail of 64-wide tiles)
    G("g_5x9", 2, 5, 9, 32, 40, 3, pad=(1, 1)),
    G("g_9x5", 2, 9, 5, 32, 40, 3, pad=(1, 1)),
    # strides, 3x3 and 1x1; (H + 2p - k) % s != 0 in several: the last rows / columns of x lie under no window
    G("g_s12_3", 2, 6, 9, 32, 32, 3, stride=(1, 2), pad=(1, 1)),
    G("g_s21_3", 2, 9, 6, 32, 32, 3, stride=(2, 1), pad=(1, 1)),
    G("g_s22_3", 2, 8, 10, 32, 32, 3, stride=(2, 2), pad=(1, 1)),   # (8 + 2 - 3) % 2 = 1, (10 + 2 - 3) % 2 = 1
    G("g_s33_3", 2, 9, 11, 32, 32, 3, stride=(3, 3), pad=(1, 1)),   # (9 + 2 - 3) % 3 = 2, (11 + 2 - 3) % 3 = 1
    G("g_s32_3", 2, 10, 7, 32, 32, 3, stride=(3, 2), pad=(1, 1)),   # (10 + 2 - 3) % 3 = 0, (7 + 2 - 3) % 2 = 0
    G("g_s12_1", 2, 6, 9, 32, 32, 1, stride=(1, 2)),
    G("g_s21_1", 2, 9, 6, 32, 32, 1, stride=(2, 1)),
    G("g_s22_1", 2, 8, 10, 32, 32, 1, stride=(2, 2)),               # parities (1, *), (*, 1): no taps, K = 0
    G("g_s33_1", 2, 9, 11, 32, 32, 1, stride=(3, 3)),               # (9 - 1) % 3 = 2, (11 - 1) % 3 = 1
    G("g_s32_1", 2, 10, 7, 32, 32, 1, stride=(3, 2)),
    G("g_s33_3p0", 1, 11, 12, 24, 16, 3, stride=(3, 3)),            # pad 0: (11 - 3) % 3 = 2, (12 - 3) % 3 = 0
    # pads
    G("g_p01", 2, 6, 7, 32, 32, 3, pad=(0, 1)),
    G("g_p10", 2, 6, 7, 32, 32, 3, pad=(1, 0)),
    G("g_p21", 2, 6, 7, 32, 32, 3, pad=(2, 1)),
    G("g_p4", 2, 6, 7, 32, 32, 3, pad=(2, 0, 1, 2)),                # [t, l, b, r], t != b, l != r
    G("g_p4s2", 2, 7, 6, 32, 32, 3, stride=(2, 2), pad=(0, 2, 1, 1)),
    # pads above R-1: the stride-1 data grad's forward form has a NEGATIVE pad R-1-p
    G("g_p3", 1, 5, 6, 32, 32, 3, pad=(3, 3)),
    G("g_1x1p1", 2, 5, 6, 32, 32, 1, pad=(1, 1)),                   # not pointwise (is_pointwise wants pad 0)
    G("g_1x1p1c24", 2, 5, 6, 24, 40, 1, pad=(1, 1)),                # the same on the register-staged kernel
    # dilation at stride 1: forward / weight grad with dh, dw; data grad on A_CONV_DGRAD x B_CONV_DGRAD
    G("g_d22", 2, 8, 9, 32, 32, 3, pad=(2, 2), dil=(2, 2)),
    G("g_d12", 2, 7, 9, 32, 40, 3, pad=(1, 2), dil=(1, 2)),
    G("g_d22c24", 1, 8, 9, 24, 16, 3, pad=(1, 0), dil=(2, 2)),
    # non-square filters (R*S <= 32: also inside the LDS-DMA kernel's tap mask)
    G("g_1x3", 2, 5, 8, 32, 32, (1, 3), pad=(0, 1)),
    G("g_3x1", 2, 8, 5, 32, 32, (3, 1), pad=(1, 0)),
    G("g_1x7", 2, 4, 9, 32, 32, (1, 7), pad=(0, 3)),
    G("g_7x1", 2, 9, 4, 32, 32, (7, 1), pad=(3, 0)),
    G("g_2x5", 2, 6, 8, 32, 32, (2, 5), pad=(1, 2)),
    G("g_5x5", 2, 7, 8, 32, 32, 5, pad=(2, 2)),
    G("g_5x5s2", 1, 9, 12, 16, 24, 5, stride=(2, 2), pad=(2, 2)),
    # M = 1: N = 1, H = W = k, pad 0
    G("g_m1_3", 1, 3, 3, 32, 32, 3),
    G("g_m1_1", 1, 1, 1, 32, 32, 1),                                # pointwise but N < 2K: dense igemm roles
    G("g_m1_5", 1, 5, 5, 8, 8, 5),
    # channel counts: C in {8, 16, 24, 40} (register-staged; 24 and 40 are no multiple of the 32-wide K step),
    # Cout in {8, 40, 72} (72: two 64-wide N tiles with a tail of 8)
    G("g_c8", 2, 6, 7, 8, 8, 3, pad=(1, 1)),
    G("g_c16", 2, 6, 7, 16, 40, 3, pad=(1, 1)),
    G("g_c24", 2, 6, 7, 24, 72, 3, pad=(1, 1)),
    G("g_c40", 2, 6, 7, 40, 72, 3, stride=(2, 2), pad=(1, 1)),
    G("g_c40_1", 3, 5, 7, 40, 8, 1),                                # pointwise, dense loaders, K tail
    G("g_k72", 2, 6, 7, 32, 72, 3, stride=(2, 2), pad=(1, 1)),
]
STRIDED = [g.name for g in GENERAL if g.stride != (1, 1)]

# ----- persistent GEMM with an implicit-im2col operand (hgemm.hip).  Forward and stride-1 data grad: hconv_ok
# (taps, C a power of two >= 64, >= 256 output columns, R*S <= 32) and a plan_bnb plan; weight grad: Cout >= 256,
# C a power of two, pixel count % 64 == 0 (conv_wgrad's g_hgemm_conv branch).  set_hgemm_conv(False): igemm.
HGEMM = [
    G("h_3x3_p01", 2, 5, 9, 64, 256, 3, pad=(0, 1)),                # fwd; M = 2*3*9 = 54 (tail)
    G("h_full", 2, 4, 8, 256, 256, 3, pad=(1, 1)),                  # fwd, dgrad, wgrad (64 pixels)
    G("h_dg_p21", 2, 3, 9, 256, 64, 3, pad=(2, 1)),                 # dgrad: forward form, pad (0, 1), M = 54
    G("h_dg_1x7", 1, 4, 9, 256, 64, (1, 7), pad=(0, 3)),            # dgrad, non-square flipped filter (smagic of S = 7), M = 36
    G("h_dg_2x5", 2, 5, 6, 256, 64, (2, 5), pad=(1, 2)),            # dgrad, 2x5, forward-form pad (0, 2), M = 60
    G("h_1x7", 1, 9, 5, 64, 256, (1, 7), pad=(0, 1)),               # fwd, M = 9
    G("h_7x1", 1, 9, 5, 64, 256, (7, 1), pad=(2, 0)),               # fwd, M = 7*5 = 35
    G("h_2x5_s21", 2, 6, 11, 128, 256, (2, 5), stride=(2, 1), pad=(0, 1)),  # fwd strided, M = 2*3*9 = 54
    G("h_wg_1x3", 2, 4, 8, 64, 256, (1, 3), pad=(0, 1)),            # wgrad: 64 pixels, non-square
    G("h_wg_2x5", 1, 7, 8, 8, 256, (2, 5), pad=(1, 2)),             # wgrad: C = 8 (the smallest), 8 x 8 = 64 pixels
]

# ----- streaming pointwise kernel (pwconv.hip; pw_plan: K in {64, 128, 256}, N >= 2K, N % (4 wn) == 0).
# "f": the forward (K = Cin) takes it; "d": the data grad (K = Cout) takes it.  M in {1, 7, 63, 65}.
_PW_M = {1: (1, 1, 1), 7: (1, 1, 7), 63: (1, 7, 9), 65: (1, 5, 13)}
PW = [G(f"pw_{d}{k}_m{m}", *_PW_M[m], *((k, n) if d == "f" else (n, k)), 1)
      for k, n in ((64, 256), (128, 256), (256, 512)) for d in "fd" for m in (1, 7, 63, 65)]

# ----- persistent GEMM, pointwise at depth >= 1024 (conv_fwd's HACT_BNF branch with want_stats; conv_dgrad_bn's
# HACT_BNB branch: K = Cout >= 1024, no residual / mask)
HG_PW = [
    G("hp_f_m1", 1, 1, 1, 1024, 64, 1), G("hp_f_tail", 2, 3, 9, 1024, 64, 1),
    G("hp_d_m1", 1, 1, 1, 64, 1024, 1), G("hp_d_tail", 2, 3, 9, 64, 1024, 1),
]

# ----- row-walking 64 -> 64 3x3 (rowconv.hip; rowconv_geom: stride 1, pad 1, W <= 64, H >= 2 -- at H = 1 the
# dispatch falls back to the implicit GEMM, which the (1, 1, *) cases pin)
ROW = [G(f"row_{n}_{h}_{w}", n, h, w, 64, 64, 3, pad=(1, 1)) for n, h, w in ((1, 1, 1), (1, 1, 64), (2, 3, 5), (1, 9, 64))]

# ----- s2d stem (stem.hip: 16 -> 64, 4x4, pad [2, 2, 1, 1]).  conv_fwd takes the stem kernel only when
# dpe_stem_blocks(N, H, W) > 0, i.e. H >= 3 and 97 <= W <= 112 (3 N blocks): (1, 3, 97) and (2, 4, 112) are the
# smallest shapes at the two ends of that envelope.  (1, 1, 1), (1, 2, 7) and (2, 5, 33) lie outside it and pin the
# fallback: the forward runs on the implicit GEMM's C = 16 two-taps-per-K-step path whatever set_stem_kernel says.
# The stem weight grad's envelope is H >= 2, W <= 112 (dpe_stem_wgrad_scratch > 0): all but (1, 1, 1) reach it.
STEM_IN = [(1, 3, 97), (2, 4, 112)]
STEM = [G(f"stem_{n}_{h}_{w}", n, h, w, 16, 64, 4, pad=(2, 2, 1, 1))
        for n, h, w in [(1, 1, 1), (1, 2, 7), (2, 5, 33)] + STEM_IN]

# ----- conv_dgrad_bn on the dyadic grid: igemm plain / strided / 1x1, streaming pointwise, row-walking
DGRAD_BN = ["g_5x9", "g_s22_3", "g_s33_1", "g_c24", "g_1x1p1", "g_d22", "pw_d64_m63", "pw_d128_m65", "row_2_3_5",
            "h_dg_p21", "h_dg_1x7", "hp_d_tail", "hp_d_m1"]

GEOMS = {g.name: g for g in GENERAL + HGEMM + PW + HG_PW + ROW + STEM}
assert len(GEOMS) == len(GENERAL + HGEMM + PW + HG_PW + ROW + STEM)
TIER_A = list(GEOMS)

# Tier B (randn, rounding budgets): one or more per route, each with an M tail and an N tail where the route
# allows one (the streaming, row-walking and stem kernels have fixed channel counts)
TIER_B = ["g_5x9", "g_c24", "g_s22_3", "g_k72", "g_d12", "h_3x3_p01", "h_dg_p21", "h_full", "pw_f64_m63", "pw_d128_m65",
          "hp_f_tail", "hp_d_tail", "row_2_3_5", "stem_2_5_33", "stem_1_3_97", "h_dg_1x7"]


# ================================================================ convolution
def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _conv64(x, w, g):
    t, l, b, r = g.pad4
    return F.conv2d(F.pad(x, (l, r, t, b)), w, None, g.stride, 0, g.dil)


def _conv_all(x, w, dy, g):
    xd = _nchw(x.double()).contiguous().requires_grad_(True)
    wd = _nchw(w.double()).contiguous().requires_grad_(True)
    y = _conv64(xd, wd, g)
    y.backward(_nchw(dy.double()).contiguous())
    return (y.detach().permute(0, 2, 3, 1).contiguous(), xd.grad.permute(0, 2, 3, 1).contiguous(),
            wd.grad.permute(0, 2, 3, 1).contiguous())


def conv_ref(x, w, dy, g, bounds=True):
    """x [N,H,W,C], w [K,R,S,C], dy [N,OH,OW,K] (any float dtype) -> dict of fp64 y, dx, dw in those layouts
    and, with ``bounds``, the budgets evaluated on the reference:
        a_* = n u32 * (the same conv applied to |x|, |w|, |dy|): the fp32 accumulation term, n the number of
              products per output (R S C for y, R S K for dx, N OH OW for dw)
        b_y, b_dx = U (|ref| + a) + a     one bf16 rounding of the accumulated value
        b_dxres(res) = b_dx + U |dx + res|: the epilogues round the data grad to bf16, add the residual in
                       fp32 and round again (igemm.hip finish_row, pwconv.hip): one more rounding
        b_dw = a_dw + u32 |dw|            fp32 output: accumulation plus the final fp32 add into dw."""
    y, dx, dw = _conv_all(x, w, dy, g)
    out = {"y": y, "dx": dx, "dw": dw}
    if bounds:
        ay, adx, adw = _conv_all(x.double().abs(), w.double().abs(), dy.double().abs(), g)
        oh, ow = g.out_hw
        a_y = g.R * g.S * g.C * u32 * ay
        a_dx = g.R * g.S * g.K * u32 * adx
        a_dw = g.N * oh * ow * u32 * adw
        out.update(b_y=U * (y.abs() + a_y) + a_y + FLOOR, b_dx=U * (dx.abs() + a_dx) + a_dx + FLOOR,
                   b_dw=a_dw + u32 * dw.abs() + FLOOR, a_dx=a_dx)
    return out


def b_dxres(ref, res):
    return ref["b_dx"] + U * (ref["dx"] + res.double()).abs()


def conv_emulate(x, w, dy, g, res=None):
    """The kernels' roundings in torch on the CPU (no kernel): bf16 inputs widened to fp32, fp32 F.conv2d and
    its fp32 gradients, outputs rounded to bf16 (dw stays fp32); with ``res`` the data grad is rounded, the
    residual added in fp32, and the sum rounded again."""
    xf = _nchw(x.float()).contiguous().requires_grad_(True)
    wf = _nchw(w.float()).contiguous().requires_grad_(True)
    y = _conv64(xf, wf, g)
    y.backward(_nchw(dy.float()).contiguous())
    dx = xf.grad.permute(0, 2, 3, 1).contiguous().to(BF)
    if res is not None:
        dx = (dx.float() + res.float()).to(BF)
    return y.detach().permute(0, 2, 3, 1).contiguous().to(BF), dx, wf.grad.permute(0, 2, 3, 1).contiguous()


def randn_case(g, seed=0):
    """Tier B inputs: randn x and dy, w scaled by 1 / sqrt(R S C), a randn residual; all bf16 (CPU)."""
    gen = torch.Generator().manual_seed(seed)
    oh, ow = g.out_hw
    x = torch.randn(g.N, g.H, g.W, g.C, generator=gen).to(BF)
    w = (torch.randn(g.K, g.R, g.S, g.C, generator=gen) / (g.R * g.S * g.C) ** 0.5).to(BF)
    dy = torch.randn(g.N, oh, ow, g.K, generator=gen).to(BF)
    res = torch.randn(g.N, g.H, g.W, g.C, generator=gen).to(BF)
    return x, w, dy, res


# ------------------------------------------------------- Tier A integer cases
def _sparse_int(shape, dens, gen, lo=-2, hi=2):
    v = torch.randint(lo, hi + 1, shape, generator=gen).double()
    keep = torch.rand(shape, generator=gen) < dens
    return v * keep + 0.0  # (+ 0.0: no -0, whose bits differ from the +0 an accumulation from zero produces)


def weight_coverage(w):
    """(taps, input-channel residues mod 32, output-channel residues mod 64) that carry a nonzero weight."""
    nz = (w != 0).nonzero()
    S = w.shape[2]
    return (set((nz[:, 1] * S + nz[:, 2]).tolist()), set((nz[:, 3] % 32).tolist()), set((nz[:, 0] % 64).tolist()))


def check_int_case(g, c):
    """The builder's claims (asserted by int_case itself and, for every case, by test_resnet_ref_cpu.py)."""
    taps, cres, kres = weight_coverage(c["w"].double())
    assert taps == set(range(g.R * g.S)), (g.name, "taps", taps)
    assert cres == set(range(min(g.C, 32))), (g.name, "input-channel residues", cres)
    assert kres == set(range(min(g.K, 64))), (g.name, "output-channel residues", kres)
    for k in ("y", "dx", "dw"):
        r = c[k]
        assert torch.equal(r, r.round()), (g.name, k, "not integral")
        assert r.abs().max().item() <= INT_MAX, (g.name, k, r.abs().max().item())
    for k in ("x", "w", "dy", "res", "dx0", "dw0"):
        assert torch.equal(c[k].double(), c[k].double().round()), (g.name, k)
    assert (c["dx"] + c["res"].double()).abs().max().item() <= INT_MAX
    assert (c["dx"] + c["dx0"].double()).abs().max().item() <= INT_MAX


@functools.lru_cache(maxsize=None)
def int_case(name, seed=0):
    """Tier A case of GEOMS[name]: x, w, dy, res (a residual for dx), dx0 (a prefill of dx for conv_dgrad_acc)
    as bf16 and dw0 (a prefill of dw) as fp32, all small sparse integers, with the fp64 y, dx, dw, every
    element of which is an integer of magnitude <= 248 (so also <= 256 after res / dx0, |.| <= 4, are added).
    Such values are exact in bf16, every product and every partial sum in any order is an integer below 2^24,
    exact in fp32: the kernels must reproduce the reference bit for bit.  The density of the random part
    shrinks until the bound holds; on top of it one weight per j < max(R S, C, K) at (k, tap, c) = (j mod K,
    j mod R S, j mod C) guarantees the coverage check_int_case asserts.
    ``stats_exact``: M max|y|^2 < 2^24, so the BN sums of y and y^2 are exact in fp32 as well.  Cached: the
    tensors are shared between tests and must not be modified."""
    g = GEOMS[name]
    gen = torch.Generator().manual_seed(1000 + seed)
    oh, ow = g.out_hw
    dens = 0.5
    for _ in range(24):
        x = _sparse_int((g.N, g.H, g.W, g.C), dens, gen)
        dy = _sparse_int((g.N, oh, ow, g.K), dens, gen)
        w = _sparse_int((g.K, g.R, g.S, g.C), dens, gen)
        for j in range(max(g.R * g.S, g.C, g.K)):
            t = j % (g.R * g.S)
            if w[j % g.K, t // g.S, t % g.S, j % g.C] == 0:
                w[j % g.K, t // g.S, t % g.S, j % g.C] = (1, -1, 2, -2)[j % 4]
        ref = conv_ref(x, w, dy, g, bounds=False)
        if max(ref[k].abs().max().item() for k in ("y", "dx", "dw")) <= INT_MAX - 8:
            break
        dens *= 0.8
    c = dict(ref)
    c.update(x=x.to(BF), w=w.to(BF), dy=dy.to(BF),
             res=_sparse_int((g.N, g.H, g.W, g.C), 0.7, gen, -4, 4).to(BF),
             dx0=_sparse_int((g.N, g.H, g.W, g.C), 0.7, gen, -4, 4).to(BF),
             dw0=_sparse_int((g.K, g.R, g.S, g.C), 0.7, gen, -9, 9).float(), density=dens)
    ymax = ref["y"].abs().max().item()
    c["stats_exact"] = g.M * ymax * ymax < 2 ** 24
    check_int_case(g, c)
    return c


def dyadic_bn(shape, seed=0, zero_frac=0.08):
    """Tier A operands of a BN + ReLU backward epilogue: h (bf16, ``shape`` [..., C]) and coef [4][C] fp32 =
    (scale, shift, mean, invstd), every value a multiple of 1/8 of magnitude <= 8 (scale a nonzero power of
    two in [1/4, 2] with either sign).  h * scale + shift is then a multiple of 1/32 below 2^5: exact in fp32
    with or without fma, so the kernel's ReLU decision is the fp64 one.  shift = -scale * h0 with h0 on the
    grid and |h0| <= 4, and ``zero_frac`` of the elements of every channel are set to h0: they sit exactly at
    0, where only a strict > 0 is right.  Returns (h, coef, pre) with pre = h * scale + shift in fp64."""
    gen = torch.Generator().manual_seed(2000 + seed)
    C = shape[-1]
    h = torch.randint(-64, 65, shape, generator=gen).double() / 8
    scale = torch.tensor([0.25, 0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 4, (C,), generator=gen)]
    scale = scale * (torch.randint(0, 2, (C,), generator=gen).double() * 2 - 1)
    step = 0.125 / scale.abs().clamp(max=1.0)  # h0 on the grid, coarse enough that scale * h0 is on it too
    h0 = ((torch.rand(C, generator=gen) * 8 - 4) / step).round() * step
    shift = -scale * h0
    mean = torch.randint(-64, 65, (C,), generator=gen).double() / 8
    invstd = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (C,), generator=gen)]
    at0 = torch.rand(shape, generator=gen) < zero_frac
    h = torch.where(at0, h0.expand(shape), h)
    h, shift = h + 0.0, shift + 0.0  # (no -0: the sign of an exact zero is not under test)
    coef = torch.stack([scale, shift, mean, invstd]).float()
    pre = h * scale + shift
    assert torch.equal(h.to(BF).double(), h) and torch.equal(coef.double()[:3], torch.stack([scale, shift, mean]))
    assert torch.equal(coef.double() * 8, (coef.double() * 8).round()) and coef.abs().max() <= 8 and h.abs().max() <= 8
    return h.to(BF), coef, pre


def pack_bits(mask):
    """bool [..., C] -> uint8 [..., C/8], bit e of byte j = mask[..., 8 j + e] (bn_apply's want_mask layout)."""
    m = mask.reshape(*mask.shape[:-1], mask.shape[-1] // 8, 8).to(torch.int32)
    wts = (2 ** torch.arange(8, dtype=torch.int32, device=mask.device))
    return (m * wts).sum(-1).to(torch.uint8)


def dgrad_bn_ref(dx, h, coef, mask=None):
    """fp64 (dz, [sum dz, sum dz (h - mean)] per channel) of the BN-backward epilogue: dz = dx where
    h * scale + shift > 0 (or where ``mask``), else 0."""
    c = coef.double()
    m = (h.double() * c[0] + c[1]) > 0 if mask is None else mask
    dz = dx * m
    C = dx.shape[-1]
    return dz, torch.stack([dz.reshape(-1, C).sum(0), (dz * (h.double() - c[2])).reshape(-1, C).sum(0)])


# ================================================================== BatchNorm
BN_EPS = 1e-5
BN_MOM = 0.1


def bn_case(M, C, seed=0):
    """x [M, C] bf16 randn with four special channels (when C >= 8): 0 constant 1.5 (var = 0 exactly: the
    fp32 sums of 1.5 and 2.25 are exact), 1 mean 16 / std 1, 2 mean -64 / std 0.5 (E[x^2] >> var: the
    cancellation in var = E[x^2] - mean^2), 3 all zeros; gamma / beta / running stats / dy / residual randn,
    gamma[0] and beta[0] bf16-exact."""
    gen = torch.Generator().manual_seed(3000 + seed)
    x = torch.randn(M, C, generator=gen)
    x[:, 0] = 1.5
    x[:, 1] = 16 + torch.randn(M, generator=gen)
    x[:, 2] = -64 + 0.5 * torch.randn(M, generator=gen)
    x[:, 3] = 0
    gamma = 1 + 0.25 * torch.randn(C, generator=gen)
    beta = 0.5 * torch.randn(C, generator=gen)
    gamma[0], beta[0] = 1.25, 0.5
    return dict(x=x.to(BF), gamma=gamma, beta=beta, rmean=torch.randn(C, generator=gen),
                rvar=torch.rand(C, generator=gen) + 0.5, dy=torch.randn(M, C, generator=gen).to(BF),
                res=torch.randn(M, C, generator=gen).to(BF))


def bn_fwd_ref(x, gamma, beta, rmean, rvar, eps=BN_EPS, mom=BN_MOM):
    """fp64 (mean, var, invstd, scale, shift, new running mean, new running var) per channel of training-mode
    BatchNorm over the rows of x [M, C]: biased variance for the normalisation, unbiased (M / (M - 1), only
    when M > 1) for the running variance."""
    xd = x.double()
    M = xd.shape[0]
    mean = xd.mean(0)
    var = ((xd - mean) ** 2).mean(0)
    invstd = 1 / torch.sqrt(var + eps)
    scale = gamma.double() * invstd
    shift = beta.double() - mean * scale
    unb = var * M / (M - 1) if M > 1 else var
    return dict(mean=mean, var=var, invstd=invstd, scale=scale, shift=shift,
                rmean=(1 - mom) * rmean.double() + mom * mean, rvar=(1 - mom) * rvar.double() + mom * unb)


def bn_fwd_budgets(xvals, gamma, beta, rmean, rvar, eps=BN_EPS, mom=BN_MOM):
    """Budgets of the statistics from the kernel's formula (bn.hip bn_finalize_kernel): fp32 partial sums
    s = sum x and q = sum x^2 (x^2 of a bf16 value is exact in fp32), combined in double, mean = s / M,
    var = q / M - mean^2 clamped at 0, invstd = fp32(1 / sqrt(var + eps)).
        |ds| <= M u32 sum|x|                 -> b_mean = M u32 E|x|
        |dq| <= M u32 sum x^2                -> |dvar| <= M u32 E[x^2] + 2 |mean| b_mean + b_mean^2 = b_var
    so the variance budget scales with E[x^2] (and mean^2), not with var: on a channel with mean -64 and
    std 0.5 it is M u32 * 3 * 4096, against var = 0.25.  invstd: the change of (v + eps)^-1/2 over
    v = var +- b_var (v >= 0), plus one fp32 rounding; scale = fp32(gamma * invstd): |gamma| b_invstd + one
    rounding; shift = fp32(beta - fp32(fp32(mean) * scale)): |mean| b_scale + |scale| (b_mean + u32 |mean|) +
    two roundings; the running statistics are fp32 expressions of three operations each.
    ``xvals``: the values summed (the pre-BN tensor, fp64 [M, C])."""
    r = bn_fwd_ref(xvals, gamma, beta, rmean, rvar, eps, mom)
    xd = xvals.double()
    M = xd.shape[0]
    b_mean = M * u32 * xd.abs().mean(0)
    b_var = M * u32 * (xd * xd).mean(0) + 2 * r["mean"].abs() * b_mean + b_mean ** 2
    f = lambda v: 1 / torch.sqrt(v + eps)
    lo, hi = (r["var"] - b_var).clamp(min=0), r["var"] + b_var
    b_inv = torch.maximum((f(lo) - r["invstd"]).abs(), (f(hi) - r["invstd"]).abs()) + 2 * u32 * r["invstd"]
    g = gamma.double().abs()
    b_scale = g * b_inv + u32 * r["scale"].abs()
    ms = (r["mean"] * r["scale"]).abs()
    b_shift = r["mean"].abs() * b_scale + r["scale"].abs() * (b_mean + u32 * r["mean"].abs()) + \
        2 * u32 * (ms + beta.double().abs())
    unb = M / (M - 1) if M > 1 else 1.0
    b_rmean = mom * (b_mean + u32 * r["mean"].abs()) + 3 * u32 * (rmean.double().abs() + r["mean"].abs())
    b_rvar = mom * unb * (b_var + u32 * r["var"]) + 3 * u32 * (rvar.double().abs() + unb * r["var"])
    r.update(b_mean=b_mean + u32 * r["mean"].abs() + FLOOR, b_var=b_var + FLOOR, b_invstd=b_inv + FLOOR,
             b_scale=b_scale + FLOOR, b_shift=b_shift + FLOOR, b_rmean=b_rmean + FLOOR, b_rvar=b_rvar + FLOOR)
    return r


def bn_apply_ref(x, coef, res=None, relu=False):
    """fp64 y = act(x * scale + shift (+ res)) from the coefficients the kernel used (coef [4][C], widened) and
    its budget: fp32 fma (one rounding of the exact x * scale + shift), one more fp32 add with a residual, one
    bf16 rounding of the result: U |y| + u32 (2 |x scale + shift| + |res| + |y|) (ReLU is exact)."""
    c = coef.double()
    v = x.double() * c[0] + c[1]
    t = v + (res.double() if res is not None else 0)
    y = t.clamp(min=0) if relu else t
    a = u32 * (2 * v.abs() + (res.double().abs() if res is not None else 0) + t.abs())
    return y, U * (t.abs() + a) + a + FLOOR


def bn_bwd_ref(dy, x, gamma, coef, mask=None, dgamma0=None, dbeta0=None):
    """fp64 backward of y = [relu](x_hat gamma + beta) from the statistics the kernel used (coef's mean and
    invstd, widened): dz = dy (masked), s = sum dz, q = sum dz (x - mean), dgamma = q invstd, dbeta = s,
    dx = gamma invstd (dz - s / M - (x - mean) invstd^2 q / M).  Budgets from the kernel's formula (bn.hip:
    fp32 partials of s and of q = sum fma(dz, x - mean, q), combined in double; bcoef a, b, c in fp32;
    dx = bf16(fma(a, dz, fma(b, x, c)))):
        b_s = M u32 sum|dz|,  b_q = (M + 2) u32 sum|dz (x - mean)|        (x - mean is rounded once)
        dgamma, dbeta: b_q invstd, b_s, plus the fp32 conversion and the fp32 add into the gradient buffer
        b = -k1 invstd^2 q / M (5 fp32 operations), c = -k1 s / M - b mean (4 more):
        b_b = k1 invstd^2 b_q / M + 5 u32 |b|,  b_c = k1 b_s / M + |mean| b_b + 4 u32 (|k1 s / M| + |b mean|)
        b_dx = u32 |a dz| + |x| b_b + b_c + 2 u32 (|a dz| + |b x| + |c|) + U |dx| (+ U * the rest)."""
    c = coef.double()
    mean, invstd = c[2], c[3]
    g = gamma.double()
    xd = x.double()
    M = xd.shape[0]
    dz = dy.double() * (mask if mask is not None else 1.0)
    xc = xd - mean
    s, q = dz.sum(0), (dz * xc).sum(0)
    k1 = g * invstd
    b = -k1 * invstd * invstd * q / M
    cc = -k1 * s / M - b * mean
    dx = k1 * dz + b * xd + cc
    b_s = M * u32 * dz.abs().sum(0)
    b_q = (M + 2) * u32 * (dz * xc).abs().sum(0)
    dgamma, dbeta = q * invstd, s
    g0 = dgamma0.double() if dgamma0 is not None else 0.0
    b0 = dbeta0.double() if dbeta0 is not None else 0.0
    b_dgamma = b_q * invstd + 2 * u32 * dgamma.abs() + u32 * (dgamma + g0).abs() + FLOOR
    b_dbeta = b_s + u32 * dbeta.abs() + u32 * (dbeta + b0).abs() + FLOOR
    b_b = k1.abs() * invstd ** 2 * b_q / M + 5 * u32 * b.abs()
    b_c = k1.abs() * b_s / M + mean.abs() * b_b + 4 * u32 * ((k1 * s / M).abs() + (b * mean).abs())
    rest = u32 * (k1 * dz).abs() + xd.abs() * b_b + b_c + 2 * u32 * ((k1 * dz).abs() + (b * xd).abs() + cc.abs())
    return dict(dz=dz, s=s, q=q, dx=dx, dgamma=dgamma + g0, dbeta=dbeta + b0, b_s=b_s + FLOOR, b_q=b_q + FLOOR,
                b_dgamma=b_dgamma, b_dbeta=b_dbeta, b_dx=rest + U * (dx.abs() + rest) + FLOOR)


def bn_emulate(x, gamma, beta, rmean, rvar, dy, res=None, relu=False, eps=BN_EPS, mom=BN_MOM):
    """bn.hip's arithmetic in torch on the CPU: fp32 sums of x and x^2 (torch's own summation order), the
    finalize in double with fp32 outputs, y = bf16(relu(fma(x, scale, shift) + res)); backward with fp32
    sums, fp32 coefficient arithmetic, dx = bf16(a dz + (b x + c)).  Returns a dict named like the kernels'
    outputs."""
    xf = x.float()
    M = xf.shape[0]
    s, q = xf.sum(0).double(), (xf * xf).sum(0).double()
    mean = s / M
    var = (q / M - mean * mean).clamp(min=0)
    invstd = (1 / torch.sqrt(var + eps)).float()
    sc = gamma.float() * invstd
    sh = beta.float() - mean.float() * sc
    unb = var * M / (M - 1) if M > 1 else var
    v = (xf.double() * sc.double() + sh.double()).float()  # fmaf: one rounding of the exact x * scale + shift
    if res is not None:
        v = v + res.float()
    if relu:
        v = v.clamp(min=0)
    y = v.to(BF)
    coef = torch.stack([sc, sh, mean.float(), invstd])
    dz = dy.float() * ((y.float() > 0) if relu else 1.0)
    ss = dz.sum(0).double()
    qq = (dz * (xf - coef[2])).sum(0).double()
    k1 = gamma.float() * invstd
    b = -k1 * invstd * invstd * qq.float() / M
    c = -k1 * ss.float() / M - b * coef[2]
    dx = (k1 * dz + (b * xf + c)).to(BF)
    return dict(coef=coef, y=y, rmean=(1 - mom) * rmean.float() + mom * mean.float(),
                rvar=(1 - mom) * rvar.float() + mom * unb.float(), var=var, dx=dx, dz=dz.to(BF),
                dgamma=(qq * invstd.double()).float(), dbeta=ss.float())


# ==================================================================== pooling
POOL_CFG = [(3, 2, 1), (2, 2, 0), (3, 1, 1), (3, 2, 0)]
POOL_HW = [(5, 9), (9, 6)]
POOL_C = [8, 64, 256]
GAVG_HW = [(1, 1), (7, 7), (5, 10)]
GAVG_C = [8, 2048]
BN_M = [1, 2, 97]
BN_C = [8, 64, 2048]
_POOL_VALUES = [-2.0, -1.0, 1.0, 1.0]  # three bf16 values (1.0 twice as likely): most windows hold ties


def pool_case(N, H, W, C, k, p, seed=0):
    """x [N, H, W, C] bf16 from three values (ties in most windows).  With padding, the pixels within k - p of a
    border -- every pixel that a window which also covers padding can see -- are all negative, so that a
    padding tap counted as 0, or as anything that is not below the data, would win."""
    gen = torch.Generator().manual_seed(4000 + seed)
    vals = torch.tensor(_POOL_VALUES, dtype=torch.float64)
    x = vals[torch.randint(0, 4, (N, H, W, C), generator=gen)]
    neg = vals[torch.randint(0, 2, (N, H, W, C), generator=gen)]
    b = k - p if p > 0 else 0
    hh = torch.arange(H).view(1, H, 1, 1)
    ww = torch.arange(W).view(1, 1, W, 1)
    border = (hh < b) | (hh >= H - b) | (ww < b) | (ww >= W - b)
    return torch.where(border, neg, x).to(BF)


def maxpool_ref(x, dy, k, s, p):
    """fp64 F.max_pool2d on the CPU and its autograd: (y [N,OH,OW,C], dx [N,H,W,C]).  Ties go to the first tap
    in scan order (r, then q), in the kernel (strict >) and in torch, and autograd sums dy into that tap."""
    xd = _nchw(x.double().cpu()).contiguous().requires_grad_(True)
    y = F.max_pool2d(xd, k, s, p)
    if dy is None:
        return y.detach().permute(0, 2, 3, 1).contiguous(), None
    y.backward(_nchw(dy.double().cpu()).contiguous())
    return y.detach().permute(0, 2, 3, 1).contiguous(), xd.grad.permute(0, 2, 3, 1).contiguous()


def gavg_ref(x):
    """fp64 mean over the pixels of x [N, H, W, C] -> [N, C], and its budget: HW fp32 additions, the division,
    one bf16 rounding: U (|y| + a) + a with a = (HW + 1) u32 mean|x|."""
    xd = x.double().reshape(x.shape[0], -1, x.shape[-1])
    HW = xd.shape[1]
    y = xd.mean(1)
    a = (HW + 1) * u32 * xd.abs().mean(1)
    return y, U * (y.abs() + a) + a + FLOOR
