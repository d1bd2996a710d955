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
    operand_on_load(h, coef, res, res_coef)   the operand of the kernels that apply BN + ReLU on load (bf16)
    bnrelu_maxpool_ref / pool_gather_ref / maxpool_bn_bwd_ref / stem_wgrad_ref   the fused stem pool
    pool_bn_case / conv_bn_case / bnin_fwd_case / bnin_bwd_case   cases of test_bn_fused_kernels_gpu.py

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
                b_dgamma=b_dgamma, b_dbeta=b_dbeta, b_dx=rest + U * (dx.abs() + rest) + FLOOR,
                k1=k1, b=b, c=cc, b_k1=u32 * k1.abs() + FLOOR, b_b=b_b + FLOOR, b_c=b_c + FLOOR)


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


# ==================================================== fused BN-boundary kernels
# (test_bn_fused_kernels_gpu.py: the kernels that never store the tensor between a BatchNorm and its neighbour)
def _f32(v):
    """One round-to-nearest-even rounding of an fp64 tensor to fp32, widened again."""
    return v.float().double()


def operand_on_load(h, coef, res=None, res_coef=None):
    """The conv / pool operand as the kernels form it, bf16: a = bf16(relu(fma(h, scale, shift) [+ r])).
    h * scale + shift is exact in fp64 (a bf16 times an fp32 plus an fp32) and is rounded ONCE to fp32, the fma's
    single rounding; a residual is one more fp32 addition.  With ``res_coef`` the residual is itself a BatchNorm
    output, r = bf16(fma(res, scale_d, shift_d)): a second fma, rounded to bf16 first as bn_apply's two-BN form
    and the on-load conv both do (the downsample branch is a bf16 tensor in the unfused network).  ReLU, then the
    bf16 rounding.  On the dyadic grid nothing is rounded before that last step."""
    c = coef.double()
    v = _f32(h.double() * c[0] + c[1])
    if res is not None:
        r = res.double()
        if res_coef is not None:
            rc = res_coef.double()
            r = _f32(r * rc[0] + rc[1]).to(BF).double()
        v = _f32(v + r)
    return (v.clamp(min=0) + 0.0).to(BF)


def bn_bwd_apply_ref(dz, h, bcoef):
    """dh = bf16(fma(a, dz, fma(b, h, c))) with bcoef = [a | b | c] per channel: two fp32 roundings (each of a
    value exact in fp64), then the bf16 one."""
    b = bcoef.double()
    return _f32(b[0] * dz.double() + _f32(b[1] * h.double() + b[2])).to(BF)


def _windows(a, k, s, p):
    """a [N, H, W, C] fp64 -> its pooling windows [N, OH, OW, C, k k] in scan order (r, then q); padding = -inf."""
    xp = F.pad(_nchw(a), (p, p, p, p), value=float("-inf"))
    win = xp.unfold(2, k, s).unfold(3, k, s)  # [N, C, OH, OW, k, k]
    N, C, OH, OW = win.shape[:4]
    return win.reshape(N, C, OH, OW, k * k).permute(0, 2, 3, 1, 4)


def bnrelu_maxpool_ref(h, coef, k, s, p, tie="first", relu_pad=False):
    """maxpool(relu(BN(h))) from the definition: the operand of operand_on_load, a window maximum, and the argmax
    byte r k + q of the FIRST maximal tap in scan order (the format maxpool_ref's kernels write).  Padding taps
    never win.  Returns (y fp64, idx uint8, a bf16).  ``tie="last"`` / ``relu_pad`` (padding reads relu(shift)
    instead of nothing) are the deliberately WRONG variants the CPU self-checks must tell apart."""
    a = operand_on_load(h, coef)
    win = _windows(a.double(), k, s, p)
    if relu_pad:
        pad_val = operand_on_load(torch.zeros(1, dtype=BF), coef).double()  # [C]
        win = torch.where(torch.isinf(win), pad_val.view(1, 1, 1, -1, 1).expand_as(win), win)
    y = win.amax(-1)
    taps = torch.arange(k * k, dtype=torch.float64)
    score = (win == y.unsqueeze(-1)).double() * ((k * k - taps) if tie == "first" else (taps + 1))
    return y, score.argmax(-1).to(torch.uint8), a


def last_valid_tap_idx(shape, k, s, p):
    """Argmax bytes [N, OH, OW, C] in which every window names its LAST tap inside the image."""
    win = _windows(torch.zeros(shape, dtype=torch.float64), k, s, p)
    return ((~torch.isinf(win)).double() * (torch.arange(k * k, dtype=torch.float64) + 1)).argmax(-1).to(torch.uint8)


def pool_gather_ref(dy, idx, H, W, k, s, p):
    """fp64 max-pool backward THROUGH the argmax bytes: g[n, h, w, c] = sum of dy over the windows whose byte
    names (h, w).  Returns (g, gabs) with gabs the same sum over |dy| (the rounding budget of the gather)."""
    N, OH, OW, C = dy.shape
    out = []
    for d in (dy.double(), dy.double().abs()):
        g = torch.zeros(N, H + 2 * p + k, W + 2 * p + k, C, dtype=torch.float64)
        for t in range(k * k):
            r, q = t // k, t % k
            g[:, r:r + s * OH:s, q:q + s * OW:s] += d * (idx == t)
        out.append(g[:, p:p + H, p:p + W].contiguous())
    assert (idx < k * k).all()
    return out


def maxpool_bn_bwd_ref(dy, idx, h, gamma, coef, k, s, p, dgamma0=None, dbeta0=None, relu_ge=False):
    """Backward of maxpool(relu(BN(h))): dy gathered through ``idx``, then bn_bwd_ref with the ReLU mask
    h * scale + shift > 0 (the sign of the exact value is the sign of its fp32 rounding).  The gather adds at most
    4 pooled gradients per pixel in fp32 (3 roundings, exact for integers): d = 3 u32 gabs per element, carried
    through bn_bwd_ref's formulas -- ds = sum d, dq = sum d |x - mean|, db = k1 invstd^2 dq / M,
    dc = k1 ds / M + |mean| db, and (1 + U)(|k1| d + |x| db + dc) on dx.
    ``exact``: integer dy, invstd a power of two and 8 sum |dz (x - mean)| < 2^24 -- every term of both sums is a
    multiple of 1/8 and every partial sum is exact in fp32, so dgamma and dbeta must equal the reference.
    ``relu_ge``: the WRONG mask >= 0 (for the CPU self-checks)."""
    N, H, W, C = h.shape
    g, gabs = pool_gather_ref(dy, idx, H, W, k, s, p)
    c = coef.double()
    pre = h.double() * c[0] + c[1]
    mask = (pre >= 0) if relu_ge else (pre > 0)
    r = bn_bwd_ref(g.reshape(-1, C), h.reshape(-1, C), gamma, coef, mask.reshape(-1, C), dgamma0, dbeta0)
    M = N * H * W
    mean, invstd = c[2], c[3]
    k1 = (gamma.double() * invstd).abs()
    d = 3 * u32 * (gabs * mask).reshape(-1, C)
    xc = (h.double().reshape(-1, C) - mean).abs()
    ds, dq = d.sum(0), (d * xc).sum(0)
    db = k1 * invstd ** 2 * dq / M
    dc = k1 * ds / M + mean.abs() * db
    r["b_dx"] = r["b_dx"] + (1 + U) * (k1 * d + h.double().reshape(-1, C).abs() * db + dc)
    r["b_dgamma"] = r["b_dgamma"] + dq * invstd
    r["b_dbeta"] = r["b_dbeta"] + ds
    mag = (r["dz"] * (h.double().reshape(-1, C) - mean)).abs().sum(0).max().item()
    r["exact"] = bool(torch.equal(dy.double(), dy.double().round()) and
                      torch.equal(torch.log2(invstd), torch.log2(invstd).round()) and mag * 8 < 2 ** 24 and
                      max(r["dgamma"].abs().max().item(), r["dbeta"].abs().max().item()) * 8 < 2 ** 24)
    r["gathered"] = g
    return r


# ----- family 1 / 2 / 3: the stem's BN + ReLU + max-pool (3 / 2 / 1), forward and backward
POOL_FWD = [(1, 2, 2, 64), (2, 8, 8, 64), (1, 6, 10, 64), (3, 7, 9, 64), (2, 9, 6, 64), (1, 5, 5, 16)]
POOL_FWD_B = [(2, 8, 8, 64), (3, 7, 9, 64)]
POOL_BWD = [sh for sh in POOL_FWD if sh[3] == 64] + [(4, 16, 16, 64)]  # (4, 16, 16): M / 512 = 2 partial blocks
STEM_BWD = [(1, 2, 2), (2, 8, 8), (1, 6, 10), (5, 4, 20), (4, 16, 16)]   # (N, H, W), even H and W, C = 64


@functools.lru_cache(maxsize=None)
def pool_bn_case(shape, tier, seed=0):
    """Operands of the fused stem pool at ``shape`` [N, H, W, C] (3 / 2 / 1), forward and backward.
    Tier "A": h, coef from dyadic_bn (>= 5 % of every channel exactly at the ReLU threshold, scales of either
    sign) with channel 0 given scale 0 and shift 1/2 (every tap of every window ties at 1/2) and channel 1
    scale 1, shift 0 and h = -|h| (no positive pre-activation: every maximum is the ReLU's 0 and the first tap
    inside the image must win); dy, the initial dgamma / dbeta and xs are small sparse integers.
    Tier "B": randn h (x 2 + 0.3), coefficients from bn_fwd_ref over it (gamma[0] = 0: a zero scale;
    gamma[2] < 0), randn dy / dgamma0 / dbeta0 / xs.
    Also the reference forward (y, idx, a).  Cached: shared between tests, not to be modified."""
    N, H, W, C = shape
    gen = torch.Generator().manual_seed(5000 + seed + 7 * N + 11 * H + 13 * W)
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    gamma = 1 + 0.25 * torch.randn(C, generator=gen)
    if tier == "A":
        h, coef, pre = dyadic_bn(shape, 500 + seed + N + H + W, zero_frac=0.2)
        # (off the threshold h is coarsened to multiples of 2, 9 values: the maximum of most windows is tied)
        hd, coef = torch.where(pre == 0, h.double(), (h.double() / 2).round() * 2), coef.clone()
        coef[0, 0], coef[1, 0] = 0.0, 0.5
        hd[..., 1] = torch.where(pre[..., 1] == 0, torch.zeros_like(pre[..., 1]), -hd[..., 1].abs().clamp(min=0.125))
        coef[0, 1], coef[1, 1] = 1.0, 0.0
        hd[:, 0, 0, 1] = 0.0  # (window (0, 0)'s first tap inside the image sits at the threshold and wins it)
        h = (hd + 0.0).to(BF)
        assert (coef[0] < 0).any() and torch.equal(h.double(), hd + 0.0)
        dy = _sparse_int((N, OH, OW, C), 0.7, gen, -3, 3)
        dy[:, 0, 0, 1] = 1.0  # ... with a gradient on it: a mask decided with >= shows in dbeta at every shape
        dy = dy.to(BF)
        g0 = _sparse_int((C,), 0.8, gen, -9, 9).float()
        b0 = _sparse_int((C,), 0.8, gen, -9, 9).float()
        xs = _sparse_int((N, H, W, 16), 0.5, gen).to(BF)
    else:
        h = (torch.randn(shape, generator=gen) * 2 + 0.3).to(BF)
        gamma[0] = 0.0
        gamma[2] = -gamma[2].abs()
        beta = 0.5 * torch.randn(C, generator=gen)
        f = bn_fwd_ref(h.reshape(-1, C), gamma, beta, torch.zeros(C), torch.ones(C))
        coef = torch.stack([f["scale"], f["shift"], f["mean"], f["invstd"]]).float()
        dy = torch.randn(N, OH, OW, C, generator=gen).to(BF)
        g0, b0 = torch.randn(C, generator=gen), torch.randn(C, generator=gen)
        xs = torch.randn(N, H, W, 16, generator=gen).to(BF)
    y, idx, a = bnrelu_maxpool_ref(h, coef, 3, 2, 1)
    pre = h.double() * coef.double()[0] + coef.double()[1]
    return dict(h=h, coef=coef, gamma=gamma, dy=dy, g0=g0, b0=b0, xs=xs, y=y, idx=idx, a=a, pre=pre)


def check_pool_bn_case(shape, c):
    """Tier A claims of pool_bn_case: >= 5 % of every channel at the threshold (the zero-scale channel is constant:
    none or all), ties in most windows, channel 1 without a positive pre-activation, exact pre-activations."""
    pre, C = c["pre"], shape[3]
    at0 = (pre == 0).double().reshape(-1, C).mean(0)
    if pre.numel() // C >= 100:
        assert (at0[1:] >= 0.05).all(), at0.min().item()
    assert (pre[..., 1] <= 0).all() and (pre[..., 1] < 0).any() and (pre[..., 0] == 0.5).all()
    f32 = torch.addcmul(c["coef"][1].expand(shape), c["h"].float(), c["coef"][0].expand(shape))
    assert torch.equal(f32.double(), pre) and torch.equal(pre * 32, (pre * 32).round()) and pre.abs().max() < 32
    win = _windows(c["a"].double(), 3, 2, 1)
    ties = ((win == win.amax(-1, keepdim=True)).sum(-1) > 1).double().mean().item()
    assert ties > 0.3 or shape[1] * shape[2] <= 4, ties


def stem_wgrad_ref(dh, xs):
    """fp64 filter gradient [64, 4, 4, 16] of the s2d stem conv (4x4, pad 2-2-1-1) for dL/dY = dh [N, H, W, 64]
    and input xs [N, H, W, 16], with conv_ref's fp32-accumulation budget b_dw."""
    N, H, W, _ = xs.shape
    g = G("stem_bwd", N, H, W, 16, 64, 4, pad=(2, 2, 1, 1))
    r = conv_ref(xs, torch.zeros(64, 4, 4, 16), dh, g)
    return r["dw"], r["b_dw"]


# ----- family 4 / 5: BN + ReLU on a conv's operand (in_coef), row-walking 3x3 and streaming pointwise
# row-walking kernel: 64 -> 64, 3x3 / 1 / 1, H >= 2, W <= 64.  (1, 1, 1) lies OUTSIDE it (H = 1: the plain conv
# falls back to the implicit GEMM, which has no on-load transform, so conv_fwd raises with in_coef): it is pinned as
# that error, and (1, 2, 1), the nearest shape inside, takes its place.  (16, 64, 3): the launch has
# min(resident slots, N H / 16) blocks, so N H = 1024 is the smallest row count with 64 blocks, the threshold of
# the weight grad's grouped partial reduce.
ROW_BN = [(1, 2, 1), (2, 3, 5), (1, 9, 64), (3, 5, 33), (16, 64, 3)]
ROW_BN_OUTSIDE = (1, 1, 1)
# streaming pointwise kernel: C in {64, 128}, M % 32 == 0, Cout >= 2 C and a multiple of the forward's 256-column
# block (pw_plan: N % (4 wn) == 0 with wn = 64 at both depths).  Cout = 64 lies outside for both channel counts; the
# nearest inside is 256, already listed, so 512 (two column blocks) takes the vacant place.
# M = N H W through (1, 4, 8), (2, 6, 8), (5, 13, 32).
PW_BN_M = {32: (1, 4, 8), 96: (2, 6, 8), 2080: (5, 13, 32)}
PW_BN = [(c, k, m) for c in (64, 128) for k in (256, 512) for m in PW_BN_M]


def _dyadic_relu_shift(shape, seed):
    """dyadic_bn with the sign of h and shift flipped on the channels whose shift is negative (all but every
    eighth): relu(shift) != 0 on most channels, so a padding pixel that received the transform shows in y.  The
    pre-activation flips sign with them; the elements at the threshold stay there."""
    h, coef, pre = dyadic_bn(shape, seed, zero_frac=0.2)
    C = shape[-1]
    flip = (coef[1] < 0) & (torch.arange(C) % 8 != 7)
    h = (torch.where(flip, -h.double(), h.double()) + 0.0).to(BF)
    coef = coef.clone()
    coef[1] = torch.where(flip, -coef[1], coef[1])
    pre = torch.where(flip, -pre, pre) + 0.0
    assert torch.equal(h.double() * coef.double()[0] + coef.double()[1], pre)
    return h, coef, pre


@functools.lru_cache(maxsize=None)
def conv_bn_case(g, tier, seed=0):
    """A conv of geometry ``g`` over a[.] = operand_on_load(h, coef): h, coef, w, dy, dw0 and the fp64 reference
    over the reference operand (conv_ref; with the budgets in Tier B).
    Tier "A": dyadic h / coef with relu(shift) != 0 on most channels, sparse integer w and dy.  a is a multiple
    of 2^-5 below 2^5; the builder asserts that every sum of |products| stays below 2^24 2^-5, so fp32
    accumulation is exact in any order: y must be bf16(ref) (one rounding), dw the reference itself.
    ``stats_exact``: M max|y|^2 2^10 < 2^24 (y^2 is a multiple of 2^-10).
    Tier "B": randn h, coefficients of a real bn_fwd_ref, randn w (/ sqrt(R S C)) and dy, all bf16."""
    gen = torch.Generator().manual_seed(6000 + seed)
    oh, ow = g.out_hw
    if tier == "A":
        h, coef, pre = _dyadic_relu_shift(g.xshape, 600 + seed)
        dens = 0.5 if g.N * oh * ow <= 4096 else 0.25
        w = _sparse_int((g.K, g.R, g.S, g.C), dens, gen)
        for j in range(max(g.R * g.S, g.C, g.K)):  # every tap / channel residue under a nonzero weight
            t = j % (g.R * g.S)
            if w[j % g.K, t // g.S, t % g.S, j % g.C] == 0:
                w[j % g.K, t // g.S, t % g.S, j % g.C] = (1, -1, 2, -2)[j % 4]
        dy = _sparse_int((g.N, oh, ow, g.K), dens, gen)
        dw0 = _sparse_int((g.K, g.R, g.S, g.C), 0.7, gen, -9, 9).float()
    else:
        h = torch.randn(g.xshape, generator=gen).to(BF)
        gamma, beta = 1 + 0.25 * torch.randn(g.C, generator=gen), 0.5 * torch.randn(g.C, generator=gen)
        f = bn_fwd_ref(h.reshape(-1, g.C), gamma, beta, torch.zeros(g.C), torch.ones(g.C))
        coef = torch.stack([f["scale"], f["shift"], f["mean"], f["invstd"]]).float()
        pre = h.double() * coef.double()[0] + coef.double()[1]
        w = torch.randn(g.K, g.R, g.S, g.C, generator=gen) / (g.R * g.S * g.C) ** 0.5
        dy = torch.randn(g.N, oh, ow, g.K, generator=gen)
        dw0 = torch.randn(g.K, g.R, g.S, g.C, generator=gen)
    w, dy = w.to(BF), dy.to(BF)
    a = operand_on_load(h, coef)
    c = conv_ref(a, w, dy, g, bounds=tier == "B")
    c.update(h=h, coef=coef, w=w, dy=dy, dw0=dw0, a=a, pre=pre)
    if tier == "A":
        check_conv_bn_case(g, c)
    return c


def check_conv_bn_case(g, c):
    """The exactness preconditions of a Tier A conv_bn_case ("reference not exact" when one fails)."""
    a = c["a"].double()
    assert torch.equal(a * 32, (a * 32).round()) and a.abs().max() < 32, (g.name, "operand off the 2^-5 grid")
    for k in ("w", "dy"):
        assert torch.equal(c[k].double(), c[k].double().round()) and c[k].double().abs().max() <= 2, (g.name, k)
    m = conv_ref(a.abs(), c["w"].double().abs(), c["dy"].double().abs(), g, bounds=False)
    for k in ("y", "dw"):
        assert m[k].max().item() * 32 < 2 ** 24, (g.name, k, "reference not exact: a partial sum can leave fp32")
    assert (c["dw"] / 2 + c["dw0"].double()).abs().max().item() * 64 < 2 ** 24, (g.name, "dw0 + dW / 2")
    pre, C = c["pre"], g.C
    if pre.numel() // C >= 100:
        assert ((pre == 0).double().reshape(-1, C).mean(0) >= 0.05).all(), (g.name, "threshold hits")
    sh = c["coef"][1]
    assert (sh > 0).double().mean().item() >= 0.5, (g.name, "relu(shift) != 0 on most channels")
    ymax = c["y"].abs().max().item()
    c["stats_exact"] = g.M * ymax * ymax * 1024 < 2 ** 24


def conv_bn_relu_pad_ref(c, g):
    """The WRONG forward in which the padding receives the transform (reads relu(shift), not 0): for the CPU
    self-checks."""
    t, l, b, r = g.pad4
    hp = F.pad(c["h"].double(), (0, 0, l, r, t, b))
    ap = operand_on_load(hp.to(BF), c["coef"])
    gp = G(g.name + "_padded", g.N, g.H + t + b, g.W + l + r, g.C, g.K, (g.R, g.S), g.stride, (0, 0), g.dil)
    return conv_ref(ap, c["w"], torch.zeros(g.N, *gp.out_hw, g.K), gp, bounds=False)["y"]


def row_bn_geom(n, h, w):
    return G(f"rowbn_{n}_{h}_{w}", n, h, w, 64, 64, 3, pad=(1, 1))


def pw_bn_geom(c, k, m):
    return G(f"pwbn_{c}_{k}_m{m}", *PW_BN_M[m], c, k, 1)


# ----- family 6 / 7: the BN applies on the A operand of the LDS-DMA 1x1 conv
BNIN_M = {1: (1, 1, 1), 127: (1, 1, 127), 128: (2, 8, 8), 129: (1, 3, 43), 243: (3, 9, 9)}
BNIN_FWD = [(m, c, k) for m in BNIN_M for c in (32, 64, 256) for k in (8, 64, 136)]   # x [M, C] -> y [M, K]
BNIN_BWD = [(m, k, c) for m in BNIN_M for k in (32, 64, 256) for c in (8, 64, 136)]   # dz [M, K] -> dx [M, C]


@functools.lru_cache(maxsize=None)
def bnin_fwd_case(m, C, K, tier, down, seed=0):
    """conv1x1_bnin_fwd operands at M = m rows: h, res, coef, res_coef (``down``: the residual is a BatchNorm
    output itself), w, and the reference operand x, its ReLU bits, and the geometry of the 1x1 conv over it.
    Tier "A": everything on the dyadic grid (h * scale + shift + r is a multiple of 2^-5 below 2^6: exact in
    fp32, one bf16 rounding), the residual branch 0 wherever the main branch is at its threshold, so >= 5 % of
    every channel has a pre-activation of exactly 0; sparse integer w.  Tier "B": randn, real coefficients."""
    shape = (*BNIN_M[m], C)
    g = G(f"bnin_f_{m}_{C}_{K}", *shape, K, 1)
    gen = torch.Generator().manual_seed(7000 + seed + m + 3 * C + 5 * K + down)
    if tier == "A":
        h, coef, pre = dyadic_bn(shape, 700 + seed + m + C, zero_frac=0.2)
        if down:
            res, res_coef, pre2 = dyadic_bn(shape, 750 + seed + m + C)
            h02 = (-res_coef.double()[1] / res_coef.double()[0])  # the branch's own threshold, on the grid
            res = (torch.where(pre == 0, h02.expand(shape), res.double()) + 0.0).to(BF)
        else:
            r = torch.randint(-64, 65, shape, generator=gen).double() / 8
            res, res_coef = torch.where(pre == 0, torch.zeros_like(r), r).to(BF), None
        w = _sparse_int((K, 1, 1, C), 0.4, gen)
        for j in range(max(C, K)):
            if w[j % K, 0, 0, j % C] == 0:
                w[j % K, 0, 0, j % C] = (1, -1, 2, -2)[j % 4]
    else:
        h = torch.randn(shape, generator=gen).to(BF)
        res = torch.randn(shape, generator=gen).to(BF)

        def real_coef(t):
            gamma, beta = 1 + 0.25 * torch.randn(C, generator=gen), 0.5 * torch.randn(C, generator=gen)
            f = bn_fwd_ref(t.reshape(-1, C), gamma, beta, torch.zeros(C), torch.ones(C))
            return torch.stack([f["scale"], f["shift"], f["mean"], f["invstd"]]).float()
        coef = real_coef(h)
        res_coef = real_coef(res) if down else None
        w = torch.randn(K, 1, 1, C, generator=gen) / C ** 0.5
    w = w.to(BF)
    x = operand_on_load(h, coef, res, res_coef)
    c = dict(h=h, res=res, coef=coef, res_coef=res_coef, w=w, x=x, bits=pack_bits(x > 0), g=g)
    if tier == "A":
        xd = x.double()
        assert torch.equal(xd * 32, (xd * 32).round()) and xd.max() < 64, (g.name, "operand off the 2^-5 grid")
        if xd.numel() // C >= 100:
            t = h.double() * coef.double()[0] + coef.double()[1]
            t = t + (res.double() if not down else (res.double() * res_coef.double()[0] + res_coef.double()[1]))
            assert ((t == 0).double().reshape(-1, C).mean(0) >= 0.05).all(), (g.name, "threshold hits")
        mag = conv_ref(xd, w.double().abs(), torch.zeros(*shape[:3], K), g, bounds=False)["y"].max().item()
        assert mag * 32 < 2 ** 24, (g.name, "reference not exact")
    return c


@functools.lru_cache(maxsize=None)
def bnin_bwd_case(m, K, C, tier, seed=0):
    """conv1x1_bnin_dgrad operands: dz, h3 [M, K], bcoef [3][K], w [K, 1, 1, C], and (bn_x, bn_coef) [M, C] of the
    BN + ReLU that produced the conv's input; with the reference dh = bn_bwd_apply_ref.
    Tier "A": integer dz in [-2, 2], h3 on the 1/8 grid, a a power of two in [1/2, 2] of either sign, b a multiple
    of 1/8 in [-1, 1], c one in [-2, 2]: a dz + b h3 + c is a multiple of 2^-6 below 2^4, exact in fp32 at every
    step; sparse integer w; (bn_x, bn_coef) from dyadic_bn.  Tier "B": randn, bcoef from a real bn_bwd_ref."""
    shape = (*BNIN_M[m], K)
    xshape = (*BNIN_M[m], C)
    g = G(f"bnin_b_{m}_{K}_{C}", *xshape, K, 1)
    gen = torch.Generator().manual_seed(8000 + seed + m + 3 * C + 5 * K)
    if tier == "A":
        dz = _sparse_int(shape, 0.6, gen).to(BF)
        h3 = (torch.randint(-64, 65, shape, generator=gen).double() / 8).to(BF)
        a = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (K,), generator=gen)]
        a = a * (torch.randint(0, 2, (K,), generator=gen) * 2 - 1)
        bcoef = torch.stack([a, torch.randint(-8, 9, (K,), generator=gen) / 8,
                             torch.randint(-16, 17, (K,), generator=gen) / 8]).float()
        w = _sparse_int((K, 1, 1, C), 0.3, gen)
        for j in range(max(C, K)):
            if w[j % K, 0, 0, j % C] == 0:
                w[j % K, 0, 0, j % C] = (1, -1, 2, -2)[j % 4]
        bn_x, bn_coef, pre = dyadic_bn(xshape, 800 + seed + m + C, zero_frac=0.2)
        bc = bn_coef.double()
        bn_x = bn_x.clone()
        bn_x[0, 0, 0] = (-bc[1] / bc[0]).to(BF)  # (row 0 wholly at the threshold: also M = 1 has hits)
    else:
        dz = torch.randn(shape, generator=gen).to(BF)
        h3 = torch.randn(shape, generator=gen).to(BF)
        gamma = 1 + 0.25 * torch.randn(K, generator=gen)
        f = bn_fwd_ref(h3.reshape(-1, K), gamma, torch.zeros(K), torch.zeros(K), torch.ones(K))
        c3 = torch.stack([f["scale"], f["shift"], f["mean"], f["invstd"]]).float()
        bw = bn_bwd_ref(dz.reshape(-1, K), h3.reshape(-1, K), gamma, c3)
        bcoef = torch.stack([bw["k1"], bw["b"], bw["c"]]).float()
        w = torch.randn(K, 1, 1, C, generator=gen) / K ** 0.5
        bn_x = torch.randn(xshape, generator=gen).to(BF)
        g2, b2 = 1 + 0.25 * torch.randn(C, generator=gen), 0.5 * torch.randn(C, generator=gen)
        f2 = bn_fwd_ref(bn_x.reshape(-1, C), g2, b2, torch.zeros(C), torch.ones(C))
        bn_coef = torch.stack([f2["scale"], f2["shift"], f2["mean"], f2["invstd"]]).float()
    w = w.to(BF)
    dh = bn_bwd_apply_ref(dz, h3, bcoef)
    c = dict(dz=dz, h3=h3, bcoef=bcoef, w=w, bn_x=bn_x, bn_coef=bn_coef, dh=dh, g=g)
    if tier == "A":
        b = bcoef.double()
        exact = b[0] * dz.double() + b[1] * h3.double() + b[2]
        inner = b[1] * h3.double() + b[2]
        assert torch.equal(exact.float().double(), exact) and torch.equal(inner.float().double(), inner)
        assert torch.equal(exact * 64, (exact * 64).round()) and exact.abs().max() < 16, (g.name, "dh off the 2^-6 grid")
        mag = conv_ref(torch.zeros(xshape), w.double().abs(), dh.double().abs(), g, bounds=False)["dx"].max().item()
        assert mag * 64 < 2 ** 24, (g.name, "reference not exact")
    return c


def partials_ref(dz, x, coef):
    """fp64 [sum dz, sum dz (x - mean)] per channel and the fp32 budgets of bn_bwd_ref (b_s = M u32 sum |dz|,
    b_q = (M + 2) u32 sum |dz (x - mean)|); ``exact``: every term a multiple of 2^-9 (dz of 2^-6, x - mean of
    2^-3) and 2^9 sum |terms| < 2^24, so any fp32 summation order gives the reference itself."""
    C = dz.shape[-1]
    d, xc = dz.double().reshape(-1, C), x.double().reshape(-1, C) - coef.double()[2]
    M = d.shape[0]
    ref = torch.stack([d.sum(0), (d * xc).sum(0)])
    mag = torch.stack([d.abs().sum(0), (d * xc).abs().sum(0)])
    bound = torch.stack([M * u32 * mag[0], (M + 2) * u32 * mag[1]]) + FLOOR
    on_grid = torch.equal(d * 64, (d * 64).round()) and torch.equal(xc * 8, (xc * 8).round())
    return ref, bound, bool(on_grid and mag.max().item() * 512 < 2 ** 24)


# ----- emulations (fp32 torch on the CPU, no kernel) of the arithmetic the budgets above are counted from
def conv_bn_emulate(c, g, alpha=0.5):
    """Operand on load, bf16 round, fp32 product, bf16 round (dw: fp32, dw0 + alpha dW)."""
    y, _, dw = conv_emulate(c["a"], c["w"], c["dy"], g)
    return y, c["dw0"] + alpha * dw


def pool_bn_bwd_emulate(c, idx, H, W):
    """maxpool_bn_bwd in fp32: gather (fp32 adds), mask, fp32 sums, bn.hip's finalize, dh = bf16(a dz + (b h + c)).
    Returns (dh, dgamma, dbeta) accumulated onto g0 / b0."""
    C = c["h"].shape[-1]
    g, _ = pool_gather_ref(c["dy"], idx, H, W, 3, 2, 1)
    dz = (g.float() * (c["pre"] > 0)).reshape(-1, C)
    hf, coef = c["h"].float().reshape(-1, C), c["coef"]
    M = hf.shape[0]
    s, q = dz.sum(0).double(), (dz * (hf - coef[2])).sum(0).double()
    dgamma, dbeta = c["g0"] + (q * coef[3].double()).float(), c["b0"] + s.float()
    k1, b, cc = bn_bwd_finalize_emulate(s, q, M, c["gamma"], coef)
    return (k1 * dz + (b * hf + cc)).to(BF).reshape(c["h"].shape), dgamma, dbeta


def bn_bwd_finalize_emulate(s, q, M, gamma, coef):
    """bn.hip's bn_bwd_finalize in fp32 from the (double) sums: a = k1 = gamma invstd, b = -k1 invstd^2 q / M,
    c = -k1 s / M - b mean, with 1 / M formed once in fp32."""
    k1 = gamma.float() * coef[3]
    invM = torch.tensor(1.0) / torch.tensor(float(M))
    b = -k1 * coef[3] * coef[3] * q.float() * invM
    return k1, b, -k1 * s.float() * invM - b * coef[2]


def split_partials(dz, x, coef):
    """BN-backward partials [2][C][2] as a producer's epilogue would hand them over: the fp64 sums of the first
    ceil(M / 2) rows and of the rest, each rounded once to fp32 (u32 |sum| per column: inside b_s and b_q)."""
    d = dz.double()
    xc = x.double() - coef.double()[2]
    M = d.shape[0]
    k = (M + 1) // 2
    cols = [torch.stack([d[a:b].sum(0), (d[a:b] * xc[a:b]).sum(0)]) for a, b in ((0, k), (k, M))]
    return torch.stack(cols, -1).float().contiguous()
