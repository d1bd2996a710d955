"""Edge-case tests of the dense GEMM kernels (hgemm.hip in its dense modes with hgemm_finalize, the dense fallbacks
on igemm.hip behind linear_fwd / linear_dgrad / linear_wgrad, gemm_f32.hip) against the fp64 references of
tests/_gemm_ref.py.  Every reference is computed from the values the kernel sees (bf16 operands widened); every
check is per element -- torch.equal on the bits, or a ratio against a budget computed from the reference; none
uses a tensor norm.  Outputs are written into the leading part of larger buffers of random bits (ldc = N + 8 through
the raw entry, extra rows behind M wherever a binding takes its output; linear_dgrad, linear32_fwd and linear32_dgrad
allocate theirs): the pad columns and the trailing rows must come back bit-unchanged.

Tier A (exact): integer operands whose every fp32 partial sum is exact in any order, so the outputs must equal the
reference bit for bit whatever tile, K split, slab order, atomics or schedule a route uses.
Tier B (randn): a test passes when max |err| / bound <= 1 and prints that ratio; each bound is a count of roundings
evaluated on the reference (derivations in _gemm_ref.py).  Non-finite outputs count as infinite error.

Measured (MI355X, worst |err| / bound over all cases of the test; 1.0 = at the bound):

    Tier A (bitwise)
      (a) raw hgemm, NT x 4 tiles, NN x 2, TN x 1, splits 1 / 2 / 3: HE_F32 + bias, + residual, residual aliasing
          the output, HE_ACC_F32, HE_BF16, + ReLU, GELU's aux_out, GELU backward (aux_in = +-8)        exact
          the GELU output itself (by budget, integer pre-activations)                                  0.617
      (b) TN + dbias, splits 1 / 3 / planner's (4), overwrite and accumulate: dw, db                   exact
      (c) grids of 1, 2, 7, 8, 9, 17 blocks, dynamic and static schedule, two launches on one stream
          and one on a second stream, fp32 + bias and bf16 + ReLU                                      exact
      (d) two-launch plans: linear_fwd fp32 + bias + residual and GELU's aux_out, linear_dgrad with
          gelu_in and alpha_t, linear_wgrad dw and db (overwrite and accumulate)                       exact
          linear_fwd's GELU output across the cut (by budget)                                          0.560
      (e) linear_wgrad overwrite into NaN / accumulate / column-padded dy with NaN behind a_dim,
          the atomics fallback, 12 grouped problems with and without a CU budget: dw, db               exact
      (f) implicit-GEMM fallbacks of linear_fwd and linear_dgrad                                       exact
      (g) linear32_fwd (+ bias, ReLU, dropout mask) / linear32_dgrad (+ mask) / linear32_wgrad         exact

    Tier B (randn)             f32+bias  f32+res  in place  acc    bf16   relu   gelu   aux_out  gelu_bwd
      (a) NT, tiles 0 - 3      0.002     0.009    0.008     0.008  0.982  0.973  0.979  0.982    0.980
          NN, tiles 0 - 1      0.001     0.007    0.008     0.007  0.989  0.973  0.980  0.989    0.968
          TN, tile 0           0.001     0.010    0.008     0.010  0.987  0.976  0.979  0.987    0.981
          (the four tiles of a layout give identical figures: the K order inside a unit is the same;
          bf16 outputs: the bound is one bf16 rounding plus a small fp32 term, and a rounding is reached)
      (b) TN + dbias           dw 0.014   db 0.002
      (f) linear_fwd K = 40 0.984   K = 784 0.900   fp32 + ReLU 0.007   linear_dgrad out_features % 64 != 0 0.984
          bf16 residual (two roundings, b_bf16_res): linear_fwd 0.916   linear_dgrad 0.970, 0.967 -- the fp32
          emulation of igemm.hip's finish_row gives the same three figures (test_gemm_ref_cpu.py)
      (g) linear32_fwd 0.745   linear32_dgrad 0.975   linear32_wgrad 0.561
          (linear32_fwd at K = 1 with a bias is 1.49 against K u32 mag, in plain fp32 torch too: the bias add is
          a rounding of its own, so the budget counts it -- _gemm_ref.py)

    Cut axes of (d) on the machine used (256 CUs): linear_fwd 3080 x 5128 x 256 along N and 5128 x 3080 x 256 along M
    (no reserve, bf16 and fp32 output); linear_dgrad 72 x 4168 x 1024 along N (the tail in 4 K splits) and
    584 x 5640 x 256 along M (reserve 240; like TN, NN with a bf16 output is cut along N only from K = 512 up);
    linear_wgrad 264 x 4168 x 1024 along N
    and 4168 x 264 x 1024 along M (reserve 240, the tail in 4 K splits).
    Wall time: 8.8 s for the file; slowest test 2.6 s (test_d_two_launch_linear_fwd, 15.8 M outputs per case).

Every family's test asserts the route it is named after (C.hgemm_plan / C.hgemm_plan2 or the dispatch condition of
conv.cpp); a family whose route is not taken fails.  Not covered here: stream-K (set_hgemm_sk; off by default, its
owners wait on blocks of their own grid), the implicit-im2col and BN-statistics epilogues of hgemm.hip
(test_resnet_kernels_gpu.py), the optimizer kernels.
"""
import contextlib
import functools

import pytest
import torch

import _gemm_ref as R

pytestmark = pytest.mark.gpu
dev = "cuda"
BF = torch.bfloat16
NAN = float("nan")
E_BF16, E_F32, E_ACC = 0, 1, 2                       # hgemm.h HEpi
A_NONE, A_RELU, A_GELU, A_GELU_BWD = 0, 1, 2, 3      # igemm.h Act, hgemm.h HACT_GELU_BWD


# ==================================================================== helpers
def _bits(t):
    return t.contiguous().view({BF: torch.int16, torch.float32: torch.int32}[t.dtype])


def _exact(what, got, ref64):
    """got (bf16 / fp32) must hold exactly the fp64 reference's values, bit for bit (the sign of a zero aside:
    + 0.0 on both sides before the bits are compared; a NaN never compares equal).  Compared where got lives."""
    ref64 = ref64.to(got.device) + 0.0
    want = ref64.to(got.dtype)
    assert torch.equal(want.double(), ref64), f"{what}: the reference is not representable"
    g = got.detach() + 0.0
    assert g.shape == want.shape, f"{what}: shape {tuple(g.shape)} != {tuple(want.shape)}"
    if not torch.equal(_bits(g), _bits(want)):
        bad = (_bits(g) != _bits(want)).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {bad.shape[0]} of {g.numel()} elements differ; first at {i}: got {g[i].item()}, "
                             f"want {want[i].item()}")


def _ratio(name, got, ref, bound):
    """Worst |got - ref| / bound over the elements (printed); non-finite outputs count as infinite."""
    g = got.detach().double()
    err = (g - ref.to(g.device)).abs()
    err = torch.where(torch.isfinite(g), err, torch.full_like(err, float("inf")))
    r = (err / bound.to(g.device)).max().item()
    print(f"  {name}: worst |err|/bound = {r:.3f}")
    return r


def _check(tag, rs):
    for k, r in rs.items():
        assert r <= 1.0, f"{tag}: {k} exceeds its rounding budget, worst ratio {r:.3f}"


class Canary:
    """A [rows + 3, cols + pad] buffer of random bits (pad = 8 through the raw entry, 0 where a binding wants a
    contiguous output: then only the trailing rows guard) whose leading [rows, cols] part holds ``fill`` (NaN by
    default: an element the kernel does not write stays visible); check() asserts everything else is bit-unchanged."""

    def __init__(self, rows, cols, dtype, fill=NAN, pad=8, seed=12345):
        g = torch.Generator(device="cpu").manual_seed(seed)
        shape = (rows + 3, cols + pad)
        if dtype == BF:
            raw = torch.randint(-32768, 32767, shape, generator=g, dtype=torch.int16).to(dev).view(BF)
        else:
            raw = torch.randint(-2 ** 31, 2 ** 31 - 1, shape, generator=g, dtype=torch.int32).to(dev).view(torch.float32)
        self.buf, self.view, self.rows, self.cols = raw, raw[:rows, :cols], rows, cols
        self.view.copy_(fill.to(dev).to(dtype)) if torch.is_tensor(fill) else self.view.fill_(fill)
        self.snap = self._outside()

    def _outside(self):
        b = _bits(self.buf).clone()
        b[:self.rows, :self.cols] = 0
        return b

    @property
    def ld(self):
        return self.buf.shape[1]

    @property
    def out(self):  # the contiguous [rows, cols] leading part (pad = 0 only)
        assert self.ld == self.cols
        return self.buf[:self.rows]

    def check(self, what):
        torch.cuda.synchronize()
        assert torch.equal(self._outside(), self.snap), f"{what}: stored outside its M x N output"


def _vec_canary(n, fill):
    c = Canary(1, n, torch.float32, fill.view(1, -1), pad=0)
    return c, c.buf.view(-1)[:n]


@functools.lru_cache(maxsize=None)
def _dev_case(tier, M, N, K, lay, out="f32"):
    """The case's tensors on the GPU, with the fp64 product s = A B, sum |a||b|, and (tn) the row sums of A^T."""
    c = R.int_case(M, N, K, lay, out) if tier == "A" else R.randn_case(M, N, K, lay)
    d = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in c.items()}
    Am, Bm = R._mats(d["A"], d["B"], lay)
    d["s"], d["smag"] = Am @ Bm, Am.abs() @ Bm.abs()
    if lay == "tn":
        d["rs"], d["rsmag"] = Am.sum(1), Am.abs().sum(1)
    if tier == "A":  # +-8: gelu' is exactly 1 / 0 (test_gemm_ref_cpu.py), the backward epilogue an exact mask
        g = torch.Generator().manual_seed(M * 7 + N)
        d["aux"] = (torch.randint(0, 2, (M, N), generator=g) * 16.0 - 8.0).to(BF).to(dev)
    return d


def _lds(M, N, K, lay):
    return {"nt": (K, K), "nn": (K, N), "tn": (M, N)}[lay]


@contextlib.contextmanager
def _forced(C, cfg, splits):
    C.set_hgemm_force(cfg, splits)
    try:
        yield
    finally:
        C.set_hgemm_force(-1, -1)


@contextlib.contextmanager
def _reserve(C, n):
    """A CU budget of n slots left free while a collective is marked in flight; restored on exit."""
    C.set_cu_reserve(n)
    C.set_comm_active(n > 0)
    try:
        yield
    finally:
        C.set_comm_active(False)
        C.set_cu_reserve(0)


def _plan(C, M, N, K, lay, ob, cfg=-1, splits=-1):
    """(cfg, splits, kps, grid) the planner gives this GEMM with the tile / split pinned as the raw entry pins them."""
    ak, bk = R.LAYOUTS[lay]
    with _forced(C, cfg, splits):
        return C.hgemm_plan(M, N, K, ak, bk, splits != 1, ob)[:4]


def _raw(C, d, out, epi, act=A_NONE, alpha=1.0, cfg=-1, splits=-1, bias=None, residual=None, aux_in=None, aux_out=None,
         dbias=None):
    """C.hgemm on case d into the Canary ``out`` (ldc = N + 8); residual / aux_* are Canaries of the same leading
    dimension (or ``out`` itself: the residual aliasing the output)."""
    M, N, K, lay = d["M"], d["N"], d["K"], d["layout"]
    ak, bk = R.LAYOUTS[lay]
    lda, ldb = _lds(M, N, K, lay)
    C.hgemm(d["A"], d["B"], out.buf, M, N, K, lda, ldb, out.ld, ak, bk, epi=epi, act=act, bias=bias,
            residual=None if residual is None else residual.buf, aux_in=None if aux_in is None else aux_in.buf,
            aux_out=None if aux_out is None else aux_out.buf, alpha=alpha, cfg=cfg, splits=splits, dbias=dbias)
    return out.view


# ============================================================ (a) raw C.hgemm
def _a_epilogues(C, tier, M, N, K, lay, cfg, splits, rs):
    """Every epilogue of the raw entry on one (shape, tile, split); Tier A bitwise, Tier B ratios into ``rs``."""
    ob_cfg = _plan(C, M, N, K, lay, 4, cfg, splits)
    assert ob_cfg[:2] == (cfg, splits), f"planner refused cfg {cfg} splits {splits} for {(M, N, K, lay)}: {ob_cfg}"
    tag = f"{lay} {M}x{N}x{K} cfg{cfg} s{splits}"
    f = _dev_case(tier, M, N, K, lay, "f32")
    h = _dev_case(tier, M, N, K, lay, "bf16") if tier == "A" else f
    A = tier == "A"

    def fin(name, got, y, bound=None):
        if bound is None:
            _exact(f"{tag} {name}", got, y)
        else:
            rs[name] = max(rs.get(name, 0.0), _ratio(f"{tag} {name}", got, y, bound))

    # HE_F32 + bias
    o = Canary(M, N, torch.float32)
    y, mag = 2.0 * f["s"] + f["bias"], 2.0 * f["smag"] + f["bias"].abs()
    fin("f32+bias", _raw(C, f, o, E_F32, alpha=2.0, cfg=cfg, splits=splits, bias=f["bias"]), y,
        None if A else R.b_f32(mag, K, splits))
    o.check(tag)
    # HE_F32 + residual (its own buffer)
    o, res = Canary(M, N, torch.float32), Canary(M, N, torch.float32, f["res"], seed=7)
    y, mag = 0.5 * f["s"] + f["res"], 0.5 * f["smag"] + f["res"].abs()
    fin("f32+res", _raw(C, f, o, E_F32, alpha=0.5, cfg=cfg, splits=splits, residual=res), y,
        None if A else R.b_f32(mag, K, splits))
    o.check(tag)
    # HE_F32 + bias, the residual aliasing the output
    o = Canary(M, N, torch.float32, f["res"])
    y, mag = 2.0 * f["s"] + f["bias"] + f["res"], 2.0 * f["smag"] + f["bias"].abs() + f["res"].abs()
    fin("f32 in place", _raw(C, f, o, E_F32, alpha=2.0, cfg=cfg, splits=splits, bias=f["bias"], residual=o), y,
        None if A else R.b_f32(mag, K, splits))
    o.check(tag)
    # HE_ACC_F32 with alpha
    o = Canary(M, N, torch.float32, f["acc"])
    y, mag = 0.5 * f["s"] + f["acc"], 0.5 * f["smag"] + f["acc"].abs()
    fin("acc", _raw(C, f, o, E_ACC, alpha=0.5, cfg=cfg, splits=splits), y, None if A else R.b_f32(mag, K, splits))
    o.check(tag)
    # HE_BF16 plain and with ReLU
    o = Canary(M, N, BF)
    y, mag = 0.5 * h["s"] + h["bias"], 0.5 * h["smag"] + h["bias"].abs()
    fin("bf16", _raw(C, h, o, E_BF16, alpha=0.5, cfg=cfg, splits=splits, bias=h["bias"]), y,
        None if A else R.b_bf16(y, mag, K, splits))
    o.check(tag)
    o = Canary(M, N, BF)
    y2, mag2 = 2.0 * h["s"] + h["bias"], 2.0 * h["smag"] + h["bias"].abs()
    fin("relu", _raw(C, h, o, E_BF16, A_RELU, alpha=2.0, cfg=cfg, splits=splits, bias=h["bias"]), y2.clamp(min=0),
        None if A else R.b_bf16(y2, mag2, K, splits))
    o.check(tag)
    # HE_BF16 + GELU with aux_out: the stored pre-activation exact in Tier A, the activation by budget
    o, aux = Canary(M, N, BF), Canary(M, N, BF, seed=9)
    got = _raw(C, h, o, E_BF16, A_GELU, alpha=0.5, cfg=cfg, splits=splits, bias=h["bias"], aux_out=aux)
    g, gb = R.b_gelu(y, mag, K, splits)
    rs["gelu"] = max(rs.get("gelu", 0.0), _ratio(f"{tag} gelu", got, g, gb))
    fin("aux_out", aux.view, y, None if A else R.b_bf16(y, mag, K, splits))
    o.check(tag)
    aux.check(tag + " aux_out")
    # HE_BF16 + GELU backward with aux_in (Tier A: aux = +-8, an exact mask)
    o, aux = Canary(M, N, BF), Canary(M, N, BF, h["aux"], seed=9)
    got = _raw(C, h, o, E_BF16, A_GELU_BWD, alpha=2.0, cfg=cfg, splits=splits, aux_in=aux)
    yb, bb = R.b_gelu_bwd(2.0 * h["s"], 2.0 * h["smag"], h["aux"].double(), K, splits)
    fin("gelu_bwd", got, yb, None if A else bb)
    o.check(tag)
    aux.check(tag + " aux_in")


@pytest.mark.parametrize("cfg", [0, 1, 2, 3])
@pytest.mark.parametrize("lay", ["nt", "nn", "tn"])
def test_a_raw_hgemm_tier_a_bitwise(C, lay, cfg):
    """(a) every epilogue x every candidate M / N / K x splits {1, 2, 3}, bit for bit (the GELU output by budget)."""
    if cfg not in R.CFGS[lay]:
        ak, bk = R.LAYOUTS[lay]
        with _forced(C, cfg, 1):  # layout_ok: the planner has no such kernel, and says so
            assert C.hgemm_plan(520, 520, 192, ak, bk, False, 2)[0] == -1
        return
    rs = {}
    for M, N, K, splits in R.RAW[lay]:
        _a_epilogues(C, "A", M, N, K, lay, cfg, splits, rs)
    _check(f"{lay} cfg{cfg}", rs)


@pytest.mark.parametrize("lay,cfg", [(lay, cfg) for lay in R.CFGS for cfg in R.CFGS[lay]])
def test_a_raw_hgemm_tier_b_budgets(C, lay, cfg):
    """(a) the same epilogues on randn operands against the rounding budgets."""
    rs = {}
    for M, N, K, splits in R.RAW_B[lay]:
        _a_epilogues(C, "B", M, N, K, lay, cfg, splits, rs)
    print(f"(a) {lay} cfg{cfg}: " + "  ".join(f"{k} {v:.3f}" for k, v in rs.items()))
    _check(f"{lay} cfg{cfg}", rs)


# ============================================= (b) TN with the fused bias gradient
@pytest.mark.parametrize("splits", [1, 3, -1])
@pytest.mark.parametrize("tier", ["A", "B"])
def test_b_tn_fused_bias_gradient(C, tier, splits):
    """(b) dw and db per element, overwrite (HE_F32) and accumulate, alpha != 1: db rows at the M tail, N over
    four tile columns (a sum taken once per tile column would show as a factor), K-split partials."""
    rs = {}
    for M, N, K in R.DBIAS:
        if splits == 3 and K < 64 * 12:
            continue  # (the planner takes 3 splits only with >= 4 K-tiles in each)
        cfg, s, _, _ = _plan(C, M, N, K, "tn", 4, 0, splits)
        assert cfg == 0 and (splits < 0 or s == splits), (cfg, s)
        d = _dev_case(tier, M, N, K, "tn", "f32")
        for epi, alpha in ((E_F32, 0.5), (E_ACC, 2.0)):
            tag = f"tn {M}x{N}x{K} s{s} epi{epi}"
            o = Canary(M, N, torch.float32, NAN if epi == E_F32 else d["acc"])
            dbc, db = _vec_canary(M, d["db0"])
            got = _raw(C, d, o, epi, alpha=alpha, cfg=0, splits=splits, dbias=db)
            y = alpha * d["s"] + (d["acc"] if epi == E_ACC else 0.0)
            mag = alpha * d["smag"] + (d["acc"].abs() if epi == E_ACC else 0.0)
            dbr = alpha * d["rs"] + d["db0"]
            if tier == "A":
                _exact(tag + " dw", got, y)
                _exact(tag + " db", db, dbr)
            else:
                rs["dw"] = max(rs.get("dw", 0.0), _ratio(tag + " dw", got, y, R.b_f32(mag, K, s)))
                rs["db"] = max(rs.get("db", 0.0), _ratio(tag + " db", db, dbr, R.b_db(alpha * d["rs"], alpha * d["rsmag"],
                                                                                      K, s, d["db0"])))
            o.check(tag)
            dbc.check(tag + " db")
    _check("tn dbias", rs)


# ========================================= (c) more than one unit per block
def _one_stream_twice_then_second_stream(C, run, check):
    for i in range(2):  # back to back on one stream: the claim counters must have reset themselves
        check(run(), f"launch {i}")
    s2 = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s2):
        got = run()
    s2.synchronize()
    check(got, "second stream")


MULTI_COMBOS = [("nt", 0, 1), ("nt", 0, 3), ("nt", 1, 1), ("nt", 2, 3), ("nt", 3, 1), ("nn", 1, 1), ("nn", 0, 3), ("tn", 0, 3)]


@pytest.mark.parametrize("grid", [1, 2, 7, 8, 9, 17])
def test_c_multi_unit_blocks_small_grid(C, grid):
    """(c) a CU budget shrinks the persistent grid to 1 .. 17 blocks, so every block computes several units (the next
    unit's prologue DMA is issued between the epilogue math and the epilogue stores) -- under the dynamic schedule
    (grid < 9: S = 0, every unit claimed, CK = 1, exit-count groups partly empty) and the static one, each against
    the fp64 reference bit for bit, twice on one stream and once on a second stream."""
    M, N, K = R.MULTI
    ncu = C.num_cus()
    was = C.set_hgemm_dynamic(True)
    ran = 0
    try:
        for lay, cfg, splits in MULTI_COMBOS:
            bm, bn = R.TILE[cfg]
            units = -(-M // bm) * -(-N // bn) * splits
            bpc = 2 if cfg == 3 else 1
            if units <= grid or grid < bpc:
                continue  # (no block would get a second unit; the planner never goes below one CU's blocks)
            f = _dev_case("A", M, N, K, lay, "f32")
            h = _dev_case("A", M, N, K, lay, "bf16")
            with _reserve(C, ncu * bpc - grid):
                for ob in (4, 2):
                    pl = _plan(C, M, N, K, lay, ob, cfg, splits)
                    assert (pl[0], pl[1], pl[3]) == (cfg, splits, grid), f"planned {pl}, wanted grid {grid}"
                for dyn in (True, False):
                    C.set_hgemm_dynamic(dyn)
                    tag = f"{lay} cfg{cfg} s{splits} grid{grid} dyn{int(dyn)}"
                    o32, o16 = Canary(M, N, torch.float32), Canary(M, N, BF)

                    def run32():
                        o32.view.fill_(NAN)
                        return _raw(C, f, o32, E_F32, alpha=2.0, cfg=cfg, splits=splits, bias=f["bias"])

                    def run16():
                        o16.view.fill_(NAN)
                        return _raw(C, h, o16, E_BF16, A_RELU, alpha=2.0, cfg=cfg, splits=splits, bias=h["bias"])

                    y32, y16 = 2.0 * f["s"] + f["bias"], (2.0 * h["s"] + h["bias"]).clamp(min=0)
                    _one_stream_twice_then_second_stream(C, run32, lambda g, w: _exact(f"{tag} f32 {w}", g, y32))
                    _one_stream_twice_then_second_stream(C, run16, lambda g, w: _exact(f"{tag} bf16 {w}", g, y16))
                    o32.check(tag)
                    o16.check(tag)
                    ran += 1
    finally:
        C.set_hgemm_dynamic(was)
    assert ran >= 2 * (len(MULTI_COMBOS) - 1), ran  # (grid 1: not the 2-per-CU tile; grid 17: not 12 whole-K tiles)


# ===================================================== (d) two-launch plans
# R.CUT_CANDIDATES per layout, walked under no reserve and under a reserve of all but 16 CUs until C.hgemm_plan2
# reports a cut.
CUTS_SEEN = {}


def _find_cuts(C, lay, ob):
    """{axis: (M, N, K, reserve, plan2)} over the candidate list: the first shape / reserve per cut axis."""
    ak, bk = R.LAYOUTS[lay]
    cuts = {}
    for reserve in (0, C.num_cus() - 16):
        with _reserve(C, reserve):
            for M, N, K in R.CUT_CANDIDATES[lay]:
                p = C.hgemm_plan2(M, N, K, ak, bk, True, ob)
                if p[1] >= 0 and p[1] not in cuts:
                    cuts[p[1]] = (M, N, K, reserve, p)
    assert cuts, f"no candidate of {lay} (out bytes {ob}) is planned in two launches"
    for axis, (M, N, K, reserve, p) in cuts.items():
        CUTS_SEEN[(lay, ob, axis)] = (M, N, K, reserve)
        print(f"  two-launch plan: {lay} out_bytes {ob} {M}x{N}x{K} reserve {reserve}: axis {axis} at {p[2]}, "
              f"main {p[0][:4]}, tail {p[3][:4]}")
    return cuts


def _flat_canary(rows, cols, dtype, fill=NAN):
    return Canary(rows, cols, dtype, fill, pad=0)


def test_d_two_launch_linear_fwd(C):
    """(d) linear_fwd across the cut, per element: bias + GELU + aux_out (bf16) and fp32 + bias + residual -- the
    tail launch's C, bias, residual and aux_out pointers are offset by the cut."""
    for ob in (2, 4):
        cuts = _find_cuts(C, "nt", ob)
        assert set(cuts) == {0, 1}, f"expected a cut along N and one along M, got {sorted(cuts)}"
        for axis, (M, N, K, reserve, p) in cuts.items():
            d = _dev_case("A", M, N, K, "nt", "bf16" if ob == 2 else "f32")
            tag = f"linear_fwd {M}x{N}x{K} axis {axis} out_bytes {ob}"
            with _reserve(C, reserve):
                if ob == 2:
                    o, aux = _flat_canary(M, N, BF), _flat_canary(M, N, BF)
                    y = C.linear_fwd(d["A"], d["B"], d["bias"], A_GELU, False, None, o.out, aux.out)
                    v, mag = d["s"] + d["bias"], d["smag"] + d["bias"].abs()
                    _exact(tag + " aux_out", aux.view, v)
                    g, gb = R.b_gelu(v, mag, K, max(p[0][1], p[3][1]))
                    _check(tag, {"gelu": _ratio(tag + " gelu", y, g, gb)})
                    aux.check(tag + " aux_out")
                else:
                    o, res = _flat_canary(M, N, torch.float32), d["res"].clone()
                    y = C.linear_fwd(d["A"], d["B"], d["bias"], A_NONE, True, res, o.out, None)
                    _exact(tag, y, d["s"] + d["bias"] + d["res"])
                    assert torch.equal(res, d["res"])
                o.check(tag)


def test_d_two_launch_linear_dgrad(C):
    """(d) linear_dgrad with gelu_in (+-8: an exact mask) and the alpha_t device scalar across the cut; along N the
    tail is K-split, so its slab finalize reads aux_in at the cut's offset."""
    cuts = _find_cuts(C, "nn", 2)
    assert set(cuts) == {0, 1}, f"expected a cut along N and one along M, got {sorted(cuts)}"
    alpha_t = torch.full((1,), R.ALPHA_T, device=dev)
    for axis, (M, N, K, reserve, p) in cuts.items():
        d = _dev_case("A", M, N, K, "nn", "bf16")
        with _reserve(C, reserve):
            dx = C.linear_dgrad(d["A"], d["B"], None, alpha_t, d["aux"])
        yb, _ = R.b_gelu_bwd(R.ALPHA_T * d["s"], d["smag"], d["aux"].double(), K)
        _exact(f"linear_dgrad {M}x{N}x{K} axis {axis}", dx, yb)


def test_d_two_launch_linear_wgrad(C):
    """(d) linear_wgrad with the fused bias gradient across the cut (the tail K-split: its slab finalize gets the
    offset dbias, C and a_dim), overwrite into NaN and accumulate."""
    cuts = _find_cuts(C, "tn", 4)
    assert set(cuts) == {0, 1}, f"expected a cut along N and one along M, got {sorted(cuts)}"
    for axis, (M, N, K, reserve, p) in cuts.items():
        d = _dev_case("A", M, N, K, "tn", "f32")
        for over in (True, False):
            tag = f"linear_wgrad {M}x{N}x{K} axis {axis} overwrite {over}"
            o = _flat_canary(M, N, torch.float32, NAN if over else d["acc"])
            dbc, db = _vec_canary(M, d["db0"])
            with _reserve(C, reserve):
                C.linear_wgrad(d["A"], d["B"], o.out, 0.5, None, db, 0, over)
            _exact(tag + " dw", o.view, 0.5 * d["s"] + (0.0 if over else d["acc"]))
            _exact(tag + " db", db, 0.5 * d["rs"] + d["db0"])
            o.check(tag)
            dbc.check(tag + " db")


# ======================================= (e) linear_wgrad / linear_wgrad_group
def _wgrad_case(T, n_out, n_in, ldy=None, seed=0):
    """Integer dy [T, ldy] (columns [n_out, round8) zero, [round8, ldy) NaN: never loaded), x [T, n_in], dw0, db0 on
    the GPU with the fp64 dw = dy^T x and db = colsum(dy)."""
    n8 = (n_out + 7) // 8 * 8
    c = R.wgrad_int_case(T, n_out, n_in, seed)
    dy = torch.full((T, ldy or n8), NAN, dtype=BF)
    dy[:, :n8] = c["A"]
    dy[:, n_out:n8] = 0
    d = dict(dy=dy.to(dev), x=c["B"].to(dev), dw0=c["acc"][:n_out].to(dev), db0=c["db0"][:n_out].to(dev))
    a = c["A"].double()[:, :n_out].to(dev)
    d["dw"], d["db"] = a.t() @ d["x"].double(), a.sum(0)
    return d


def test_e_linear_wgrad_overwrite_accumulate_padded(C):
    """(e) overwrite=True into NaN targets is finite and exact, overwrite=False accumulates, the bias gradient
    always accumulates; column-padded dy (N in {10, 259}, ldy 16 / 320): stage_setup clamps every 16-B load to
    a_dim = round8(N), so the NaN columns behind it must reach neither dw nor db; dw has exactly N rows."""
    for T, n_out, n_in, ldy, seed in R.WGRAD_HGEMM:
        assert T % 64 == 0 and C.hgemm_plan2(n_out, n_in, T, False, False, True, 4)[0][0] == 0  # the TN hgemm route
        d = _wgrad_case(T, n_out, n_in, ldy, seed)
        for over in (True, False):
            tag = f"linear_wgrad T{T} {n_out}x{n_in} ldy {ldy} overwrite {over}"
            o = _flat_canary(n_out, n_in, torch.float32, NAN if over else d["dw0"])
            dbc, db = _vec_canary(n_out, d["db0"])
            C.linear_wgrad(d["dy"], d["x"], o.out, 2.0, None, db, 0, over)
            _exact(tag + " dw", o.view, 2.0 * d["dw"] + (0.0 if over else d["dw0"]))
            _exact(tag + " db", db, 2.0 * d["db"] + d["db0"])
            o.check(tag)
            dbc.check(tag + " db")


def test_e_linear_wgrad_fallback_atomics(C):
    """(e) tokens % 64 != 0: the implicit GEMM with fp32 atomics plus colsum; Tier A is exact whatever the order."""
    for T, n_out, n_in, ldy, seed in R.WGRAD_ATOMIC:
        assert T % 64 != 0  # conv.cpp linear_wgrad: not the hgemm route
        d = _wgrad_case(T, n_out, n_in, ldy, seed)
        for over in (True, False):
            tag = f"linear_wgrad (atomics) T{T} {n_out}x{n_in} overwrite {over}"
            o = _flat_canary(n_out, n_in, torch.float32, NAN if over else d["dw0"])
            dbc, db = _vec_canary(n_out, d["db0"])
            C.linear_wgrad(d["dy"], d["x"], o.out, 1.0, None, db, 0, over)
            _exact(tag + " dw", o.view, d["dw"] + (0.0 if over else d["dw0"]))
            _exact(tag + " db", db, d["db"] + d["db0"])
            o.check(tag)
            dbc.check(tag + " db")


GROUP_SHAPES = R.GROUP_SHAPES


@pytest.mark.parametrize("T", R.GROUP_T)
@pytest.mark.parametrize("budget", [False, True])
def test_e_linear_wgrad_group_12(C, T, budget):
    """(e) HGEMM_MAX_GROUP = 12 problems in one launch (40 tiles; one spans 3 x 4 tiles), mixed overwrite (into
    NaN) and accumulate, with and without db, under no reserve and under one that leaves 7 slots; 13 raise."""
    assert C.HGEMM_MAX_GROUP == len(GROUP_SHAPES) == 12
    cs = [_wgrad_case(T, no, ni, None, seed=10 + i) for i, (no, ni) in enumerate(GROUP_SHAPES)]
    over = [i % 3 != 1 for i in range(12)]
    has_db = [i % 2 == 0 for i in range(12)]
    outs = [_flat_canary(no, ni, torch.float32, NAN if ov else c["dw0"]) for (no, ni), c, ov in zip(GROUP_SHAPES, cs, over)]
    dbs = [_vec_canary(no, c["db0"]) if h else None for (no, ni), c, h in zip(GROUP_SHAPES, cs, has_db)]
    tiles = sum(-(-no // 256) * -(-ni // 256) for no, ni in GROUP_SHAPES)
    with _reserve(C, C.num_cus() - 7 if budget else 0):
        assert (C.num_cus() - C.cu_reserve() < tiles) == budget
        C.linear_wgrad_group([c["dy"] for c in cs], [c["x"] for c in cs], [o.out for o in outs],
                             [b[1] if b else torch.empty(0, device=dev) for b in dbs], over)
        for i, (c, o, b) in enumerate(zip(cs, outs, dbs)):
            tag = f"group T{T} problem {i} {GROUP_SHAPES[i]} overwrite {over[i]}"
            _exact(tag + " dw", o.view, c["dw"] + (0.0 if over[i] else c["dw0"]))
            o.check(tag)
            if b:
                _exact(tag + " db", b[1], c["db"] + c["db0"])
                b[0].check(tag + " db")
        before = [_bits(o.buf).clone() for o in outs]
        with pytest.raises(RuntimeError):
            C.linear_wgrad_group([c["dy"] for c in cs] + [cs[0]["dy"]], [c["x"] for c in cs] + [cs[0]["x"]],
                                 [o.out for o in outs] + [outs[0].out], [torch.empty(0, device=dev)] * 13, over + [False])
        torch.cuda.synchronize()
        assert all(torch.equal(_bits(o.buf), b) for o, b in zip(outs, before))


# =================================== (f) dense fallbacks on the implicit GEMM
def _fwd_on_hgemm(K, N, bf16_res, out_f32, act):  # conv.cpp linear_fwd
    return K % 64 == 0 and N % 8 == 0 and not bf16_res and (act == 0 if out_f32 else True)


def _dgrad_on_hgemm(n_out, has_res):  # conv.cpp linear_dgrad
    return n_out % 64 == 0 and not has_res


def _hgemm_could(C, M, N, K, lay, ob):
    """The planner has a plan for the shape: only the epilogue keeps such a GEMM off the persistent kernel."""
    ak, bk = R.LAYOUTS[lay]
    return K % 64 == 0 and C.hgemm_plan2(M, N, K, ak, bk, True, ob)[0][0] >= 0


@pytest.mark.parametrize("tier", ["A", "B"])
def test_f_igemm_linear_fwd_fallbacks(C, tier):
    """(f) linear_fwd outside hgemm's envelope: K % 64 != 0 (K = 40, 784), a bf16 residual, fp32 output + ReLU."""
    rs = {}
    for M, N, K, what in R.FWD_FALLBACK:
        out = "f32" if what == "f32relu" else "bf16"
        d = _dev_case(tier, M, N, K, "nt", out)
        y0, mag = d["s"] + d["bias"], d["smag"] + d["bias"].abs()
        tag = f"linear_fwd {M}x{N}x{K} {what}"
        o = _flat_canary(M, N, BF if out == "bf16" else torch.float32)
        if what == "k":
            assert not _fwd_on_hgemm(K, N, False, False, 0) and not _hgemm_could(C, M, N, K, "nt", 2)
            y = C.linear_fwd(d["A"], d["B"], d["bias"], A_NONE, False, None, o.out, None)
            ref, bound = y0, R.b_bf16(y0, mag, K)
        elif what == "res":
            assert _fwd_on_hgemm(K, N, False, False, 0) and not _fwd_on_hgemm(K, N, True, False, 0)
            assert _hgemm_could(C, M, N, K, "nt", 2)
            res = d["res"].to(BF)
            y = C.linear_fwd(d["A"], d["B"], d["bias"], A_NONE, False, res, o.out, None)
            ref, bound = y0 + res.double(), R.b_bf16_res(y0, mag, res, K)
        else:
            assert _fwd_on_hgemm(K, N, False, True, 0) and not _fwd_on_hgemm(K, N, False, True, A_RELU)
            assert _hgemm_could(C, M, N, K, "nt", 4)
            y = C.linear_fwd(d["A"], d["B"], d["bias"], A_RELU, True, None, o.out, None)
            ref, bound = y0.clamp(min=0), R.b_f32(mag, K)
        if tier == "A":
            _exact(tag, y, ref)
        else:
            rs[tag] = _ratio(tag, y, ref, bound)
        o.check(tag)
    _check("linear_fwd fallbacks", rs)


@pytest.mark.parametrize("tier", ["A", "B"])
def test_f_igemm_linear_dgrad_fallbacks(C, tier):
    """(f) linear_dgrad outside hgemm's envelope: with a (bf16) residual, and at out_features % 64 != 0."""
    rs = {}
    alpha_t = torch.full((1,), R.ALPHA_T, device=dev)
    for M, n_in, n_out, with_res in R.DGRAD_FALLBACK:
        assert not _dgrad_on_hgemm(n_out, with_res) and (_dgrad_on_hgemm(n_out, False) == (n_out % 64 == 0))
        assert _hgemm_could(C, M, n_in, n_out, "nn", 2) == (n_out % 64 == 0)
        d = _dev_case(tier, M, n_in, n_out, "nn", "bf16")
        res = d["res"].to(BF) if with_res else None
        dx = C.linear_dgrad(d["A"], d["B"], res, alpha_t, None)
        y0, mag = R.ALPHA_T * d["s"], R.ALPHA_T * d["smag"]
        ref = y0 + (res.double() if with_res else 0.0)
        tag = f"linear_dgrad {M}x{n_in}x{n_out} residual {with_res}"
        if tier == "A":
            _exact(tag, dx, ref)
        else:
            rs[tag] = _ratio(tag, dx, ref, R.b_bf16_res(y0, mag, res, n_out) if with_res else R.b_bf16(y0, mag, n_out))
    _check("linear_dgrad fallbacks", rs)


# ============================================================ (g) gemm_f32.hip
@pytest.mark.parametrize("mnk", R.F32_CASES, ids=lambda c: "-".join(map(str, c)))
def test_g_gemm_f32(C, mnk):
    """(g) linear32_fwd / dgrad / wgrad: Tier A bitwise, Tier B against (K + epilogue roundings) u32 mag."""
    M, N, K = mnk
    a = {k: v.to(dev) for k, v in R.f32_case(M, N, K, "A").items()}
    y = C.linear32_fwd(a["x"], a["w"], a["bias"], True)
    _exact("linear32_fwd", y, (R.gemm_ref(a["x"], a["w"], "nt", bias=a["bias"])["y"]).clamp(min=0))
    _exact("linear32_dgrad", C.linear32_dgrad(a["dy"], a["w"]), R.gemm_ref(a["dy"], a["w"], "nn")["y"])
    o = _flat_canary(N, K, torch.float32, a["dw0"])
    C.linear32_wgrad(a["dy"], a["x"], o.out, 0.5)
    _exact("linear32_wgrad", o.view, R.gemm_ref(a["dy"], a["x"], "tn", 0.5, acc=a["dw0"])["y"])
    o.check("linear32_wgrad")
    b = {k: v.to(dev) for k, v in R.f32_case(M, N, K, "B").items()}
    rs = {}
    r = R.gemm_ref(b["x"], b["w"], "nt", bias=b["bias"])
    rs["fwd"] = _ratio("linear32_fwd", C.linear32_fwd(b["x"], b["w"], b["bias"]), r["y"], R.b_f32_plain(r["mag"], K, 1))
    r = R.gemm_ref(b["dy"], b["w"], "nn")
    rs["dgrad"] = _ratio("linear32_dgrad", C.linear32_dgrad(b["dy"], b["w"]), r["y"], R.b_f32_plain(r["mag"], N))
    dw = b["dw0"].clone()
    C.linear32_wgrad(b["dy"], b["x"], dw, 0.5)
    r = R.gemm_ref(b["dy"], b["x"], "tn", 0.5, acc=b["dw0"])
    rs["wgrad"] = _ratio("linear32_wgrad", dw, r["y"], R.b_f32_plain(r["mag"], M, 2))
    _check(f"gemm_f32 {mnk}", rs)


@pytest.mark.parametrize("M,N,K", [(63, 10, 15), (65, 10, 784), (65, 66, 17)])
def test_g_gemm_f32_dropout_mask(C, M, N, K):
    """(g) the fused dropout equals C.dropout of ones element for element -- at N = 10 the rows start at flat
    indices that are not multiples of 4, so the kernel's scalar Philox arm runs -- and linear32_dgrad's mask treats
    mask_src == 0 and -0.0 as dropped."""
    a = {k: v.to(dev) for k, v in R.f32_case(M, N, K, "A").items()}
    p, seed, offset = 0.3, 1234, 5
    plain = C.linear32_fwd(a["x"], a["w"], a["bias"], False)
    keep = C.dropout(torch.ones(M, N, device=dev), p, seed, offset)  # 0 or 1 / (1 - p)
    assert 0.55 < (keep != 0).float().mean().item() < 0.85 or M * N < 100
    got = C.linear32_fwd(a["x"], a["w"], a["bias"], False, p, seed, offset)
    _exact("linear32_fwd dropout", got, (plain * keep).double())
    g = torch.Generator().manual_seed(3)
    src = torch.tensor([0.0, -0.0, 1.0, -1.0, 1e-30, -1e-30])[torch.randint(0, 6, (M, K), generator=g)].to(dev)
    dx = C.linear32_dgrad(a["dy"], a["w"], src, 1.25)
    want = torch.where(src > 0, 1.25 * R.gemm_ref(a["dy"], a["w"], "nn")["y"], torch.zeros((), dtype=torch.float64, device=dev))
    _exact("linear32_dgrad mask", dx, want)


# =============================================================== (h) envelope
def test_h_envelope_raises_and_leaves_the_output(C):
    """(h) arguments the launchers document as outside the envelope raise RuntimeError and write nothing."""
    g = torch.Generator().manual_seed(1)
    mk = lambda *s: torch.randn(*s, generator=g).to(BF).to(dev)

    def refused(what, out, **kw):
        before = _bits(out).clone()
        with pytest.raises(RuntimeError):
            C.hgemm(C=out, **kw)
        torch.cuda.synchronize()
        assert torch.equal(_bits(out), before), f"{what}: the refused launch wrote to its output"

    f32 = lambda M, N: torch.randn(M + 2, N, generator=g).to(dev)
    for K in (100, 40, 0):  # K % 64 != 0 (40 and 0: not one K-tile)
        refused(f"K={K}", f32(64, 64), A=mk(64, 128), B=mk(64, 128), M=64, N=64, K=K, lda=128, ldb=128, ldc=64,
                a_k=True, b_k=True, epi=E_F32)
    refused("N % 4", f32(64, 6), A=mk(64, 64), B=mk(6, 64), M=64, N=6, K=64, lda=64, ldb=64, ldc=6, a_k=True, b_k=True,
            epi=E_F32)
    refused("bf16 N % 8", mk(66, 12), A=mk(64, 64), B=mk(12, 64), M=64, N=12, K=64, lda=64, ldb=64, ldc=12, a_k=True,
            b_k=True, epi=E_BF16)
    for ak, bk, B in ((True, True, mk(64, 64)), (True, False, mk(64, 64))):
        refused("dbias, not TN", f32(64, 64), A=mk(64, 64), B=B, M=64, N=64, K=64, lda=64, ldb=64, ldc=64, a_k=ak, b_k=bk,
                epi=E_ACC, dbias=torch.zeros(64, device=dev))
    refused("gelu backward without aux_in", mk(66, 64), A=mk(64, 64), B=mk(64, 64), M=64, N=64, K=64, lda=64, ldb=64,
            ldc=64, a_k=True, b_k=True, epi=E_BF16, act=A_GELU_BWD)
    with _forced(C, -1, -1):
        assert C.hgemm_plan(64, 64, 40, True, True, True, 2)[0] == -1  # (no K-tile: no plan, and no crash)
