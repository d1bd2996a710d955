"""The dense-GEMM references check themselves (no GPU, no kernel): the Tier A cases of _gemm_ref.py really are
exact in fp32 in any summation order and representable in their output type, carry the required nonzero edges and
distinct row / column patterns, and the fp32 emulation of the kernels' roundings stays inside every Tier B budget."""
import pytest
import torch

import _gemm_ref as R
from _gpt2_ref import gelu_grad_ref, gelu_ref

BF = torch.bfloat16


def _ratio(got, ref, bound):
    err = (got.double() - ref).abs()
    err = torch.where(torch.isfinite(got.double()), err, torch.full_like(err, float("inf")))
    return (err / bound).max().item()


def _tier_a():
    cases = []
    for lay, lst in R.RAW.items():
        for M, N, K, _ in lst:
            cases += [(M, N, K, lay, "f32", 0), (M, N, K, lay, "bf16", 0)]
    cases += [(M, N, K, "tn", "f32", 0) for M, N, K in R.DBIAS]
    cases += [R.MULTI + (lay, out, 0) for lay in R.LAYOUTS for out in ("f32", "bf16")]
    return sorted(set(cases + R.extra_tier_a()))  # (a), (b), (c) + (d), (e), (f): every Tier A case of the GPU file


TIER_A = _tier_a()
TIER_B = sorted({(M, N, K, lay, s) for lay, lst in R.RAW_B.items() for M, N, K, s in lst})


def _two_orders(Am, Bm):
    """fp32 A B summed k by k forwards, and in chunks of 64 taken in reverse."""
    Af, Bf = Am.float(), Bm.float()
    K = Af.shape[1]
    fwd = torch.zeros(Af.shape[0], Bf.shape[1])
    for k in range(K):
        fwd.addr_(Af[:, k], Bf[k])
    rev = torch.zeros_like(fwd)
    for k0 in reversed(range(0, K, 64)):
        rev += Af[:, k0:k0 + 64] @ Bf[k0:k0 + 64]
    return fwd, rev


@pytest.mark.parametrize("case", TIER_A, ids=lambda c: "-".join(map(str, c)))
def test_tier_a_is_exact_in_any_order(case):
    M, N, K, lay, out, seed = case
    c = R.int_case(M, N, K, lay, out, seed)
    R.check_int_case(c)  # integers, nonzero last row / column, distinct rows and columns, magnitudes
    Am, Bm = R._mats(c["A"], c["B"], lay)
    ref, mag = Am @ Bm, Am.abs() @ Bm.abs()
    fwd, rev = _two_orders(Am, Bm)
    assert torch.equal(fwd.double(), ref) and torch.equal(rev.double(), ref)
    assert torch.equal((fwd + 0.0).view(torch.int32), (rev + 0.0).view(torch.int32))
    bias = c["bias"].double()
    if out == "bf16":
        for alpha in (0.25, 0.5, 1.0, 2.0):
            y = alpha * ref + bias
            assert y.abs().max().item() <= R.INT_MAX
            assert torch.equal(y.to(BF).double(), y), alpha
        y = R.ALPHA_T * ref + c["res"].double()  # (the data grad's bf16 residual on top of alpha_t)
        assert torch.equal(y.to(BF).double(), y)
    else:
        for alpha in (0.5, 2.0):
            y = alpha * ref + bias + c["res"].double()
            assert (alpha * mag + bias.abs() + c["res"].double().abs()).max().item() < 2 ** 24
            assert torch.equal(y.float().double(), y)
    if lay == "tn":
        assert torch.equal(R.emulate_db(c["A"], 0.5, c["db0"], 3).double(), 0.5 * Am.sum(1) + c["db0"].double())


def test_tier_a_detects_a_shifted_or_transposed_tile():
    """The distinct patterns do their job: a reference with two rows (columns) swapped, or a 16 x 16 block
    transposed, differs from the true one."""
    c = R.int_case(257, 264, 128, "nt", "f32")
    y = R.gemm_ref(c["A"], c["B"], "nt")["y"]
    for i in range(0, 256, 37):
        assert not torch.equal(y[i], y[i + 1]) and not torch.equal(y[:, i], y[:, i + 1])
    blk = y[:16, :16]
    assert not torch.equal(blk, blk.t())


@pytest.mark.parametrize("case", TIER_B, ids=lambda c: "-".join(map(str, c)))
def test_emulation_stays_inside_every_budget(case):
    M, N, K, lay, splits = case
    c = R.randn_case(M, N, K, lay)
    A, B = c["A"], c["B"]
    worst = {}
    r = R.gemm_ref(A, B, lay, 1.0, bias=c["bias"], residual=c["res"])
    worst["f32+bias+res"] = _ratio(R.emulate(A, B, lay, 1.0, c["bias"], c["res"], splits=splits), r["y"],
                                   R.b_f32(r["mag"], K, splits))
    r = R.gemm_ref(A, B, lay, 2.0, acc=c["acc"])
    worst["acc"] = _ratio(R.emulate(A, B, lay, 2.0, acc=c["acc"], splits=splits), r["y"], R.b_f32(r["mag"], K, splits))
    r = R.gemm_ref(A, B, lay, 0.5, bias=c["bias"])
    worst["bf16"] = _ratio(R.emulate(A, B, lay, 0.5, c["bias"], splits=splits, out="bf16"), r["y"],
                           R.b_bf16(r["y"], r["mag"], K, splits))
    worst["relu"] = _ratio(R.emulate(A, B, lay, 0.5, c["bias"], splits=splits, out="bf16", act="relu"),
                           r["y"].clamp(min=0), R.b_bf16(r["y"], r["mag"], K, splits))
    g, v = R.emulate(A, B, lay, 0.5, c["bias"], splits=splits, act="gelu")
    gr, gb = R.b_gelu(r["y"], r["mag"], K, splits)
    worst["gelu"] = _ratio(g, gr, gb)
    worst["aux_out"] = _ratio(v, r["y"], R.b_bf16(r["y"], r["mag"], K, splits))
    r = R.gemm_ref(A, B, lay, 1.0)
    yr, yb = R.b_gelu_bwd(r["y"], r["mag"], c["aux"].double(), K, splits)
    worst["gelu_bwd"] = _ratio(R.emulate(A, B, lay, 1.0, splits=splits, act="gelu_bwd", aux=c["aux"]), yr, yb)
    if lay == "tn":
        r = R.gemm_ref(A, B, lay, 0.5)
        worst["db"] = _ratio(R.emulate_db(A, 0.5, c["db0"], splits), r["db"] + c["db0"].double(),
                             R.b_db(r["db"], r["db_mag"], K, splits, c["db0"]))
    print(case, {k: round(v, 3) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("mnk", R.DBIAS, ids=lambda c: "-".join(map(str, c)))
def test_emulation_dbias_cases(mnk):
    """(b): the HE_F32 overwrite, the accumulate and the bias gradient at 1 split, 3, and 4 (the planner's choice at
    13 K-tiles), wherever every split holds >= 4 K-tiles."""
    M, N, K = mnk
    c = R.randn_case(M, N, K, "tn")
    worst = {}
    for splits in (1, 3, 4):
        if splits > 1 and K // 64 < 4 * (splits - 1) + 1:
            continue
        r = R.gemm_ref(c["A"], c["B"], "tn", 0.5)
        worst[f"dw s{splits}"] = _ratio(R.emulate(c["A"], c["B"], "tn", 0.5, splits=splits), r["y"], R.b_f32(r["mag"], K, splits))
        worst[f"db s{splits}"] = _ratio(R.emulate_db(c["A"], 0.5, c["db0"], splits), r["db"] + c["db0"].double(),
                                        R.b_db(r["db"], r["db_mag"], K, splits, c["db0"]))
        r = R.gemm_ref(c["A"], c["B"], "tn", 2.0, acc=c["acc"])
        worst[f"acc s{splits}"] = _ratio(R.emulate(c["A"], c["B"], "tn", 2.0, acc=c["acc"], splits=splits), r["y"],
                                         R.b_f32(r["mag"], K, splits))
    print(mnk, {k: round(v, 3) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), worst


def test_emulation_fallback_cases():
    """(f): the implicit-GEMM shapes -- bf16 + bias at K = 40 / 784, fp32 + ReLU, the data grads with alpha_t."""
    worst = {}
    for M, N, K, what in R.FWD_FALLBACK:
        c = R.randn_case(M, N, K, "nt")
        r = R.gemm_ref(c["A"], c["B"], "nt", 1.0, bias=c["bias"])
        if what == "k":
            worst[f"fwd K={K}"] = _ratio(R.emulate(c["A"], c["B"], "nt", 1.0, c["bias"], out="bf16"), r["y"],
                                         R.b_bf16(r["y"], r["mag"], K))
        elif what == "f32relu":
            worst["fwd f32 relu"] = _ratio(R.emulate(c["A"], c["B"], "nt", 1.0, c["bias"], act="relu"), r["y"].clamp(min=0),
                                           R.b_f32(r["mag"], K))
    for M, ni, no, with_res in R.DGRAD_FALLBACK:
        if not with_res:
            c = R.randn_case(M, ni, no, "nn")
            r = R.gemm_ref(c["A"], c["B"], "nn", R.ALPHA_T)
            worst[f"dgrad {no}"] = _ratio(R.emulate(c["A"], c["B"], "nn", R.ALPHA_T, out="bf16"), r["y"],
                                          R.b_bf16(r["y"], r["mag"], no))
    print({k: round(v, 3) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), worst


def test_bf16_residual_rounds_twice():
    """igemm.hip finish_row rounds the result to bf16, adds the bf16 residual in fp32 and rounds again.  On the (f)
    shapes the emulation of exactly that stays inside b_bf16_res and EXCEEDS the one-rounding budget U |y| + f32
    term -- the reason the residual cases carry the two-rounding budget."""
    cases = [("nt", M, N, K, 1.0, True) for M, N, K, what in R.FWD_FALLBACK if what == "res"]
    cases += [("nn", M, ni, no, R.ALPHA_T, False) for M, ni, no, with_res in R.DGRAD_FALLBACK if with_res]
    for lay, M, N, K, alpha, with_bias in cases:
        c = R.randn_case(M, N, K, lay)
        res = c["res"].to(BF)
        bias = c["bias"] if with_bias else None
        r0 = R.gemm_ref(c["A"], c["B"], lay, alpha, bias=bias)
        ref = r0["y"] + res.double()
        got = R.emulate(c["A"], c["B"], lay, alpha, bias, out="bf16", res_bf16=res)
        two = _ratio(got, ref, R.b_bf16_res(r0["y"], r0["mag"], res, K))
        one = _ratio(got, ref, R.b_bf16(ref, r0["mag"] + res.double().abs(), K))
        print(f"{lay} {M}x{N}x{K}: two-rounding budget {two:.3f}   one-rounding budget {one:.3f}")
        assert two <= 1.0 < one
    # Tier A: both roundings are exact
    c = R.int_case(65, 72, 64, "nt", "bf16")
    res = c["res"].to(BF)
    got = R.emulate(c["A"], c["B"], "nt", 1.0, c["bias"], out="bf16", res_bf16=res)
    assert torch.equal(got.double(), R.gemm_ref(c["A"], c["B"], "nt", 1.0, bias=c["bias"])["y"] + res.double())


def test_gelu_fast_formulas_absolute_terms():
    """hgemm.hip's exp-based GELU and GELU' in fp32 torch against fp64 over [-12, 12]: the measured errors, in
    u32 per max(1, |x|) and per w(x), are G_C and GP_C (the hardware's extra ulps are derived in _gemm_ref.py)."""
    x = torch.linspace(-12, 12, 400001, dtype=torch.float64).float()
    e = ((R.gelu_fast32(x).double() - gelu_ref(x)).abs() / x.double().abs().clamp(min=1.0)).max().item() / R.u32
    ep = ((R.gelu_grad_fast32(x).double() - gelu_grad_ref(x)).abs() / R.gp_weight(x)).max().item() / R.u32
    print(f"gelu {e:.2f} u32 per max(1, |x|)   gelu' {ep:.2f} u32 per w(x)")
    assert e <= R.G_C <= 1.05 * e and ep <= R.GP_C <= 1.05 * ep  # the constants ARE the measured figures, rounded up
    # +-8 as a pre-activation makes gelu' exactly 1 / 0 in fp64 and in the fp32 formula (the Tier A mask)
    pm = torch.tensor([8.0, -8.0])
    assert gelu_grad_ref(pm).tolist() == [1.0, 0.0] and R.gelu_grad_fast32(pm).tolist() == [1.0, 0.0]


@pytest.mark.parametrize("mnk", R.F32_CASES, ids=lambda c: "-".join(map(str, c)))
def test_f32_cases(mnk):
    """gemm_f32.hip's cases: Tier A exact in both summation orders; fp32 torch inside K u32 mag on Tier B."""
    M, N, K = mnk
    a = R.f32_case(M, N, K, "A")
    for A, B, lay in ((a["x"], a["w"], "nt"), (a["dy"], a["w"], "nn"), (a["dy"], a["x"], "tn")):
        Am, Bm = R._mats(A, B, lay)
        fwd, rev = _two_orders(Am, Bm)
        assert torch.equal(fwd.double(), Am @ Bm) and torch.equal(rev.double(), Am @ Bm)
        assert (A[-1] != 0).all() and (A[:, -1] != 0).all() and (B[-1] != 0).all() and (B[:, -1] != 0).all()
    b = R.f32_case(M, N, K, "B")
    r = R.gemm_ref(b["x"], b["w"], "nt", bias=b["bias"])
    got = (b["x"] @ b["w"].t()) + b["bias"]
    plain = _ratio(got, r["y"], R.b_f32_plain(r["mag"], K))
    ratio = _ratio(got, r["y"], R.b_f32_plain(r["mag"], K, 1))
    print(mnk, f"K u32 mag: {plain:.3f}   (K + 1) u32 mag (the bias add): {ratio:.3f}")
    assert ratio <= 1.0
    r = R.gemm_ref(b["dy"], b["w"], "nn")
    assert _ratio(b["dy"] @ b["w"], r["y"], R.b_f32_plain(r["mag"], N)) <= 1.0
    r = R.gemm_ref(b["dy"], b["x"], "tn", 0.5, acc=b["dw0"])  # the weight grad: alpha and the add into dw
    assert _ratio(0.5 * (b["dy"].t() @ b["x"]) + b["dw0"], r["y"], R.b_f32_plain(r["mag"], M, 2)) <= 1.0


def test_case_lists_cover_the_candidate_values():
    """Every candidate M, N, K of the issue appears with every layout (hence every tile configuration the layout
    accepts: the GPU test loops over CFGS[layout]); splits 1, 2 and 3 each appear with an uneven last split."""
    for lay, lst in R.RAW.items():
        Ms = {8, 264, 520} if lay == "tn" else {1, 255, 257, 520}
        assert Ms <= {c[0] for c in lst} and {8, 264, 520} <= {c[1] for c in lst}, lay
        assert {64, 128, 192, 832} <= {c[2] for c in lst} and {1, 2, 3} <= {c[3] for c in lst}, lay
        for M, N, K, s in lst:
            if s > 1:
                b = R.split_bounds(K, s)
                assert len(b) == s and (b[0][1] - b[0][0]) // 64 >= 4 and b[-1][1] - b[-1][0] < b[0][1] - b[0][0]
    assert {m for m, _, _ in R.F32_CASES} == set(R.F32_M) and {n for _, n, _ in R.F32_CASES} == set(R.F32_N)
    assert {k for _, _, k in R.F32_CASES} == set(R.F32_K)
