"""CPU checks of tests/_resnet_ref.py: the fp64 references against torch's own gradient formulas, the Tier A
builders' claims for every case the GPU file runs, and -- for every Tier B case -- a torch emulation of the
kernels' roundings (bf16 inputs, fp32 arithmetic, bf16 outputs; no kernel) against the rounding budgets, so a
budget that the arithmetic itself cannot meet is found here, before a kernel is blamed for it."""
import pytest
import torch
import torch.nn.functional as F

import _resnet_ref as R

BF = torch.bfloat16


def _ratio(got, ref, bound):
    err = (got.double() - ref).abs()
    err = torch.where(torch.isfinite(got.double()), err, torch.full_like(err, float("inf")))
    return (err / bound).max().item()


# ------------------------------------------------------------------ conv_ref
REF_GEOMS = [
    R.G("c_plain", 2, 6, 7, 5, 4, 3, pad=(1, 1)),
    R.G("c_dil", 2, 9, 8, 3, 6, (3, 2), pad=(2, 1), dil=(2, 3)),
    R.G("c_stride", 1, 9, 11, 4, 5, 3, stride=(3, 2), pad=(1, 1)),
]


@pytest.mark.parametrize("g", REF_GEOMS, ids=[g.name for g in REF_GEOMS])
def test_conv_ref_matches_torch_grad(g):
    """conv_ref's y, dx, dw (fp64 autograd through F.pad + F.conv2d) == F.conv2d with its own padding and
    torch.nn.grad.conv2d_input / conv2d_weight in fp64."""
    gen = torch.Generator().manual_seed(5)
    oh, ow = g.out_hw
    x = torch.randn(g.N, g.H, g.W, g.C, generator=gen, dtype=torch.float64)
    w = torch.randn(g.K, g.R, g.S, g.C, generator=gen, dtype=torch.float64)
    dy = torch.randn(g.N, oh, ow, g.K, generator=gen, dtype=torch.float64)
    ref = R.conv_ref(x, w, dy, g)
    xn, wn, dn = (t.permute(0, 3, 1, 2).contiguous() for t in (x, w, dy))
    y = F.conv2d(xn, wn, None, g.stride, g.pad, g.dil)
    assert tuple(y.shape[2:]) == (oh, ow)
    dx = torch.nn.grad.conv2d_input(xn.shape, wn, dn, g.stride, g.pad, g.dil)
    dw = torch.nn.grad.conv2d_weight(xn, wn.shape, dn, g.stride, g.pad, g.dil)
    for k, t in (("y", y), ("dx", dx), ("dw", dw)):
        assert torch.allclose(ref[k], t.permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12), k
    for k in ("b_y", "b_dx", "b_dw"):
        assert (ref[k] > 0).all() and torch.isfinite(ref[k]).all()


def test_conv_ref_four_sided_pad():
    """pad [t, l, b, r]: the same as zero-padding x by hand."""
    g = R.G("c_p4", 1, 5, 6, 3, 4, 3, stride=(2, 1), pad=(2, 0, 1, 2))
    gen = torch.Generator().manual_seed(6)
    oh, ow = g.out_hw
    x = torch.randn(1, 5, 6, 3, generator=gen, dtype=torch.float64)
    w = torch.randn(4, 3, 3, 3, generator=gen, dtype=torch.float64)
    dy = torch.randn(1, oh, ow, 4, generator=gen, dtype=torch.float64)
    xp = torch.zeros(1, 5 + 3, 6 + 2, 3, dtype=torch.float64)
    xp[:, 2:7, 0:6] = x
    gp = R.G("c_p4_padded", 1, 8, 8, 3, 4, 3, stride=(2, 1))
    a, b = R.conv_ref(x, w, dy, g, bounds=False), R.conv_ref(xp, w, dy, gp, bounds=False)
    assert torch.equal(a["y"], b["y"]) and torch.equal(a["dw"], b["dw"])
    assert torch.equal(a["dx"], b["dx"][:, 2:7, 0:6])


# -------------------------------------------------------------------- Tier A
@pytest.mark.parametrize("name", R.TIER_A)
def test_int_case_claims(name):
    """Every Tier A case: integral y / dx / dw of magnitude <= 256 (also after the residual / the dx prefill),
    every tap, every input-channel residue mod 32 and every output-channel residue mod 64 under a nonzero
    weight; the inputs are bf16-exact integers."""
    g = R.GEOMS[name]
    c = R.int_case(name)
    R.check_int_case(g, c)
    for k in ("x", "w", "dy", "res", "dx0"):
        assert c[k].dtype == BF and torch.equal(c[k].double().to(BF), c[k])
    ymax = c["y"].abs().max().item()
    assert c["stats_exact"] == (g.M * ymax * ymax < 2 ** 24)
    assert (c["x"] != 0).any() and (c["dy"] != 0).any()


def test_tier_a_list_covers_the_issue():
    """The shapes the case list must contain."""
    gs = [R.GEOMS[n] for n in R.TIER_A]
    gen = R.GENERAL
    assert {(5, 9), (9, 5)} <= {(g.H, g.W) for g in gen}
    for k in (3, 1):
        assert {(1, 2), (2, 1), (2, 2), (3, 3), (3, 2)} <= {g.stride for g in gen if (g.R, g.S) == (k, k)}
    assert any((g.H + 2 * g.pad[0] - g.R) % g.stride[0] for g in gen if g.stride[0] > 1)
    assert {(0, 1), (1, 0), (2, 1)} <= {g.pad for g in gen}
    assert any(len(g.pad) == 4 and g.pad[0] != g.pad[2] and g.pad[1] != g.pad[3] for g in gen)
    assert any((g.R, g.S) == (3, 3) and g.pad == (3, 3) for g in gen) and any((g.R, g.S) == (1, 1) and g.pad == (1, 1) for g in gen)
    assert {(2, 2), (1, 2)} <= {g.dil for g in gen if g.stride == (1, 1)}
    assert {(1, 3), (3, 1), (1, 7), (7, 1), (2, 5), (5, 5)} <= {(g.R, g.S) for g in gen}
    assert any(g.M == 1 and g.N == 1 and g.H == g.R and g.W == g.S for g in gen)
    assert {8, 16, 24, 40} <= {g.C for g in gen} and {8, 40, 72} <= {g.K for g in gen}
    assert all(g.N <= 3 and max(g.H, g.W) <= 12 for g in gen)
    for k in (64, 128, 256):
        assert {1, 7, 63, 65} <= {g.M for g in R.PW if g.C == k and g.K >= 2 * k}
        assert {1, 7, 63, 65} <= {g.M for g in R.PW if g.K == k and g.C >= 2 * k}
    assert {(1, 1, 1), (1, 1, 64), (2, 3, 5), (1, 9, 64)} == {(g.N, g.H, g.W) for g in R.ROW}
    assert {(1, 1, 1), (1, 2, 7), (2, 5, 33)} <= {(g.N, g.H, g.W) for g in R.STEM}
    assert all(h >= 3 and 97 <= w <= 112 for _, h, w in R.STEM_IN)  # the stem forward kernel's envelope
    assert all(n in R.GEOMS for n in R.TIER_B + R.DGRAD_BN + R.STRIDED) and len(gs) == len(set(R.TIER_A))


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("shape", [(2, 5, 9, 32), (1, 1, 1, 64), (2, 3, 5, 24), (90, 1024)])
def test_dyadic_grid(shape, seed):
    """At least 5 % of the elements exactly at the ReLU threshold, none inside (0, 2^-10) of it, everything on
    the 1/8 grid, and the pre-activation exact in fp32 with or without fma."""
    h, coef, pre = R.dyadic_bn(shape, seed)
    at0 = (pre == 0).double().mean().item()
    assert at0 >= 0.05 or h.numel() < 200, at0  # (tiny tensors: the 8 % draw need not reach 5 %)
    assert not ((pre > 0) & (pre < 2.0 ** -10)).any() and not ((pre < 0) & (pre > -(2.0 ** -10))).any()
    assert torch.equal(h.double() * 8, (h.double() * 8).round()) and h.double().abs().max() <= 8
    assert torch.equal(coef.double() * 8, (coef.double() * 8).round()) and coef.abs().max() <= 8
    f32 = h.float() * coef[0] + coef[1]
    assert torch.equal(f32.double(), pre) and torch.equal(torch.addcmul(coef[1].expand(h.shape), h.float(), coef[0].expand(h.shape)).double(), pre)


def test_dyadic_grid_five_percent_over_all_cases():
    """The >= 5 % claim on the shapes conv_dgrad_bn is tested at."""
    for i, name in enumerate(R.DGRAD_BN):
        g = R.GEOMS[name]
        _, _, pre = R.dyadic_bn(g.xshape, i)
        if pre.numel() >= 200:
            assert (pre == 0).double().mean().item() >= 0.05, name


def test_pack_bits():
    m = torch.zeros(2, 16, dtype=torch.bool)
    m[0, 0] = m[0, 9] = m[1, 7] = m[1, 15] = True
    assert R.pack_bits(m).tolist() == [[1, 2], [128, 128]]


# -------------------------------------------------------------------- Tier B
@pytest.mark.parametrize("name", R.TIER_B)
def test_conv_emulation_within_budgets(name):
    """bf16 inputs, fp32 F.conv2d and gradients on the CPU, bf16 outputs: inside every conv budget."""
    g = R.GEOMS[name]
    x, w, dy, res = R.randn_case(g, seed=7)
    ref = R.conv_ref(x, w, dy, g)
    y, dx, dw = R.conv_emulate(x, w, dy, g)
    _, dxr, _ = R.conv_emulate(x, w, dy, g, res)
    rs = {"y": _ratio(y, ref["y"], ref["b_y"]), "dx": _ratio(dx, ref["dx"], ref["b_dx"]),
          "dw": _ratio(dw, ref["dw"], ref["b_dw"]),
          "dx+res": _ratio(dxr, ref["dx"] + res.double(), R.b_dxres(ref, res))}
    print(name, {k: round(v, 3) for k, v in rs.items()})
    assert all(v <= 1.0 for v in rs.values()), rs
    # a one-ulp error of the largest output is far outside (the budgets are not slack by an order of magnitude)
    i = ref["y"].abs().argmax()
    bad = y.clone().view(-1)
    bad[i] = bad[i] * (1 + 2.0 ** -6)
    assert _ratio(bad.view_as(y), ref["y"], ref["b_y"]) > 1.0


BN_SHAPES = [(M, C) for M in R.BN_M for C in R.BN_C]  # every shape the GPU test runs


@pytest.mark.parametrize("M,C", BN_SHAPES)
@pytest.mark.parametrize("relu,use_res", [(False, False), (True, False), (True, True)])
def test_bn_emulation_within_budgets(M, C, relu, use_res):
    """bn.hip's arithmetic in fp32 torch: statistics inside the budgets derived from E[x^2], y / dx / dgamma /
    dbeta inside theirs (from the emulation's own coefficients, as the GPU test does with the kernel's)."""
    c = R.bn_case(M, C, seed=M + C)
    res = c["res"] if use_res else None
    e = R.bn_emulate(c["x"], c["gamma"], c["beta"], c["rmean"], c["rvar"], c["dy"], res, relu)
    b = R.bn_fwd_budgets(c["x"].double(), c["gamma"], c["beta"], c["rmean"], c["rvar"])
    rs = {"mean": _ratio(e["coef"][2], b["mean"], b["b_mean"]), "var": _ratio(e["var"], b["var"], b["b_var"]),
          "invstd": _ratio(e["coef"][3], b["invstd"], b["b_invstd"]), "scale": _ratio(e["coef"][0], b["scale"], b["b_scale"]),
          "shift": _ratio(e["coef"][1], b["shift"], b["b_shift"]), "rmean": _ratio(e["rmean"], b["rmean"], b["b_rmean"]),
          "rvar": _ratio(e["rvar"], b["rvar"], b["b_rvar"])}
    y, b_y = R.bn_apply_ref(c["x"], e["coef"], res, relu)
    rs["y"] = _ratio(e["y"], y, b_y)
    mask = (e["y"].double() > 0) if relu else None
    bw = R.bn_bwd_ref(c["dy"], c["x"], c["gamma"], e["coef"], mask)
    rs["dx"] = _ratio(e["dx"], bw["dx"], bw["b_dx"])
    rs["dgamma"] = _ratio(e["dgamma"], bw["dgamma"], bw["b_dgamma"])
    rs["dbeta"] = _ratio(e["dbeta"], bw["dbeta"], bw["b_dbeta"])
    print(M, C, relu, use_res, {k: round(v, 3) for k, v in rs.items()})
    assert all(v <= 1.0 for v in rs.values()), rs
    if C >= 8:
        # the constant channel: var = 0 exactly, invstd = eps^-1/2
        assert e["var"][0].item() == 0.0 and b["var"][0].item() == 0.0
        assert abs(e["coef"][3, 0].item() - R.BN_EPS ** -0.5) <= 2.0 ** -23 * R.BN_EPS ** -0.5
        if not relu and not use_res:
            assert torch.equal(e["y"][:, 0], torch.full((M,), 0.5, dtype=BF))  # == beta[0]
        if M > 1:
            # the cancellation channels: the budget is far above u32 * var and still a fraction of var at M = 97
            assert b["b_var"][2] > 1000 * R.u32 * b["var"][2] or b["var"][2] == 0


def test_bn_ref_matches_torch_batch_norm():
    """bn_fwd_ref / bn_bwd_ref == F.batch_norm (training) and its autograd in fp64."""
    c = R.bn_case(97, 8, seed=1)
    x = c["x"].double().requires_grad_(True)
    g, b = c["gamma"].double().requires_grad_(True), c["beta"].double().requires_grad_(True)
    rm, rv = c["rmean"].double().clone(), c["rvar"].double().clone()
    y = F.batch_norm(x, rm, rv, g, b, True, R.BN_MOM, R.BN_EPS)
    y.backward(c["dy"].double())
    r = R.bn_fwd_ref(c["x"], c["gamma"], c["beta"], c["rmean"], c["rvar"])
    assert torch.allclose(r["rmean"], rm, rtol=1e-12, atol=1e-12) and torch.allclose(r["rvar"], rv, rtol=1e-12, atol=1e-12)
    coef = torch.stack([r["scale"], r["shift"], r["mean"], r["invstd"]])
    yr, _ = R.bn_apply_ref(c["x"], coef)
    assert torch.allclose(yr, y.detach(), rtol=1e-10, atol=1e-10)
    bw = R.bn_bwd_ref(c["dy"], c["x"], c["gamma"], coef)
    assert torch.allclose(bw["dx"], x.grad, rtol=1e-8, atol=1e-8)
    assert torch.allclose(bw["dgamma"], g.grad, rtol=1e-10, atol=1e-10) and torch.allclose(bw["dbeta"], b.grad, rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------- pooling
@pytest.mark.parametrize("k,s,p", R.POOL_CFG)
@pytest.mark.parametrize("H,W", R.POOL_HW)
def test_pool_case_has_ties_and_negative_borders(k, s, p, H, W):
    """Most windows hold their maximum more than once; every window that reaches padding sees only negative
    data; the reference sends a tied window's gradient to its first tap."""
    x = R.pool_case(2, H, W, 8, k, p, seed=H)
    xn = x.double().permute(0, 3, 1, 2)
    xp = F.pad(xn, (p, p, p, p), value=float("-inf"))
    win = xp.unfold(2, k, s).unfold(3, k, s).reshape(*xn.shape[:2], -1, k * k)  # [N, C, windows, taps]
    mx = win.amax(-1, keepdim=True)
    ties = ((win == mx).sum(-1) > 1).double().mean().item()
    assert ties > 0.5, ties
    touches = torch.isinf(win).any(-1)
    if touches.any():
        assert (mx.squeeze(-1)[touches] < 0).all()
    y, dx = R.maxpool_ref(x, torch.ones(2, *y_hw(H, W, k, s, p), 8), k, s, p)
    assert torch.equal(y, mx.squeeze(-1).reshape(*xn.shape[:2], *y.shape[1:3]).permute(0, 2, 3, 1))
    first = (win == mx).double().argmax(-1)  # first maximal tap in scan order
    cnt = torch.zeros_like(xp)
    OH, OW = y.shape[1:3]
    for t in range(k * k):
        r, q = t // k, t % k
        sel = (first == t).reshape(*xn.shape[:2], OH, OW).double()
        cnt[:, :, r:r + s * OH:s, q:q + s * OW:s] += sel
    cnt = cnt[:, :, p:p + H, p:p + W]
    assert torch.equal(dx, cnt.permute(0, 2, 3, 1))


def y_hw(H, W, k, s, p):
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


@pytest.mark.parametrize("C", R.GAVG_C)
@pytest.mark.parametrize("H,W", R.GAVG_HW)
def test_gavg_emulation_within_budget(H, W, C):
    """fp32 sum over the pixels, division, bf16 rounding -- and dx = bf16(fp32(dy / HW)) -- inside the budgets,
    at every shape the GPU test runs."""
    gen = torch.Generator().manual_seed(H * W + C)
    x = (torch.randn(3, H, W, C, generator=gen) + 0.5).to(BF)
    dy = torch.randn(3, C, generator=gen).to(BF)
    y, b = R.gavg_ref(x)
    assert torch.allclose(y, x.double().mean((1, 2))) and (b > 0).all()
    e = (x.float().sum((1, 2)) / (H * W)).to(BF)
    assert _ratio(e, y, b) <= 1.0
    dxr = dy.double() / (H * W)
    assert _ratio((dy.float() * (1.0 / (H * W))).to(BF), dxr, (R.U + 3 * R.u32) * dxr.abs() + R.FLOOR) <= 1.0
