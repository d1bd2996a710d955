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


# ------------------------------------------- fused BN-boundary kernels (test_bn_fused_kernels_gpu.py)
def _rows(t, C):
    return t.reshape(-1, C)


def test_fused_case_lists_cover_the_issue():
    assert set(R.POOL_FWD) == {(1, 2, 2, 64), (2, 8, 8, 64), (1, 6, 10, 64), (3, 7, 9, 64), (2, 9, 6, 64), (1, 5, 5, 16)}
    assert set(R.POOL_FWD_B) == {(2, 8, 8, 64), (3, 7, 9, 64)}
    assert set(R.POOL_BWD) == {s for s in R.POOL_FWD if s[3] == 64} | {(4, 16, 16, 64)} and 4 * 16 * 16 // 512 == 2
    assert set(R.STEM_BWD) == {(1, 2, 2), (2, 8, 8), (1, 6, 10), (5, 4, 20), (4, 16, 16)}
    # (1, 1, 1) is outside the row-walking kernel (H >= 2): pinned as an error, (1, 2, 1) in its place
    assert {(2, 3, 5), (1, 9, 64), (3, 5, 33), (1, 2, 1)} <= set(R.ROW_BN) and R.ROW_BN_OUTSIDE == (1, 1, 1)
    assert any(n * h // 16 >= 64 for n, h, _ in R.ROW_BN) and min(n * h for n, h, _ in R.ROW_BN if n * h // 16 >= 64) == 1024
    assert {m for _, _, m in R.PW_BN} == {32, 96, 2080} and {c for c, _, _ in R.PW_BN} == {64, 128}
    assert all(k >= 2 * c and k % 256 == 0 for c, k, _ in R.PW_BN) and 256 in {k for _, k, _ in R.PW_BN}
    assert all(n * h * w == m for m, (n, h, w) in list(R.PW_BN_M.items()) + list(R.BNIN_M.items()))
    assert set(R.BNIN_M) == {1, 127, 128, 129, 243}
    assert {(c, k) for _, c, k in R.BNIN_FWD} == {(c, k) for c in (32, 64, 256) for k in (8, 64, 136)}
    assert {(k, c) for _, k, c in R.BNIN_BWD} == {(k, c) for k in (32, 64, 256) for c in (8, 64, 136)}


def test_operand_on_load():
    """Tier A: nothing rounds before the bf16 store (plain fp32 arithmetic gives the same bits).  randn: one fp32
    rounding of the exact h * scale + shift, inside bn_apply_ref's budget, and NOT always the single-rounding fp64
    value (the reason the reference exists)."""
    h, coef, pre = R.dyadic_bn((2, 5, 9, 32), 3)
    a = R.operand_on_load(h, coef)
    assert torch.equal(a, (h.float() * coef[0] + coef[1]).clamp(min=0).to(BF)) and torch.equal(a.double(), pre.clamp(min=0).to(BF).double())
    c = R.bnin_fwd_case(243, 64, 8, "B", True)
    for res, rc in ((None, None), (c["res"], None), (c["res"], c["res_coef"])):
        a = R.operand_on_load(c["h"], c["coef"], res, rc)
        r = res if rc is None else R.operand_on_load(res, rc).double() * 0 + R._f32(res.double() * rc.double()[0] + rc.double()[1]).to(BF).double()
        y, b = R.bn_apply_ref(c["h"], c["coef"], r, True)
        assert _ratio(a, y, b) <= 1.0
    v = (c["h"].double() * c["coef"].double()[0] + c["coef"].double()[1])
    assert (v.float() != v).any()


@pytest.mark.parametrize("shape", sorted(set(R.POOL_FWD + R.POOL_BWD + [(*s, 64) for s in R.STEM_BWD])))
def test_pool_bn_case_tier_a(shape):
    """Tier A claims of the fused stem pool cases; the reference forward / gather against torch's max_pool2d and
    its autograd over the reference operand; and the four deliberately wrong references are told apart."""
    N, H, W, C = shape
    c = R.pool_bn_case(shape, "A")
    R.check_pool_bn_case(shape, c)
    y, dx = R.maxpool_ref(c["a"], c["dy"], 3, 2, 1)
    g, gabs = R.pool_gather_ref(c["dy"], c["idx"], H, W, 3, 2, 1)
    assert torch.equal(y, c["y"]) and torch.equal(dx, g) and (gabs >= g.abs()).all()
    assert (c["y"][..., 1] == 0).all() and (c["y"][..., 0] == 0.5).all()
    # first tap inside the image on the constant channels: tap 4 at window (0, 0), 3 on the first row, 1 on the first column
    for ch in (0, 1):
        assert c["idx"][0, 0, 0, ch] == 4
        if c["idx"].shape[1] > 1 and c["idx"].shape[2] > 1:
            assert c["idx"][0, 0, 1, ch] == 3 and c["idx"][0, 1, 0, ch] == 1 and c["idx"][0, 1, 1, ch] == 0
    # wrong: last-tap tie break; relu(shift) in the padding
    _, idx_last, _ = R.bnrelu_maxpool_ref(c["h"], c["coef"], 3, 2, 1, tie="last")
    assert not torch.equal(idx_last, c["idx"])
    y_pad, idx_pad, _ = R.bnrelu_maxpool_ref(c["h"], c["coef"], 3, 2, 1, relu_pad=True)
    assert not torch.equal(idx_pad, c["idx"]) or not torch.equal(y_pad, c["y"])
    if C != 64:
        return
    args = (c["h"], c["gamma"], c["coef"], 3, 2, 1, c["g0"], c["b0"])
    r = R.maxpool_bn_bwd_ref(c["dy"], c["idx"], *args)
    assert r["exact"], "reference not exact"
    # wrong: ReLU with >=; the gather recomputing the max instead of following idx
    ge = R.maxpool_bn_bwd_ref(c["dy"], c["idx"], *args, relu_ge=True)
    assert not torch.equal(ge["dbeta"], r["dbeta"]) and ((ge["dx"] - r["dx"]).abs() > r["b_dx"]).any()
    last = R.last_valid_tap_idx(shape, 3, 2, 1)
    assert (last >= c["idx"]).all() and not torch.equal(last, c["idx"])
    rl = R.maxpool_bn_bwd_ref(c["dy"], last, *args)
    assert ((rl["dx"] - r["dx"]).abs() > r["b_dx"]).any() and not torch.equal(rl["gathered"], r["gathered"])
    # emulation: exact dgamma / dbeta, dh inside its budget
    dh, dg, db = R.pool_bn_bwd_emulate(c, c["idx"], H, W)
    assert torch.equal(dg.double(), r["dgamma"]) and torch.equal(db.double(), r["dbeta"])
    assert _ratio(_rows(dh, C), r["dx"], r["b_dx"]) <= 1.0
    dh, dg, db = R.pool_bn_bwd_emulate(c, last, H, W)
    assert torch.equal(dg.double(), rl["dgamma"]) and _ratio(_rows(dh, C), rl["dx"], rl["b_dx"]) <= 1.0


@pytest.mark.parametrize("shape", R.POOL_FWD_B + [(4, 16, 16, 64)])
def test_pool_bn_bwd_emulation_within_budgets(shape):
    """randn: fp32 gather, sums, finalize and apply stay inside maxpool_bn_bwd_ref's budgets; the stem weight grad
    from the rounded dh inside stem_wgrad_ref's."""
    N, H, W, C = shape
    c = R.pool_bn_case(shape, "B")
    r = R.maxpool_bn_bwd_ref(c["dy"], c["idx"], c["h"], c["gamma"], c["coef"], 3, 2, 1, c["g0"], c["b0"])
    dh, dg, db = R.pool_bn_bwd_emulate(c, c["idx"], H, W)
    rs = {"dh": _ratio(_rows(dh, C), r["dx"], r["b_dx"]), "dgamma": _ratio(dg, r["dgamma"], r["b_dgamma"]),
          "dbeta": _ratio(db, r["dbeta"], r["b_dbeta"])}
    if H % 2 == 0 and W % 2 == 0:
        dw, b_dw = R.stem_wgrad_ref(dh, c["xs"])
        dw0 = torch.randn(64, 4, 4, 16, generator=torch.Generator().manual_seed(1))
        xn = F.pad(c["xs"].float().permute(0, 3, 1, 2), (2, 1, 2, 1))
        e = torch.nn.grad.conv2d_weight(xn, [64, 16, 4, 4], dh.float().permute(0, 3, 1, 2)).permute(0, 2, 3, 1) + dw0
        rs["dw"] = _ratio(e, dw + dw0.double(), b_dw + R.u32 * (dw + dw0.double()).abs())
        # a dropped border tap is far outside
        bad = dh.clone()
        bad[:, 0, 0] = 0
        dwb, _ = R.stem_wgrad_ref(bad, c["xs"])
        assert _ratio(dwb.float(), dw, b_dw) > 1.0
    print(shape, {k: round(v, 3) for k, v in rs.items()})
    assert all(v <= 1.0 for v in rs.values()), rs


CONV_BN_GEOMS = [R.row_bn_geom(*s) for s in R.ROW_BN] + [R.pw_bn_geom(*s) for s in R.PW_BN]


@pytest.mark.parametrize("g", CONV_BN_GEOMS, ids=[g.name for g in CONV_BN_GEOMS])
def test_conv_bn_cases(g):
    """Tier A: the exactness preconditions hold (asserted by the builder), the fp32 emulation reproduces the
    reference bit for bit, and a padding that received the transform is told apart (3x3).  Tier B: the emulation
    stays inside conv_ref's budgets over the reference operand."""
    c = R.conv_bn_case(g, "A")
    R.check_conv_bn_case(g, c)
    y, dw = R.conv_bn_emulate(c, g)
    assert torch.equal(y, c["y"].to(BF)) and torch.equal(dw.double(), c["dw0"].double() + c["dw"] / 2)
    if g.R == 3:
        assert not torch.equal(R.conv_bn_relu_pad_ref(c, g).to(BF), c["y"].to(BF))
    c = R.conv_bn_case(g, "B")
    y, dw = R.conv_bn_emulate(c, g)
    dwref = c["dw0"].double() + c["dw"] / 2
    rs = {"y": _ratio(y, c["y"], c["b_y"]), "dw": _ratio(dw, dwref, c["b_dw"] / 2 + R.u32 * dwref.abs())}
    assert all(v <= 1.0 for v in rs.values()), rs


@pytest.mark.parametrize("m,C,K", R.BNIN_FWD)
def test_bnin_fwd_cases(m, C, K):
    for down in (False, True):
        c = R.bnin_fwd_case(m, C, K, "A", down)
        g = c["g"]
        ref = R.conv_ref(c["x"], c["w"], torch.zeros(*g.xshape[:3], K), g, bounds=False)
        y, _, _ = R.conv_emulate(c["x"], c["w"], torch.zeros(*g.xshape[:3], K), g)
        assert torch.equal(y, ref["y"].to(BF))
        assert not torch.equal(R.pack_bits(c["x"] >= 0), c["bits"])  # wrong: ReLU bits decided with >=
        c = R.bnin_fwd_case(m, C, K, "B", down)
        ref = R.conv_ref(c["x"], c["w"], torch.zeros(*g.xshape[:3], K), g)
        y, _, _ = R.conv_emulate(c["x"], c["w"], torch.zeros(*g.xshape[:3], K), g)
        assert _ratio(y, ref["y"], ref["b_y"]) <= 1.0


@pytest.mark.parametrize("m,K,C", R.BNIN_BWD)
def test_bnin_bwd_cases(m, K, C):
    c = R.bnin_bwd_case(m, K, C, "A")
    g = c["g"]
    b = c["bcoef"]
    assert torch.equal((b[0] * c["dz"].float() + (b[1] * c["h3"].float() + b[2])).to(BF), c["dh"])
    ref = R.conv_ref(torch.zeros(g.xshape), c["w"], c["dh"], g, bounds=False)
    _, dx, _ = R.conv_emulate(torch.zeros(g.xshape).to(BF), c["w"], c["dh"], g)
    assert torch.equal(dx, ref["dx"].to(BF))
    dz, pref = R.dgrad_bn_ref(dx.double(), c["bn_x"], c["bn_coef"])
    cd = c["bn_coef"].double()
    _, wrong = R.dgrad_bn_ref(dx.double(), c["bn_x"], c["bn_coef"], (c["bn_x"].double() * cd[0] + cd[1]) >= 0)
    assert not torch.equal(wrong, pref), "a mask decided with >= would pass"
    p2, bound, exact = R.partials_ref(dz, c["bn_x"], c["bn_coef"])
    assert torch.equal(p2, pref)
    e = torch.stack([dz.float().reshape(-1, C).sum(0), (dz.float() * (c["bn_x"].float() - c["bn_coef"][2])).reshape(-1, C).sum(0)])
    assert _ratio(e, pref, bound) <= 1.0 and (not exact or torch.equal(e.double(), pref))
    c = R.bnin_bwd_case(m, K, C, "B")
    b = c["bcoef"]
    e = (b[0] * c["dz"].float() + (b[1] * c["h3"].float() + b[2])).to(BF)  # (no fma: up to one more fp32 rounding)
    d = c["dh"].double()
    mag = (b[0].double() * c["dz"].double()).abs() + (b[1].double() * c["h3"].double()).abs() + b[2].double().abs()
    # (two bf16 roundings of pre-rounding values 3 u32 mag apart: at most the two half-spacings plus that distance;
    # few elements differ at all -- the GPU test compares the kernel's fma chain bit for bit)
    assert _ratio(e, d, 2 * R.U * d.abs() + (1 + R.U) * 3 * R.u32 * mag + R.FLOOR) <= 1.0
    assert m == 1 or (e != c["dh"]).double().mean().item() < 0.01  # (M = 1: dh is pure cancellation, ~0)
    ref = R.conv_ref(torch.zeros(g.xshape), c["w"], c["dh"], g)
    _, dx, _ = R.conv_emulate(torch.zeros(g.xshape).to(BF), c["w"], c["dh"], g)
    assert _ratio(dx, ref["dx"], ref["b_dx"]) <= 1.0


@pytest.mark.parametrize("M,C", BN_SHAPES)
def test_bn_bwd_coef_emulation_within_budgets(M, C):
    """bn_bwd_finalize's fp32 coefficient arithmetic from partials rounded to fp32 (as the GPU test feeds them):
    a, b, c inside b_k1, b_b, b_c of bn_bwd_ref."""
    c = R.bn_case(M, C, seed=M + C)
    f = R.bn_fwd_ref(c["x"], c["gamma"], c["beta"], c["rmean"], c["rvar"])
    coef = torch.stack([f["scale"], f["shift"], f["mean"], f["invstd"]]).float()
    bw = R.bn_bwd_ref(c["dy"], c["x"], c["gamma"], coef)
    part = R.split_partials(bw["dz"], c["x"], coef)
    k1, b, cc = R.bn_bwd_finalize_emulate(part[0].double().sum(-1), part[1].double().sum(-1), M, c["gamma"], coef)
    rs = {"a": _ratio(k1, bw["k1"], bw["b_k1"]), "b": _ratio(b, bw["b"], bw["b_b"]), "c": _ratio(cc, bw["c"], bw["b_c"])}
    print(M, C, {k: round(v, 3) for k, v in rs.items()})
    assert all(v <= 1.0 for v in rs.values()), rs
