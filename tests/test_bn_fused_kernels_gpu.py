"""Edge-case tests of the ResNet-50 kernels that never store the tensor between a BatchNorm and its neighbour --
the stem's BN + ReLU + max-pool and its backward (pool.hip, stem.hip), BN + ReLU applied to a conv's operand on
load (in_coef: rowconv.hip, pwconv.hip, the LDS-DMA weight grad of igemm.hip), the BN applies on the A operand of
the LDS-DMA 1x1 conv (igemm.hip AXform), bn_bwd_dual and bn_bwd_coef (bn.hip) -- against the fp64 references of
tests/_resnet_ref.py.  Conventions of test_resnet_kernels_gpu.py: every check is per element, or per channel for
statistics; a non-finite output counts as infinite error; every test prints its worst |err| / bound before it
asserts <= 1; every bound is a count of roundings evaluated on the reference (no constant above 1).

The operand "as the kernel sees it" is R.operand_on_load: h * scale + shift rounded ONCE to fp32 (the fma), one
more fp32 addition with a residual, ReLU, one bf16 rounding.  Where a kernel stores that operand as a by-product
(conv1x1_bnin_fwd's x_out / x_bits, conv1x1_bnin_dgrad's dh_out) it is compared bit for bit, in both tiers, and
the RETURNED tensor is the input of the reference product.

Tier A (exact): h and coef on the dyadic grid with >= 5 % of every channel exactly at the ReLU threshold, sparse
small-integer weights and gradients: the operand is a multiple of 2^-5 below 2^5 (2^-6 below 2^4 for dh), every
partial sum is exact in fp32 in any order, so a bf16 output must be bf16(reference) -- one rounding of an exactly
accumulated value -- and an fp32 output the reference itself.  The builders assert these preconditions on the CPU
("reference not exact").  Tier B (randn): rounding budgets.

Routes.  Families 4 and 5 assert the dispatch predicates (row_bn_on_load, pw_bn_on_load) and pin the error
outside both envelopes; 6 and 7 assert the partial-column count ceil(M / 128) of the on-load kernel; family 4's
(16, 64, 3) asserts the >= 64 blocks of the weight grad's grouped reduce.  The pool kernels (families 1 - 3)
write no partials and have no predicate binding: the forward's kernel is chosen by set_pool_legacy and C == 64
(dpe_bnrelu_maxpool_fwd), both settings run at every shape; the backward's by the parity of H and W
(dpe_maxpool_bn_bwd_reduce), both parities are in the list.
Shapes replaced: (1, 1, 1) lies outside the row-walking kernel (H >= 2) and is pinned as the error conv_fwd
raises, with (1, 2, 1) in its place; Cout = 64 lies outside the streaming pointwise kernel (Cout >= 2 C and a
multiple of its 256-column block) for both channel counts: the nearest inside is 256, already listed, so 512 (two
column blocks) takes the vacant place.  y of conv1x1_bnin_fwd and dx of conv1x1_bnin_dgrad are
allocated by the op and cannot be guarded; x_out, x_bits, dh_out, dw, dgamma and dbeta are.

Measured (MI355X, worst |err| / bound over all cases of the test; 1.0 = at the bound):

    Tier A (dyadic grid, sparse integers)
      1 bnrelu_maxpool_fwd (key-max and per-tap kernels, 6 shapes)   y exact   argmax bytes exact   -0 never stored
      2 maxpool_bn_bwd (7 shapes; forward's bytes and last-tap bytes) dgamma exact   dbeta exact   dh 0.962
      3 stem_bwd_fused (5 shapes)                                    dgamma exact   dbeta exact   dw 0.493
      4 in_coef, row-walking 3x3 (5 shapes)                          y exact   dw exact   stats 0.051
      5 in_coef, streaming pointwise (12 shapes; dw plain / determ.) y exact   dw exact   stats 0.049
      6 conv1x1_bnin_fwd (45 shapes x RES / RES2 x tile)             x_out exact   x_bits exact   y exact   stats 0.020
      7 conv1x1_bnin_dgrad (45 shapes)                               dh_out exact   dx exact   partials exact where
                                                                     2^9 sum |terms| < 2^24 (0.000 elsewhere)
        (dh, dw of 2 / 3: b and c of the BN backward divide by M, and dW is formed from the rounded dh: budgets.
        stats: sums of y^2 leave the exact range of fp32 at these magnitudes; the rows that stay inside it are
        asserted equal, the figure is the worst of the others against (M + 1) u32 sum |terms|.)

    Tier B (randn)
      1 bnrelu_maxpool_fwd                y exact   argmax bytes exact (no rounding after the operand)
      2 maxpool_bn_bwd                    dh 0.993   dgamma 0.417   dbeta 0.356
      3 stem_bwd_fused                    dw 0.989   dgamma 0.417   dbeta 0.356
      4 in_coef, row-walking 3x3          y 0.962   dw 0.963   stats 0.185
      5 in_coef, streaming pointwise      y 0.994   dw 0.549 (plain and deterministic)   stats 0.060
      6 conv1x1_bnin_fwd                  x_out exact   x_bits exact   y 0.995   stats 0.020
      7 conv1x1_bnin_dgrad                dh_out exact   dx 0.993   partials 0.009
      8 bn_bwd_dual (M in {1, 2, 97} x C in {8, 64, 2048})
                                          dx 0.993   dx2 0.993   dgamma 0.581   dbeta 0.866   dgamma2 0.663   dbeta2 0.938
        bn_bwd_coef                       a 0.984   b 0.331   c 0.337   dgamma 0.675   dbeta 0.788
      (bf16 outputs: the bound is one bf16 rounding plus a small fp32 term, and a rounding is reached)
"""
import pytest
import torch

import _resnet_ref as R

pytestmark = pytest.mark.gpu
dev = "cuda"
BF = torch.bfloat16
POOL = (3, 2, 1)
_id = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)
_VIEW = {BF: torch.int16, torch.float32: torch.int32, torch.uint8: torch.uint8}


# ==================================================================== helpers
def _bits(t):
    return t.contiguous().view(_VIEW[t.dtype])


def _exact(what, got, ref64, rounded=False):
    """got (GPU) must hold the fp64 reference bit for bit (the sign of a zero aside; a NaN never compares equal).
    ``rounded``: the reference is an exactly accumulated value and got its ONE rounding to got's dtype; else the
    reference must be representable."""
    want = (ref64 + 0.0).to(got.dtype)
    if not rounded:
        assert torch.equal(want.double(), ref64 + 0.0), f"{what}: the reference is not representable"
    else:
        assert torch.equal(ref64.float().double(), ref64), f"{what}: reference not exact in fp32"
    g = got.detach().cpu() + 0.0
    want = want + 0.0
    assert g.shape == want.shape, f"{what}: shape {tuple(g.shape)} != {tuple(want.shape)}"
    if not torch.equal(_bits(g), _bits(want)):
        bad = (_bits(g) != _bits(want)).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {bad.shape[0]} of {g.numel()} elements differ; first at {i}: got {g[i].item()}, "
                             f"want {want[i].item()}")


def _same_bits(what, got, want):
    """Raw bits equal (bf16 / uint8 / fp32), signs of zeros included."""
    g, w = got.detach().cpu(), want.cpu()
    assert g.shape == w.shape, f"{what}: shape {tuple(g.shape)} != {tuple(w.shape)}"
    if not torch.equal(_bits(g), _bits(w)):
        bad = (_bits(g) != _bits(w)).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {bad.shape[0]} of {g.numel()} elements differ; first at {i}: got {g[i].item()}, "
                             f"want {w[i].item()}")


def _ratio(name, got, ref, bound):
    g = got.detach().double().cpu()
    err = (g - ref).abs()
    err = torch.where(torch.isfinite(g), err, torch.full_like(err, float("inf")))
    r = (err / bound).max().item()
    print(f"  {name}: worst |err|/bound = {r:.3f}")
    return r


def _check(tag, rs):
    for k, r in rs.items():
        assert r <= 1.0, f"{tag}: {k} exceeds its rounding budget, worst ratio {r:.3f}"


def _guarded(shape, dtype, fill=None, extra=4096):
    """A buffer of random bits with ``extra`` guard elements on BOTH sides of a view of ``shape`` (holding ``fill``,
    or left as random bits -- NaN patterns among them -- where the op must overwrite all of it); returns (the
    view, a checker that both guards came back bit-unchanged)."""
    n = 1
    for s in shape:
        n *= s
    g = torch.Generator(device="cpu").manual_seed(12345)
    lo, hi = {BF: (-32768, 32767), torch.float32: (-2 ** 31, 2 ** 31 - 1), torch.uint8: (0, 256)}[dtype]
    raw = torch.randint(lo, hi, (n + 2 * extra,), generator=g, dtype=_VIEW[dtype]).to(dev).view(dtype)
    head, tail = _bits(raw[:extra]).clone(), _bits(raw[extra + n:]).clone()
    view = raw[extra:extra + n].view(shape)
    if fill is not None:
        view.copy_(fill.to(dev).to(dtype))

    def unchanged(what):
        torch.cuda.synchronize()
        assert torch.equal(_bits(raw[:extra]), head), f"{what}: stored before the start of its output"
        assert torch.equal(_bits(raw[extra + n:]), tail), f"{what}: stored past the end of its output"

    return view, unchanged


def _stats(tag, st, y_got, cols=None):
    """BN-forward partials [2][K][cols] against the sums of the STORED y (every conv epilogue sums the rounded
    values): exact where y sits on the 2^-5 grid and 2^5 sum |y| (2^10 sum y^2) stays below 2^24, and inside
    (M + 1) u32 sum |terms| (fp32 accumulation in any order) always."""
    K = y_got.shape[-1]
    assert st is not None and st.dim() == 3 and st.shape[0] == 2 and st.shape[1] == K, f"{tag}: stats shape"
    assert cols is None or st.shape[2] == cols, f"{tag}: {st.shape[2]} partial columns, not the route's {cols}"
    yk = y_got.detach().double().cpu().reshape(-1, K)
    got = st.double().sum(-1).cpu()
    ref = torch.stack([yk.sum(0), (yk * yk).sum(0)])
    if torch.equal(yk * 32, (yk * 32).round()):
        for row, scale in ((0, 32), (1, 1024)):
            if (yk.abs() if row == 0 else yk * yk).sum(0).max().item() * scale < 2 ** 24:
                assert torch.equal(got[row], ref[row]), f"{tag}: BN partial sums (row {row}) differ from the exact sums of y"
    M = yk.shape[0]
    bound = (M + 1) * R.u32 * torch.stack([yk.abs().sum(0), (yk * yk).sum(0)]) + R.FLOOR
    return _ratio(f"{tag} stats", got, ref, bound)


def _partials(tag, part, dz, x, coef, cols):
    """BN-backward partials [2][C][cols] against fp64 sums of dz and dz (x - mean): exact where partials_ref can
    promise it, inside b_s / b_q always."""
    C_ = dz.shape[-1]
    assert part.shape == (2, C_, cols), f"{tag}: partials {tuple(part.shape)}, not the route's [2][{C_}][{cols}]"
    ref, bound, exact = R.partials_ref(dz, x, coef)
    got = part.double().sum(-1).cpu()
    if exact:
        assert torch.equal(got, ref), f"{tag}: BN-backward partials differ from the exact sums"
    return _ratio(f"{tag} partials", got, ref, bound)


def _affine(tag, tier, dgv, dbv, r, rs):
    """dgamma / dbeta (accumulated onto nonzero buffers): exact in Tier A, where the reference asserts it can be."""
    if tier == "A":
        assert r["exact"], f"{tag}: reference not exact"
        _exact(f"{tag} dgamma", dgv, r["dgamma"])
        _exact(f"{tag} dbeta", dbv, r["dbeta"])
    else:
        rs["dgamma"] = max(rs.get("dgamma", 0.0), _ratio(f"{tag} dgamma", dgv, r["dgamma"], r["b_dgamma"]))
        rs["dbeta"] = max(rs.get("dbeta", 0.0), _ratio(f"{tag} dbeta", dbv, r["dbeta"], r["b_dbeta"]))


# =============================================== 1. fused stem pool, forward
def _pool_fwd(C, shape, tier):
    c = R.pool_bn_case(shape, tier)
    h, coef = c["h"].to(dev), c["coef"].to(dev)
    hb = _bits(h).clone()
    try:
        for legacy in (False, True):
            C.set_pool_legacy(legacy)
            y, idx = C.bnrelu_maxpool_fwd(h, coef, *POOL)
            torch.cuda.synchronize()
            tag = f"bnrelu_maxpool_fwd {shape} legacy={legacy}"
            _exact(f"{tag} y", y, c["y"])
            assert torch.equal(idx.cpu(), c["idx"]), f"{tag}: {(idx.cpu() != c['idx']).sum().item()} argmax bytes differ"
            if tier == "A":  # the channel without a positive input: max = relu's 0, stored as +0
                assert not _bits(y[..., 1]).any(), f"{tag}: a -0 (or nonzero) maximum on the all-negative channel"
    finally:
        C.set_pool_legacy(False)
    assert torch.equal(_bits(h), hb), "the input was modified"


@pytest.mark.parametrize("shape", R.POOL_FWD, ids=_id)
def test_pool_fwd_tier_a(C, shape):
    """bnrelu_maxpool_fwd(h, coef, 3, 2, 1) on the key-max kernel and on the per-tap kernel (set_pool_legacy), at
    (N, H, W, C) from one window to odd borders and C = 16 (off the 64-channel kernel): y and the argmax bytes
    bitwise equal to the reference (operand on load, window maximum, FIRST maximal tap in scan order).  Ties are
    everywhere: h takes 9 values off the threshold, >= 5 % of every channel is at it, negative scales, a zero
    scale on which every tap ties at 1/2, and a channel without a positive input (max 0, first tap inside the
    image wins, stored as +0)."""
    _pool_fwd(C, shape, "A")


@pytest.mark.parametrize("shape", R.POOL_FWD_B, ids=_id)
def test_pool_fwd_tier_b(C, shape):
    """randn h, coefficients of a real BatchNorm (one zero and one negative gamma): still bitwise -- with the
    operand reference, max and argmax involve no further rounding."""
    _pool_fwd(C, shape, "B")


# ============================================== 2. fused stem pool, backward
def _pool_bwd(C, shape, tier, rs):
    N, H, W, C_ = shape
    c = R.pool_bn_case(shape, tier)
    h, coef, dy, gamma = c["h"].to(dev), c["coef"].to(dev), c["dy"].to(dev), c["gamma"].to(dev)
    _, idx = C.bnrelu_maxpool_fwd(h, coef, *POOL)
    torch.cuda.synchronize()
    assert torch.equal(idx.cpu(), c["idx"]), "forward argmax bytes (held by the forward tests)"
    last = R.last_valid_tap_idx(shape, *POOL)
    out = {}
    for which, ix in (("idx", idx), ("last tap", last.to(dev))):
        tag = f"maxpool_bn_bwd {shape} {tier} ({which})"
        dgv, dg_ok = _guarded((C_,), torch.float32, c["g0"])
        dbv, db_ok = _guarded((C_,), torch.float32, c["b0"])
        dh = C.maxpool_bn_bwd(dy, ix, h, gamma, coef, dgv, dbv, *POOL)
        dg_ok(f"{tag} dgamma")
        db_ok(f"{tag} dbeta")
        r = R.maxpool_bn_bwd_ref(c["dy"], ix.cpu(), c["h"], c["gamma"], c["coef"], *POOL, c["g0"], c["b0"])
        _affine(tag, tier, dgv, dbv, r, rs)
        rs["dh"] = max(rs.get("dh", 0.0), _ratio(f"{tag} dh", dh.reshape(-1, C_), r["dx"], r["b_dx"]))
        out[which] = dh
    return c, idx, out["idx"]


@pytest.mark.parametrize("tier", ["A", "B"])
@pytest.mark.parametrize("shape", R.POOL_BWD, ids=_id)
def test_pool_bn_bwd(C, shape, tier):
    """maxpool_bn_bwd on even H, W (quad kernels) and odd H or W (general gather), one window to two partial
    blocks ((4, 16, 16): M / 512 = 2): dy gathered through the argmax bytes the GPU forward produced (verified
    equal to the reference's), then BatchNorm backward with the mask h * scale + shift > 0.  dh per element inside
    b_dx; dgamma / dbeta accumulate onto nonzero guarded buffers -- exact in Tier A (integer dy, invstd a power of
    two), inside their budgets in Tier B.  Run a second time with hand-built bytes in which every window names its
    LAST tap inside the image: the gather must follow the byte, not recompute the maximum."""
    print(f"pool bwd {shape} tier {tier}")
    rs = {}
    _pool_bwd(C, shape, tier, rs)
    _check(f"maxpool_bn_bwd {shape}", rs)


# ========================================================== 3. stem_bwd_fused
@pytest.mark.parametrize("tier", ["A", "B"])
@pytest.mark.parametrize("nhw", R.STEM_BWD, ids=_id)
def test_stem_bwd_fused(C, nhw, tier):
    """stem_bwd_fused (C = 64, xs [N, H, W, 16], even H and W): dgamma / dbeta as maxpool_bn_bwd's; dW in two
    stages so that the bound stays tight -- dh is held per element by test_pool_bn_bwd, and dW is compared with the
    fp64 weight grad of the s2d stem conv (pad 2-2-1-1, filter [64, 4, 4, 16]) formed from the bf16 dh that
    maxpool_bn_bwd RETURNED, with a budget of fp32 accumulation only (n u32 sum |terms|, plus the add into dw).
    This rests on the documented contract that the on-the-fly dY has the stored dh's bits (pool.hip's quad apply
    kernel and stem.hip's fused weight grad share one fmaf chain).  xs sparse integers in Tier A: a dropped border
    tap or quad is a whole term.  dw starts at randn: the result is dw0 + dW."""
    shape = (*nhw, 64)
    print(f"stem_bwd_fused {shape} tier {tier}")
    rs = {}
    c, idx, dh = _pool_bwd(C, shape, tier, rs)
    tag = f"stem_bwd_fused {shape} {tier}"
    gen = torch.Generator().manual_seed(9)
    dw0 = torch.randn(64, 4, 4, 16, generator=gen)
    dwv, dw_ok = _guarded((64, 4, 4, 16), torch.float32, dw0)
    dgv, dg_ok = _guarded((64,), torch.float32, c["g0"])
    dbv, db_ok = _guarded((64,), torch.float32, c["b0"])
    C.stem_bwd_fused(c["dy"].to(dev), idx, c["h"].to(dev), c["xs"].to(dev), c["gamma"].to(dev), c["coef"].to(dev),
                     dgv, dbv, dwv)
    for ok, what in ((dw_ok, "dw"), (dg_ok, "dgamma"), (db_ok, "dbeta")):
        ok(f"{tag} {what}")
    r = R.maxpool_bn_bwd_ref(c["dy"], c["idx"], c["h"], c["gamma"], c["coef"], *POOL, c["g0"], c["b0"])
    _affine(tag, tier, dgv, dbv, r, rs)
    dw, b_dw = R.stem_wgrad_ref(dh.cpu(), c["xs"])
    dwref = dw + dw0.double()
    rs["dw"] = _ratio(f"{tag} dw", dwv, dwref, b_dw + R.u32 * dwref.abs())
    _check(tag, rs)


# ================================ 4. BN + ReLU on load, row-walking 3x3 kernel
ZR = ([1, 1], [1, 1], [1, 1])
ZP = ([1, 1], [0, 0], [1, 1])


def _conv_bn(C, g, tier, z, det=(False,), min_blocks=0):
    """conv_fwd / conv_wgrad with in_coef at geometry g: y (with and without statistics, bit-identical), the BN
    partial rows against the sums of the stored y, dw0 + alpha dW with alpha = 1/2 onto a guarded buffer."""
    c = R.conv_bn_case(g, tier)
    h, coef, w, dy = c["h"].to(dev), c["coef"].to(dev), c["w"].to(dev), c["dy"].to(dev)
    hb = _bits(h).clone()
    y0, st0 = C.conv_fwd(h, w, *z, False, None, coef)
    y, st = C.conv_fwd(h, w, *z, True, None, coef)
    torch.cuda.synchronize()
    tag = f"{g.name} {tier}"
    print(f"in_coef {tag}")
    assert st0 is None or st0.numel() == 0
    assert torch.equal(_bits(y0), _bits(y)), f"{tag}: want_stats changed y"
    assert st.shape[2] >= min_blocks, f"{tag}: {st.shape[2]} blocks, fewer than {min_blocks}"
    rs = {}
    if tier == "A":
        _exact(f"{tag} y", y, c["y"], rounded=True)
    else:
        rs["y"] = _ratio("y", y, c["y"], c["b_y"])
    rs["stats"] = _stats(tag, st, y)
    dwref = c["dw0"].double() + c["dw"] / 2
    for d in det:
        dwv, dw_ok = _guarded((g.K, g.R, g.S, g.C), torch.float32, c["dw0"])
        C.conv_wgrad(dy, h, dwv, *z, 0.5, coef, 0, d)
        dw_ok(f"{tag} dw")
        if tier == "A":
            _exact(f"{tag} dw (deterministic={d})", dwv, dwref)
        else:  # (alpha = 1/2 is exact: the accumulation budget halves with it; one more rounding for the add)
            rs[f"dw det={int(d)}"] = _ratio(f"dw (deterministic={d})", dwv, dwref, c["b_dw"] / 2 + R.u32 * dwref.abs())
        if d:
            dw2 = c["dw0"].to(dev).clone()
            C.conv_wgrad(dy, h, dw2, *z, 0.5, coef, 0, True)
            assert torch.equal(_bits(dw2), _bits(dwv)), f"{tag}: the deterministic weight grad is not reproducible"
    assert torch.equal(_bits(h), hb), f"{tag}: the pre-BN input was modified"
    _check(tag, rs)


@pytest.mark.parametrize("tier", ["A", "B"])
@pytest.mark.parametrize("nhw", R.ROW_BN, ids=_id)
def test_row_bn_on_load(C, nhw, tier):
    """conv_fwd(h, w, ..., in_coef) and conv_wgrad(dy, h, dw, ..., alpha, in_coef) on the row-walking 64 -> 64 3x3
    kernels (row_bn_on_load asserted): shifts with relu(shift) != 0 on most channels, so a padding row or pixel
    that received the transform shows in y at the border.  (1, 2, 1): every tap but one column is padding;
    (1, 9, 64) the widest row; (3, 5, 33) an odd width over a half-filled pixel fragment; (16, 64, 3): N H = 1024
    rows, the smallest count at which the launch has 64 blocks (min(resident slots, N H / 16)) and the weight grad
    its grouped partial reduce.  Tier A exact (y = bf16(ref), dw = ref), Tier B inside conv_ref's budgets over the
    reference operand."""
    g = R.row_bn_geom(*nhw)
    assert C.row_bn_on_load(g.xshape, [64, 3, 3, 64], *ZR), f"{g.name}: not on the row-walking kernels"
    _conv_bn(C, g, tier, ZR, min_blocks=64 if nhw == (16, 64, 3) else 1)


# ============================ 5. BN + ReLU on load, streaming pointwise kernel
@pytest.mark.parametrize("tier", ["A", "B"])
@pytest.mark.parametrize("ckm", R.PW_BN, ids=_id)
def test_pw_bn_on_load(C, ckm, tier):
    """The streaming pointwise forward and the LDS-DMA 1x1 weight grad (plain and deterministic, the latter
    reproducible bit for bit) with in_coef, C in {64, 128}, M in {32, 96, 2080} (pw_bn_on_load asserted: it needs
    M % 32 == 0; 2080 rows are 65 K-steps of the weight grad, enough for a K split), Cout in {256, 512} (64 is
    outside the kernel: the module docstring)."""
    g = R.pw_bn_geom(*ckm)
    assert C.pw_bn_on_load(g.xshape, g.K), f"{g.name}: not on the streaming kernel"
    _conv_bn(C, g, tier, ZP, det=(False, True))


def test_in_coef_outside_both_envelopes_raises(C):
    """conv_fwd / conv_wgrad with in_coef raise where no kernel applies the transform (a 3x3 stride-2 conv; the
    64 -> 64 3x3 at H = 1, below the row-walking kernel's envelope; Cout = 64 < 2 C pointwise) instead of convolving
    the raw pre-BN tensor, and leave the input and dw untouched."""
    h, coef, _ = R.dyadic_bn((2, 8, 8, 64), 5)
    w3 = R.int_case("row_2_3_5")["w"].to(dev)
    for shape, w, z in (((2, 8, 8, 64), w3, ([2, 2], [1, 1], [1, 1])), ((1, 1, 1, 64), w3, ZR),
                        ((1, 4, 8, 64), w3[:, :1, :1].contiguous(), ZP)):
        hd, cd = R.dyadic_bn(shape, 5)[0].to(dev), coef.to(dev)
        hb = _bits(hd).clone()
        assert not C.row_bn_on_load(list(shape), list(w.shape), *z)
        assert w.shape[1] != 1 or not C.pw_bn_on_load(list(shape), w.shape[0])
        with pytest.raises(RuntimeError, match="in_coef"):
            C.conv_fwd(hd, w, *z, True, None, cd)
        torch.cuda.synchronize()
        assert torch.equal(_bits(hd), hb), "the input changed in the failed call"
    hd = h.to(dev)
    dw = torch.ones(64, 3, 3, 64, device=dev)
    with pytest.raises(RuntimeError, match="in_coef"):
        C.conv_wgrad(torch.zeros(2, 4, 4, 64, dtype=BF, device=dev), hd, dw, [2, 2], [1, 1], [1, 1], 1.0, coef.to(dev))
    torch.cuda.synchronize()
    assert (dw == 1).all() and torch.equal(hd.cpu(), h)


# ======================================================== 6. conv1x1_bnin_fwd
@pytest.mark.parametrize("m,C_,K", R.BNIN_FWD)
def test_conv1x1_bnin_fwd(C, m, C_, K):
    """x = relu(BN(h) + res) (AX_BN_RES) and x = relu(BN(h) + bf16(BN_d(res))) (AX_BN_RES2) formed on the A
    operand of the LDS-DMA 1x1 conv, tile_m 128 and (K = 64) 256, M in {1, 127, 128, 129, 243}: the by-products
    x_out and x_bits bitwise against operand_on_load / pack_bits in both tiers, inside buffers guarded on both
    sides (the by-product store in a tile's tail is the likeliest out-of-range write); y (Tier A: bf16 of the exact
    product; Tier B: conv_ref's budget) and the BN partials against the fp64 product of the RETURNED x_out.
    Route: ceil(M / 128) partial columns."""
    print(f"conv1x1_bnin_fwd M={m} C={C_} K={K}")
    rs = {}
    for tier in "AB":
        for down in (False, True):
            c = R.bnin_fwd_case(m, C_, K, tier, down)
            g = c["g"]
            for tile in ((128, 256) if K == 64 else (128,)):
                tag = f"{g.name} {tier} down={int(down)} tile={tile}"
                xo, xo_ok = _guarded(g.xshape, BF)
                xb, xb_ok = _guarded((*g.xshape[:3], C_ // 8), torch.uint8)
                rc = c["res_coef"].to(dev) if down else None
                y, st = C.conv1x1_bnin_fwd(c["h"].to(dev), c["res"].to(dev), c["coef"].to(dev), rc, c["w"].to(dev),
                                           xo, xb, True, tile)
                xo_ok(f"{tag} x_out")
                xb_ok(f"{tag} x_bits")
                _same_bits(f"{tag} x_out", xo + 0.0, c["x"])
                _same_bits(f"{tag} x_bits", xb, c["bits"])
                ref = R.conv_ref(xo.cpu(), c["w"], torch.zeros(*g.xshape[:3], K), g, bounds=tier == "B")
                if tier == "A":
                    _exact(f"{tag} y", y, ref["y"], rounded=True)
                else:
                    rs["y"] = max(rs.get("y", 0.0), _ratio(f"{tag} y", y, ref["y"], ref["b_y"]))
                rs["stats"] = max(rs.get("stats", 0.0), _stats(tag, st, y, cols=(m + 127) // 128))
    _check(f"conv1x1_bnin_fwd M={m} C={C_} K={K}", rs)


# ====================================================== 7. conv1x1_bnin_dgrad
@pytest.mark.parametrize("m,K,C_", R.BNIN_BWD)
def test_conv1x1_bnin_dgrad(C, m, K, C_):
    """dh = a dz + b h3 + c formed on the A operand of the 1x1 data grad: the by-product dh_out bitwise against
    bf16(fma(a, dz, fma(b, h3, c))) in both tiers (Tier A: bcoef on the dyadic grid, nothing rounds before the bf16
    store) inside a guarded buffer; dx against the fp64 product of the RETURNED dh_out; the two partial rows against
    dgrad_bn_ref over the stored dx (the epilogue sums the rounded values) with >= 5 % of bn_x at the ReLU
    threshold.  Route: ceil(M / 128) partial columns."""
    print(f"conv1x1_bnin_dgrad M={m} K={K} C={C_}")
    rs = {}
    for tier in "AB":
        c = R.bnin_bwd_case(m, K, C_, tier)
        g = c["g"]
        tag = f"{g.name} {tier}"
        dho, dh_ok = _guarded((*g.xshape[:3], K), BF)
        dx, part = C.conv1x1_bnin_dgrad(c["dz"].to(dev), c["h3"].to(dev), c["bcoef"].to(dev), c["w"].to(dev), dho,
                                        c["bn_x"].to(dev), c["bn_coef"].to(dev))
        dh_ok(f"{tag} dh_out")
        _same_bits(f"{tag} dh_out", dho + 0.0, c["dh"] + 0.0)
        ref = R.conv_ref(torch.zeros(g.xshape), c["w"], dho.cpu(), g, bounds=tier == "B")
        if tier == "A":
            _exact(f"{tag} dx", dx, ref["dx"], rounded=True)
        else:
            rs["dx"] = _ratio(f"{tag} dx", dx, ref["dx"], ref["b_dx"])
        dz2, _ = R.dgrad_bn_ref(dx.double().cpu(), c["bn_x"], c["bn_coef"])
        rs[f"partials {tier}"] = _partials(tag, part, dz2, c["bn_x"], c["bn_coef"], (m + 127) // 128)
    _check(f"conv1x1_bnin_dgrad M={m} K={K} C={C_}", rs)


# ============================================= 8. bn_bwd_dual and bn_bwd_coef
@pytest.mark.parametrize("C_", R.BN_C)
@pytest.mark.parametrize("M", R.BN_M)
def test_bn_bwd_dual_and_coef(C, M, C_):
    """bn_bwd_dual: two BatchNorms fed by one dz (the first from handed-over partials, the second reduced in the
    first's apply pass) against two independent bn_bwd_ref calls, both dgamma / dbeta pairs accumulating onto
    nonzero guarded buffers; bn_bwd_coef: its [3][C] against bn_bwd_ref's k1, b, c inside b_k1, b_b, b_c.  On
    bn_case data (a constant channel, the two cancellation channels, a zero channel).  The partials are the fp64
    sums of two row halves, each rounded once to fp32."""
    c1, c2 = R.bn_case(M, C_, seed=M + C_), R.bn_case(M, C_, seed=M + C_ + 1)
    coefs = []
    for c in (c1, c2):
        f = R.bn_fwd_ref(c["x"], c["gamma"], c["beta"], c["rmean"], c["rvar"])
        coefs.append(torch.stack([f["scale"], f["shift"], f["mean"], f["invstd"]]).float())
    dz = c1["dy"]
    gen = torch.Generator().manual_seed(M * C_)
    pre = [torch.randn(C_, generator=gen) for _ in range(6)]
    bw = [R.bn_bwd_ref(dz, c["x"], c["gamma"], cf, None, pre[2 * i], pre[2 * i + 1])
          for i, (c, cf) in enumerate(zip((c1, c2), coefs))]
    part = R.split_partials(bw[0]["dz"], c1["x"], coefs[0]).to(dev)
    bufs = [_guarded((C_,), torch.float32, p) for p in pre]
    dx, dx2 = C.bn_bwd_dual(dz.to(dev), c1["x"].to(dev), c1["gamma"].to(dev), coefs[0].to(dev), part, bufs[0][0], bufs[1][0],
                            c2["x"].to(dev), c2["gamma"].to(dev), coefs[1].to(dev), bufs[2][0], bufs[3][0])
    bcoef = C.bn_bwd_coef(part, M, c1["gamma"].to(dev), coefs[0].to(dev), bufs[4][0], bufs[5][0])
    for i, (_, ok) in enumerate(bufs):
        ok(f"bn_bwd_dual / bn_bwd_coef gradient buffer {i}")
    print(f"bn_bwd_dual M={M} C={C_}")
    r3 = R.bn_bwd_ref(dz, c1["x"], c1["gamma"], coefs[0], None, pre[4], pre[5])
    rs = {"dx": _ratio("dx", dx, bw[0]["dx"], bw[0]["b_dx"]), "dx2": _ratio("dx2", dx2, bw[1]["dx"], bw[1]["b_dx"]),
          "dgamma": _ratio("dgamma", bufs[0][0], bw[0]["dgamma"], bw[0]["b_dgamma"]),
          "dbeta": _ratio("dbeta", bufs[1][0], bw[0]["dbeta"], bw[0]["b_dbeta"]),
          "dgamma2": _ratio("dgamma2", bufs[2][0], bw[1]["dgamma"], bw[1]["b_dgamma"]),
          "dbeta2": _ratio("dbeta2", bufs[3][0], bw[1]["dbeta"], bw[1]["b_dbeta"]),
          "coef a": _ratio("bn_bwd_coef a", bcoef[0], r3["k1"], r3["b_k1"]),
          "coef b": _ratio("bn_bwd_coef b", bcoef[1], r3["b"], r3["b_b"]),
          "coef c": _ratio("bn_bwd_coef c", bcoef[2], r3["c"], r3["b_c"]),
          "coef dgamma": _ratio("bn_bwd_coef dgamma", bufs[4][0], r3["dgamma"], r3["b_dgamma"]),
          "coef dbeta": _ratio("bn_bwd_coef dbeta", bufs[5][0], r3["dbeta"], r3["b_dbeta"])}
    _check(f"bn_bwd_dual M={M} C={C_}", rs)
