"""Edge-case tests of the ResNet-50 kernels (igemm.hip, the implicit-im2col modes of hgemm.hip, pwconv.hip,
rowconv.hip, stem.hip, bn.hip, pool.hip) against the fp64 references of tests/_resnet_ref.py.  Every reference is
computed from the values the kernel sees (bf16-rounded inputs, widened); every check is per element, or per
channel for statistics -- none uses a tensor norm.

Tier A (exact): small sparse integers whose y, dx, dw are integers of magnitude <= 256, and BN operands on a
dyadic grid with >= 5 % of the elements exactly at the ReLU threshold.  Every fp32 partial sum is exact in any
order, so outputs must equal the reference bit for bit, whatever tile, split or atomics a route uses.
Tier B (randn): a test passes when max |err| / bound <= 1 and prints that ratio; each bound is a count of
roundings evaluated on the reference (derivations in _resnet_ref.py).  Non-finite outputs count as infinite error.

Measured (MI355X, worst |err| / bound over all cases of the test; 1.0 = at the bound):

    Tier A (bitwise; conv_dgrad_acc always runs on the implicit GEMM)      y      stats  dx     dx+res dx acc dw
      implicit GEMM, LDS-DMA and register-staged kernels   exact  exact  exact  exact  exact  exact
        (40 geometries; strided data grads per parity and grouped)
      persistent GEMM, implicit im2col (on / off)          exact  exact  exact  exact  exact  exact
      streaming pointwise kernel (on / off)                exact  exact  exact  exact  exact  exact
      persistent GEMM, pointwise at depth >= 1024          exact  exact  exact  exact  exact  exact
      row-walking 3x3 (on / off; weight grad on / off)     exact  exact  exact  exact  exact  exact
      s2d stem kernel at (1, 3, 97), (2, 4, 112) (on / off) and its fallback at the three small shapes
                                                           exact  exact  exact  exact  exact  exact
      conv_dgrad_bn on the dyadic grid (13 geometries over all routes): dx, masked dz, both partial rows,
        with bn_mask and residual_mask bits: exact;  bn_apply y and mask bits: exact
      maxpool_fwd / maxpool_bwd (3/2/1, 2/2/0, 3/1/1, 3/2/0; tie-heavy data): exact;  bn_bwd dz: exact
      Every family's test asserts the route it is named after (partial-column count or the dispatch condition).
      Not reached at these sizes, and so NOT covered here: the forced LDS-DMA tiles (set_conv_tile 1 / 2 / 3 act
      only on 128-row tiles, M >= 32768) and stream-K (set_hgemm_sk needs more tiles than CUs; the cases have
      one or two, so the switch is only pinned to be inert).

    Tier B convs (randn)              y      dx     dx+res dw     stats  bn y from the conv's partials
      implicit GEMM  g_5x9            0.927  0.959  0.959  0.014  0.012  0.976
                     g_c24            0.960  0.902  0.840  0.018  0.018  0.985
                     g_s22_3          0.957  0.958  0.949  0.029  0.032  0.914
                     g_k72            0.926  0.923  0.901  0.067  0.049  0.952
                     g_d12 (dilated)  0.968  0.932  0.893  0.014  0.010  0.987
      persistent GEMM h_3x3_p01       0.917  0.738  0.734  0.030  0.034  0.995
                     h_dg_p21         0.711  0.926  0.928  0.020  0.014  0.959
                     h_dg_1x7         0.751  0.949  0.938  0.048  0.047  0.968
                     h_full           0.721  0.713  0.733  0.028  0.025  0.992
      streaming      pw_f64_m63       0.985  0.942  0.950  0.019  0.038  0.995
                     pw_d128_m65      0.964  0.986  0.971  0.026  0.027  0.990
      depth >= 1024  hp_f_tail        0.805  0.986  0.975  0.030  0.024  0.970
                     hp_d_tail        0.989  0.841  0.785  0.027  0.034  0.994
      row-walking    row_2_3_5        0.916  0.889  0.916  0.057  0.052  0.973
      stem kernel    stem_1_3_97      0.976  0.859  0.821  0.007  0.003  0.991
      stem fallback  stem_2_5_33      0.966  0.861  0.783  0.003  0.003  0.984  (implicit GEMM, C = 16)
      (bf16 outputs: the bound is one bf16 rounding plus a small fp32 term, and a rounding is reached)
      coefficients from a conv's partials, worst over the cases: mean 0.012  invstd 0.090  scale 0.100
        shift 0.056  running mean 0.326  running var 0.286

    BatchNorm (M in {1, 2, 97} x C in {8, 64, 2048})
      bn_fwd_train      mean 0.010  invstd 0.456  scale 0.557  shift 0.291  running mean 0.554  running var 0.586
                        y 0.996 (plain, ReLU, ReLU + residual)
      cancellation channels (mean 16 / std 1; mean -64 / std 0.5): the budget scales with E[x^2]; measured
        |var err| <= 1.2 * 2^-24 var on both (var recovered from the fp32 invstd, so one rounding of that is in
        it), i.e. <= 0.001 of the budget: the fp32 partials are short (<= 97 rows) and combined in double
      bn_bwd            dx 0.994  dgamma 0.833  dbeta 0.947 (plain / dz / mask from y / mask from bits)
      bn_bwd_partials   dx 0.990  dgamma 0.119  dbeta 0.273 (from conv_dgrad_bn's exact partials)
      bn_fwd_eval       y 0.987
    gavgpool            y 0.990   dx 0.927
"""
import contextlib

import pytest
import torch

import _resnet_ref as R

pytestmark = pytest.mark.gpu
dev = "cuda"
BF = torch.bfloat16


# ==================================================================== helpers
def _bits(t):
    return t.contiguous().view({BF: torch.int16, torch.float32: torch.int32, torch.uint8: torch.uint8}[t.dtype])


def _exact(what, got, ref64):
    """got (bf16 / fp32, GPU) must hold exactly the fp64 reference's values, bit for bit (the sign of a zero
    aside: -0 + 0 = +0 on both sides before the bits are compared; a NaN never compares equal)."""
    want = (ref64 + 0.0).to(got.dtype)
    assert torch.equal(want.double(), ref64 + 0.0), f"{what}: the reference is not representable"
    g = got.detach().cpu() + 0.0
    assert g.shape == want.shape, f"{what}: shape {tuple(g.shape)} != {tuple(want.shape)}"
    if not torch.equal(_bits(g), _bits(want)):
        bad = (_bits(g) != _bits(want)).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {bad.shape[0]} of {g.numel()} elements differ; first at {i}: got {g[i].item()}, "
                             f"want {want[i].item()}")


def _ratio(name, got, ref, bound):
    """Worst |got - ref| / bound over the elements (printed); non-finite outputs count as infinite."""
    g = got.detach().double().cpu()
    err = (g - ref).abs()
    err = torch.where(torch.isfinite(g), err, torch.full_like(err, float("inf")))
    r = (err / bound).max().item()
    print(f"  {name}: worst |err|/bound = {r:.3f}")
    return r


def _check(tag, rs):
    for k, r in rs.items():
        assert r <= 1.0, f"{tag}: {k} exceeds its rounding budget, worst ratio {r:.3f}"


def _canary(n_real, dtype, fill, extra=4096):
    """A flat buffer of n_real + extra elements of random bits whose first n_real elements hold ``fill``
    (flattened); returns (the leading view, a checker that the tail came back bit-unchanged)."""
    g = torch.Generator(device="cpu").manual_seed(12345)
    if dtype == BF:
        raw = torch.randint(-32768, 32767, (n_real + extra,), generator=g, dtype=torch.int16).to(dev).view(BF)
    else:
        raw = torch.randint(-2 ** 31, 2 ** 31 - 1, (n_real + extra,), generator=g, dtype=torch.int32).to(dev).view(torch.float32)
    tail = _bits(raw[n_real:]).clone()
    raw[:n_real] = fill.reshape(-1).to(dev).to(dtype)

    def unchanged(what):
        torch.cuda.synchronize()
        assert torch.equal(_bits(raw[n_real:]), tail), f"{what}: stored past the end of its output"

    return raw[:n_real], unchanged


_DEFAULTS = {"set_pw_stream": True, "set_hgemm_conv": True, "set_rowconv": True, "set_row_wgrad": True,
             "set_stem_kernel": True, "set_phase_group": False, "set_hgemm_sk": False}


@contextlib.contextmanager
def _toggles(C, **kw):
    """C.set_<name>(value) for the block; every toggle back at its default in ``finally``."""
    try:
        for k, v in kw.items():
            getattr(C, "set_" + k)(v)
        yield
    finally:
        for k in kw:
            getattr(C, "set_" + k)(_DEFAULTS["set_" + k])


def _stats_check(tag, st, y_ref, exact, y_got):
    """BN-forward partials [2][K][nb]: every conv epilogue sums the STORED (rounded) values (igemm.hip finish_row,
    hgemm.hip HACT_BNF, pwconv.hip PW_FWD, rowconv.hip, stem.hip all unpack the packed bf16 tile), so the
    reference is the sums of the kernel's own y.  Exact where M max|y|^2 < 2^24; else M fp32 additions."""
    K = y_ref.shape[-1]
    assert st is not None and st.dim() == 3 and st.shape[0] == 2 and st.shape[1] == K, f"{tag}: stats shape"
    assert torch.isfinite(st).all(), f"{tag}: non-finite partials"
    got = st.double().sum(-1).cpu()
    yk = y_got.detach().double().cpu().reshape(-1, K)
    ref = torch.stack([yk.sum(0), (yk * yk).sum(0)])
    if exact:
        assert torch.equal(got, ref), f"{tag}: BN partial sums differ from the exact sums of y"
        return 0.0
    M = yk.shape[0]
    bound = (M + 1) * R.u32 * torch.stack([yk.abs().sum(0), (yk * yk).sum(0)]) + R.FLOOR
    return _ratio(f"{tag} stats", got, ref, bound)


# ============================================================ Tier A: convs
def _tier_a(C, name, tag, parts=("fwd", "dgrad", "acc", "wgrad")):
    """All Tier A checks of one case under the toggles in force.  Returns the raw outputs (for bitwise
    comparisons between toggle settings)."""
    g, c = R.GEOMS[name], R.int_case(name)
    x, dy = c["x"].to(dev), c["dy"].to(dev)
    w = c["w"].to(dev)  # a fresh tensor per call: the flipped-filter cache is keyed by tensor identity
    out = {}
    if "fwd" in parts:
        y0, st0 = C.conv_fwd(x, w, *g.args, False, None)
        y1, st1 = C.conv_fwd(x, w, *g.args, True, None)
        torch.cuda.synchronize()
        assert st0 is None or st0.numel() == 0
        _exact(f"{tag} conv_fwd", y0, c["y"])
        _exact(f"{tag} conv_fwd (want_stats)", y1, c["y"])
        _check(tag, {"stats": _stats_check(tag, st1, c["y"], c["stats_exact"], y1)})
        out["y"], out["nb"] = y0, st1.shape[2]
    if "dgrad" in parts:
        res = c["res"].to(dev)
        dx = C.conv_dgrad(dy, w, g.xshape, *g.args, None)
        dxr = C.conv_dgrad(dy, w, g.xshape, *g.args, res)
        torch.cuda.synchronize()
        _exact(f"{tag} conv_dgrad", dx, c["dx"])
        _exact(f"{tag} conv_dgrad + residual", dxr, c["dx"] + c["res"].double())
        out["dx"], out["dxr"] = dx, dxr
    if "acc" in parts:
        n = c["dx0"].numel()
        view, unchanged = _canary(n, BF, c["dx0"])
        dxa = view.view(g.xshape)
        C.conv_dgrad_acc(dy, w, dxa, *g.args)
        unchanged(f"{tag} conv_dgrad_acc")
        # (parities no tap reaches and rows under no window: dx = 0 there, so dx0 must come back as it was)
        _exact(f"{tag} conv_dgrad_acc", dxa, c["dx"] + c["dx0"].double())
        out["dxa"] = dxa
    if "wgrad" in parts:
        view, unchanged = _canary(c["dw0"].numel(), torch.float32, c["dw0"])
        dw = view.view(g.K, g.R, g.S, g.C)
        C.conv_wgrad(dy, x, dw, *g.args, 1.0)
        unchanged(f"{tag} conv_wgrad")
        _exact(f"{tag} conv_wgrad", dw, c["dw"] + c["dw0"].double())
        out["dw"] = dw
    return out


def _same(tag, a, b):
    for k in (set(a) & set(b)) - {"nb"}:
        assert torch.equal(_bits(a[k]), _bits(b[k])), f"{tag}: {k} differs between the two settings"


# ---- which kernel ran.  Every route falls back silently, so each family's test pins its dispatch.  The last
# dimension of the partials tells the routes apart: the implicit GEMM writes one column per M tile of pick_cfg's
# tile (ceil(M / bm), 1 at M <= 64), the persistent GEMM one per wave row of its >= 128-row tile (>= 2), the
# stem kernel 3 N.  Where the counts can coincide the dispatch condition itself is queried instead (rowconv:
# row_bn_on_load is rowconv_geom; streaming kernel: only it accepts in_coef / sum_mask, conv.cpp raises otherwise).
def _igemm_cols(C, M, N, K):
    bm = C.pick_gemm_cfg(M, N, K, False)[0]
    return (M + bm - 1) // bm


def _dgrad_bn_cols(C, name, seed=0):
    """Partial columns of conv_dgrad_bn at the case's shape (dyadic operands; values checked elsewhere)."""
    g, c = R.GEOMS[name], R.int_case(name)
    h, coef, _ = R.dyadic_bn(g.xshape, seed)
    _, part = C.conv_dgrad_bn(c["dy"].to(dev), c["w"].to(dev), g.xshape, *g.args, None, h.to(dev), coef.to(dev))
    torch.cuda.synchronize()
    return part.shape[2]


@pytest.mark.parametrize("name", [g.name for g in R.GENERAL])
def test_tier_a_general(C, name):
    """The general implicit GEMM at every geometry of the list (routes: the comment at R.GENERAL).
    (set_conv_tile is not exercised: dma_tile acts only where pick_cfg chose a 128-row tile, which takes >= 512
    tiles, M of 32768 and more -- far above the sizes an exact per-element test needs.)"""
    g = R.GEOMS[name]
    out = _tier_a(C, name, name)
    assert out["nb"] == _igemm_cols(C, g.M, g.K, g.R * g.S * g.C), f"{name}: not the implicit GEMM's partial layout"


@pytest.mark.parametrize("name", R.STRIDED)
def test_tier_a_strided_phase_group(C, name):
    """Strided data grads: one launch per output parity vs all parities in one grid -- both equal to the
    reference and to each other, bit for bit.  Stride 3 has parities no tap reaches (the K = 0 sub-GEMM that
    stores zeros + residual, skipped by conv_dgrad_acc)."""
    outs = {}
    for grp in (False, True):
        with _toggles(C, phase_group=grp):
            outs[grp] = _tier_a(C, name, f"{name} group={grp}", ("dgrad", "acc"))
    _same(name, outs[False], outs[True])


@pytest.mark.parametrize("name", [g.name for g in R.HGEMM])
def test_tier_a_hgemm_conv(C, name):
    """Persistent GEMM with an implicit-im2col operand (conv_smagic division by S for non-square filters, tap
    masks, M tails) on and off.  set_hgemm_sk(True) is run as well, but stream-K needs more tiles than CUs and
    these cases have one or two: the plan never takes it here, so that run only pins that the switch is inert.
    conv_dgrad_acc always runs on the implicit GEMM (acc_into disables the other branches): here with C = 64 to
    256, several N tiles of the read-then-overwrite epilogue."""
    g = R.GEOMS[name]
    outs = {}
    for on in (True, False):
        with _toggles(C, hgemm_conv=on):
            outs[on] = _tier_a(C, name, f"{name} hgemm_conv={on}")
            outs[on]["pb"] = _dgrad_bn_cols(C, name)
    with _toggles(C, hgemm_sk=True):
        outs["sk"] = _tier_a(C, name, f"{name} hgemm_sk", ("fwd", "dgrad", "wgrad"))
    for k in ("y", "dx", "dxr"):
        assert torch.equal(_bits(outs[True][k]), _bits(outs[False][k])) and torch.equal(_bits(outs[True][k]), _bits(outs["sk"][k]))
    # routes (hconv_ok): forward with C a power of two >= 64 and Cout >= 256; data grad with Cout a power of two
    # >= 64 and C >= 256.  Every such case has <= 64 rows: one implicit-GEMM column, >= 2 persistent-GEMM ones.
    pow2 = lambda v: v >= 64 and v & (v - 1) == 0
    ig_f = _igemm_cols(C, g.M, g.K, g.R * g.S * g.C)
    ig_d = _igemm_cols(C, g.N * g.H * g.W, g.C, g.R * g.S * g.K)
    if g.stride != (1, 1):  # (strided data grads: one sub-GEMM per parity on the implicit GEMM, columns per parity)
        ig_d = outs[False]["pb"]
    assert outs[False]["nb"] == ig_f and outs[False]["pb"] == ig_d, f"{name}: set_hgemm_conv(False) is not the implicit GEMM"
    if pow2(g.C) and g.K >= 256:
        assert g.M <= 64 and outs[True]["nb"] >= 2 and outs[True]["nb"] != ig_f, f"{name}: forward not on the persistent GEMM"
    else:
        assert outs[True]["nb"] == ig_f
    if pow2(g.K) and g.C >= 256:
        assert g.N * g.H * g.W <= 64 and outs[True]["pb"] >= 2 and outs[True]["pb"] != ig_d, f"{name}: data grad not on the persistent GEMM"
    else:
        assert outs[True]["pb"] == ig_d


@pytest.mark.parametrize("name", [g.name for g in R.PW])
def test_tier_a_pw_stream(C, name):
    """Streaming pointwise kernel on / off at M in {1, 7, 63, 65}, K in {64, 128, 256}; conv_dgrad_acc (always
    the implicit GEMM, here with up to 512 columns in 128-wide N tiles).  Route: only the streaming kernel takes
    in_coef (forward) or sum_mask (data grad); with it off conv.cpp raises."""
    g, c = R.GEOMS[name], R.int_case(name)
    fwd = g.K >= 2 * g.C
    outs = {}
    for on in (True, False):
        with _toggles(C, pw_stream=on):
            outs[on] = _tier_a(C, name, f"{name} pw_stream={on}")
            x, dy, w = c["x"].to(dev), c["dy"].to(dev), c["w"].to(dev)
            if fwd:
                _, coef, _ = R.dyadic_bn(g.xshape, 1)
                call = lambda: C.conv_fwd(x, w, *g.args, False, None, coef.to(dev))
            else:
                bits = torch.zeros(g.N, g.H, g.W, g.C // 8, dtype=torch.uint8, device=dev)
                call = lambda: C.conv_dgrad_bn(dy, w, g.xshape, *g.args, None, None, None, None, None, False, bits)
            if on:
                call()  # inside the streaming kernel's envelope
                torch.cuda.synchronize()
            else:
                with pytest.raises(RuntimeError, match="streaming"):
                    call()
    _same(name, {k: outs[True][k] for k in ("y", "dx", "dxr", "dxa")}, outs[False])


@pytest.mark.parametrize("name", [g.name for g in R.HG_PW])
def test_tier_a_hgemm_pointwise(C, name):
    """1x1 convs at depth >= 1024: the forward with statistics (HACT_BNF) and conv_dgrad_bn (HACT_BNB) on the
    persistent GEMM, at M = 1 and at an M tail (54 rows); conv_dgrad_acc on the implicit GEMM with up to 1024
    columns.  Route: <= 64 rows are one implicit-GEMM partial column and >= 2 persistent-GEMM ones."""
    g = R.GEOMS[name]
    out = _tier_a(C, name, name)
    assert g.M <= 64
    if g.C >= 1024:
        assert out["nb"] >= 2 and out["nb"] != _igemm_cols(C, g.M, g.K, g.C), f"{name}: forward not on the persistent GEMM"
    else:
        pb = _dgrad_bn_cols(C, name)
        assert pb >= 2 and pb != _igemm_cols(C, g.M, g.C, g.K), f"{name}: conv_dgrad_bn not on the persistent GEMM"


@pytest.mark.parametrize("name", [g.name for g in R.ROW])
def test_tier_a_rowconv(C, name):
    """Row-walking 64 -> 64 3x3 kernels (forward, data grad as a forward over dy, weight grad) on and off.  At
    H = 1 the kernel's envelope (H >= 2) sends the case to the implicit GEMM: the result must not change.
    Route: row_bn_on_load is rowconv_geom, the dispatch condition itself.  conv_dgrad_acc: implicit GEMM."""
    g = R.GEOMS[name]
    outs = {}
    for on in (True, False):
        with _toggles(C, rowconv=on, row_wgrad=on):
            outs[on] = _tier_a(C, name, f"{name} rowconv={on}")
            taken = C.row_bn_on_load(g.xshape, [g.K, g.R, g.S, g.C], list(g.stride), list(g.pad), list(g.dil))
            assert taken == (on and g.H >= 2), f"{name}: row-walking dispatch"
    with _toggles(C, row_wgrad=False):
        _tier_a(C, name, f"{name} row_wgrad=False", ("wgrad",))
    _same(name, {k: outs[True][k] for k in ("y", "dx", "dxr", "dxa")}, outs[False])


@pytest.mark.parametrize("name", [g.name for g in R.STEM])
def test_tier_a_stem(C, name):
    """s2d stem (16 -> 64, 4x4, pad [2, 2, 1, 1]) on its kernel and on the implicit GEMM; the weight grad also
    with the two-element pad [2, 2] the stem's autograd function passes.  The forward kernel's envelope is
    H >= 3, 97 <= W <= 112 (R.STEM_IN; 3 N partial columns); the three small shapes pin the fallback to the
    implicit GEMM (ceil(M / bm) columns) under either setting."""
    g, c = R.GEOMS[name], R.int_case(name)
    inside = (g.N, g.H, g.W) in R.STEM_IN
    for on in (True, False):
        with _toggles(C, stem_kernel=on):
            out = _tier_a(C, name, f"{name} stem_kernel={on}", ("fwd", "dgrad", "acc", "wgrad"))
            ig = _igemm_cols(C, g.M, g.K, g.R * g.S * g.C)
            assert ig != 3 * g.N or not inside
            assert out["nb"] == (3 * g.N if on and inside else ig), f"{name}: stem forward dispatch"
            dw = torch.zeros(g.K, g.R, g.S, g.C, device=dev)
            C.conv_wgrad(c["dy"].to(dev), c["x"].to(dev), dw, [1, 1], [2, 2], [1, 1], 1.0)
            _exact(f"{name} conv_wgrad pad [2, 2]", dw, c["dw"])


# ----------------------------------------------- conv_dgrad_bn, dyadic grid
def _partials_exact(tag, part, ref, dz, h, coef):
    got = part.double().sum(-1).cpu()
    # exactness precondition: every term is a multiple of 1/8 and the sums of magnitudes stay below 2^24 / 8
    C_ = dz.shape[-1]
    mag = (dz * (h.double() - coef.double()[2])).abs().reshape(-1, C_).sum(0).max().item()
    assert mag * 8 < 2 ** 24, f"{tag}: the case cannot promise exact partials"
    assert torch.equal(got, ref), f"{tag}: BN-backward partials differ from the exact sums (worst {(got - ref).abs().max().item()})"


@pytest.mark.parametrize("name", R.DGRAD_BN)
def test_tier_a_dgrad_bn(C, name):
    """conv_dgrad_bn on the dyadic grid: dx, the masked dz (mask-bits variants store it), and both partial
    rows exact; >= 5 % of the pre-activations sit exactly at 0, where only a strict > 0 is right.  Variants:
    mask recomputed from the pre-BN input; bn_mask bits; bn_mask + a residual masked by residual_mask bits.
    The bits come from bn_apply on the same grid and are themselves checked against the packed reference.
    Then bn_bwd_partials consumes the partials (budgets of bn_bwd_ref)."""
    g, c = R.GEOMS[name], R.int_case(name)
    seed = R.DGRAD_BN.index(name)
    h, coef, pre = R.dyadic_bn(g.xshape, seed)
    gen = torch.Generator().manual_seed(77 + seed)
    dy, w = c["dy"].to(dev), c["w"].to(dev)
    hd, cd = h.to(dev), coef.to(dev)
    # --- mask from the pre-BN input
    dx, part = C.conv_dgrad_bn(dy, w, g.xshape, *g.args, None, hd, cd)
    torch.cuda.synchronize()
    _exact(f"{name} dgrad_bn dx", dx, c["dx"])
    dz, pref = R.dgrad_bn_ref(c["dx"], h, coef)
    _partials_exact(f"{name} dgrad_bn", part, pref, dz, h, coef)
    # --- bits of relu(BN(h) + r) from bn_apply; r on the grid, 0 where the pre-activation is 0
    def grid_bits(k):
        r = torch.randint(-64, 65, g.xshape, generator=gen).double() / 8
        r = torch.where(pre == 0, torch.zeros_like(r), r)
        yb, bits = C.bn_apply(hd, cd, r.to(BF).to(dev), None, True, True)
        torch.cuda.synchronize()
        _exact(f"{name} bn_apply y ({k})", yb, (pre + r).clamp(min=0).to(BF).double())
        m = (pre + r) > 0
        assert torch.equal(bits.cpu(), R.pack_bits(m)), f"{name}: bn_apply mask bits ({k})"
        assert ((pre + r) == 0).double().mean().item() >= 0.05 or pre.numel() < 200
        return bits, m
    bits, m = grid_bits("bn_mask")
    rbits, rm = grid_bits("residual_mask")
    dxm, partm = C.conv_dgrad_bn(dy, w, g.xshape, *g.args, None, hd, cd, bits)
    torch.cuda.synchronize()
    dzm, prefm = R.dgrad_bn_ref(c["dx"], h, coef, m)
    _exact(f"{name} dgrad_bn (bn_mask) dz", dxm, dzm)
    _partials_exact(f"{name} dgrad_bn (bn_mask)", partm, prefm, dzm, h, coef)
    res = c["res"]
    full = c["dx"] + res.double() * rm
    dxr = C.conv_dgrad(dy, w, g.xshape, *g.args, res.to(dev), rbits)
    dxmr, partmr = C.conv_dgrad_bn(dy, w, g.xshape, *g.args, res.to(dev), hd, cd, bits, rbits)
    torch.cuda.synchronize()
    _exact(f"{name} conv_dgrad (residual_mask)", dxr, full)
    dzmr, prefmr = R.dgrad_bn_ref(full, h, coef, m)
    _exact(f"{name} dgrad_bn (bn_mask, residual_mask) dz", dxmr, dzmr)
    _partials_exact(f"{name} dgrad_bn (bn_mask, residual_mask)", partmr, prefmr, dzmr, h, coef)
    # --- bn_bwd_partials on the first variant's outputs
    Cc = g.C
    gamma = 1 + 0.25 * torch.randn(Cc, generator=gen)
    g0, b0 = torch.randn(Cc, generator=gen), torch.randn(Cc, generator=gen)
    dgv, dg_ok = _canary(Cc, torch.float32, g0)
    dbv, db_ok = _canary(Cc, torch.float32, b0)
    dh = C.bn_bwd_partials(dx, hd, gamma.to(dev), cd, part, dgv, dbv, True)
    dg_ok(f"{name} bn_bwd_partials dgamma")
    db_ok(f"{name} bn_bwd_partials dbeta")
    bw = R.bn_bwd_ref(c["dx"].reshape(-1, Cc), h.reshape(-1, Cc), gamma, coef, (pre > 0).reshape(-1, Cc), g0, b0)
    print(f"dgrad_bn {name}")
    _check(name, {"dh": _ratio("bn_bwd_partials dx", dh.reshape(-1, Cc), bw["dx"], bw["b_dx"]),
                  "dgamma": _ratio("bn_bwd_partials dgamma", dgv, bw["dgamma"], bw["b_dgamma"]),
                  "dbeta": _ratio("bn_bwd_partials dbeta", dbv, bw["dbeta"], bw["b_dbeta"])})


# ------------------------------------------------------------ pinned errors
def test_conv_dgrad_strided_dilated_raises(C):
    w = torch.zeros(32, 3, 3, 32, dtype=BF, device=dev)
    dy = torch.zeros(1, 5, 5, 32, dtype=BF, device=dev)  # (9 + 2 * 2 - 2 * 2 - 1) // 2 + 1 = 5: a consistent shape
    with pytest.raises(RuntimeError, match="dilation"):
        C.conv_dgrad(dy, w, [1, 9, 9, 32], [2, 2], [2, 2], [2, 2], None)
    with pytest.raises(RuntimeError, match="dilation"):
        C.conv_dgrad_acc(dy, w, torch.zeros(1, 9, 9, 32, dtype=BF, device=dev), [2, 2], [2, 2], [2, 2])


@pytest.mark.parametrize("name", ["g_5x9", "g_s22_3", "g_d12", "g_p4", "g_1x1p1", "pw_d64_m63", "row_2_3_5", "stem_2_5_33"])
def test_conv_grads_reject_wrong_dy_shape(C, name):
    """conv_dgrad / conv_dgrad_acc / conv_dgrad_bn / conv_wgrad raise when dy's OH or OW is not the forward
    conv's output size for xshape, stride, pad and dilation (too small and too large, each axis), and accept
    the right one.  (A two-element pad names the top / left pad only: there the size with a bottom / right pad
    one smaller is accepted too -- the stem's [2, 2] for [2, 2, 1, 1] -- and nothing else.)"""
    g, c = R.GEOMS[name], R.int_case(name)
    oh, ow = g.out_hw
    w, x = c["w"].to(dev), c["x"].to(dev)
    dw = torch.zeros(g.K, g.R, g.S, g.C, device=dev)
    four = len(g.pad) == 4
    h, coef, _ = R.dyadic_bn(g.xshape, 3)
    hd, cd = h.to(dev), coef.to(dev)
    for doh, dow in ((1, 0), (0, 1), (-2, 0), (0, -2), (-1, 0), (0, -1)):
        if oh + doh < 1 or ow + dow < 1:
            continue
        dy = torch.zeros(g.N, oh + doh, ow + dow, g.K, dtype=BF, device=dev)
        if not four:
            # the two-element form's lower end: the size with a bottom / right pad of ph - 1 / pw - 1
            lo_h = (g.H + g.pad[0] + max(g.pad[0] - 1, 0) - g.dil[0] * (g.R - 1) - 1) // g.stride[0] + 1
            lo_w = (g.W + g.pad[1] + max(g.pad[1] - 1, 0) - g.dil[1] * (g.S - 1) - 1) // g.stride[1] + 1
            if oh + doh >= max(1, lo_h) and oh + doh <= oh and ow + dow >= max(1, lo_w) and ow + dow <= ow:
                continue
        with pytest.raises(RuntimeError, match="conv_dgrad: dy is"):
            C.conv_dgrad(dy, w, g.xshape, *g.args, None)
        with pytest.raises(RuntimeError, match="conv_dgrad: dy is"):
            C.conv_dgrad_acc(dy, w, torch.zeros(g.xshape, dtype=BF, device=dev), *g.args)
        with pytest.raises(RuntimeError, match="conv_dgrad: dy is"):
            C.conv_dgrad_bn(dy, w, g.xshape, *g.args, None, hd, cd)
        with pytest.raises(RuntimeError, match="conv_wgrad: dy is"):
            C.conv_wgrad(dy, x, dw, *g.args, 1.0)
    assert not dw.any()
    dy = c["dy"].to(dev)
    C.conv_dgrad(dy, w, g.xshape, *g.args, None)
    C.conv_dgrad_bn(dy, w, g.xshape, *g.args, None, hd, cd)
    C.conv_wgrad(dy, x, dw, *g.args, 1.0)
    torch.cuda.synchronize()


# ============================================================ Tier B: convs
@pytest.mark.parametrize("name", R.TIER_B)
def test_tier_b_conv(C, name):
    """randn data, per-element rounding budgets (conv_ref): y (with and without statistics, bit-identical),
    dx, dx + residual, dw accumulated into a canary-tailed prefilled buffer, the BN-forward partials against
    the sums of the stored y; then bn_fwd_train consuming those partials (budgets of bn_fwd_budgets on the
    stored y)."""
    g = R.GEOMS[name]
    x, w, dy, res = R.randn_case(g, seed=11)
    ref = R.conv_ref(x, w, dy, g)
    xd, wd, dyd, resd = x.to(dev), w.to(dev), dy.to(dev), res.to(dev)
    print(f"tier B {name}")
    y0, _ = C.conv_fwd(xd, wd, *g.args, False, None)
    y, st = C.conv_fwd(xd, wd, *g.args, True, None)
    dx = C.conv_dgrad(dyd, wd, g.xshape, *g.args, None)
    dxr = C.conv_dgrad(dyd, wd, g.xshape, *g.args, resd)
    gen = torch.Generator().manual_seed(5)
    dw0 = torch.randn(g.K, g.R, g.S, g.C, generator=gen)
    view, unchanged = _canary(dw0.numel(), torch.float32, dw0)
    dw = view.view(g.K, g.R, g.S, g.C)
    C.conv_wgrad(dyd, xd, dw, *g.args, 1.0)
    unchanged(f"{name} conv_wgrad")
    assert torch.equal(_bits(y0), _bits(y)), f"{name}: want_stats changed y"
    dwref = ref["dw"] + dw0.double()
    rs = {"y": _ratio("y", y, ref["y"], ref["b_y"]), "dx": _ratio("dx", dx, ref["dx"], ref["b_dx"]),
          "dx+res": _ratio("dx + residual", dxr, ref["dx"] + res.double(), R.b_dxres(ref, res)),
          "dw": _ratio("dw", dw, dwref, ref["b_dw"] + R.u32 * dwref.abs()),
          "stats": _stats_check(name, st, ref["y"], False, y)}
    _check(name, rs)
    # bn_fwd_train from the conv's partials
    K = g.K
    yk = y.double().cpu().reshape(-1, K)
    gamma, beta = 1 + 0.25 * torch.randn(K, generator=gen), 0.5 * torch.randn(K, generator=gen)
    rm0, rv0 = torch.randn(K, generator=gen), torch.rand(K, generator=gen) + 0.5
    rm, rv = rm0.to(dev), rv0.to(dev)
    y2, coef = C.bn_fwd_train(y, gamma.to(dev), beta.to(dev), rm, rv, R.BN_MOM, R.BN_EPS, True, None, st)
    torch.cuda.synchronize()
    b = R.bn_fwd_budgets(yk, gamma, beta, rm0, rv0)
    yr, b_y = R.bn_apply_ref(yk, coef.cpu(), None, True)
    _check(name, _bn_stat_ratios(coef, rm, rv, b) | {"bn y": _ratio("bn y", y2.reshape(-1, K), yr, b_y)})


# ======================================================== Tier B: BatchNorm
def _bn_stat_ratios(coef, rm, rv, b, tag=""):
    return {"mean": _ratio(tag + "mean", coef[2], b["mean"], b["b_mean"]),
            "invstd": _ratio(tag + "invstd", coef[3], b["invstd"], b["b_invstd"]),
            "scale": _ratio(tag + "scale", coef[0], b["scale"], b["b_scale"]),
            "shift": _ratio(tag + "shift", coef[1], b["shift"], b["b_shift"]),
            "rmean": _ratio(tag + "running mean", rm, b["rmean"], b["b_rmean"]),
            "rvar": _ratio(tag + "running var", rv, b["rvar"], b["b_rvar"])}


@pytest.mark.parametrize("C_", R.BN_C)
@pytest.mark.parametrize("M", R.BN_M)
def test_bn_train_fwd_bwd(C, M, C_):
    """bn_fwd_train from its own statistics (plain; ReLU; ReLU + residual) and bn_bwd (plain; with dz for the
    residual branch; mask from y; mask from y's bits) against fp64, per element and per channel.  Channels:
    0 constant (var = 0 exactly, invstd = eps^-1/2, y == beta), 1 mean 16 / std 1, 2 mean -64 / std 0.5 (the
    variance budget scales with E[x^2]; the realistic ratio var error / (u32 * var) on these is printed),
    3 all zeros.  M = 1: the running variance takes no M / (M - 1) factor.  dgamma / dbeta accumulate into
    prefilled canary-tailed buffers."""
    c = R.bn_case(M, C_, seed=M + C_)
    x, dy, res = c["x"].to(dev), c["dy"].to(dev), c["res"].to(dev)
    gam, bet = c["gamma"].to(dev), c["beta"].to(dev)
    b = R.bn_fwd_budgets(c["x"].double(), c["gamma"], c["beta"], c["rmean"], c["rvar"])
    print(f"bn M={M} C={C_}")
    rs = {}
    for relu, use_res in ((False, False), (True, False), (True, True)):
        tag = f"relu={int(relu)} res={int(use_res)} "
        rm, rv = c["rmean"].to(dev), c["rvar"].to(dev)
        y, coef = C.bn_fwd_train(x, gam, bet, rm, rv, R.BN_MOM, R.BN_EPS, relu, res if use_res else None, None)
        torch.cuda.synchronize()
        if not relu:
            rs.update(_bn_stat_ratios(coef, rm, rv, b))
            ch = [1, 2]
            var_k = 1 / coef.double().cpu()[3] ** 2 - R.BN_EPS
            real = ((var_k - b["var"]).abs()[ch] / (R.u32 * b["var"][ch] + R.FLOOR)).tolist() if M > 1 else [0, 0]
            print(f"  cancellation channels (mean 16 / std 1, mean -64 / std 0.5): |var err| / (2^-24 var) = "
                  f"{real[0]:.1f}, {real[1]:.1f}; |var err| / budget = "
                  f"{((var_k - b['var']).abs()[ch] / b['b_var'][ch]).max().item():.3f} (var recovered from the fp32 invstd)")
            # constant channel
            assert abs(coef[3, 0].item() - R.BN_EPS ** -0.5) <= 2.0 ** -23 * R.BN_EPS ** -0.5
            assert torch.equal(y[:, 0].cpu(), torch.full((M,), 0.5, dtype=BF)), "constant channel: y != beta"
            assert torch.equal(y[:, 3].cpu(), c["beta"][3].to(BF).expand(M)), "zero channel: y != beta"
        else:
            cf = coef.cpu()
            assert torch.equal(cf, coef0), "the coefficients depend on relu / residual"
        coef0 = coef.cpu()
        yr, b_y = R.bn_apply_ref(c["x"], coef0, c["res"] if use_res else None, relu)
        rs[tag + "y"] = _ratio(tag + "y", y, yr, b_y)
        # backward
        for variant in (("y", "bits") if relu else ("plain", "dz")):
            gen = torch.Generator().manual_seed(C_ + len(variant))
            g0, b0 = torch.randn(C_, generator=gen), torch.randn(C_, generator=gen)
            dgv, dg_ok = _canary(C_, torch.float32, g0)
            dbv, db_ok = _canary(C_, torch.float32, b0)
            ym = y
            if variant == "bits":
                ym, bits = C.bn_apply(x, coef, res if use_res else None, None, True, True)
                dx, dz = C.bn_bwd(dy, None, x, gam, coef, dgv, dbv, True, bits)
                assert torch.equal(bits.cpu(), R.pack_bits(ym.cpu() > 0)), "bn_apply mask bits"
            else:
                dx, dz = C.bn_bwd(dy, y if relu else None, x, gam, coef, dgv, dbv, variant != "plain", None)
            dg_ok(f"bn_bwd dgamma ({variant})")
            db_ok(f"bn_bwd dbeta ({variant})")
            mask = (ym.double().cpu() > 0) if relu else None
            bw = R.bn_bwd_ref(c["dy"], c["x"], c["gamma"], coef0, mask, g0, b0)
            if variant != "plain":
                _exact(f"bn_bwd dz ({variant})", dz, bw["dz"])
            t = tag + variant + " "
            rs[t + "dx"] = _ratio(t + "dx", dx, bw["dx"], bw["b_dx"])
            rs[t + "dgamma"] = _ratio(t + "dgamma", dgv, bw["dgamma"], bw["b_dgamma"])
            rs[t + "dbeta"] = _ratio(t + "dbeta", dbv, bw["dbeta"], bw["b_dbeta"])
    _check(f"bn M={M} C={C_}", rs)


@pytest.mark.parametrize("M,C_", [(1, 8), (97, 64), (2, 2048)])
def test_bn_eval(C, M, C_):
    """bn_fwd_eval: y = relu((x - rmean) gamma / sqrt(rvar + eps) + beta + res).  The coefficients come from
    rsqrtf (within 1 ulp: 2^-23 relative, plus the fp32 rounding of rvar + eps halved by the square root), so
    b_scale = 2^-22 |scale|, b_shift = |rmean| b_scale + 2 u32 (|rmean scale| + |beta|); then bn_apply_ref's
    budget around the fp64 coefficients."""
    c = R.bn_case(M, C_, seed=9)
    y = C.bn_fwd_eval(c["x"].to(dev), c["gamma"].to(dev), c["beta"].to(dev), c["rmean"].to(dev), c["rvar"].to(dev),
                      R.BN_EPS, True, c["res"].to(dev))
    torch.cuda.synchronize()
    inv = 1 / torch.sqrt(c["rvar"].double() + R.BN_EPS)
    sc = c["gamma"].double() * inv
    sh = c["beta"].double() - c["rmean"].double() * sc
    yr, b_y = R.bn_apply_ref(c["x"], torch.stack([sc, sh, sc, sc]), c["res"], True)
    b_sc = 2.0 ** -22 * sc.abs()
    b_sh = c["rmean"].double().abs() * b_sc + 2 * R.u32 * ((c["rmean"].double() * sc).abs() + c["beta"].double().abs())
    print(f"bn_eval M={M} C={C_}")
    _check("bn_eval", {"y": _ratio("y", y, yr, b_y + (c["x"].double().abs() * b_sc + b_sh) * (1 + R.U))})


@pytest.mark.parametrize("shape", [(1, 1, 1, 8), (2, 5, 9, 64), (3, 2048)])
def test_bn_apply_dyadic(C, shape):
    """bn_apply on the dyadic grid (exact in fp32, one bf16 rounding): y bitwise, the ReLU bits against the
    packed reference, with >= 5 % of the pre-activations exactly at 0; plain, + residual, and + a BN'd
    residual (bn_apply2: the residual branch rounded to bf16 first)."""
    h, coef, pre = R.dyadic_bn(shape, 31)
    h2, coef2, pre2 = R.dyadic_bn(shape, 32)
    hd, cd = h.to(dev), coef.to(dev)
    for relu in (True, False):
        y, bits = C.bn_apply(hd, cd, None, None, relu, True)
        torch.cuda.synchronize()
        want = pre.clamp(min=0) if relu else pre
        _exact("bn_apply y", y, want.to(BF).double())
        assert torch.equal(bits.cpu(), R.pack_bits(want.to(BF) > 0)), "bn_apply mask bits"
    r = torch.where(pre == 0, torch.zeros_like(pre), h2.double())
    y, bits = C.bn_apply(hd, cd, r.to(BF).to(dev), None, True, True)
    torch.cuda.synchronize()
    _exact("bn_apply y (+ residual)", y, (pre + r).clamp(min=0).to(BF).double())
    assert torch.equal(bits.cpu(), R.pack_bits((pre + r) > 0)), "bn_apply mask bits (+ residual)"
    y, bits = C.bn_apply(hd, cd, h2.to(dev), coef2.to(dev), True, True)
    torch.cuda.synchronize()
    t = pre + pre2.to(BF).double()
    _exact("bn_apply y (+ BN'd residual)", y, t.clamp(min=0).to(BF).double())
    assert torch.equal(bits.cpu(), R.pack_bits(t > 0)), "bn_apply mask bits (+ BN'd residual)"


# ========================================================= Tier A: pooling
@pytest.mark.parametrize("C_", R.POOL_C)
@pytest.mark.parametrize("H,W", R.POOL_HW)
@pytest.mark.parametrize("k,s,p", R.POOL_CFG)
def test_maxpool_ties(C, k, s, p, H, W, C_):
    """maxpool_fwd / maxpool_bwd on data of three values (ties in most windows), negative wherever a window
    reaches padding: y bitwise equal to F.max_pool2d, and with integer dy, dx bitwise equal to its fp64
    autograd (first tap in scan order wins a tie; overlapping windows sum into it).  3/2/1, 2/2/0 and 3/1/1
    run the compile-time-k kernel for k = 3 and the run-time-k path for k = 2; 3/2/0 leaves the last column of
    the 9 x 6 input under no window (dx = 0 there)."""
    N = 2
    x = R.pool_case(N, H, W, C_, k, p, seed=H * 10 + k)
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    gen = torch.Generator().manual_seed(3)
    dy = torch.randint(-3, 4, (N, OH, OW, C_), generator=gen).to(BF)
    yr, dxr = R.maxpool_ref(x, dy, k, s, p)
    y, idx = C.maxpool_fwd(x.to(dev), k, s, p)
    dx = C.maxpool_bwd(dy.to(dev), idx, [N, H, W, C_], k, s, p)
    torch.cuda.synchronize()
    _exact("maxpool_fwd", y, yr)
    assert idx.max().item() < k * k
    _exact("maxpool_bwd", dx, dxr)


@pytest.mark.parametrize("C_", R.GAVG_C)
@pytest.mark.parametrize("H,W", R.GAVG_HW)
def test_gavgpool(C, H, W, C_):
    """gavgpool_fwd at HW in {1, 49, 50}: per element within one bf16 rounding plus the fp32 sum term;
    gavgpool_bwd: dx = bf16(dy / HW) (one fp32 multiply or divide, one bf16 rounding)."""
    gen = torch.Generator().manual_seed(H * W + C_)
    x = (torch.randn(3, H, W, C_, generator=gen) + 0.5).to(BF)
    dy = torch.randn(3, C_, generator=gen).to(BF)
    y = C.gavgpool_fwd(x.to(dev))
    dx = C.gavgpool_bwd(dy.to(dev), [3, H, W, C_])
    torch.cuda.synchronize()
    yr, b = R.gavg_ref(x)
    dxr = (dy.double() / (H * W)).view(3, 1, 1, C_).expand(3, H, W, C_)
    print(f"gavgpool HW={H * W} C={C_}")
    _check("gavgpool", {"y": _ratio("y", y, yr, b),
                        "dx": _ratio("dx", dx, dxr, (R.U + 3 * R.u32) * dxr.abs() + R.FLOOR)})
