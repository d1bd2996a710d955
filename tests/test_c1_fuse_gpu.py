"""The next block's conv1 formed inside conv3's streaming pass (DPE_C1_FUSE; pwconv.hip's C1 variant of
pw_stream_kernel, conv1x1_apply_next, models/_resnet_fused.py).

The pass that writes block i's output out = relu(BN3(a2 W3^T) + x) holds every output row, rounded to bf16, in LDS
on the way to the store; it also computes h1 = out W1^T (block i+1's conv1: 256 -> 64 or 128) from those rows and
BN1's forward sums of the stored h1.  out and its ReLU bits must be bitwise conv1x1_apply's; h1 differs from
conv_fwd's over the stored out only by the order of the fp32 sums.

Op level (K = 64, Cout3 = 256, c1 in {64, 128}; M = 64: one tile, 96: a 32-row tail half, 320: five tiles, 70,432:
1,100 tiles + a 32-row tail, several tiles per row group): out / bits bitwise, h1 against an fp64 CPU product of the
stored out with W1 (per-element budget of tests/_c1_fuse_ref.py, and a worst error of at most 1.25 x conv_fwd's on
the same stored out -- both measured here and printed), the partial sums against fp64 sums of the stored h1, two
calls bitwise equal, outputs inside guard regions, and the CU budget: no dynamic-schedule variant is built, so
c1_fuse_ok is false under a budget and the caller's two-call path runs.

Block level (N = 2, 16 x 16, forward + backward; identity -> identity and identity -> stride-2 downsample block
with a 128-wide conv1): block i's output bitwise with the flag on and off; block i+1's output, BN1 running
statistics and every gradient within 1.25 x what DPE_BN3_GRAM on/off moves them; flag off: deterministic and no new
op.

Measured on an MI355X, worst |h1 - fp64| of the fused pass / of conv_fwd on the same stored out (ratio; bound
1.25), 256 -> 64 and 256 -> 128: M = 64 1.2457e-1 / 1.2457e-1 (1.000) and 1.2484e-1 / 1.2484e-1 (1.000); M = 96
1.2473e-1 / 1.2473e-1 (1.000) and 1.2488e-1 / 1.2488e-1 (1.000); M = 320 1.2489e-1 / 1.2489e-1 (1.000) and
1.2497e-1 / 1.2497e-1 (1.000); M = 70,432 1.2501e-1 / 1.2501e-1 (1.000) and 1.2500e-1 / 1.2500e-1 (1.000): the
worst element is one bf16 rounding of a value near 32 in both.  Worst error / per-element budget: 0.95 - 0.98 for both
paths.  Partial sums: worst error / budget 3.0e-2 (M = 64) down to 4e-6 (M = 70,432).  docs/perf_notes.md, "Next
block's conv1 inside conv3's streaming pass".
"""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

import _c1_fuse_ref as R  # noqa: E402

from distributed_pytorch_example_amd.ops._ext import ext  # noqa: E402

DEV = "cuda"
EPS = 1e-5
MOM = 0.1
CONF = ([1, 1], [0, 0], [1, 1])
K, N = 64, 256
# M = 64 (one tile), 96 (a 32-row tail half), 320 (five tiles), 70,432 (1,100 tiles + a 32-row tail)
SHAPES = [(1, 8, 8), (1, 8, 12), (1, 16, 20), (1, 124, 568)]
C1S = [64, 128]


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _inputs(shape, c1, seed):
    """bf16-rounded inputs of one identity block's tail and the next conv1 (as tests/test_down_cat_gpu.py's): h2 with
    BN2's coefficients (one negative scale), the residual x (non-negative, channels at mean / std of 1, 10 and 30,
    one constant channel), W3, BN3's affine parameters (one gamma = 0), and W1 with a zero column and a zero row."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    h2 = (0.3 + torch.randn(*shape, K, device=DEV, generator=g)).bfloat16()
    hf = h2.float().reshape(-1, K)
    mean2, invstd2 = hf.mean(0), (hf.var(0, unbiased=False) + EPS).rsqrt()
    gamma2 = 1 + 0.2 * torch.randn(K, device=DEV, generator=g)
    gamma2[2] = -0.8  # a negative BN2 scale
    beta2 = 0.2 * torch.randn(K, device=DEV, generator=g)
    c2 = torch.stack([gamma2 * invstd2, beta2 - mean2 * gamma2 * invstd2, mean2, invstd2]).float().contiguous()
    ratio = torch.tensor([1.0, 10.0, 30.0], device=DEV)[torch.arange(N, device=DEV) % 3]
    std = 0.5 + torch.rand(N, device=DEV, generator=g)
    x = (ratio * std + std * torch.randn(*shape, N, device=DEV, generator=g)).clamp_(min=0)
    x[..., 5] = 1.5  # a constant channel
    x = x.bfloat16()
    w3 = (torch.randn(N, 1, 1, K, device=DEV, generator=g) * K ** -0.5).bfloat16()
    g3 = 1 + 0.1 * torch.randn(N, device=DEV, generator=g)
    b3 = 0.1 * torch.randn(N, device=DEV, generator=g)
    g3[3] = 0.0
    w1 = torch.randn(c1, 1, 1, N, device=DEV, generator=g) * N ** -0.5
    w1[..., 9] = 0.0   # a zero column (input channel)
    w1[11] = 0.0       # a zero row (output channel)
    w1 = w1.bfloat16()
    g1 = 1 + 0.1 * torch.randn(c1, device=DEV, generator=g)
    b1 = 0.1 * torch.randn(c1, device=DEV, generator=g)
    return dict(h2=h2, c2=c2, x=x, w3=w3, g3=g3, b3=b3, w1=w1, g1=g1, b1=b1)


def _bn3(X, d):
    M = d["h2"].numel() // K
    G, sv = X.bn_gram(d["h2"], d["c2"], d["c2"])
    return X.bn_gram_coef(G, sv, d["w3"], M, d["g3"], d["b3"], None, None, MOM, EPS)[0], M


def _todays_path(X, d, c3):
    out, bits = X.conv1x1_apply(d["h2"], d["w3"], d["c2"], c3, d["x"], None)
    h1, st = X.conv_fwd(out, d["w1"], *CONF, True, None)
    return out, bits, h1, st


def _new_path(X, d, c3, outs=None):
    return X.conv1x1_apply_next(d["h2"], d["w3"], d["c2"], c3, d["x"], None, d["w1"], outs)


_CASES = {}


def _case(shape, c1):
    """One (shape, c1)'s inputs, both paths' results and the fp64 reference of h1 over the stored out: computed once,
    shared, left unchanged."""
    key = (shape, c1)
    if key not in _CASES:
        X = ext()
        assert X.c1_fuse_ok([*shape, K], N, c1)
        d = _inputs(shape, c1, 300 + c1 + shape[2])
        c3, M = _bn3(X, d)
        old, new = _todays_path(X, d, c3), _new_path(X, d, c3)
        torch.cuda.synchronize()
        _CASES[key] = (d, c3, M, old, new, R.h1_ref(new[0].reshape(M, N), d["w1"].reshape(c1, N)))
    return _CASES[key]


@pytest.mark.parametrize("c1", C1S)
@pytest.mark.parametrize("shape", SHAPES)
def test_out_and_bits_bitwise(shape, c1):
    """The block output and its ReLU bits are bitwise conv1x1_apply's (M = 96: the all-invalid half stores nothing
    into the rows the reference call wrote)."""
    _, _, _, old, new, _ = _case(shape, c1)
    assert new[0].shape == old[0].shape and new[1].shape == old[1].shape and new[1].dtype == torch.uint8
    assert torch.equal(new[0], old[0]) and torch.equal(new[1], old[1])
    assert (new[0].float() > 0).any()


@pytest.mark.parametrize("c1", C1S)
@pytest.mark.parametrize("shape", SHAPES)
def test_h1_against_fp64(shape, c1):
    """h1 against the fp64 product of the stored out with W1: inside the per-element budget, and a worst error of at
    most 1.25 x conv_fwd's on the same stored out (the same fp32 sums in another order)."""
    d, _, M, old, new, (ref, bound) = _case(shape, c1)
    h_new, h_old = new[2].reshape(M, c1).double().cpu(), old[2].reshape(M, c1).double().cpu()
    assert tuple(new[2].shape) == (*shape, c1) and torch.isfinite(h_new).all()
    e_new, e_old = (h_new - ref).abs(), (h_old - ref).abs()
    w_new, w_old = e_new.max().item(), e_old.max().item()
    print(f"\nh1 {shape} 256->{c1}: worst |err| fused {w_new:.4e}, conv_fwd {w_old:.4e}, ratio {w_new / max(w_old, 1e-30):.3f}; "
          f"worst err / budget fused {(e_new / bound).max().item():.3f}, conv_fwd {(e_old / bound).max().item():.3f}")
    assert (e_new <= bound).all(), (e_new / bound).max().item()
    assert w_new <= 1.25 * w_old, (w_new, w_old)
    assert (h_new[:, 11] == 0).all()  # W1's zero row


@pytest.mark.parametrize("c1", C1S)
@pytest.mark.parametrize("shape", SHAPES)
def test_partial_sums(shape, c1):
    """st [2][c1][row groups]: the sums over the row groups against fp64 sums of the STORED h1 (rows past M take no
    part); a row group without tiles holds zeros; bn_coef takes it unchanged.  The largest shape has several tiles
    in some row group (from the launch's own row-group count)."""
    X = ext()
    d, _, M, old, new, _ = _case(shape, c1)
    h1, st = new[2], new[3]
    rg, tiles = st.shape[2], (M + 63) // 64
    assert tuple(st.shape[:2]) == (2, c1) and st.dtype == torch.float32 and torch.isfinite(st).all()
    if shape == SHAPES[3]:
        assert tiles > rg, (tiles, rg)  # several tiles in some row group
    if rg > tiles:
        assert (st[:, :, tiles:] == 0).all()
    ref, bound = R.stats_ref(h1.reshape(M, c1))
    err = (st.double().cpu().sum(-1) - ref).abs()
    print(f"\nst {shape} 256->{c1}: {rg} row groups, {tiles} tiles; worst err / budget {(err / bound).max().item():.3e}")
    assert (err <= bound).all(), (err / bound).max().item()
    c_new = X.bn_coef(st, M, d["g1"], d["b1"], None, None, MOM, EPS)
    c_old = X.bn_coef(old[3], M, d["g1"], d["b1"], None, None, MOM, EPS)
    assert tuple(c_new.shape) == tuple(c_old.shape) and torch.isfinite(c_new).all()
    # BN1's mean (row 2) from the two h1 tensors: each element is within its budget of the same exact value, and
    # each mean is an fp32 sum of M terms
    _, hb = R.h1_ref(new[0].reshape(M, N), d["w1"].reshape(c1, N))
    mb = 2 * hb.mean(0) + 2 * (M + 1) * R.u32 * old[2].reshape(M, c1).double().cpu().abs().mean(0)
    assert ((c_new[2] - c_old[2]).double().cpu().abs() <= mb).all()


@pytest.mark.parametrize("c1", C1S)
def test_deterministic(c1):
    X = ext()
    d, c3, _, _, new, _ = _case(SHAPES[3], c1)
    again = _new_path(X, d, c3)
    for a, b in zip(new, again):
        assert torch.equal(a, b)


def _guarded(like, pad=4096):
    """A tensor of ``like``'s shape and type between two guard regions of ``pad`` bytes: (view, whole buffer)."""
    nb = like.numel() * like.element_size()
    buf = torch.full((pad + nb + pad,), 0xA5, dtype=torch.uint8, device=DEV)
    return buf[pad:pad + nb].view(like.dtype).view(like.shape), buf


@pytest.mark.parametrize("c1", C1S)
@pytest.mark.parametrize("shape", SHAPES[:3])
def test_guard_regions(shape, c1):
    """out, bits, h1 and st written inside guard regions: the canaries on both sides survive, the results are those
    of the allocating call (M = 96 and 320: the tiles' rows past M store nothing)."""
    X = ext()
    d, c3, _, _, new, _ = _case(shape, c1)
    pairs = [_guarded(t) for t in new]
    res = _new_path(X, d, c3, [v for v, _ in pairs])
    torch.cuda.synchronize()
    for (v, buf), r, n in zip(pairs, res, new):
        assert r.data_ptr() == v.data_ptr() and torch.equal(v, n)
        assert (buf[:4096] == 0xA5).all() and (buf[-4096:] == 0xA5).all()


def test_envelope_and_cu_budget():
    """Inside: conv3 64 -> 256 beside a conv1 to 64 / 128.  No dynamic-schedule variant is built: under a CU budget
    c1_fuse_ok is false (the caller makes the two separate calls, which do have one) and the op refuses."""
    X = ext()
    assert X.c1_fuse_ok([2, 16, 16, 64], 256, 64) and X.c1_fuse_ok([2, 16, 16, 64], 256, 128)
    assert not X.c1_fuse_ok([2, 16, 16, 128], 512, 128)  # layers 2-4: several column blocks
    assert not X.c1_fuse_ok([2, 16, 16, 64], 256, 256)
    assert not X.c1_fuse_ok([2, 16, 16, 64], 128, 64)
    d, c3, _, _, new, _ = _case(SHAPES[2], 64)
    X.set_cu_reserve(16)
    X.set_comm_active(True)
    try:
        assert X.cu_reserve() == 16
        assert not X.c1_fuse_ok([*SHAPES[2], K], N, 64)
        with pytest.raises(RuntimeError):
            _new_path(X, d, c3)
    finally:
        X.set_comm_active(False)
        X.set_cu_reserve(0)
    again = _new_path(X, d, c3)
    assert all(torch.equal(a, b) for a, b in zip(new, again))


# ----------------------------------------------------------------------------- block level
class _Spy:
    """The extension module with every call recorded by name."""

    def __init__(self, real):
        self._real, self.names = real, []

    def __getattr__(self, name):
        f = getattr(self._real, name)
        if not callable(f):
            return f

        def call(*a, **k):
            self.names.append(name)
            return f(*a, **k)

        return call


def _make_blocks(seed, down):
    import torch.nn as nn

    from distributed_pytorch_example_amd.models.resnet import Bottleneck

    torch.manual_seed(seed)
    second = Bottleneck(256, 128, 2, True) if down else Bottleneck(256, 64, 1, False)
    base = nn.ModuleList([Bottleneck(256, 64, 1, False), second]).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(seed + 1)
    for b in base:  # non-trivial affine parameters
        for m in b.modules():
            if isinstance(m, nn.BatchNorm2d):
                with torch.no_grad():
                    m.weight.add_(0.1 * torch.randn(m.weight.shape, device=DEV, generator=g))
                    m.bias.add_(0.1 * torch.randn(m.bias.shape, device=DEV, generator=g))
    x0 = torch.randn(2, 16, 16, 256, device=DEV, generator=g).abs().bfloat16()
    hw = 8 if down else 16
    gy = torch.randn(2, hw, hw, 512 if down else 256, device=DEV, generator=g).bfloat16()
    return base, x0, gy


def _run_blocks(RF, base, x0, gy, c1_fuse, gram=True, budget=False):
    """Forward + backward of the two chained blocks (deep copies of ``base``), the first handed its successor as the
    ResNet's block loop does: (block 0's output, block 1's output, {name: grad}, dx, block 1's BN1 running
    statistics, forward call names)."""
    saved = RF._C1_FUSE, RF._GRAM, RF.ext
    real = ext()
    rec = _Spy(real)
    try:
        RF._C1_FUSE, RF._GRAM = c1_fuse and gram, gram
        RF.ext = lambda: rec
        if budget:
            real.set_cu_reserve(16)
            real.set_comm_active(True)
        blocks = copy.deepcopy(base)
        x = x0.clone().requires_grad_(True)
        h, link, mids = x, None, []
        for i, b in enumerate(blocks):
            nxt = blocks[i + 1] if i + 1 < len(blocks) else None
            gn = RF.gram_successor_width(nxt) if nxt is not None else 0
            h, link = b.forward_chained(h, link, gram_next=gn, next_block=nxt)
            mids.append(h.detach().clone())
        fwd_names = list(rec.names)
        (h.float() * gy.float()).sum().backward()
        torch.cuda.synchronize()
        grads = {n: p.grad.detach().clone() for n, p in blocks.named_parameters()}
        bufs = (blocks[1].c1.bn.running_mean.clone(), blocks[1].c1.bn.running_var.clone())
        return mids[0], mids[1], grads, x.grad.detach().clone(), bufs, fwd_names
    finally:
        RF._C1_FUSE, RF._GRAM, RF.ext = saved
        if budget:
            real.set_comm_active(False)
            real.set_cu_reserve(0)


@pytest.mark.parametrize("down", [False, True], ids=["identity", "stride2_down_128"])
def test_blocks_flag_on_vs_off(down):
    """An identity block then an identity block / a stride-2 downsample block with a 128-wide conv1 (ResNet-50's
    layer1.1 -> layer1.2 / layer1.2 -> layer2.0), forward + backward, DPE_C1_FUSE on vs off."""
    from distributed_pytorch_example_amd.models import _resnet_fused as RF

    if not RF._GRAM:
        pytest.skip("DPE_BN3_GRAM=0")
    base, x0, gy = _make_blocks(51 + int(down), down)
    o0_on, o1_on, g_on, dx_on, buf_on, names_on = _run_blocks(RF, base, x0, gy, True)
    o0_off, o1_off, g_off, dx_off, buf_off, names_off = _run_blocks(RF, base, x0, gy, False)
    o0_off2, o1_off2, g_off2, dx_off2, buf_off2, names_off2 = _run_blocks(RF, base, x0, gy, False)
    o0_ng, o1_ng, g_ng, dx_ng, buf_ng, _ = _run_blocks(RF, base, x0, gy, False, gram=False)
    # flag off: no new op, deterministic
    assert "conv1x1_apply_next" not in names_off and "c1_fuse_ok" not in names_off and names_off == names_off2
    assert torch.equal(o0_off, o0_off2) and torch.equal(o1_off, o1_off2) and torch.equal(dx_off, dx_off2)
    assert all(torch.equal(g_off[n], g_off2[n]) for n in g_off)
    assert all(torch.equal(a, b) for a, b in zip(buf_off, buf_off2))
    # flag on: the fused op instead of one conv1x1_apply and one conv_fwd (block 1's conv1); nothing else differs
    assert names_on.count("conv1x1_apply_next") == 1
    assert names_on.count("conv1x1_apply") == names_off.count("conv1x1_apply") - 1
    assert names_on.count("conv_fwd") == names_off.count("conv_fwd") - 1
    changed = {"conv1x1_apply_next", "conv1x1_apply", "conv_fwd", "c1_fuse_ok"}
    assert [n for n in names_on if n not in changed] == [n for n in names_off if n not in changed]
    # block 0's output: bitwise
    assert torch.equal(o0_on, o0_off)
    # block 1's output, BN1's running statistics, every gradient: within 1.25 x the BN3 Gram on/off yardstick
    rows = [("out[1]", o1_on, o1_off, o1_ng), ("c1.bn.running_mean", buf_on[0], buf_off[0], buf_ng[0]),
            ("c1.bn.running_var", buf_on[1], buf_off[1], buf_ng[1]), ("dx", dx_on, dx_off, dx_ng)]
    rows += [(n, g_on[n], g_off[n], g_ng[n]) for n in g_on]
    bad = []
    for name, on, off, ng in rows:
        assert torch.isfinite(on.float()).all(), name
        e, y = _rel(on, off), _rel(off, ng)
        print(f"  {name:24s} C1_FUSE on vs off {e:.3e}   BN3 Gram on vs off {y:.3e}")
        if not e <= 1.25 * y:
            bad.append((name, e, y))
    assert not bad, bad


def test_blocks_under_cu_budget_take_the_separate_calls():
    """Under a CU budget with the flag on the caller's two-call path runs: no fused op, results bitwise the flag-off
    ones under the same budget."""
    from distributed_pytorch_example_amd.models import _resnet_fused as RF

    if not RF._GRAM:
        pytest.skip("DPE_BN3_GRAM=0")
    base, x0, gy = _make_blocks(57, False)
    o0_a, o1_a, g_a, dx_a, _, names_a = _run_blocks(RF, base, x0, gy, True, budget=True)
    o0_b, o1_b, g_b, dx_b, _, names_b = _run_blocks(RF, base, x0, gy, False, budget=True)
    assert "conv1x1_apply_next" not in names_a and names_a.count("c1_fuse_ok") == 1
    assert [n for n in names_a if n != "c1_fuse_ok"] == names_b
    assert torch.equal(o0_a, o0_b) and torch.equal(o1_a, o1_b) and torch.equal(dx_a, dx_b)
    assert all(torch.equal(g_a[n], g_b[n]) for n in g_a)
