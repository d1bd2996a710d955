"""The downsample conv folded into conv3's streaming pass (DPE_DOWN_CAT; pwconv.hip PW_CAT, bngram.hip's
gram_coef_kernel, models/_resnet_fused.py).

hd = x W_d^T is linear in the block input x, so BN_d's FORWARD coefficients follow from (G_x, s_x, W_d) as BN3's do
from (G, s, W3), and the block output relu(BN3(a2 W3^T) + BN_d(x W_d^T)) is one pass over the concatenated K
[a2 | x] with two fp32 accumulator sets scaled per output channel: no hd tensor, no downsample conv launch, no
bn_finalize for BN_d.

Op level: the new chain (bn_gram_pilot -> bn_gram -> bn_gram_coef -> conv1x1_apply_cat) and today's chain (conv_fwd
-> bn_coef -> conv1x1_apply) are both measured against an fp64 CPU reference over the same bf16 inputs (batch
statistics in fp64, a2 formed with one fp32 rounding as the kernels' fma does); the new chain may deviate at most
1.25 x as far as today's (today's rounds hd to bf16, the new one rounds only the output: the margin covers a
different reduction order).  The figures are printed before they are asserted.

Measured relative L2 errors of out vs fp64 (new / today's): see docs/perf_notes.md, "Downsample conv folded into
conv3".
"""
import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from distributed_pytorch_example_amd.ops._ext import ext  # noqa: E402

DEV = "cuda"
EPS = 1e-5
MOM = 0.1
CONF = ([1, 1], [0, 0], [1, 1])
SHAPES = [(3, 10, 10), (1, 8, 8), (5, 30, 30)]  # M = 300 (tail, no multiple of 32 / 64), 64 (one tile), 4500


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _inputs(shape, C, seed):
    """bf16-rounded inputs of one downsample block's tail: h2 with BN2's coefficients (one negative scale), the
    block input x (non-negative, channels at mean / std of 1, 10 and 30, one constant channel), W3 / W_d, BN3's
    and BN_d's affine parameters (one gamma = 0 each) and BN_d's running statistics at non-trivial values."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    N = 4 * C
    h2 = (0.3 + torch.randn(*shape, C, device=DEV, generator=g)).bfloat16()
    hf = h2.float().reshape(-1, C)
    mean2, invstd2 = hf.mean(0), (hf.var(0, unbiased=False) + EPS).rsqrt()
    gamma2 = 1 + 0.2 * torch.randn(C, device=DEV, generator=g)
    gamma2[2] = -0.8  # a negative BN2 scale
    beta2 = 0.2 * torch.randn(C, device=DEV, generator=g)
    c2 = torch.stack([gamma2 * invstd2, beta2 - mean2 * gamma2 * invstd2, mean2, invstd2]).float().contiguous()
    ratio = torch.tensor([1.0, 10.0, 30.0], device=DEV)[torch.arange(C, device=DEV) % 3]
    std = 0.5 + torch.rand(C, device=DEV, generator=g)
    x = (ratio * std + std * torch.randn(*shape, C, device=DEV, generator=g)).clamp_(min=0)
    x[..., 5] = 1.5  # a constant input channel
    x = x.bfloat16()
    w3 = (torch.randn(N, 1, 1, C, device=DEV, generator=g) * C ** -0.5).bfloat16()
    wd = (torch.randn(N, 1, 1, C, device=DEV, generator=g) * C ** -0.5).bfloat16()
    g3, gd = (1 + 0.1 * torch.randn(N, device=DEV, generator=g) for _ in range(2))
    b3, bd = (0.1 * torch.randn(N, device=DEV, generator=g) for _ in range(2))
    g3[3] = 0.0
    gd[7] = 0.0
    rm = torch.randn(N, device=DEV, generator=g)
    rv = 0.5 + torch.rand(N, device=DEV, generator=g)
    return dict(h2=h2, c2=c2, x=x, w3=w3, wd=wd, g3=g3, b3=b3, gd=gd, bd=bd, rm=rm, rv=rv)


def _fp64(d):
    """relu(BN3(a2 W3^T) + BN_d(x W_d^T)) on the CPU in fp64, BN_d's (scale, shift, mean, invstd) and its updated
    running statistics."""
    C = d["h2"].shape[-1]
    c = {k: v.detach().cpu() for k, v in d.items()}
    h2 = c["h2"].double().reshape(-1, C)
    # a2 as the kernels form it: fma in fp32 (one rounding), ReLU, rounded to bf16
    a2 = (h2 * c["c2"][0].double() + c["c2"][1].double()).float().clamp_min(0).bfloat16().double()
    x = c["x"].double().reshape(-1, C)
    M = x.shape[0]
    h3 = a2 @ c["w3"].double().reshape(-1, C).t()
    hd = x @ c["wd"].double().reshape(-1, C).t()

    def bn(h, gamma, beta):
        mean, var = h.mean(0), h.var(0, unbiased=False)
        invstd = (var + EPS).rsqrt()
        sc = gamma.double() * invstd
        return h * sc + (beta.double() - mean * sc), torch.stack([sc, beta.double() - mean * sc, mean, invstd]), var

    y3, _, _ = bn(h3, c["g3"], c["b3"])
    yd, cd, var = bn(hd, c["gd"], c["bd"])
    rm = (1 - MOM) * c["rm"].double() + MOM * cd[2]
    rv = (1 - MOM) * c["rv"].double() + MOM * var * M / max(M - 1, 1)
    return (y3 + yd).clamp_min(0), cd, rm, rv


def _bn3(X, d):
    M = d["h2"].numel() // d["h2"].shape[-1]
    G, sv = X.bn_gram(d["h2"], d["c2"], d["c2"])
    return X.bn_gram_coef(G, sv, d["w3"], M, d["g3"], d["b3"], None, None, MOM, EPS)[0], M


def _todays_path(X, d):
    c3, M = _bn3(X, d)
    rm, rv = d["rm"].clone(), d["rv"].clone()
    hd, st = X.conv_fwd(d["x"], d["wd"], *CONF, True, None)
    cd = X.bn_coef(st, M, d["gd"], d["bd"], rm, rv, MOM, EPS)
    out, bits = X.conv1x1_apply(d["h2"], d["w3"], d["c2"], c3, hd, cd)
    return out, bits, cd, rm, rv


def _new_path(X, d):
    c3, M = _bn3(X, d)
    rm, rv = d["rm"].clone(), d["rv"].clone()
    Gx, sx = X.bn_gram(d["x"], None, X.bn_gram_pilot(d["x"], False), False)
    cd, ud = X.bn_gram_coef(Gx, sx, d["wd"], M, d["gd"], d["bd"], rm, rv, MOM, EPS)
    out, bits = X.conv1x1_apply_cat(d["h2"], d["w3"], d["c2"], c3, d["x"], d["wd"], cd)
    return out, bits, cd, rm, rv


def _pack_bits(out):
    """(out > 0) packed as relu_mask_byte does: bit e of byte (m N + n) / 8 is channel n = 8 (n / 8) + e."""
    b = (out.float() > 0).reshape(*out.shape[:-1], out.shape[-1] // 8, 8).to(torch.int32)
    return (b << torch.arange(8, device=out.device, dtype=torch.int32)).sum(-1).to(torch.uint8)


_CASES = {}


def _case(shape, C):
    """One (shape, width)'s inputs, fp64 reference and both paths' results: computed once, shared, left unchanged."""
    key = (shape, C)
    if key not in _CASES:
        X = ext()
        assert X.down_cat_ok([*shape, C], C, 4 * C, 1)
        d = _inputs(shape, C, 100 + C + shape[1])
        _CASES[key] = (d, _fp64(d), _todays_path(X, d), _new_path(X, d))
        torch.cuda.synchronize()
    return _CASES[key]


@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("shape", SHAPES)
def test_out_against_fp64(shape, C):
    """The block output of the fused pass vs fp64, at most 1.25 x the error of conv_fwd + bn_coef + conv1x1_apply."""
    _, (ref, _, _, _), old, new = _case(shape, C)
    assert torch.isfinite(new[0].float()).all()
    e_new, e_old = _rel(new[0].reshape(ref.shape), ref), _rel(old[0].reshape(ref.shape), ref)
    print(f"\nout {shape} {C}+{C}->{4 * C}: fused pass {e_new:.4e}, today's path {e_old:.4e} (rel. L2 vs fp64)")
    assert e_new <= 1.25 * e_old, (e_new, e_old)


@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("shape", SHAPES)
def test_mask_bits(shape, C):
    """The ReLU bits are the bits of the stored bf16 output, every row up to the last (M is no multiple of the
    64-row tile at two of the shapes: the rows past M are neither stored nor do they disturb the last bytes)."""
    _, _, _, new = _case(shape, C)
    out, bits = new[0], new[1]
    assert bits.dtype == torch.uint8 and tuple(bits.shape) == (*out.shape[:-1], out.shape[-1] // 8)
    assert torch.equal(bits, _pack_bits(out))
    assert (out.float() >= 0).all() and (out.float() > 0).any()


@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("shape", SHAPES)
def test_bnd_coefficients_and_running_stats(shape, C):
    """BN_d's [4][N] coefficients and its running mean / variance (momentum update from non-trivial values) from the
    Gram pass vs the fp64 statistics of x W_d^T, at most 1.25 x the error of today's bn_coef values; x has channels
    at mean / std up to 30, where an uncentred Gram would cancel."""
    _, (_, cd64, rm64, rv64), old, new = _case(shape, C)
    bad = []
    rows = [("scale", new[2][0], old[2][0], cd64[0]), ("shift", new[2][1], old[2][1], cd64[1]),
            ("mean", new[2][2], old[2][2], cd64[2]), ("invstd", new[2][3], old[2][3], cd64[3]),
            ("running_mean", new[3], old[3], rm64), ("running_var", new[4], old[4], rv64)]
    for name, n, o, r in rows:
        assert torch.isfinite(n).all(), name
        e_new, e_old = _rel(n, r), _rel(o, r)
        print(f"\nBN_d {name} {shape} {C}: Gram {e_new:.3e}, today's bn_coef {e_old:.3e} (rel. L2 vs fp64)")
        if not e_new <= 1.25 * e_old:
            bad.append((name, e_new, e_old))
    assert not bad, bad


@pytest.mark.parametrize("C", [64, 128])
def test_deterministic(C):
    X = ext()
    d, _, _, new = _case(SHAPES[2], C)
    again = _new_path(X, d)
    for a, b in zip(new, again):
        assert torch.equal(a, b)


@pytest.mark.parametrize("C", [64, 128])
def test_dynamic_schedule_under_cu_budget(C):
    """Under a CU budget the fused pass runs more row groups than resident block rows and claims the rest at run
    time: the output and its bits are bitwise the unbudgeted ones, in two budgeted runs, and the claim counters are
    left zeroed (the unbudgeted run after them is bitwise the first one).  M = 125,440 rows: every row group keeps
    at least 7 tiles."""
    X = ext()
    d = _inputs((40, 56, 56), C, 7 + C)
    c3, M = _bn3(X, d)
    Gx, sx = X.bn_gram(d["x"], None, X.bn_gram_pilot(d["x"], False), False)
    cd, _ = X.bn_gram_coef(Gx, sx, d["wd"], M, d["gd"], d["bd"], None, None, MOM, EPS)

    def run():
        r = X.conv1x1_apply_cat(d["h2"], d["w3"], d["c2"], c3, d["x"], d["wd"], cd)
        torch.cuda.synchronize()
        return r

    y0, b0 = run()
    X.set_cu_reserve(16)
    X.set_comm_active(True)
    try:
        assert X.cu_reserve() == 16
        (y1, b1), (y2, b2) = run(), run()
    finally:
        X.set_comm_active(False)
        X.set_cu_reserve(0)
    y3, b3 = run()
    assert torch.equal(y0, y1) and torch.equal(b0, b1)
    assert torch.equal(y1, y2) and torch.equal(b1, b2)
    assert torch.equal(y3, y0) and torch.equal(b3, b0)
    assert torch.equal(b0, _pack_bits(y0))


def test_envelope():
    X = ext()
    assert X.down_cat_ok([2, 16, 16, 64], 64, 256, 1) and X.down_cat_ok([2, 16, 16, 128], 128, 512, 1)
    assert not X.down_cat_ok([2, 16, 16, 64], 64, 256, 2)      # strided downsample conv
    assert not X.down_cat_ok([2, 16, 16, 256], 128, 512, 1)    # conv3's operand narrower than the block input
    assert not X.down_cat_ok([2, 16, 16, 256], 256, 1024, 1)   # no 256-wide instantiation
    assert not X.down_cat_ok([2, 16, 16, 64], 64, 128, 1)      # Cout != 4 Cin


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


def _make_blocks(seed):
    import torch.nn as nn

    from distributed_pytorch_example_amd.models.resnet import Bottleneck

    torch.manual_seed(seed)
    base = nn.ModuleList([Bottleneck(64, 64, 1, True), Bottleneck(256, 64, 1, False)]).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(seed + 1)
    for b in base:  # non-trivial affine parameters
        for m in b.modules():
            if isinstance(m, nn.BatchNorm2d):
                with torch.no_grad():
                    m.weight.add_(0.1 * torch.randn(m.weight.shape, device=DEV, generator=g))
                    m.bias.add_(0.1 * torch.randn(m.bias.shape, device=DEV, generator=g))
    x0 = torch.randn(2, 16, 16, 64, device=DEV, generator=g).abs().bfloat16()
    gy = torch.randn(2, 16, 16, 256, device=DEV, generator=g).bfloat16()
    return base, x0, gy


def _run_blocks(RF, base, x0, gy, down_cat, gram=True, bnd=True):
    """Forward + backward of the chained blocks (deep copies of ``base``): (out, {name: grad}, dx, buffers of the
    downsample BN, forward call names)."""
    saved = RF._DOWN_CAT, RF._GRAM, RF.ext, RF._BND_GRAM
    rec = _Spy(ext())
    try:
        RF._DOWN_CAT, RF._GRAM, RF._BND_GRAM = down_cat and gram, gram, bnd and gram
        RF.ext = lambda: rec
        blocks = copy.deepcopy(base)
        x = x0.clone().requires_grad_(True)
        h, link = x, None
        for i, b in enumerate(blocks):
            gn = RF.gram_successor_width(blocks[i + 1]) if i + 1 < len(blocks) else 0
            h, link = b.forward_chained(h, link, gram_next=gn)
        fwd_names = list(rec.names)
        (h.float() * gy.float()).sum().backward()
        torch.cuda.synchronize()
        grads = {n: p.grad.detach().clone() for n, p in blocks.named_parameters()}
        bufs = (blocks[0].down.bn.running_mean.clone(), blocks[0].down.bn.running_var.clone())
        return h.detach().clone(), grads, x.grad.detach().clone(), bufs, fwd_names
    finally:
        RF._DOWN_CAT, RF._GRAM, RF.ext, RF._BND_GRAM = saved


def _torch_blocks(base, x0, gy):
    """fp32 torch autograd of the two blocks over the bf16-rounded weights: ({name: grad}, dx NHWC)."""
    prev = torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32
    torch.backends.cudnn.allow_tf32 = torch.backends.cuda.matmul.allow_tf32 = False
    try:
        P = {}

        def cb(name, m, t, stride=1, pad=0):
            w = m.conv.weight.detach().bfloat16().float()
            if w.shape[1] != t.shape[1]:  # stored [Cout, kh, kw, Cin]
                w = w.permute(0, 3, 1, 2)
            w = w.contiguous().requires_grad_(True)
            g, b = m.bn.weight.detach().clone().requires_grad_(True), m.bn.bias.detach().clone().requires_grad_(True)
            P[name + ".conv.weight"], P[name + ".bn.weight"], P[name + ".bn.bias"] = w, g, b
            return F.batch_norm(F.conv2d(t, w, None, stride, pad), None, None, g, b, True, MOM, m.bn.eps)

        x = x0.float().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        h = x
        for i, blk in enumerate(base):
            idn = cb(f"{i}.down", blk.down, h) if blk.down is not None else h
            t = torch.relu(cb(f"{i}.c1", blk.c1, h))
            t = torch.relu(cb(f"{i}.c2", blk.c2, t, 1, 1))
            h = torch.relu(cb(f"{i}.c3", blk.c3, t) + idn)
        (h * gy.float().permute(0, 3, 1, 2)).sum().backward()
        return {n: p.grad for n, p in P.items()}, x.grad.permute(0, 2, 3, 1).contiguous()
    finally:
        torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32 = prev


def test_blocks_flag_on_vs_off():
    """A downsample block then an identity block (N = 2, 16 x 16, 64 / 256 wide: ResNet-50's layer1.0 -> layer1.1),
    forward + backward, DPE_DOWN_CAT on vs off.  On: one fused call, no downsample conv, no bn_coef for BN_d, no
    bn_gram_u.  Off: none of the new calls, and two runs are bitwise equal.  Every tensor's on-vs-off deviation is
    printed beside the DPE_BN3_GRAM on-vs-off yardstick, and dW_d, dgamma_d and dx against fp32 torch autograd are no
    worse than 1.25 x the flag-off path."""
    from distributed_pytorch_example_amd.models import _resnet_fused as RF

    if not (RF._GRAM and RF._BND_GRAM):
        pytest.skip("DPE_BN3_GRAM=0 or DPE_BND_GRAM=0")
    base, x0, gy = _make_blocks(41)
    out_on, g_on, dx_on, buf_on, names_on = _run_blocks(RF, base, x0, gy, True)
    out_off, g_off, dx_off, buf_off, names_off = _run_blocks(RF, base, x0, gy, False)
    out_off2, g_off2, dx_off2, buf_off2, names_off2 = _run_blocks(RF, base, x0, gy, False)
    out_ng, g_ng, dx_ng, _, _ = _run_blocks(RF, base, x0, gy, False, gram=False)
    # flag off: none of the new calls, deterministic
    assert "conv1x1_apply_cat" not in names_off and "bn_gram_u" in names_off and names_off == names_off2
    assert torch.equal(out_off, out_off2) and torch.equal(dx_off, dx_off2)
    assert all(torch.equal(g_off[n], g_off2[n]) for n in g_off)
    # flag on: one fused call instead of the downsample conv + its bn_coef + conv1x1_apply; u_d from bn_gram_coef
    assert names_on.count("conv1x1_apply_cat") == 1 and "bn_gram_u" not in names_on
    assert names_on.count("conv_fwd") == names_off.count("conv_fwd") - 1
    assert names_on.count("bn_coef") == names_off.count("bn_coef") - 1
    assert names_on.count("conv1x1_apply") == names_off.count("conv1x1_apply") - 1
    assert names_on.count("bn_gram_coef") == names_off.count("bn_gram_coef") + 1
    # nothing else differs (kernel launches: -1, bn_gram_coef being bn_gram_u + one kernel)
    changed = {"conv1x1_apply_cat", "conv_fwd", "bn_coef", "conv1x1_apply", "bn_gram_coef", "bn_gram_u", "down_cat_ok"}
    assert sorted(n for n in names_on if n not in changed) == sorted(n for n in names_off if n not in changed)
    print(f"\n  {'out':24s} DOWN_CAT on vs off {_rel(out_on, out_off):.3e}   BN3 Gram on vs off {_rel(out_off, out_ng):.3e}")
    for k, nm in enumerate(("down.bn.running_mean", "down.bn.running_var")):
        print(f"  {nm:24s} DOWN_CAT on vs off {_rel(buf_on[k], buf_off[k]):.3e}")
    for n in g_on:
        print(f"  {n:24s} DOWN_CAT on vs off {_rel(g_on[n], g_off[n]):.3e}   BN3 Gram on vs off {_rel(g_off[n], g_ng[n]):.3e}")
    print(f"  {'dx':24s} DOWN_CAT on vs off {_rel(dx_on, dx_off):.3e}   BN3 Gram on vs off {_rel(dx_off, dx_ng):.3e}")
    ref, dx_ref = _torch_blocks(base, x0, gy)
    bad = []
    for n in ("0.down.conv.weight", "0.down.bn.weight", "dx"):
        r = dx_ref if n == "dx" else ref[n]
        on, off = (dx_on, dx_off) if n == "dx" else (g_on[n], g_off[n])
        if n.endswith("conv.weight"):
            on, off, r = on.reshape(256, -1), off.reshape(256, -1), r.reshape(256, -1)
        e_on, e_off = _rel(on.float(), r), _rel(off.float(), r)
        print(f"  {n:24s} vs fp32 autograd: flag on {e_on:.3e}, flag off {e_off:.3e}")
        if not e_on <= 1.25 * e_off:
            bad.append((n, e_on, e_off))
    assert not bad, bad


def test_blocks_output_independent_of_bnd_backward_form():
    """The fused forward does not ask which backward form BN_d takes: with the Gram backward of BN_d switched off
    in-process the block output and BN_d's running statistics are bitwise those with it on (the same fused pass; hd
    is produced beside it for bn_bwd_partials only), and the gradients are finite."""
    from distributed_pytorch_example_amd.models import _resnet_fused as RF

    if not (RF._GRAM and RF._BND_GRAM and RF._DOWN_CAT):
        pytest.skip("DPE_BN3_GRAM=0, DPE_BND_GRAM=0 or DPE_DOWN_CAT=0")
    base, x0, gy = _make_blocks(43)
    out_a, g_a, dx_a, buf_a, names_a = _run_blocks(RF, base, x0, gy, True)
    out_b, g_b, dx_b, buf_b, names_b = _run_blocks(RF, base, x0, gy, True, bnd=False)
    assert names_b.count("conv1x1_apply_cat") == 1 and names_b.count("conv_fwd") == names_a.count("conv_fwd") + 1
    assert torch.equal(out_a, out_b) and torch.equal(buf_a[0], buf_b[0]) and torch.equal(buf_a[1], buf_b[1])
    assert all(torch.isfinite(g_b[n]).all() for n in g_b) and torch.isfinite(dx_b.float()).all()
