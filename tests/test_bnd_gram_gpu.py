"""The downsample BatchNorm's backward by Gram algebra (DPE_BND_GRAM; csrc/kernels/bngram.hip, the BN-free
pw_cat_kernel of pwconv.hip, models/_resnet_fused.py).

hd = x W_d^T is linear in the block input x, so BN_d's backward follows from G_x = x^T x, s_x = colsum(x) and
P_d = dz3^T x: no dhd tensor, no apply pass, no hd re-read in the next block's data-grad epilogue.  Stride 1
(ResNet-50's layer1.0, 64 -> 256) and stride 2 (layer2.0, 256 -> 512 over the even pixels of x).

Op level: the new chain (bn_gram_pilot -> bn_gram -> bn_gram_u, deterministic conv_wgrad, bn_gram_bwd,
conv1x1_dgrad_cat_plain) and today's chain (bn_bwd_partials -> conv_wgrad -> conv_dgrad) are both measured
against the fp32 torch autograd of conv1x1 -> training-mode BN over the same bf16 inputs; the new chain may
deviate at most twice as far as today's (the margin of tests/test_model_parity_gpu.py for a reformulation of
this kind).
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
CONF = ([1, 1], [0, 0], [1, 1])  # stride, padding, dilation of the downsample conv
CONF2 = ([2, 2], [0, 0], [1, 1])  # ... of layer2.0's


def _rel(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()


def _reference(x, w, gamma, beta, dz, stride=1):
    """fp32 autograd of 1x1 conv -> training-mode BN, loss = sum(y * dz): (dW [Cout, Cin], dgamma, dbeta, dx NHWC)."""
    prev = torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32
    torch.backends.cudnn.allow_tf32 = torch.backends.cuda.matmul.allow_tf32 = False
    try:
        Cout, Cin = w.shape[0], w.shape[-1]
        xr = x.float().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        wr = w.float().reshape(Cout, Cin, 1, 1).clone().requires_grad_(True)
        gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        y = F.batch_norm(F.conv2d(xr, wr, stride=stride), None, None, gr, br, True, 0.1, EPS)
        (y * dz.float().permute(0, 3, 1, 2)).sum().backward()
        return wr.grad.reshape(Cout, Cin), gr.grad, br.grad, xr.grad.permute(0, 2, 3, 1).contiguous()
    finally:
        torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32 = prev


def _forward(X, x, w, gamma, beta, stride=1):
    hd, st = X.conv_fwd(x, w, *(CONF2 if stride == 2 else CONF), True, None)
    M = hd.numel() // hd.shape[-1]
    return hd, X.bn_coef(st, M, gamma, beta, None, None, 0.1, EPS), M


def _todays_path(X, x, w, gamma, beta, dz, stride=1):
    """bn_bwd_partials(dz3, hd) -> conv_wgrad(dhd, x) -> conv_dgrad(dhd, W_d), the partials as the next block's
    data-grad epilogue emits them (sum dz, sum dz (hd - mean)).  Stride 2: dx is the compact [N, H/2, W/2, Cin]
    grid, as the model computes it."""
    hd, cd, M = _forward(X, x, w, gamma, beta, stride)
    Cout = w.shape[0]
    dzf, hdf = dz.float().reshape(M, Cout), hd.float().reshape(M, Cout)
    part = torch.stack([dzf.sum(0), (dzf * (hdf - cd[2])).sum(0)]).reshape(2, Cout, 1).contiguous()
    dg, db = torch.zeros(Cout, device=DEV), torch.zeros(Cout, device=DEV)
    dhd = X.bn_bwd_partials(dz, hd, gamma, cd, part, dg, db, relu_mask=False)
    dw = torch.zeros(w.shape, dtype=torch.float32, device=DEV)
    X.conv_wgrad(dhd, x, dw, *(CONF2 if stride == 2 else CONF), 1.0, None)
    dx = X.conv_dgrad(dhd, w, [x.shape[0], x.shape[1] // stride, x.shape[2] // stride, x.shape[3]], *CONF)
    return dw.reshape(Cout, -1), dg, db, dx


def _gram_path(X, x, w, gamma, beta, dz, stride=1):
    hd, cd, M = _forward(X, x, w, gamma, beta, stride)
    Cout = w.shape[0]
    s2 = stride == 2
    G, s = X.bn_gram(x, None, X.bn_gram_pilot(x, s2), s2)
    u = X.bn_gram_u(G, w)
    P = torch.full(w.shape, float("nan"), dtype=torch.float32, device=DEV)
    X.conv_wgrad(dz, x, P, *(CONF2 if s2 else CONF), 1.0, None, deterministic=True, overwrite=True)
    part = torch.full((2, Cout, 1), float("nan"), device=DEV)  # row 1 is never read (sum-dz-only epilogue)
    part[0, :, 0] = dz.float().reshape(M, Cout).sum(0)
    dg, db = torch.zeros(Cout, device=DEV), torch.zeros(Cout, device=DEV)
    dw = torch.zeros(w.shape, dtype=torch.float32, device=DEV)
    bcat, e = X.bn_gram_bwd(part, P, w, u, s, cd, gamma, M, dg, db, dw)
    dx = X.conv1x1_dgrad_cat_plain(dz, x, bcat, e, s2)
    return dw.reshape(Cout, -1), dg, db, dx


def _params(Cin, Cout, g):
    w = (torch.randn(Cout, 1, 1, Cin, device=DEV, generator=g) * Cin ** -0.5).bfloat16()
    gamma = 1 + 0.1 * torch.randn(Cout, device=DEV, generator=g)
    beta = 0.1 * torch.randn(Cout, device=DEV, generator=g)
    return w, gamma, beta


def _compare(name, x, w, gamma, beta, dz, stride=1):
    """Both chains against the fp32 reference; returns the new chain's outputs."""
    X = ext()
    ref = list(_reference(x, w, gamma, beta, dz, stride))
    if stride == 2:
        assert not ref[3][:, 1::2].any() and not ref[3][:, :, 1::2].any()  # the branch reaches the even pixels only
        ref[3] = ref[3][:, ::2, ::2].contiguous()
    old = _todays_path(X, x, w, gamma, beta, dz, stride)
    new = _gram_path(X, x, w, gamma, beta, dz, stride)
    out, bad = {}, []
    for q, r, o, n in zip(("dW_d", "dgamma_d", "dbeta_d", "dx_d"), ref, old, new):
        assert torch.isfinite(n.float()).all(), (name, q)
        e_new, e_old = _rel(n.float(), r), _rel(o.float(), r)
        out[q] = (e_new, e_old)
        print(f"{name} {q}: Gram path {e_new:.3e}, today's path {e_old:.3e} (vs fp32 autograd)")
        if not e_new <= 2 * e_old:
            bad.append((q, e_new, e_old))
    assert not bad, (name, bad)
    return new


def test_op_stride2_against_fp32_autograd():
    """N = 3, 10 x 10 -> 5 x 5: M = 75 rows of the stride-2 subsample (a tail inside the first tiles), 256 -> 512.
    Also: conv1's streaming data grad adds the compact dx_d at the even pixels only -- the odd pixels of the
    full-resolution gradient are bit for bit those of the data grad without the branch."""
    X = ext()
    g = torch.Generator(device=DEV).manual_seed(2)
    x = torch.randn(3, 10, 10, 256, device=DEV, generator=g).abs().bfloat16()
    w, gamma, beta = _params(256, 512, g)
    dz = torch.randn(3, 5, 5, 512, device=DEV, generator=g).bfloat16()
    dxd = _compare("stride2 256->512", x, w, gamma, beta, dz, 2)[3]
    assert tuple(dxd.shape) == (3, 5, 5, 256)
    dh1 = torch.randn(3, 10, 10, 128, device=DEV, generator=g).bfloat16()
    w1 = (torch.randn(128, 1, 1, 256, device=DEV, generator=g) * 128 ** -0.5).bfloat16()
    base = X.conv_dgrad(dh1, w1, list(x.shape), *CONF)
    full = X.conv_dgrad_bn(dh1, w1, list(x.shape), *CONF, dxd, None, None, None, None, True)[0]
    odd = torch.ones(10, 10, dtype=torch.bool, device=DEV)
    odd[::2, ::2] = False
    assert torch.equal(full[:, odd], base[:, odd])
    even_ref = (dh1.float().reshape(-1, 128) @ w1.float().reshape(128, 256)).reshape(3, 10, 10, 256)[:, ::2, ::2] + dxd.float()
    assert _rel(full[:, ::2, ::2].float(), even_ref) < 5e-3


def test_strided_gram_pass_matches_compact_copy():
    """The Gram pass over x[:, ::2, ::2] by row addressing == the pass over a compacted copy, bit for bit (same
    tiles, same order), at a row count of many tiles per block with a tail."""
    X = ext()
    g = torch.Generator(device=DEV).manual_seed(4)
    for C, shape in ((256, (5, 46, 50)), (64, (3, 10, 10))):
        x = torch.randn(*shape, C, device=DEV, generator=g).abs().bfloat16()
        xs = x[:, ::2, ::2].contiguous()
        pil = X.bn_gram_pilot(x, True)
        assert torch.equal(pil, X.bn_gram_pilot(xs))
        G, s = X.bn_gram(x, None, pil, True)
        G2, s2 = X.bn_gram(xs, None, pil)
        assert torch.equal(G, G2) and torch.equal(s, s2), C


@pytest.mark.parametrize("M_hw", [10, 15])
def test_deterministic_weight_grad_tail_with_bn_on_load(M_hw):
    """The weight grad's K-tail step together with BN + ReLU on load (relu(shift) rows past K times A's zeros)."""
    X = ext()
    g = torch.Generator(device=DEV).manual_seed(12)
    x = torch.randn(3, M_hw, M_hw, 64, device=DEV, generator=g).bfloat16()
    dz = torch.randn(3, M_hw, M_hw, 256, device=DEV, generator=g).bfloat16()
    c = torch.stack([1 + 0.2 * torch.randn(64, device=DEV, generator=g), 0.5 + torch.rand(64, device=DEV, generator=g),
                     torch.zeros(64, device=DEV), torch.ones(64, device=DEV)]).float()
    P = torch.full((256, 1, 1, 64), float("nan"), device=DEV)
    X.conv_wgrad(dz, x, P, *CONF, 1.0, c, deterministic=True, overwrite=True)
    a = torch.relu(x.float() * c[0] + c[1]).bfloat16().double().reshape(-1, 64)
    assert _rel(P.reshape(256, 64), dz.double().reshape(-1, 256).t() @ a) < 1e-6


@pytest.mark.parametrize("Cin", [64, 128])
def test_op_stride1_against_fp32_autograd(Cin):
    """N = 3, 10 x 10: M = 300 rows, a tail past the 32-row tiles of the Gram pass / the data grad and past the
    32-deep K steps of the weight grad.  (Cin = 128: the other instantiation of the data-grad kernel.)"""
    g = torch.Generator(device=DEV).manual_seed(Cin)
    x = torch.randn(3, 10, 10, Cin, device=DEV, generator=g).abs().bfloat16()
    w, gamma, beta = _params(Cin, 4 * Cin, g)
    dz = torch.randn(3, 10, 10, 4 * Cin, device=DEV, generator=g).bfloat16()
    _compare(f"stride1 {Cin}->{4 * Cin}", x, w, gamma, beta, dz)


def test_robust_large_mean_channels():
    """Channels of x at mean / std of 1, 10 and 30 (post-ReLU inputs are non-negative with a large common-mode
    part): the correction diag(b)(W_d G_x) + c s_x^T cancels like E[h^2] - mean^2 unless the Gram pass is
    centred on the pilot shift."""
    Cin, Cout = 64, 256
    g = torch.Generator(device=DEV).manual_seed(7)
    ratio = torch.tensor([1.0, 10.0, 30.0], device=DEV)[torch.arange(Cin, device=DEV) % 3]
    std = 0.5 + torch.rand(Cin, device=DEV, generator=g)
    x = (ratio * std + std * torch.randn(4, 16, 16, Cin, device=DEV, generator=g)).clamp_(min=0).bfloat16()
    w, gamma, beta = _params(Cin, Cout, g)
    dz = torch.randn(4, 16, 16, Cout, device=DEV, generator=g).bfloat16()
    # the pilot is within a fraction of one std of every column mean
    pil = ext().bn_gram_pilot(x)
    xf = x.float().reshape(-1, Cin)
    assert ((pil[2] - xf.mean(0)).abs() <= 0.5 * xf.std(0)).all()
    _compare("mean/std 1,10,30", x, w, gamma, beta, dz)


def test_robust_zero_gamma_and_constant_channel():
    Cin, Cout = 64, 256
    g = torch.Generator(device=DEV).manual_seed(8)
    x = torch.randn(4, 16, 16, Cin, device=DEV, generator=g).abs().bfloat16()
    x[..., 5] = 1.5  # a constant input channel
    w, gamma, beta = _params(Cin, Cout, g)
    gamma[3] = 0.0
    dz = torch.randn(4, 16, 16, Cout, device=DEV, generator=g).bfloat16()
    _compare("gamma = 0 / constant channel", x, w, gamma, beta, dz)


@pytest.mark.parametrize("stride", [1, 2])
def test_deterministic(stride):
    X = ext()
    g = torch.Generator(device=DEV).manual_seed(9)
    Cin = 64 if stride == 1 else 256
    x = torch.randn(3, 10, 10, Cin, device=DEV, generator=g).abs().bfloat16()
    w, gamma, beta = _params(Cin, 256 if stride == 1 else 512, g)
    dz = torch.randn(3, 10 // stride, 10 // stride, w.shape[0], device=DEV, generator=g).bfloat16()
    a = _gram_path(X, x, w, gamma, beta, dz, stride)
    b = _gram_path(X, x, w, gamma, beta, dz, stride)
    for q, t, u in zip(("dW_d", "dgamma_d", "dbeta_d", "dx_d"), a, b):
        assert torch.equal(t, u), q


def test_deterministic_weight_grad_many_splits():
    """P_d at a row count whose weight grad splits K (slab partials summed in split order) and ends mid-step."""
    X = ext()
    g = torch.Generator(device=DEV).manual_seed(10)
    x = torch.randn(5, 30, 30, 64, device=DEV, generator=g).abs().bfloat16()  # M = 4500 = 140 * 32 + 20
    dz = torch.randn(5, 30, 30, 256, device=DEV, generator=g).bfloat16()
    out = []
    for _ in range(2):
        P = torch.full((256, 1, 1, 64), float("nan"), device=DEV)
        X.conv_wgrad(dz, x, P, *CONF, 1.0, None, deterministic=True, overwrite=True)
        out.append(P)
    assert torch.equal(out[0], out[1])
    ref = dz.double().reshape(-1, 256).t() @ x.double().reshape(-1, 64)
    assert _rel(out[0].reshape(256, 64), ref) < 1e-6


# ----------------------------------------------------------------------------- block level
class _Spy:
    """The extension module with every call recorded as (name, args, kwargs, result)."""

    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        f = getattr(self._real, name)
        if not callable(f):
            return f

        def call(*a, **k):
            r = f(*a, **k)
            self.calls.append((name, a, k, r))
            return r

        return call


def _run_blocks(RF, base, x0, gy, bnd, gram=True, spy=False):
    """Forward + backward of the chained blocks (deep copies of ``base``) with the switches set as given:
    (loss, {name: grad}, dx, forward link of block 0, recorded backward calls, output shape)."""
    saved = RF._BND_GRAM, RF._BND_GRAM_S2, RF._GRAM, RF.ext
    rec = _Spy(ext()) if spy else None
    try:
        RF._BND_GRAM, RF._BND_GRAM_S2, RF._GRAM = bnd, bnd, gram  # (DPE_BND_GRAM_S2: the stride-2 form, opt-in)
        blocks = copy.deepcopy(base)
        x = x0.clone().requires_grad_(True)
        h, link, links = x, None, []
        for i, b in enumerate(blocks):
            gn = RF.gram_successor_width(blocks[i + 1]) if i + 1 < len(blocks) else 0
            h, link = b.forward_chained(h, link, gram_next=gn)
            links.append((link.h3 is None, link.gram))
        loss = (h.float() * gy.float()).sum()
        if rec is not None:
            RF.ext = lambda: rec  # (the backward's calls only)
        loss.backward()
        torch.cuda.synchronize()
        grads = {n: p.grad.detach().clone() for n, p in blocks.named_parameters()}
        return loss.item(), grads, x.grad.detach().clone(), links, (rec.calls if rec else None), tuple(h.shape)
    finally:
        RF._BND_GRAM, RF._BND_GRAM_S2, RF._GRAM, RF.ext = saved


def _make_blocks(inplanes, planes, seed, stride=1):
    import torch.nn as nn

    from distributed_pytorch_example_amd.models.resnet import Bottleneck

    torch.manual_seed(seed)
    base = nn.ModuleList([Bottleneck(inplanes, planes, stride, True), Bottleneck(4 * planes, planes, 1, False)]).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(seed + 1)
    x0 = torch.randn(2, 16, 16, inplanes, device=DEV, generator=g).abs().bfloat16()
    gy = torch.randn(2, 16 // stride, 16 // stride, 4 * planes, device=DEV, generator=g).bfloat16()
    return base, x0, gy


@pytest.mark.parametrize("inplanes,planes,stride", [(64, 64, 1), (256, 128, 2)])
def test_blocks_switch_on_vs_off(inplanes, planes, stride):
    """A downsample block then an identity block (N = 2, 16 x 16; widths 64 / 256 at stride 1 and 128 / 512 at
    stride 2, ResNet-50's layer1.0 and layer2.0): loss and every gradient with DPE_BND_GRAM on vs off, bounded per
    tensor by twice the deviation DPE_BN3_GRAM on vs off makes on the same input (measured here)."""
    from distributed_pytorch_example_amd.models import _resnet_fused as RF

    if not RF._GRAM:
        pytest.skip("DPE_BN3_GRAM=0")
    base, x0, gy = _make_blocks(inplanes, planes, 11 + planes, stride)
    l_on, g_on, dx_on, links_on, calls, oshape = _run_blocks(RF, base, x0, gy, True, spy=True)
    l_off, g_off, dx_off, links_off, calls_off, _ = _run_blocks(RF, base, x0, gy, False, spy=True)
    l_ng, g_ng, dx_ng, _, _, _ = _run_blocks(RF, base, x0, gy, False, gram=False)
    # the successor of the downsample block: sum-dz-only partials on the new path (no hd handed over), the
    # (sum dz, sum dz (hd - mean_d)) pair on today's
    assert links_on[0] == (True, True) and links_off[0] == (False, True), (links_on, links_off)
    names = [c[0] for c in calls]
    assert "conv1x1_dgrad_cat_plain" in names and "bn_gram_bwd" in names
    succ = [c for c in calls if c[0] == "conv_dgrad_bn" and tuple(c[1][2]) == oshape]  # its conv1 data grad
    assert len(succ) == 1 and succ[0][1][7] is None and succ[0][1][12] is not None, "successor epilogue: sum dz only"
    dz3 = succ[0][3][0]
    assert tuple(dz3.shape) == oshape
    # no BN backward pass reads dz3 on the new path ...
    assert not [c[0] for c in calls if c[0].startswith("bn_bwd") and c[1][0].data_ptr() == dz3.data_ptr()]

    def made(cs):  # ops that returned a tensor of dz3's (= dhd's) shape and type in backward
        return sorted(c[0] for c in cs for r in (c[3] if isinstance(c[3], (list, tuple)) else [c[3]])
                      if torch.is_tensor(r) and tuple(r.shape) == oshape and r.dtype == torch.bfloat16)

    # ... and exactly one tensor of that shape fewer than today is produced: dhd (the rest: dz3 itself and the
    # last block's own standalone BN3 backward)
    assert made(calls_off) == sorted(made(calls) + ["bn_bwd_partials"]), (made(calls), made(calls_off))
    assert l_on == l_off  # the forward is unchanged
    yard = {n: _rel(g_off[n], g_ng[n]) for n in g_off}
    yard["dx"] = _rel(dx_off, dx_ng)
    dev = {n: _rel(g_on[n], g_off[n]) for n in g_off}
    dev["dx"] = _rel(dx_on, dx_off)
    print(f"\nloss BN3 Gram on/off: {l_off:.6g} / {l_ng:.6g}")
    bad = []
    for n in dev:
        print(f"  {n:24s} BND on vs off {dev[n]:.3e}   BN3 Gram on vs off {yard[n]:.3e}")
        if not dev[n] <= 2 * yard[n]:
            bad.append((n, dev[n], yard[n]))
    assert not bad, bad


def test_blocks_switch_off_is_todays_path_bitwise():
    """DPE_BND_GRAM=0: the downsample branch's gradients are those of bn_bwd_partials(dz3, hd) -> conv_wgrad ->
    conv_dgrad_acc, bit for bit -- the recorded calls replayed as standalone ops in this process."""
    from distributed_pytorch_example_amd.models import _resnet_fused as RF

    if not RF._GRAM:
        pytest.skip("DPE_BN3_GRAM=0")
    X = ext()
    base, x0, gy = _make_blocks(64, 64, 31)
    _, grads, dx, _, calls, oshape = _run_blocks(RF, base, x0, gy, False, spy=True)
    names = [c[0] for c in calls]
    assert not {"bn_gram_pilot", "bn_gram_u", "conv1x1_dgrad_cat_plain"} & set(names)
    (bnb,) = [c for c in calls if c[0] == "bn_bwd_partials" and tuple(c[1][0].shape) == oshape and c[1][1].shape == c[1][0].shape
              and c[2].get("relu_mask") is False]
    dz3, hd, gamma, cd, part = bnb[1][:5]
    dg, db = torch.zeros_like(gamma), torch.zeros_like(gamma)
    dhd = X.bn_bwd_partials(dz3, hd, gamma, cd, part, dg, db, relu_mask=False)
    assert torch.equal(dhd, bnb[3])
    assert torch.equal(dg, grads["0.down.bn.weight"]) and torch.equal(db, grads["0.down.bn.bias"])
    wd = base[0].down.conv.weight
    dw = torch.zeros(wd.shape, dtype=torch.float32, device=DEV)
    X.conv_wgrad(dhd, x0, dw, *CONF, 1.0, None)
    assert torch.equal(dw, grads["0.down.conv.weight"])
    # dx = dh1 . W1, then the downsample branch accumulated in place
    (acc,) = [c for c in calls if c[0] == "conv_dgrad_acc"]
    (d1,) = [c for c in calls if c[0] == "conv_dgrad"]
    dxr = X.conv_dgrad(*d1[1])
    X.conv_dgrad_acc(dhd, acc[1][1], dxr, *acc[1][3:])
    assert torch.equal(dxr, dx)
