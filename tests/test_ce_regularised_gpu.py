"""Label smoothing and z-loss inside the fused cross-entropy kernels (the REG instantiations of loss.hip) against
fp64 torch: every kernel path, ignored rows, the padding's exact zeros, and the untouched default path."""
import copy

import pytest
import torch

import _ce_reg_ref as R

pytestmark = pytest.mark.gpu
dev = "cuda"
BF = torch.bfloat16

# (B, V, ld, dtype, in place): the smallest shapes that reach every code path
CASES = [
    pytest.param(8, 16, 16, torch.float32, False, id="one-wave-NT64"),
    pytest.param(8, 1000, 1000, torch.float32, False, id="NT128-f32"),
    pytest.param(8, 1000, 1000, BF, False, id="NT128-bf16"),
    pytest.param(8, 1003, 1008, torch.float32, False, id="partial-tail-chunk"),
    pytest.param(8, 1001, 1001, torch.float32, False, id="fallback-ld-odd"),
    pytest.param(4, 50257, 50304, BF, True, id="lm-head-NT1024-MAXC8-inplace"),
]
REGS = [(0.1, 0.0), (0.0, 1e-4), (0.0, 1e-2), (0.1, 1e-4), (0.1, 1e-2)]


def _inputs(B, V, ld, dtype, seed=0):
    """Logits (3 sigma; the padding columns hold finite junk), labels with ignored rows (not only), one label V - 1."""
    g = torch.Generator().manual_seed(1234 + seed + V)
    z = (3.0 * torch.randn(B, ld, generator=g)).to(dtype)
    y = torch.randint(0, V, (B,), generator=g)
    y[0] = V - 1
    y[1] = -100
    if B > 5:
        y[5] = -100
    return z.to(dev), y.to(dev)


def _E0(zf32, y, V, C):
    """The plain kernel's own max-abs gradient error against fp64 plain CE on the same logits (fp32 in and out)."""
    _, d0 = C.cross_entropy_mean(zf32, y, V, False, -100, False)
    _, g0 = R.autograd_ref(zf32.double(), y, V, 0.0, 0.0)
    return (d0.double() - g0).abs().max().item()


@pytest.mark.parametrize("B,V,ld,dtype,inplace", CASES)
def test_regularised_ce_against_fp64(C, B, V, ld, dtype, inplace):
    z, y = _inputs(B, V, ld, dtype)
    z64 = z.double()  # the (bf16-rounded where applicable) logits
    E0 = _E0(z.float().contiguous(), y, V, C)
    bound = R.f32_bound(E0)
    keep = y != -100
    assert 0 < int(keep.sum()) < B
    for eps, lam in REGS:
        loss_ref, g_ref = R.autograd_ref(z64, y, V, eps, lam)
        zin = z.clone()
        out4, d = C.cross_entropy_mean(zin, y, V, dtype == BF, -100, inplace, label_smoothing=eps, z_loss=lam)
        torch.cuda.synchronize()
        assert d.dtype == dtype and (d.data_ptr() == zin.data_ptr()) == inplace
        if not inplace:
            assert torch.equal(zin, z)
        loss_err = abs(out4[2].item() - loss_ref) / abs(loss_ref)
        err = (d.double() - g_ref).abs()
        print(f"CE reg B={B} V={V} ld={ld} {dtype} eps={eps} lam={lam}: E0 {E0:.3e} bound {bound:.3e} "
              f"new max-abs err {err.max().item():.3e} loss rel err {loss_err:.3e}")
        assert loss_err < 1e-4
        if dtype == torch.float32:
            assert err.max().item() <= bound
        else:  # one bf16 rounding of the reference on top of the fp32 bound
            assert bool((err <= 2.0 ** -8 * g_ref.abs() + bound).all()), (err - 2.0 ** -8 * g_ref.abs()).max().item()
        assert d[~keep].float().abs().max().item() == 0.0  # ignored rows: exact zero rows
        if ld > V:
            assert d[:, V:].float().abs().max().item() == 0.0  # the padding: exact zeros, no -eps / V leak


def test_all_rows_ignored(C):
    for V, ld, dtype in ((1000, 1000, torch.float32), (1003, 1008, BF), (1001, 1001, torch.float32)):
        z, _ = _inputs(8, V, ld, dtype)
        y = torch.full((8,), -100, dtype=torch.int64, device=dev)
        out4, d = C.cross_entropy_mean(z, y, V, dtype == BF, -100, False, label_smoothing=0.1, z_loss=1e-2)
        assert out4[2].item() == 0.0 and out4[0].item() == 0.0
        assert d.float().abs().max().item() == 0.0


@pytest.mark.parametrize("B,V,ld", [(8, 16, 16), (8, 1000, 1000)])
def test_the_bound_sees_each_term(C, B, V, ld):
    """A reference with any one term left out misses the fp32 bound (with the measured E0) by 3x at least, and
    the loss bound likewise: the checks above cannot pass with a term missing."""
    z, y = _inputs(B, V, ld, torch.float32)
    bound = R.f32_bound(_E0(z, y, V, C))
    for eps, lam in REGS:
        for drop, (gr, lr) in R.sensitivity(z.double().cpu(), y.cpu(), V, eps, lam, bound).items():
            print(f"V={V} eps={eps} lam={lam} without {drop}: gradient {gr:.1f}x the bound, loss {lr:.1f}x")
            assert gr >= 3.0 and lr >= 3.0, (drop, eps, lam, gr, lr)


@pytest.mark.parametrize("B,V,ld,dtype,inplace", CASES)
def test_default_arguments_are_the_plain_kernel_bitwise(C, B, V, ld, dtype, inplace):
    z, y = _inputs(B, V, ld, dtype, seed=1)
    za, zb = z.clone(), z.clone()
    o1, d1 = C.cross_entropy_mean(za, y, V, dtype == BF, -100, inplace)
    o2, d2 = C.cross_entropy_mean(zb, y, V, dtype == BF, -100, inplace, label_smoothing=0.0, z_loss=0.0)
    assert torch.equal(o1, o2) and torch.equal(d1, d2)


def test_smoothed_loss_is_bitwise_repeatable(C):
    g = torch.Generator().manual_seed(11)
    z = (3.0 * torch.randn(4096, 1000, generator=g)).to(BF).to(dev)
    y = torch.randint(0, 1000, (4096,), generator=g).to(dev)
    losses = [C.cross_entropy_mean(z, y, 1000, True, -100, False, label_smoothing=0.1, z_loss=1e-4)[0][2].item()
              for _ in range(8)]
    assert len(set(losses)) == 1, losses


def test_argument_validation(C):
    z, y = _inputs(8, 16, 16, torch.float32)
    for kw in (dict(label_smoothing=1.0), dict(label_smoothing=-0.1), dict(z_loss=-1e-3)):
        with pytest.raises(RuntimeError):
            C.cross_entropy_mean(z, y, 16, False, -100, False, **kw)


def test_functional_and_module_autograd(C):
    """Fx.cross_entropy / CrossEntropyLoss: loss and the gradient autograd hands back (the 1 / count included)."""
    from distributed_pytorch_example_amd.ops import functional as Fx
    from distributed_pytorch_example_amd.ops.layers import CrossEntropyLoss

    z, y = _inputs(8, 1003, 1008, torch.float32)
    n = int((y != -100).sum())
    loss_ref, g_ref = R.autograd_ref(z.double(), y, 1003, 0.1, 1e-2)
    zz = z.clone().requires_grad_(True)
    loss = Fx.cross_entropy(zz, y, 1003, label_smoothing=0.1, z_loss=1e-2)
    (2.0 * loss).backward()
    assert abs(loss.item() - loss_ref) < 1e-4 * abs(loss_ref)
    # the kernel's bound scaled by 2 / n, plus the fp32 rounding of that scaling
    bound = 2.0 / n * R.f32_bound(_E0(z, y, 1003, C))
    assert bool(((zz.grad.double() - 2.0 * g_ref / n).abs() <= bound + 2.0 ** -22 * (2.0 * g_ref / n).abs()).all())
    zz = z[:, :1003].contiguous().requires_grad_(True)
    loss = CrossEntropyLoss(label_smoothing=0.1, z_loss=1e-2)(zz, y)
    assert abs(loss.item() - loss_ref) < 1e-4 * abs(loss_ref)


def test_gpt2_tiny_lm_head_ce_regularised(C):
    """GPT2Config.tiny() with label_smoothing 0.1 and z_loss 1e-2, B = 2, T = 128: model(idx, targets) (the fused
    LM head + in-place regularised CE) against the per-op logits + the fp64 formula, within the bounds the
    unregularised pair is held to (test_models_gpu.test_gpt2_fused_lm_head_ce)."""
    from distributed_pytorch_example_amd.models import get_model

    def rel(a, b):
        return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()

    def cos(a, b):
        a, b = a.float().flatten(), b.float().flatten()
        return (a @ b / (a.norm() * b.norm() + 1e-12)).item()

    eps, lam = 0.1, 1e-2
    torch.manual_seed(7)
    m1 = get_model("gpt2-tiny").to(dev)
    m2 = get_model("gpt2-tiny", label_smoothing=eps, z_loss=lam).to(dev)
    m2.load_state_dict(copy.deepcopy(m1.state_dict()))
    assert m2.cfg.label_smoothing == eps and m2.cfg.z_loss == lam
    idx = torch.randint(0, 512, (2, 128), device=dev)
    tgt = torch.randint(0, 512, (2, 128), device=dev)
    tgt[0, :7] = -100
    logits = m1(idx)
    z64 = logits.double().reshape(-1, logits.shape[-1])
    y = tgt.reshape(-1)
    keep = y != -100
    l1 = torch.nn.functional.cross_entropy(z64[:, :512], y, label_smoothing=eps, ignore_index=-100) \
        + lam * (torch.logsumexp(z64[:, :512], dim=1).square() * keep).sum() / keep.sum()
    (3.0 * l1).backward()
    l2 = m2(idx, tgt)
    (3.0 * l2).backward()
    assert abs(l1.item() - l2.item()) < 1e-3 * abs(l1.item())
    l_plain = torch.nn.functional.cross_entropy(z64[:, :512].detach(), y, ignore_index=-100).item()
    assert abs(l_plain - l1.item()) > 1e-2 * abs(l1.item())  # the regularisers are well above that bound
    g1 = dict(m1.named_parameters())
    for n, p in m2.named_parameters():  # wte.grad, and through x.grad everything below the head
        assert cos(p.grad, g1[n].grad) > 0.999, n
        assert rel(p.grad, g1[n].grad) < 0.02, n
