"""The two-label (MIX) arm of the fused cross-entropy kernels against fp64: every kernel path of the image-sized rows,
scalar and per-row weights, ignored rows, rows without partner, y == y2, and w = 1 bitwise the one-label call."""
import pytest
import torch

import _ce_reg_ref as P
import _mix_ref as R

pytestmark = pytest.mark.gpu
dev = "cuda"
BF = torch.bfloat16

# (B, V, ld, dtype): the first five shapes of test_ce_regularised_gpu.CASES and the 10-class row of SimpleNet /
# resnet_tiny, which takes ce_kernel (ld = 10 is no multiple of 8)
CASES = [
    pytest.param(8, 16, 16, torch.float32, id="one-wave-NT64"),
    pytest.param(8, 1000, 1000, torch.float32, id="NT128-f32"),
    pytest.param(8, 1000, 1000, BF, id="NT128-bf16"),
    pytest.param(8, 1003, 1008, torch.float32, id="partial-tail-chunk"),
    pytest.param(8, 1001, 1001, torch.float32, id="fallback-ld-odd"),
    pytest.param(8, 10, 10, torch.float32, id="ten-classes-ce_kernel"),
]
REGS = [(0.0, 0.0), (0.1, 0.0), (0.1, 1e-4)]
WS = [0.2, 0.5, 0.8]


def _inputs(B, V, ld, dtype, seed=0):
    """Logits (3 sigma; finite junk in the padding), labels with an ignored row, labels V - 1 and 0, a row whose
    second label is ignored (no partner), a row with y == y2, and a row ignored by its first label only."""
    g = torch.Generator().manual_seed(4321 + seed + V)
    z = (3.0 * torch.randn(B, ld, generator=g)).to(dtype)
    y = torch.randint(0, V, (B,), generator=g)
    y2 = torch.randint(0, V, (B,), generator=g)
    y[0], y2[0] = V - 1, 0
    y[1] = -100                 # ignored (whatever y2 says)
    y2[2] = -100                # no partner
    y2[3] = y[3]                # the two label terms add
    y[4], y2[4] = 0, V - 1
    y[5], y2[5] = -100, -100
    return z.to(dev), y.to(dev), y2.to(dev)


def _E0(zf32, y, V, C):
    """The plain kernel's own max-abs gradient error against fp64 plain CE on the same logits (fp32 in and out)."""
    _, d0 = C.cross_entropy_mean(zf32, y, V, False, -100, False)
    _, g0 = P.autograd_ref(zf32.double(), y, V, 0.0, 0.0)
    return (d0.double() - g0).abs().max().item()


def _weights(w, B, per_row):
    if not per_row:
        return torch.tensor([w], dtype=torch.float32, device=dev)
    g = torch.Generator().manual_seed(int(w * 100))
    return (w + 0.2 * (torch.rand(B, generator=g) - 0.5)).float().to(dev)  # around w, different in every row


@pytest.mark.parametrize("per_row", [False, True], ids=["scalar-w", "per-row-w"])
@pytest.mark.parametrize("B,V,ld,dtype", CASES)
def test_two_label_ce_against_fp64(C, B, V, ld, dtype, per_row):
    z, y, y2 = _inputs(B, V, ld, dtype)
    z64 = z.double()
    E0 = _E0(z.float().contiguous(), y, V, C)
    bound = R.mix_bound(E0)
    keep = y != -100
    for eps, zl in REGS:
        for w in WS:
            wt = _weights(w, B, per_row)
            loss_ref, g_ref = R.ce_autograd_ref(z64, y, y2, wt.double(), V, eps, zl)
            zin = z.clone()
            out4, d = C.cross_entropy_mean(zin, y, V, dtype == BF, -100, False, label_smoothing=eps, z_loss=zl,
                                           labels2=y2, mix_w=wt)
            torch.cuda.synchronize()
            assert d.dtype == dtype and torch.equal(zin, z)
            loss_err = abs(out4[2].item() - loss_ref) / abs(loss_ref)
            err = (d.double() - g_ref).abs()
            print(f"CE mix B={B} V={V} ld={ld} {dtype} eps={eps} zl={zl} w={w} per_row={per_row}: E0 {E0:.3e} "
                  f"bound {bound:.3e} max-abs err {err.max().item():.3e} loss rel err {loss_err:.3e}")
            assert loss_err < 1e-4
            if dtype == torch.float32:
                assert err.max().item() <= bound
            else:  # one bf16 rounding of the reference on top of the fp32 bound
                assert bool((err <= 2.0 ** -8 * g_ref.abs() + bound).all()), (err - 2.0 ** -8 * g_ref.abs()).max().item()
            assert abs(out4[3].item() * int(keep.sum()) - 1.0) < 1e-6  # the count follows labels alone
            assert d[~keep].float().abs().max().item() == 0.0
            if ld > V:
                assert d[:, V:].float().abs().max().item() == 0.0


@pytest.mark.parametrize("B,V,ld", [(8, 16, 16), (8, 1000, 1000), (8, 10, 10)])
def test_the_bound_sees_the_partner_term(C, B, V, ld):
    """The reference without the partner term misses the gradient bound (with the measured E0) by 3x at least at every
    tested w: the check above cannot pass with the term missing."""
    z, y, y2 = _inputs(B, V, ld, torch.float32)
    bound = R.mix_bound(_E0(z, y, V, C))
    for eps, zl in REGS:
        for w in WS:
            wt = torch.tensor([w], dtype=torch.float64)
            _, g = R.ce_formula_ref(z.double().cpu(), y.cpu(), y2.cpu(), wt, V, eps, zl)
            _, gd = R.ce_formula_ref(z.double().cpu(), y.cpu(), y2.cpu(), wt, V, eps, zl, drop="partner")
            ratio = (g - gd).abs().max().item() / bound
            print(f"V={V} eps={eps} zl={zl} w={w}: without the partner term {ratio:.3g}x the bound")
            assert ratio >= 3.0


@pytest.mark.parametrize("B,V,ld,dtype", CASES)
def test_weight_one_is_the_one_label_call_bitwise(C, B, V, ld, dtype):
    z, y, y2 = _inputs(B, V, ld, dtype, seed=1)
    for eps, zl in REGS:
        o1, d1 = C.cross_entropy_mean(z.clone(), y, V, dtype == BF, -100, False, label_smoothing=eps, z_loss=zl)
        for wt in (torch.ones(1, device=dev), torch.ones(B, device=dev)):
            o2, d2 = C.cross_entropy_mean(z.clone(), y, V, dtype == BF, -100, False, label_smoothing=eps, z_loss=zl,
                                          labels2=y2, mix_w=wt)
            assert torch.equal(o1, o2) and torch.equal(d1, d2), (eps, zl, wt.numel())
    # no partner anywhere: any weight is the one-label call
    none = torch.full_like(y2, -100)
    o1, d1 = C.cross_entropy_mean(z.clone(), y, V, dtype == BF, -100, False, label_smoothing=0.1)
    o2, d2 = C.cross_entropy_mean(z.clone(), y, V, dtype == BF, -100, False, label_smoothing=0.1, labels2=none,
                                  mix_w=torch.full((1,), 0.3, device=dev))
    assert torch.equal(o1, o2) and torch.equal(d1, d2)


def test_argument_validation(C):
    z, y, y2 = _inputs(8, 16, 16, torch.float32)
    w = torch.tensor([0.5], device=dev)
    bad = [dict(labels2=y2), dict(mix_w=w), dict(labels2=y2, mix_w=w.cpu()), dict(labels2=y2[:4], mix_w=w),
           dict(labels2=y2, mix_w=torch.ones(3, device=dev)), dict(labels2=y2.int(), mix_w=w),
           dict(labels2=y2, mix_w=w.double())]
    for kw in bad:
        with pytest.raises(RuntimeError):
            C.cross_entropy_mean(z, y, 16, False, -100, False, **kw)


def test_functional_autograd(C):
    """Fx.cross_entropy with two labels: loss and the gradient autograd hands back for loss * 2 (the 1 / count
    included), the weight being a view of a decision row."""
    from distributed_pytorch_example_amd.ops import functional as Fx

    z, y, y2 = _inputs(8, 1003, 1008, torch.float32)
    n = int((y != -100).sum())
    row = torch.tensor([1.0, 0.3, 0, 0, 0, 0, 2, 0.3], device=dev)
    loss_ref, g_ref = R.ce_autograd_ref(z.double(), y, y2, row[1:2].double(), 1003, 0.1, 1e-4)
    zz = z.clone().requires_grad_(True)
    loss = Fx.cross_entropy(zz, y, 1003, label_smoothing=0.1, z_loss=1e-4, labels2=y2, mix_w=row[1:2])
    (loss * 2.0).backward()
    assert abs(loss.item() - loss_ref) < 1e-4 * abs(loss_ref)
    bound = 2.0 / n * R.mix_bound(_E0(z, y, 1003, C))
    assert bool(((zz.grad.double() - 2.0 * g_ref / n).abs() <= bound + 2.0 ** -22 * (2.0 * g_ref / n).abs()).all())
    with pytest.raises(ValueError):
        Fx.cross_entropy(zz, y, 1003, labels2=y2)
    with pytest.raises(TypeError):
        Fx.cross_entropy(zz, y, 1003, labels2=y2, mix_w=0.3)
