"""ViT on the GPU: vit-tiny against the CPU path, the fused blocks against the per-op blocks, a few optimizer steps, and
one vit-s16 forward / backward (197 tokens in 256 rows)."""
import copy

import pytest
import torch

from distributed_pytorch_example_amd.models import get_model
from distributed_pytorch_example_amd.ops import functional as Fx

pytestmark = pytest.mark.gpu
dev = "cuda"


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


def _cos(a, b):
    a, b = a.float().flatten(), b.float().flatten()
    return (a @ b / (a.norm() * b.norm() + 1e-12)).item()


def _perturbed_tiny(seed):
    """vit-tiny with biases and gains moved off their 0 / 1 initial values, so every term carries signal."""
    torch.manual_seed(seed)
    m = get_model("vit-tiny")
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("bias"):
                p.normal_(0, 0.05)
            elif p.ndim == 1:
                p.add_(0.1 * torch.randn_like(p))
    return m


def test_vit_tiny_gpu_vs_cpu(C):
    """The tolerances of test_models_gpu.py::test_gpt2_tiny_gpu_vs_cpu."""
    cpu = _perturbed_tiny(4)
    gpu = copy.deepcopy(cpu).to(dev)
    x = torch.randn(8, 3, 32, 32)
    tgt = torch.randint(0, 10, (8,))
    lc = Fx.cross_entropy(cpu(x), tgt)
    lc.backward()
    lg = Fx.cross_entropy(gpu(x.to(dev)), tgt.to(dev))
    lg.backward()
    assert abs(lc.item() - lg.item()) < 2e-2 * abs(lc.item())
    gc = dict(cpu.named_parameters())
    for n, p in gpu.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
        assert _cos(p.grad.cpu(), gc[n].grad) > 0.98, n
        assert _rel(p.grad.cpu(), gc[n].grad) < 0.1, n


def test_vit_fused_blocks_match_per_op(C):
    """BlockFn in the bidirectional mode == the per-op graph through Fx.attention, on the same weights (the tolerances
    of test_models_gpu.py::test_gpt2_fused_lm_head_ce)."""
    m1 = _perturbed_tiny(7).to(dev)
    m2 = copy.deepcopy(m1)
    for b in m1.blocks:
        b.fused = True
    for b in m2.blocks:
        b.fused = False
    x = torch.randn(8, 3, 32, 32, device=dev)
    tgt = torch.randint(0, 10, (8,), device=dev)
    l1 = Fx.cross_entropy(m1(x), tgt)
    (3.0 * l1).backward()
    l2 = Fx.cross_entropy(m2(x), tgt)
    (3.0 * l2).backward()
    assert abs(l1.item() - l2.item()) < 1e-3 * abs(l1.item())
    g1 = dict(m1.named_parameters())
    for n, p in m2.named_parameters():
        assert _cos(p.grad, g1[n].grad) > 0.999, n
        assert _rel(p.grad, g1[n].grad) < 0.02, n


def test_vit_tiny_three_adamw_steps(C):
    from distributed_pytorch_example_amd.optim import AdamW

    torch.manual_seed(5)
    m = get_model("vit-tiny").to(dev)
    opt = AdamW(m.parameters(), lr=1e-3, weight_decay=0.05)
    x = torch.randn(16, 3, 32, 32, device=dev)
    tgt = torch.randint(0, 10, (16,), device=dev)
    losses = []
    for _ in range(3):
        loss = Fx.cross_entropy(m(x), tgt)
        loss.backward()
        opt.step()
        for p in m.parameters():
            p.grad = None
        losses.append(loss.item())
    assert all(torch.isfinite(torch.tensor(losses)))
    assert 1.8 < losses[0] < 2.8 and losses[2] < losses[1] < losses[0]  # ln(10) = 2.30 at initialisation


def test_vit_tiny_eval_forward_matches_training_forward(C):
    """Without grad the blocks leave the fused path (Fx.attention's Function runs the same kernels)."""
    m = _perturbed_tiny(9).to(dev)
    x = torch.randn(4, 3, 32, 32, device=dev)
    a = m(x)
    with torch.no_grad():
        b = m(x)
    assert _rel(a, b) < 0.02


def test_vit_s16_forward_backward(C):
    torch.manual_seed(6)
    m = get_model("vit-s16").to(dev)
    assert sum(p.numel() for p in m.parameters()) == 22050664
    x = torch.randn(2, 3, 224, 224, device=dev)
    logits = m(x)
    assert logits.shape == (2, 1000) and torch.isfinite(logits.float()).all()
    Fx.cross_entropy(logits, torch.tensor([3, 7], device=dev)).backward()
    for n, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
        assert p.grad.abs().max().item() > 0, n
