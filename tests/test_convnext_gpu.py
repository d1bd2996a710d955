"""ConvNeXt on the GPU: convnext-test against the CPU fp32 path (the tolerances of
test_vit_gpu.py::test_vit_tiny_gpu_vs_cpu), three AdamW steps, and one convnext-tiny forward / backward."""
import copy

import pytest
import torch

from distributed_pytorch_example_amd.models import get_model
from distributed_pytorch_example_amd.ops import functional as Fx

pytestmark = pytest.mark.gpu
dev = "cuda"


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


def test_convnext_test_gpu_vs_cpu(C):
    torch.manual_seed(4)
    cpu = get_model("convnext-test", layer_scale_init=0.5)  # a layer scale at which the blocks carry signal
    with torch.no_grad():
        for n, p in cpu.named_parameters():
            if n.endswith("bias"):
                p.normal_(0, 0.05)
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
        assert _rel(p.grad.cpu(), gc[n].grad) < 0.1, n


def test_convnext_test_three_adamw_steps(C):
    from distributed_pytorch_example_amd.optim import AdamW

    torch.manual_seed(5)
    m = get_model("convnext-test", layer_scale_init=0.5).to(dev)
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
    assert 1.8 < losses[0] < 2.8 and losses[2] < losses[1] < losses[0]  # ln(10) = 2.30 at initialisation


def test_convnext_tiny_forward_backward(C):
    torch.manual_seed(6)
    m = get_model("convnext-tiny").to(dev)
    logits = m(torch.randn(2, 3, 224, 224, device=dev))
    assert logits.shape == (2, 1000) and torch.isfinite(logits.float()).all()
    loss = Fx.cross_entropy(logits, torch.tensor([3, 7], device=dev))
    loss.backward()
    assert torch.isfinite(loss)
    for n, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
