"""optim.Muon has no GPU kernels yet: on GPU parameters a step is an error, not a quiet fall-back to eager torch
ops, and it touches nothing."""
import pytest
import torch

pytestmark = pytest.mark.gpu
dev = "cuda"


def test_a_gpu_step_raises_and_changes_nothing(C):
    from distributed_pytorch_example_amd.optim import Muon, build_optimizer

    torch.manual_seed(0)
    w = torch.randn(64, 128, device=dev, requires_grad=True)
    b = torch.randn(128, device=dev, requires_grad=True)
    w.grad, b.grad = torch.randn_like(w), torch.randn_like(b)
    w0, b0 = w.detach().clone(), b.detach().clone()
    opt = build_optimizer("muon", [w, b], lr=0.02, weight_decay=0.01)
    assert isinstance(opt, Muon) and [g["use_muon"] for g in opt.param_groups] == [True, False]
    with pytest.raises(NotImplementedError, match="no GPU kernels"):
        opt.step()
    torch.cuda.synchronize()
    assert torch.equal(w.detach(), w0) and torch.equal(b.detach(), b0)
    assert len(opt.state) == 0
