"""Fx.patchify on the GPU (patchify_kernel of eltwise.hip) against the CPU formula: bit for bit after one RNE rounding."""
import pytest
import torch

from distributed_pytorch_example_amd.ops import functional as Fx

pytestmark = pytest.mark.gpu
dev = "cuda"


@pytest.mark.parametrize("shape,p", [((2, 3, 32, 32), 8), ((1, 3, 224, 224), 16)])
def test_patchify_equals_cpu_formula(C, shape, p):
    g = torch.Generator().manual_seed(shape[-1] + p)
    x = torch.randn(*shape, generator=g) * 3.0
    x[0, 0, 0, :4] = torch.tensor([0.0, -0.0, 1.00390625, 1.01171875])  # two RNE ties (to even: down, then up)
    B, Cn, H, W = shape
    want = Fx.patchify(x, p)  # unfold / reshape on the CPU, fp32
    assert want.shape == (B, (H // p) * (W // p), Cn * p * p) and want.dtype == torch.float32
    # the CPU formula, spelled out: row (ty, tx), column (c, py, px)
    ty, tx, c, py, px = 1, 2, 1, 3, 5
    assert want[B - 1, ty * (W // p) + tx, (c * p + py) * p + px] == x[B - 1, c, ty * p + py, tx * p + px]
    got = Fx.patchify(x.to(dev), p)
    assert got.dtype == torch.bfloat16 and got.shape == want.shape and got.is_contiguous()
    assert torch.equal(got.cpu().view(torch.int16), want.to(torch.bfloat16).view(torch.int16))


def test_patchify_refuses_other_patches(C):
    x = torch.randn(1, 3, 24, 24, device=dev)
    with pytest.raises(RuntimeError):
        Fx.patchify(x, 12)  # not a multiple of 8: no 16-B stores
    with pytest.raises(ValueError):
        Fx.patchify(x, 16)  # does not divide the image
