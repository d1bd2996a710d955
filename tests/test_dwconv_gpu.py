"""The depthwise 7x7 kernels (csrc/kernels/dwconv.hip) against fp64: bit-exact on integer operands (the indexing
test), within derived rounding budgets on randn operands, bitwise repeatable weight gradients, and the refusals."""
import pytest
import torch

import _dwconv_ref as R
from distributed_pytorch_example_amd.ops import functional as Fx

pytestmark = pytest.mark.gpu
dev = "cuda"
DTYPES = [torch.bfloat16, torch.float32]


def _operands(shape, exact, dtype):
    c = R.case(shape, exact)
    return c, c["x"].to(dev).to(dtype), c["w"].to(dev), c["b"].to(dev), c["dy"].to(dev).to(torch.bfloat16)


def _worst(name, got, ref, bound):
    err = (got.double().cpu() - ref).abs()
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{name}: worst |err| / bound = {ratio:.3f}")
    assert (err <= bound).all(), (name, ratio)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_exact_on_integers(C, shape, dtype):
    """|y| <= 98 + 3: every sum is exact in bf16 and fp32, so all four results equal fp64 bit for bit (through the
    autograd Function: the tap-major and flipped shadows are part of what is tested)."""
    c, x, w, b, dy = _operands(shape, True, dtype)
    x.requires_grad_(), w.requires_grad_(), b.requires_grad_()
    y = Fx.depthwise_conv2d_nhwc(x, w, b)
    assert y.dtype == torch.bfloat16 and y.shape == x.shape
    y.backward(dy)
    assert x.grad.dtype == dtype
    for name, got, ref in (("y", y, c["y"]), ("dx", x.grad, c["dx"]), ("dw", w.grad, c["dw"]), ("db", b.grad, c["db"])):
        assert torch.equal(got.detach().double().cpu(), ref), name


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_rounding_budget(C, shape, dtype):
    c, x, w, b, dy = _operands(shape, False, dtype)
    _worst("y", C.dwconv7_fwd(x, Fx._dw_taps(w), b), c["y"], R.rows_bound(c["y"], c["s_y"]))
    _worst("dx", C.dwconv7_dgrad(dy, Fx._dw_taps_flipped(w)), c["dx"], R.rows_bound(c["dx"], c["s_dx"]))
    dw, db = torch.full_like(w, 7.0), torch.full_like(b, 7.0)  # overwritten, not added to
    C.dwconv7_wgrad(dy, x, dw, db, False)
    _worst("dw", dw, c["dw"], R.wgrad_bound(shape, c["s_dw"]))
    _worst("db", db, c["db"], R.wgrad_bound(shape, c["s_db"]))


@pytest.mark.parametrize("shape", [(2, 30, 14, 40), (2, 56, 56, 96)], ids=str)
def test_wgrad_repeatable_and_accumulating(C, shape):
    c, x, w, b, dy = _operands(shape, False, torch.bfloat16)
    out = [(torch.empty_like(w), torch.empty_like(b)) for _ in range(2)]
    for dw, db in out:
        C.dwconv7_wgrad(dy, x, dw, db, False)
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    g0w, g0b = torch.randn_like(w), torch.randn_like(b)
    gw, gb = g0w.clone(), g0b.clone()
    C.dwconv7_wgrad(dy, x, gw, gb, True)
    for got, g0, fresh in ((gw, g0w, out[0][0]), (gb, g0b, out[0][1])):
        want = g0.double() + fresh.double()  # the same fixed-order sum, then one fp32 rounding
        assert ((got.double() - want).abs() <= 2.0 ** -24 * want.abs()).all()
    C.dwconv7_wgrad(dy, x, gw, None, False)  # no bias gradient wanted
    assert torch.equal(gw, out[0][0])


def test_refusals(C):
    x = torch.zeros(1, 8, 8, 16, device=dev, dtype=torch.bfloat16)
    w49 = torch.zeros(49, 16, device=dev, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        C.dwconv7_fwd(x[..., :12].contiguous(), w49[:, :12].contiguous(), None)
    with pytest.raises(RuntimeError, match="contiguous"):
        C.dwconv7_fwd(x.transpose(1, 2), w49, None)
    with pytest.raises(RuntimeError, match=r"\[49, C\]"):
        C.dwconv7_fwd(x, w49.t().contiguous(), None)
    with pytest.raises(RuntimeError, match="contiguous"):
        C.dwconv7_wgrad(x.transpose(1, 2), x.transpose(1, 2), torch.zeros(16, 1, 7, 7, device=dev), None, False)
