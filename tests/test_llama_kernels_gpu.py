"""The kernels of csrc/kernels/llama.hip (RoPE, RMSNorm, SwiGLU) against the fp64 references of _llama_ref.py, computed
from the values the kernel reads.  Every check is max |err| / bound <= 1 per element (printed); the bounds are one bf16
output rounding with 2x margin plus an fp32-arithmetic term, stated at each check.

Measured (MI355X, worst |err| / bound over the cases of the test):

    RoPE      y 0.996
    RMSNorm   rstd 0.013   y 0.996   dx 0.981 (bf16 x), 0.007 (fp32 x)   dw 0.238   dw after a second call 0.217
    SwiGLU    u 0.993   dg 0.996   dv 0.995
    (0.98 .. 1.0: the bound is one bf16 output rounding, up to 2^-9 of the value, with 2x margin, as for LayerNorm.)
"""
import pytest
import torch

import _llama_ref as R
from _packed_attn_ref import doc_start_of
from distributed_pytorch_example_amd.ops import functional as Fx
from test_gpt2_kernels_gpu import BF, _bits, _canary, _ratio, _same_bits, dev

pytestmark = pytest.mark.gpu


def _guarded(shape):
    """A bf16 output of ``shape`` (random bits) directly followed by 8 canary rows: (tensor, check(what))."""
    n = torch.Size(shape).numel()
    buf, flat, can = _canary((n // shape[-1] + 8, shape[-1]), BF, n)

    def check(what):
        assert torch.equal(_bits(buf.view(-1)[n:]), can), f"{what} stored past the end of its output"

    return flat.view(shape), check


@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inverse"])
@pytest.mark.parametrize("packed", [False, True], ids=["t", "pos"])
@pytest.mark.parametrize("B,T,Hq,Hkv", [(2, 5, 2, 1), (1, 70, 3, 3), (1, 128, 8, 2)])
def test_rope(C, B, T, Hq, Hkv, packed, inverse):
    """Token tail of a block (B T = 10, 70), head counts 3, 6 and 10 = one clamped trip, a full one, two trips; in
    place and out of place give the same bits, the V heads pass untouched, nothing is stored behind the buffer."""
    W, n_rot = Hq + 2 * Hkv, Hq + Hkv
    x = torch.randn(B, T, W, 64, generator=torch.Generator().manual_seed(T + Hq)).to(BF).to(dev)
    cos, sin = Fx.rope_table(T + 3, device=dev)
    pos = Fx.doc_bounds(doc_start_of(T, [s for s in (3, 64) if s < T]).expand(B, T).to(dev))[2] if packed else None
    rows = pos.long() if packed else torch.arange(T, device=dev).expand(B, T)
    inp, chk_i = _guarded((B, T, W, 64))
    out, chk_o = _guarded((B, T, W, 64))
    inp.copy_(x)
    assert C.rope(inp, cos, sin, pos, n_rot, inverse, out=inp).data_ptr() == inp.data_ptr()
    C.rope(x, cos, sin, pos, n_rot, inverse, out=out)
    torch.cuda.synchronize()
    chk_i("rope (in place)"), chk_o("rope")
    assert _same_bits(inp, out) and _same_bits(out[:, :, n_rot:], x[:, :, n_rot:])
    assert _same_bits(C.rope(x, cos, sin, pos, n_rot, inverse), out)
    ref, bound = R.rope_ref(x, cos, sin, rows, n_rot, inverse)
    print(f"rope B={B} T={T} Hq={Hq} Hkv={Hkv} packed={packed} inverse={inverse}")
    assert _ratio("y", out[:, :, :n_rot], ref, bound) <= 1.0


def test_rope_clamps_the_table_row(C):
    """The table is rows 1 .. P of a buffer whose rows 0 and P + 1 are NaN; positions -1 and P must read rows 0 and
    P - 1 of the table: an unclamped index shows as a NaN, inside the allocation."""
    P = 6
    cos, sin = (torch.full((P + 2, 32), float("nan"), device=dev) for _ in range(2))
    cos[1:P + 1], sin[1:P + 1] = Fx.rope_table(P, device=dev)
    x = torch.randn(1, 2, 3, 64, generator=torch.Generator().manual_seed(1)).to(BF).to(dev).repeat(1, 2, 1, 1)
    pos = torch.tensor([[-1, P, 0, P - 1]], dtype=torch.int32, device=dev)
    y = C.rope(x, cos[1:P + 1], sin[1:P + 1], pos, 2)
    assert torch.isfinite(y.float()).all() and _same_bits(y[:, :2], y[:, 2:])


@pytest.mark.parametrize("bad", ["head_dim", "n_rot", "strided", "T_gt_P"])
def test_rope_refusals(C, bad):
    x = torch.zeros(1, 8, 3, 32 if bad == "head_dim" else 64, dtype=BF, device=dev)
    if bad == "strided":
        x = torch.zeros(1, 8, 6, 64, dtype=BF, device=dev)[:, :, ::2]
    cos, sin = Fx.rope_table(4 if bad == "T_gt_P" else 8, device=dev)
    with pytest.raises(RuntimeError):
        C.rope(x, cos, sin, None, 4 if bad == "n_rot" else 2)


# D: the ends of each chunk count, clamped tail lanes (520, 1016), both sides of the wave / block split (2048, 2056);
# (64, 8200): dpe_rmsnorm_bwd_nblocks saturates at 1024 and a wave walks more than 2 rows
RMS_CASES = [(D, r) for D in (8, 520, 768, 1016, 2048, 2056, 4096, 8192) for r in (5, 333)] + [(64, 8200)]


@pytest.mark.parametrize("x_dt", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("D,rows", RMS_CASES)
def test_rmsnorm(C, D, rows, x_dt):
    g = torch.Generator().manual_seed(D + rows)
    x = (torch.randn(rows, D, generator=g) * 1.5 + 0.3).to(x_dt).to(dev)
    w = (1.0 + 0.5 * torch.randn(D, generator=g)).to(dev)
    dy = torch.randn(rows, D, generator=g).to(BF).to(dev)
    yr, rr, xh, dxr, dwr = R.rms_ref(x, w, dy)
    y, rstd = C.rmsnorm_fwd(x, w, 1e-5)
    dw = torch.zeros(D, device=dev)
    dx = C.rmsnorm_bwd(dy, x, w, rstd, dw)
    dw1 = dw.clone()
    C.rmsnorm_bwd(dy, x, w, rstd, dw)  # accumulates: the same values again
    dw2 = torch.zeros(D, device=dev)
    C.rmsnorm_bwd(dy, x, w, rstd, dw2)
    torch.cuda.synchronize()
    assert y.dtype == BF and dx.dtype == x_dt and _same_bits(dw2, dw1), "dw is not bitwise repeatable"
    with pytest.raises(RuntimeError):  # outside the envelope: an error, never a fallback
        C.rmsnorm_fwd(x[:, :4].contiguous(), w[:4].contiguous(), 1e-5)
    dyd = dy.double()
    bw = 1e-6 * (dyd * xh).abs().sum(0) + R.FLOOR
    # dx, bf16 x: one output rounding (2x margin) of the row's largest element; fp32 x: the row's sum |dy w| rstd
    bx = 2.0 ** -8 * dxr.abs().amax(1) + R.FLOOR if x_dt == BF else 1e-5 * (dyd * w.double()).abs().sum(1) * rr + R.FLOOR
    print(f"rmsnorm D={D} rows={rows} {x_dt}")
    rs = [_ratio("rstd", rstd.double() / rr, torch.ones_like(rr), torch.full_like(rr, 1e-5)),
          _ratio("y", y, yr, 2.0 ** -8 * yr.abs() + 1e-6 * (w.double() * xh).abs() + R.FLOOR),
          _ratio("dx", dx, dxr, bx.unsqueeze(1).expand_as(dxr)),
          _ratio("dw", dw1, dwr, bw),
          _ratio("dw += dw", dw, 2 * dwr, 2 * bw + 2.0 ** -23 * (2 * dwr).abs())]
    assert max(rs) <= 1.0, f"ratios (rstd, y, dx, dw, dw twice) = {rs}"


@pytest.mark.parametrize("M,F", [(3, 8), (5, 1032), (257, 5632)])
def test_swiglu(C, M, F):
    """One thread's two chunks both clamped (3, 8); a partial last block; several blocks with rows that start inside a
    thread's pair.  Gates at 0, -0, +-6, +-30, +-100: a saturated exponent must end in sigma = 0 or 1."""
    g = torch.Generator().manual_seed(M + F)
    gu = (2.0 * torch.randn(M, 2 * F, generator=g)).to(BF)
    gu[0, :8] = torch.tensor([0.0, -0.0, 6.0, -6.0, 30.0, -30.0, 100.0, -100.0]).to(BF)
    gu, du = gu.to(dev), (2.0 * torch.randn(M, F, generator=g)).to(BF).to(dev)
    u, chk_u = _guarded((M, F))
    dgu, chk_d = _guarded((M, 2 * F))
    C.swiglu_fwd(gu, out=u)
    C.swiglu_bwd(du, gu, out=dgu)
    torch.cuda.synchronize()
    chk_u("swiglu_fwd"), chk_d("swiglu_bwd")
    assert _same_bits(C.swiglu_fwd(gu), u) and _same_bits(C.swiglu_bwd(du, gu), dgu)
    ur, dgr, dvr = R.swiglu_ref(gu, du)
    (gd, vd), dd = gu.double().chunk(2, dim=-1), du.double()
    print(f"swiglu M={M} F={F}")
    rs = [_ratio("u", u, ur, 2.0 ** -8 * ur.abs() + 1e-6 * vd.abs().clamp(min=1.0)),
          _ratio("dg", dgu[:, :F], dgr, 2.0 ** -8 * dgr.abs() + 1e-6 * (dd * vd).abs().clamp(min=1.0)),
          _ratio("dv", dgu[:, F:], dvr, 2.0 ** -8 * dvr.abs() + 1e-6 * (dd * gd).abs().clamp(min=1.0))]
    assert max(rs) <= 1.0, f"ratios (u, dg, dv) = {rs}"
