"""Bidirectional attention with a key-length bound (the BIDIR instantiations of the three LDS-DMA kernels of
attn.hip, reached with causal=False and seq_len=L) against the fp64 reference of tests/_bidir_attn_ref.py.  As in
test_gpt2_kernels_gpu.py every check is per element, every bound is the project's rounding budget evaluated on the
reference, and a test passes when max |err| / bound <= 1 and prints that worst ratio.  Besides the bounds: rows >= L
of out and dqkv are zero bits, nothing is stored past a buffer, and nothing at or past row L of qkv or dout reaches
an output bit.

Measured (MI355X, worst |err| / bound over all cases of the test; 1.0 = at the bound):

                                          out    lse2   dQ     dK     dV
      the eight shapes                    0.404  0.194  0.077  0.074  0.281
        of them (1, 64, 1, L 1)           0.000  0.000  0.000  0.000  0.000   (one key: P = 1, every value exact)
      pad independence (both fills)       0.412  0.255  0.097  0.089  0.346
      rescale staircase, L 197            0.563  0.484  0.108  0.037  0.139
      independence (3, 128, 5, L 100)     0.377  0.201  0.071  0.068  0.248
    torch fallback (Tp 100; D 32)         0.347  -      dqkv 0.207
    (no budget is exceeded: C_LSE and C_DV of _gpt2_ref.py stay as they are)
"""
import math

import pytest
import torch

import _bidir_attn_ref as BR
import _gpt2_ref as R
from distributed_pytorch_example_amd.ops import functional as Fx
from test_gpt2_kernels_gpu import _Staged, _attn_check, _bits, _canary, _ratio, _same_bits

pytestmark = pytest.mark.gpu
dev = "cuda"
BF = torch.bfloat16
SCALE = 0.125  # 1 / sqrt(64)


def _run(C, qkv, dout, L, guard=False):
    """attn_fwd + attn_bwd with causal=False, seq_len=L; ``guard``: the canary rows of
    test_gpt2_kernels_gpu._attn_run behind every output must come back bit-unchanged."""
    B, T, _, H, D = qkv.shape
    if not guard:
        out, lse = C.attn_fwd(qkv, H, SCALE, False, seq_len=L)
        dqkv = C.attn_bwd(qkv, out, dout, lse, H, SCALE, False, seq_len=L)
        torch.cuda.synchronize()
        return out, lse, dqkv
    bo, fo, co = _canary((B, T + 128, H, D), BF, B * T * H * D)
    bl, fl, cl = _canary((B, H, T + 128), torch.float32, B * H * T)
    bd, fd, cd = _canary((B, T + 128, 3, H, D), BF, B * T * 3 * H * D)
    out, lse, dqkv = fo.view(B, T, H, D), fl.view(B, H, T), fd.view(B, T, 3, H, D)
    C.attn_fwd(qkv, H, SCALE, False, out=out, lse=lse, seq_len=L)
    C.attn_bwd(qkv, out, dout, lse, H, SCALE, False, dqkv=dqkv, seq_len=L)
    torch.cuda.synchronize()
    assert torch.equal(_bits(bo.view(-1)[fo.numel():]), co), "attn_fwd stored past the end of out"
    assert torch.equal(_bits(bl.view(-1)[fl.numel():]), cl), "attn_fwd stored past the end of lse"
    assert torch.equal(_bits(bd.view(-1)[fd.numel():]), cd), "attn_bwd stored past the end of dqkv"
    return out, lse, dqkv


def _case(B, T, H, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, T, 3, H, 64, generator=g).to(BF).to(dev)
    dout = torch.randn(B, T, H, 64, generator=g).to(BF).to(dev)
    return qkv, dout


def _zero_rows(got, L):
    out, lse, dqkv = got
    assert not _bits(out[:, L:]).any(), "out rows >= L are not zero bits"
    assert not _bits(dqkv[:, L:]).any(), "dqkv rows >= L are not zero bits"
    assert torch.isfinite(lse).all(), "lse2 holds a non-finite value"


# (B, Tp, H, L): one full tile; one key; wave 0 straddles L with waves 1-3 and the second key tile dead; one key in the
# tail tile; no tail; Tp % 128 == 64 plus a tail; the ViT shape; two query workgroups and a tail
SHAPES = [(1, 64, 1, 64), (1, 64, 1, 1), (1, 128, 1, 17), (2, 128, 2, 65), (1, 128, 2, 128), (1, 192, 2, 129),
          (1, 256, 2, 197), (2, 320, 2, 300)]


@pytest.mark.parametrize("B,T,H,L", SHAPES)
def test_bidir_shapes(C, B, T, H, L):
    """The budgets, the zero rows and the canary rows behind every output, at every tile / wave arrangement of L."""
    qkv, dout = _case(B, T, H, 1000 + 7 * T + L)
    ref = BR.bidir_attn_ref(qkv, dout, SCALE, L)
    got = _run(C, qkv, dout, L, guard=True)
    _zero_rows(got, L)
    _attn_check(f"bidir B={B} T={T} H={H} L={L}", got, ref)


@pytest.mark.parametrize("B,T,H,L", [(2, 256, 2, 197), (1, 128, 2, 17), (1, 192, 1, 65)])
def test_bidir_pad_independence(C, B, T, H, L):
    """Rows >= L of qkv and dout reach no output bit.  Base: the padding keys are 16x larger, so the masked scores
    of the tail tile overflow the exp2 before the select (asserted on the fp64 scores: they exceed the rows' lse2
    by more than 64); then every padding row of qkv and dout is refilled with other values, 16x larger.  Both runs
    are finite and within the bounds, and bit-identical."""
    qkv, dout = _case(B, T, H, 77 + L)
    qkv[:, L:, 1] *= 16
    ref = BR.bidir_attn_ref(qkv, dout, SCALE, L)
    tail_end = (L + 63) // 64 * 64  # the padding keys the kernels load: the rest of the tail tile
    q, k = qkv[:, :L, 0].double(), qkv[:, L:tail_end, 1].double()
    s_masked = SCALE * R.LOG2E * torch.einsum("bihd,bjhd->bhij", q, k)
    assert (s_masked.amax() - ref["lse2"][..., :L].amin()).item() > 64, "masked scores are not large"
    got = _run(C, qkv, dout, L)
    for t in got:
        assert torch.isfinite(t.float()).all()
    _zero_rows(got, L)
    _attn_check(f"pad independence L={L} (base)", got, ref)
    qkv2, dout2 = qkv.clone(), dout.clone()
    o2, d2 = _case(B, T, H, 78 + L)
    qkv2[:, L:], dout2[:, L:] = o2[:, L:] * 16, d2[:, L:] * 16
    got2 = _run(C, qkv2, dout2, L)
    for t in got2:
        assert torch.isfinite(t.float()).all()
    for name, a, b in zip(("out", "lse2", "dqkv"), got, got2):
        assert _same_bits(a, b), f"{name} depends on the rows >= L"
    _attn_check(f"pad independence L={L} (refilled)", got2, BR.bidir_attn_ref(qkv2, dout2, SCALE, L))


def test_bidir_rescale_staircase(C):
    """Scores that step up once per 64-key tile, under the bidirectional mask with L = 197 (three full tiles and a
    tail).  Head 0: the a_hi rows' tile maximum rises by more than 2^8 at later tiles (the rescale branch), the a = 0
    rows of the same wave do not.  Head 1: rises inside (4, 8): deferred.  Both asserted on the fp64 scores, for the
    rows < L, before the kernel runs."""
    T, L = 256, 197
    qkv, a = R.staircase_qkv(T, (12.0, 6.5))
    g = torch.Generator().manual_seed(7)
    dout = torch.randn(1, T, 2, 64, generator=g).to(BF).to(dev)
    qkv = qkv.to(dev)
    hi = (a > 0).to(dev)[:L]
    tm = BR.bidir_tile_row_max(qkv, SCALE, L)[0][:, :L]  # [H, L, tiles]
    assert torch.isfinite(tm).all()  # every row < L sees a key of every tile, the tail included
    jump = tm[..., 1:] - tm[..., :-1]
    later, defer, dist = R.deferred_max_trace(tm)
    assert dist.min().item() > 0.25, "a branch decision sits too close to the threshold to be predicted in fp64"
    assert (jump[0][hi] > 8).sum(-1).max().item() >= 2 and not (jump[0][~hi] > 8).any()
    j1 = jump[1][hi]
    assert ((j1 > 4) & (j1 < 8)).any() and not (jump[1] > 8).any()
    assert later[0][hi].max().item() >= 2 and later[0][~hi].max().item() == 0
    assert 4 < defer[1][hi].max().item() < 8  # P up to 2^defer accumulated under the old maximum
    ref = BR.bidir_attn_ref(qkv, dout, SCALE, L)
    got = _run(C, qkv, dout, L, guard=True)
    _zero_rows(got, L)
    _attn_check("bidir staircase", got, ref)


def test_bidir_batch_head_independence(C):
    """Permuting the batch and head axes of the inputs permutes the outputs, bitwise."""
    B, T, H, L = 3, 128, 5, 100
    qkv, dout = _case(B, T, H, 41)
    pb, ph = torch.tensor([2, 0, 1], device=dev), torch.tensor([3, 0, 4, 1, 2], device=dev)
    got = _run(C, qkv, dout, L)
    _attn_check("bidir independence base", got, BR.bidir_attn_ref(qkv, dout, SCALE, L))
    out_p, lse_p, dqkv_p = _run(C, qkv[pb][:, :, :, ph].contiguous(), dout[pb][:, :, ph].contiguous(), L)
    assert _same_bits(out_p, got[0][pb][:, :, ph])
    assert _same_bits(lse_p, got[1][pb][:, ph])
    assert _same_bits(dqkv_p, got[2][pb][:, :, :, ph])


def test_bidir_determinism(C):
    """Identical inputs, identical bits, forward and backward."""
    qkv, dout = _case(2, 192, 3, 51)
    a, b = _run(C, qkv, dout, 150), _run(C, qkv, dout, 150)
    for x, y in zip(a, b):
        assert _same_bits(x, y)


def test_bidir_default_seq_len_is_T(C):
    """seq_len = 0 (the default) is L = T."""
    qkv, dout = _case(1, 128, 2, 61)
    out, lse = C.attn_fwd(qkv, 2, SCALE, False)
    dqkv = C.attn_bwd(qkv, out, dout, lse, 2, SCALE, False)
    for x, y in zip((out, lse, dqkv), _run(C, qkv, dout, 128)):
        assert _same_bits(x, y)


def test_bidir_refusals(C):
    """What the mode does not take is an error, not a fallback."""
    B, T, H = 1, 128, 2
    qkv, dout = _case(B, T, H, 71)
    ds = torch.zeros(B, T, dtype=torch.int32, device=dev)
    de = torch.full((B, T), T, dtype=torch.int32, device=dev)
    rng = torch.zeros(2, dtype=torch.int64, device=dev)
    out, lse = C.attn_fwd(qkv, H, SCALE, False, seq_len=100)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError):
        C.attn_fwd(qkv, H, SCALE, False, doc_start=ds, doc_end=de, seq_len=100)
    with pytest.raises(RuntimeError):
        C.attn_bwd(qkv, out, dout, lse, H, SCALE, False, doc_start=ds, doc_end=de, seq_len=100)
    with pytest.raises(RuntimeError):
        C.attn_fwd(qkv, H, SCALE, False, dropout_p=0.1, rng=rng, seq_len=100)
    with pytest.raises(RuntimeError):
        C.attn_bwd(qkv, out, dout, lse, H, SCALE, False, dropout_p=0.1, rng=rng, seq_len=100)
    with _Staged(C, True):
        with pytest.raises(RuntimeError):
            C.attn_fwd(qkv, H, SCALE, False, seq_len=100)
        with pytest.raises(RuntimeError):
            C.attn_bwd(qkv, out, dout, lse, H, SCALE, False, seq_len=100)
    with pytest.raises(RuntimeError):
        C.attn_fwd(qkv, H, SCALE, True, seq_len=100)
    with pytest.raises(RuntimeError):
        C.attn_bwd(qkv, out, dout, lse, H, SCALE, True, seq_len=100)
    with pytest.raises(RuntimeError):
        C.attn_fwd(qkv, H, SCALE, False, seq_len=T + 1)
    torch.cuda.synchronize()


@pytest.mark.parametrize("L", [197, 256])
def test_fx_attention_runs_the_kernels(C, L):
    """Fx.attention on the GPU at a kernel shape: the autograd Function gives what the direct calls give, bit for bit."""
    B, T, H = 2, 256, 2
    qkv, dout = _case(B, T, H, 81)
    x = qkv.view(B, T, 3 * H * 64).clone().requires_grad_(True)
    out = Fx.attention(x, H, L)
    out.backward(dout.view(B, T, H * 64))
    want = _run(C, qkv, dout, L)
    assert _same_bits(out.detach().view(B, T, H, 64), want[0])
    assert _same_bits(x.grad.view(B, T, 3, H, 64), want[2])


@pytest.mark.parametrize("T,D,L", [(100, 64, 77), (128, 32, 128), (128, 32, 70)])
def test_fx_attention_fallback_shapes(C, T, D, L):
    """Fx.attention on the GPU for Tp % 64 != 0 or head dim != 64: the torch path, autograd through it, under the same
    budgets (its only roundings are the bf16 outputs), with the same zero rows."""
    B, H = 2, 3
    g = torch.Generator().manual_seed(70 + T + D)
    qkv = torch.randn(B, T, 3 * H * D, generator=g).to(BF).to(dev).requires_grad_(True)
    dout = torch.randn(B, T, H * D, generator=g).to(BF).to(dev)
    out = Fx.attention(qkv, H, L)
    assert out.shape == (B, T, H * D) and out.dtype == BF
    out.backward(dout)
    ref = BR.bidir_attn_ref(qkv.detach().view(B, T, 3, H, D), dout.view(B, T, H, D), 1.0 / math.sqrt(D), L)
    print(f"bidir fallback T={T} D={D} L={L}")
    assert _ratio("out", out.detach().view(B, T, H, D), ref["out"], ref["b_out"]) <= 1.0
    assert _ratio("dqkv", qkv.grad.view(B, T, 3, H, D), ref["dqkv"], ref["b_dqkv"]) <= 1.0
    assert not _bits(out.detach()[:, L:]).any() and not _bits(qkv.grad[:, L:]).any()
