"""Edge-case tests of the GPT-2 kernels (attn.hip, loss.hip, norm.hip, the embedding / elementwise kernels
of eltwise.hip) against the fp64 references of tests/_gpt2_ref.py.  Every reference is computed from the
values the kernel sees (bf16-rounded where the kernel reads bf16); every check is per element or per row --
none uses a whole-tensor norm.  Each bound is a rounding budget evaluated on the reference (see _gpt2_ref.py
and the comment at each check); a test passes when max |err| / bound <= 1 and prints that worst ratio.

Measured (MI355X, worst |err| / bound over all cases of the test; 1.0 = at the bound):

    attention (LDS-DMA kernels)      out    lse2   dQ     dK     dV
      tails                          0.522  0.359  0.130  0.250  0.542
      rescale staircase              0.572  0.484  0.144  0.149  0.571
      causal leak                    0.662  0.717  0.191  0.279  0.677
      independence / (2,256,12)      0.643  0.333  0.181  0.205  0.534
    attention (staged kernels)
      tails                          0.694  0.000  0.136  0.250  0.542
      rescale staircase              0.662  0.001  0.144  0.149  0.571
    torch fallback (T 100, 65; D 32) 0.481  -      dqkv 0.322
    (lse2 and dV against 1.5x the constants the bounds started with: 1.076 and 1.015 on the causal-leak case
     before, the same as the torch emulation of the algorithm's roundings -- derivation in _gpt2_ref.py.  The
     staged forward sums the unrounded P, hence its lse2.)

    cross-entropy    loss rows 0.599   gradient 0.982 (bf16: at one output rounding)   mean 0.009
                     ce_grad_scale 0.942   Fx.cross_entropy logits.grad 0.882
    LayerNorm        mean 0.047   rstd 0.024   y 0.996   dx 0.987   dw 0.217   db 0.029
                     (y, and dx with bf16 x: the bound is one bf16 rounding of the output, which is reached)
    embedding_bwd    dwte 0.122   dwpe 0.141
    add 0.996 (bf16)   gelu 0.985   gelu_bwd 0.996 (bf16; fp32 below 0.1)
"""
import copy
import math

import pytest
import torch
import torch.nn.functional as F

import _gpt2_ref as R
from distributed_pytorch_example_amd.models import get_model
from distributed_pytorch_example_amd.ops import functional as Fx

pytestmark = pytest.mark.gpu
dev = "cuda"
BF = torch.bfloat16
SCALE = 0.125  # 1 / sqrt(64)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _ratio(name, got, ref, bound):
    """Worst |got - ref| / bound over the elements (printed); non-finite outputs count as infinite."""
    err = (got.double() - ref).abs()
    err = torch.where(torch.isfinite(got.double()), err, torch.full_like(err, float("inf")))
    r = (err / bound).max().item()
    print(f"  {name}: worst |err|/bound = {r:.3f}")
    return r


# ================================================================== attention
def _canary(shape, dtype, n_real):
    """A buffer of ``shape`` filled with random bits; returns (buffer, the first n_real elements as a flat
    tensor sharing its storage, a copy of the rest = the canary rows that directly follow them)."""
    g = torch.Generator(device="cpu").manual_seed(12345)
    if dtype == BF:
        raw = torch.randint(-32768, 32767, shape, generator=g, dtype=torch.int16).to(dev).view(BF)
    else:
        raw = torch.randint(-2 ** 31, 2 ** 31 - 1, shape, generator=g, dtype=torch.int32).to(dev).view(torch.float32)
    flat = raw.view(-1)
    return raw, flat[:n_real], _bits(flat[n_real:]).clone()


def _attn_run(C, qkv, dout, guard=False):
    """attn_fwd + attn_bwd; with ``guard`` the outputs are the leading part of larger buffers whose remaining
    128 rows (per batch entry's worth of storage, directly behind the outputs) must come back bit-unchanged."""
    B, T, _, H, D = qkv.shape
    if not guard:
        out, lse = C.attn_fwd(qkv, H, SCALE, True)
        dqkv = C.attn_bwd(qkv, out, dout, lse, H, SCALE, True)
        torch.cuda.synchronize()
        return out, lse, dqkv
    bo, fo, co = _canary((B, T + 128, H, D), BF, B * T * H * D)
    bl, fl, cl = _canary((B, H, T + 128), torch.float32, B * H * T)
    bd, fd, cd = _canary((B, T + 128, 3, H, D), BF, B * T * 3 * H * D)
    out, lse, dqkv = fo.view(B, T, H, D), fl.view(B, H, T), fd.view(B, T, 3, H, D)
    C.attn_fwd(qkv, H, SCALE, True, out=out, lse=lse)
    C.attn_bwd(qkv, out, dout, lse, H, SCALE, True, dqkv=dqkv)
    torch.cuda.synchronize()
    assert torch.equal(_bits(bo.view(-1)[fo.numel():]), co), "attn_fwd stored past the end of out"
    assert torch.equal(_bits(bl.view(-1)[fl.numel():]), cl), "attn_fwd stored past the end of lse"
    assert torch.equal(_bits(bd.view(-1)[fd.numel():]), cd), "attn_bwd stored past the end of dqkv"
    return out, lse, dqkv


def _attn_check(tag, got, ref):
    out, lse, dqkv = got
    print(tag)
    rs = {
        "out": _ratio("out", out, ref["out"], ref["b_out"]),
        "lse2": _ratio("lse2", lse, ref["lse2"], torch.full_like(ref["lse2"], ref["b_lse2"])),
        "dQ": _ratio("dQ", dqkv[:, :, 0], ref["dqkv"][:, :, 0], ref["b_dqkv"][:, :, 0]),
        "dK": _ratio("dK", dqkv[:, :, 1], ref["dqkv"][:, :, 1], ref["b_dqkv"][:, :, 1]),
        "dV": _ratio("dV", dqkv[:, :, 2], ref["dqkv"][:, :, 2], ref["b_dqkv"][:, :, 2]),
    }
    for k, r in rs.items():
        assert r <= 1.0, f"{tag}: {k} exceeds its rounding budget, worst ratio {r:.3f}"
    return rs


def _randn_case(B, T, H, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, T, 3, H, 64, generator=g).to(BF).to(dev)
    dout = torch.randn(B, T, H, 64, generator=g).to(BF).to(dev)
    return qkv, dout


class _Staged:
    """set_attn_staged(on) for the block, the previous setting restored on exit."""

    def __init__(self, C, on):
        self.C, self.on = C, on

    def __enter__(self):
        self.prev = self.C.set_attn_staged(self.on)

    def __exit__(self, *exc):
        self.C.set_attn_staged(self.prev)


TAILS = [(1, 64, 1), (2, 192, 3), (1, 320, 2), (2, 128, 2)]


@pytest.mark.parametrize("staged", [False, True], ids=["dma", "staged"])
@pytest.mark.parametrize("B,T,H", TAILS)
def test_attn_tails(C, B, T, H, staged):
    """1a (and 2): T % 128 == 64 leaves half a workgroup without queries (forward, dQ) or keys (dK/dV); the
    rows right behind every output stay bit-unchanged."""
    qkv, dout = _randn_case(B, T, H, 100 + T)
    ref = R.attn_ref(qkv, dout, SCALE)
    with _Staged(C, staged):
        got = _attn_run(C, qkv, dout, guard=True)
    _attn_check(f"tails B={B} T={T} H={H} staged={staged}", got, ref)


@pytest.mark.parametrize("staged", [False, True], ids=["dma", "staged"])
@pytest.mark.parametrize("reverse", [False, True], ids=["rising", "falling"])
def test_attn_rescale_staircase(C, reverse, staged):
    """1b (and 2): scores that step up once per 64-key tile.  Head 0: the a_hi rows' tile maximum jumps by more
    than 2^8 at two later tiles (the rescale branch after the first tile), the a = 0 rows of the same wave do
    not (need[0] != need[1]: alpha = 1 for one 16-row block).  Head 1: jumps inside (4, 8): deferred, P grows
    past 2^4 under an unmoved maximum.  Falling: later tiles contribute P ~ 0.  All of it asserted on the fp64
    scores before the kernel runs."""
    qkv, a = R.staircase_qkv(256, (12.0, 6.5), reverse=reverse)
    g = torch.Generator().manual_seed(7)
    dout = torch.randn(1, 256, 2, 64, generator=g).to(BF).to(dev)
    qkv = qkv.to(dev)
    hi = (a > 0).to(dev)
    tm = R.tile_row_max(qkv, SCALE)[0]  # [H, T, tiles]
    jump, fin = tm[..., 1:] - tm[..., :-1], torch.isfinite(tm[..., 1:])
    later, defer, dist = R.deferred_max_trace(tm)
    assert dist.min().item() > 0.25, "a branch decision sits too close to the threshold to be predicted in fp64"
    if not reverse:
        assert ((jump[0][hi] > 8) & fin[0][hi]).sum(-1).max().item() >= 2
        assert not ((jump[0][~hi] > 8) & fin[0][~hi]).any()
        j1 = jump[1][hi]
        assert ((j1 > 4) & (j1 < 8) & fin[1][hi]).any() and not ((jump[1] > 8) & fin[1]).any()
        assert later[0][hi].max().item() >= 2 and later[0][~hi].max().item() == 0
        assert defer[1][hi].max().item() > 4  # P up to 2^defer accumulated under the old maximum
    else:
        assert later.max().item() == 0 and ((jump[0][hi] < -8) & fin[0][hi]).any()
    ref = R.attn_ref(qkv, dout, SCALE)
    with _Staged(C, staged):
        got = _attn_run(C, qkv, dout, guard=True)
    _attn_check(f"staircase reverse={reverse} staged={staged}", got, ref)


def test_attn_causal_leak(C):
    """1c: keys from position 100 on are 16x larger, so the scores above the diagonal of the earlier rows are
    huge (exp2 overflows before the mask zeroes it).  Bounds hold, everything is finite, and what the first
    100 positions receive does not depend on anything at or behind position 100, bit for bit."""
    B, T, H, CUT = 2, 192, 2, 100
    qkv, dout = _randn_case(B, T, H, 31)
    qkv[:, CUT:, 1] *= 16
    ref = R.attn_ref(qkv, dout, SCALE)
    q, k = qkv[:, :, 0].double(), qkv[:, :, 1].double()
    s_above = SCALE * R.LOG2E * torch.einsum("bihd,bjhd->bhij", q[:, :CUT], k[:, CUT:])
    assert (s_above.amax() - ref["lse2"][..., :CUT].amin()).item() > 64, "masked scores are not large"
    got = _attn_run(C, qkv, dout)
    for t in got:
        assert torch.isfinite(t.float()).all()
    _attn_check("causal leak", got, ref)
    qkv2, dout2 = qkv.clone(), dout.clone()
    o2, d2 = _randn_case(B, T, H, 32)
    qkv2[:, CUT:], dout2[:, CUT:] = o2[:, CUT:] * 3, d2[:, CUT:]
    got2 = _attn_run(C, qkv2, dout2)
    assert _same_bits(got[0][:, :CUT], got2[0][:, :CUT]), "out of rows < 100 depends on later positions"
    assert _same_bits(got[1][..., :CUT], got2[1][..., :CUT]), "lse of rows < 100 depends on later positions"
    assert _same_bits(got[2][:, :CUT, 0], got2[2][:, :CUT, 0]), "dQ of rows < 100 depends on later positions"


def test_attn_batch_head_independence(C):
    """1d: permuting batch and head axes of the inputs permutes the outputs, bitwise (no atomics, and no
    workgroup reads another (b, h)'s rows)."""
    B, T, H = 3, 128, 5
    qkv, dout = _randn_case(B, T, H, 41)
    pb, ph = torch.tensor([2, 0, 1], device=dev), torch.tensor([3, 0, 4, 1, 2], device=dev)
    got = _attn_run(C, qkv, dout)
    _attn_check("independence base", got, R.attn_ref(qkv, dout, SCALE))
    qkv_p = qkv[pb][:, :, :, ph].contiguous()
    dout_p = dout[pb][:, :, ph].contiguous()
    out_p, lse_p, dqkv_p = _attn_run(C, qkv_p, dout_p)
    assert _same_bits(out_p, got[0][pb][:, :, ph])
    assert _same_bits(lse_p, got[1][pb][:, ph])
    assert _same_bits(dqkv_p, got[2][pb][:, :, :, ph])


@pytest.mark.parametrize("staged", [False, True], ids=["dma", "staged"])
def test_attn_determinism(C, staged):
    """1e: identical inputs, identical bits, forward and backward."""
    qkv, dout = _randn_case(2, 192, 3, 51)
    with _Staged(C, staged):
        a = _attn_run(C, qkv, dout)
        b = _attn_run(C, qkv, dout)
    for x, y in zip(a, b):
        assert _same_bits(x, y)


def test_attn_sanity_larger(C):
    """1f: (2, 256, 12) under the per-element bounds."""
    qkv, dout = _randn_case(2, 256, 12, 61)
    _attn_check("sanity (2,256,12)", _attn_run(C, qkv, dout), R.attn_ref(qkv, dout, SCALE))


def test_set_attn_staged_returns_previous(C):
    prev = C.set_attn_staged(True)
    try:
        assert prev is False  # the default
        assert C.set_attn_staged(False) is True
        assert C.set_attn_staged(False) is False
    finally:
        C.set_attn_staged(prev)


# ------------------------------------------------- 3. shapes outside the kernels
@pytest.mark.parametrize("T,D", [(100, 64), (65, 64), (128, 32)])
def test_causal_attention_unsupported_shapes(C, T, D):
    """Fx.causal_attention on the GPU for T % 64 != 0 or head dim != 64: a torch implementation, autograd
    through it, under the same budgets as the kernels (its only roundings are the bf16 outputs)."""
    B, H = 2, 3
    g = torch.Generator().manual_seed(70 + T + D)
    qkv = torch.randn(B, T, 3 * H * D, generator=g).to(BF).to(dev).requires_grad_(True)
    dout = torch.randn(B, T, H * D, generator=g).to(BF).to(dev)
    out = Fx.causal_attention(qkv, H)
    assert out.shape == (B, T, H * D) and out.dtype == BF
    out.backward(dout)
    ref = R.attn_ref(qkv.detach().view(B, T, 3, H, D), dout.view(B, T, H, D), 1.0 / math.sqrt(D))
    print(f"fallback T={T} D={D}")
    assert _ratio("out", out.detach().view(B, T, H, D), ref["out"], ref["b_out"]) <= 1.0
    assert _ratio("dqkv", qkv.grad.view(B, T, 3, H, D), ref["dqkv"], ref["b_dqkv"]) <= 1.0


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


def _cos(a, b):
    a, b = a.float().flatten(), b.float().flatten()
    return (a @ b / (a.norm() * b.norm() + 1e-12)).item()


def test_gpt2_tiny_T100_gpu_vs_cpu(C):
    """The model at a sequence length the attention kernels do not take (T = 100): the block leaves the fused
    path, attention falls back; same tolerance as test_models_gpu.py::test_gpt2_tiny_gpu_vs_cpu."""
    torch.manual_seed(4)
    cpu = get_model("gpt2-tiny")
    gpu = copy.deepcopy(cpu).to(dev)
    idx = torch.randint(0, 512, (2, 100))
    tgt = torch.randint(0, 512, (2, 100))
    lc = Fx.cross_entropy(cpu(idx), tgt)
    lc.backward()
    lg = Fx.cross_entropy(gpu(idx.to(dev)), tgt.to(dev))
    lg.backward()
    assert abs(lc.item() - lg.item()) < 2e-2 * abs(lc.item())
    gc = dict(cpu.named_parameters())
    for n, p in gpu.named_parameters():
        assert _cos(p.grad.cpu(), gc[n].grad) > 0.98, n
        assert _rel(p.grad.cpu(), gc[n].grad) < 0.1, n


# ============================================================== cross-entropy
GS = 0.37
CE_B = 48
# (ld, V, logits dtype, gradient dtype, in place, ignore_index, offset case): the kernel each (ld, V) reaches
# is the issue's table -- ce_vec_kernel (256,1) x2, (1024,1), (1024,2), (1024,4), scalar ce_kernel with 256
# and with 1024 threads; all four dtype pairs, in place for both equal pairs and for the scalar kernel.
CE_CASES = [
    (2048, 2048, BF, BF, True, -100, False),
    (1032, 1025, torch.float32, BF, False, 7, False),
    (8192, 8192, BF, torch.float32, False, -100, False),
    (16384, 16000, torch.float32, torch.float32, True, 3, False),
    (32768, 32768, BF, BF, False, -100, False),
    (1001, 1001, torch.float32, torch.float32, True, 5, False),
    (4099, 4099, BF, torch.float32, False, -100, False),
    (4099, 4099, torch.float32, BF, False, 11, False),
    (2048, 2048, torch.float32, torch.float32, False, -100, True),
    (1032, 1025, BF, BF, True, 7, True),
]


def _ce_inputs(B, ld, V, dt, ign, offset, seed):
    """Logits (padding columns hold +30 above everything: they must be ignored) and labels: rows 0..2 carry the
    labels 0, V-1, V-8; rows 3..5 and 11 are ignored; rows 6..9 are labelled with their argmax.  One bumped
    column per row makes the maximum unique by more than a bf16 ulp (2^-6 |max| > ulp, and at least 1)."""
    g = torch.Generator().manual_seed(seed)
    if offset:
        z = 80.0 + 60.0 * (torch.rand(B, ld, generator=g) - 0.5)
    else:
        z = 2.0 * torch.randn(B, ld, generator=g)
    col = torch.randint(0, V, (B,), generator=g)
    if ign >= 0:
        col[3] = ign  # an ignored row whose argmax equals its label: must not count as correct
    top = z[:, :V].amax(1)
    z[torch.arange(B), col] = top + torch.maximum(torch.ones(B), top.abs() * 2.0 ** -5)
    z[:, V:] = z[:, :V].amax() + 30.0
    z = z.to(dt)
    labels = torch.randint(0, V, (B,), generator=g)
    labels[0], labels[1], labels[2] = 0, V - 1, V - 8
    labels[6:10] = col[6:10]
    labels[[3, 4, 5, 11]] = ign
    zz = z.double()[:, :V]
    t2 = zz.topk(2, dim=1).values
    assert ((t2[:, 0] - t2[:, 1]) > 2.0 ** -7 * t2[:, 0].abs()).all(), "row maximum not unique by a bf16 ulp"
    return z.to(dev), labels.to(dev)


def _ce_check_grad(d, gref, valid, V, out_dt, gs, tag):
    assert d.dtype == out_dt
    dd = d.double()
    assert (dd[:, V:] == 0).all(), f"{tag}: padding columns of the gradient must be exactly 0"
    assert (dd[~valid] == 0).all(), f"{tag}: ignored rows must have an exactly zero gradient"
    if out_dt == BF:  # one output rounding (at most 2^-8: bf16 keeps 8 significant bits) plus the fp32 arithmetic
        bound = 2.0 ** -8 * gref.abs() + 1e-7 * gs
    else:
        bound = 1e-6 + 2.0 ** -20 * gref.abs()
    return _ratio(f"{tag} grad", d, gref, bound)


@pytest.mark.parametrize("ld,V,in_dt,out_dt,inplace,ign,offset", CE_CASES)
def test_cross_entropy_rows(C, ld, V, in_dt, out_dt, inplace, ign, offset):
    z, labels = _ce_inputs(CE_B, ld, V, in_dt, ign, offset, seed=ld + V)
    loss_ref, gref, am, valid = R.ce_ref(z, labels, V, GS, ign)
    assert (~valid).sum().item() >= 4 and valid.sum().item() >= 40
    zin = z.clone()
    rows, s, correct, d = C.cross_entropy(zin, labels, V, GS, True, out_dt == BF, ign, inplace)
    torch.cuda.synchronize()
    if inplace:
        assert d.data_ptr() == zin.data_ptr()
    else:
        assert torch.equal(zin, z), "the logits changed in an out-of-place call"
    tag = f"CE ld={ld} V={V} {in_dt}->{out_dt}"
    print(tag)
    # the kernel's arithmetic is fp32: per row 1e-5 max(1, |ref|)
    rb = 1e-5 * loss_ref.abs().clamp(min=1.0)
    assert (rows.double()[~valid] == 0).all(), "ignored rows must give loss 0"
    assert _ratio("loss rows", rows, loss_ref, rb) <= 1.0
    # the sum: the row budgets plus the fp32 summation of B terms
    assert abs(s.item() - loss_ref.sum().item()) <= rb.sum().item() + 1e-6 * loss_ref.abs().sum().item()
    assert correct.item() == ((am == labels) & valid).sum().item()
    assert _ce_check_grad(d, gref, valid, V, out_dt, GS, tag) <= 1.0


@pytest.mark.parametrize("in_dt", [BF, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("B", [1, 257, 2049])
def test_cross_entropy_mean_and_grad_scale(C, B, in_dt):
    """cross_entropy_mean / ce_grad_scale (the pair _CEFn and _LMHeadCEFn call): mean over the non-ignored
    rows, 1 / count exactly, the scaled gradient; B crosses ce_sum_kernel's 256-thread and 2048-row trips."""
    ld, V, ign = 72, 70, 2
    g = torch.Generator().manual_seed(B)
    z = (2.0 * torch.randn(B, ld, generator=g)).to(in_dt).to(dev)
    labels = torch.randint(0, V, (B,), generator=g)
    labels[::5] = ign
    if B == 1:
        labels[0] = 9
    labels = labels.to(dev)
    loss_ref, gref, am, valid = R.ce_ref(z, labels, V, 1.0, ign)
    n = int(valid.sum().item())
    out4, d = C.cross_entropy_mean(z, labels, V, in_dt == BF, ign, False)
    torch.cuda.synchronize()
    mean_ref = loss_ref.sum().item() / n
    print(f"CE mean B={B} {in_dt}: mean err / bound = {abs(out4[2].item() - mean_ref) / (1e-5 * max(1.0, mean_ref)):.3f}")
    assert abs(out4[2].item() - mean_ref) <= 1e-5 * max(1.0, abs(mean_ref))  # the row budget carries to the mean
    assert abs(out4[0].item() - loss_ref.sum().item()) <= 1e-5 * loss_ref.abs().clamp(min=1.0).sum().item()
    assert out4[1].item() == ((am == labels) & valid).sum().item()
    inv = (torch.ones((), dtype=torch.float32) / torch.tensor(float(n), dtype=torch.float32)).item()
    assert out4[3].item() == inv, "out4[3] must be 1 / count, correctly rounded"
    assert _ce_check_grad(d, gref, valid, V, in_dt, 1.0, "mean form") <= 1.0
    gsc = torch.tensor([2.5], device=dev)
    o = C.ce_grad_scale(d, gsc, out4[3:4])
    want = d.double() * 2.5 / n
    # one rounding of the output dtype: fp32 2^-24, bf16 (8 significant bits) 2^-8; plus the fp32 roundings of
    # 1 / count, g * inv_n and the product in front of it (1.5 * 2^-23 <= 2^-22)
    rel = 2.0 ** -22 + (2.0 ** -8 if in_dt == BF else 0.0)
    assert o.dtype == d.dtype and _ratio("ce_grad_scale", o, want, rel * want.abs() + R.FLOOR) <= 1.0
    # every row ignored: loss 0, 1 / count == 1, zero gradient
    out4, d = C.cross_entropy_mean(z, torch.full_like(labels, ign), V, in_dt == BF, ign, False)
    assert out4[0].item() == 0 and out4[1].item() == 0 and out4[2].item() == 0 and out4[3].item() == 1
    assert (d.double() == 0).all()


@pytest.mark.parametrize("in_dt", [BF, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("ign", [-100, 4])
def test_functional_cross_entropy_ignore_index(C, ign, in_dt):
    """Fx.cross_entropy(..., ignore_index) and logits.grad against F.cross_entropy in fp64."""
    B, ld, V = 300, 136, 130
    g = torch.Generator().manual_seed(5 + ign % 7)
    z = (2.0 * torch.randn(B, ld, generator=g)).to(in_dt).to(dev).requires_grad_(True)
    labels = torch.randint(0, V, (B,), generator=g)
    labels[::7] = ign
    labels = labels.to(dev)
    loss = Fx.cross_entropy(z, labels, V, ignore_index=ign)
    (loss * 2.5).backward()
    zr = z.detach().double().requires_grad_(True)
    lr = F.cross_entropy(zr[:, :V], labels, ignore_index=ign)
    (lr * 2.5).backward()
    assert abs(loss.item() - lr.item()) <= 1e-5 * max(1.0, abs(lr.item()))
    n = int((labels != ign).sum().item())
    k = 2.5 / n  # what the per-row gradient is scaled by
    if in_dt == BF:  # two bf16 roundings (softmax - onehot, then its scaled copy) of at most 2^-8 each
        bound = 2.0 ** -7 * zr.grad.abs() + 1e-7 * k
    else:
        bound = (1e-6 + 2.0 ** -20 * (zr.grad.abs() / k)) * k + 2.0 ** -22 * zr.grad.abs()
    assert z.grad.dtype == in_dt
    assert (z.grad.double()[:, V:] == 0).all() and (z.grad.double()[labels == ign] == 0).all()
    print(f"Fx.cross_entropy ign={ign} {in_dt}")
    assert _ratio("logits.grad", z.grad, zr.grad, bound) <= 1.0


# ================================================================== LayerNorm
def _ln_inputs(rows, D, x_dt, bias, seed, mean300=False):
    g = torch.Generator().manual_seed(seed)
    if mean300:
        # multiples of 2^-5 around a per-row mean that is itself one, the second half of the row mirroring the
        # first: every fp32 partial sum (< 2^19, multiples of 2^-5) and the mean are then exact, so the
        # test isolates cancellation in the variance (an E[x^2] - mean^2 kernel loses ~1e-3 of rstd here)
        # from the rounding of an fp32 mean near 300 (ulp 3e-5, by itself above the y budget where |xhat| is small)
        e = torch.round(torch.randn(rows, D // 2, generator=g, dtype=torch.float64) * 32.0) / 32.0
        e = torch.cat([e, -e], dim=1)
        x = (300.0 + (torch.arange(rows, dtype=torch.float64) % 8).unsqueeze(1) / 8.0 + e).float()
        assert (x.double().mean(1) == 300.0 + (torch.arange(rows) % 8) / 8.0).all()
    else:
        # elements that sit (almost) on their row's mean are moved off it: there y ~ 0 and its relative budget
        # 2^-8 |y| falls below what the rounding of any fp32 mean (half an ulp, 1.5e-8 at 0.3) does to y, so
        # no fp32 LayerNorm can meet it.  _ln_fwd_check asserts the condition on the reference.
        x = (torch.randn(rows, D, generator=g) * 1.5 + 0.3).to(x_dt)
        for _ in range(3):
            xd = x.double()
            dev_ = xd - xd.mean(1, keepdim=True)
            near = dev_.abs() < 2.0 ** -5
            x = torch.where(near, xd + torch.where(dev_ >= 0, 0.125, -0.125), xd).to(x_dt)
    x = x.to(dev)
    w = (1.0 + 0.5 * torch.randn(D, generator=g)).to(dev)
    b = (0.5 * torch.randn(D, generator=g)).to(dev) if bias else None
    dy = torch.randn(rows, D, generator=g).to(BF).to(dev)
    return x, w, b, dy


def _ln_fwd_check(C, x, w, b, tag, exact_mean=False):
    yr, mr, rr, xh = R.ln_ref(x, w, b)
    amax = x.double().abs().amax(1).clamp(min=1.0)
    if not exact_mean:
        # the y budget must cover what the mean's own tolerance (below) does to y: |w| rstd 1e-6 max(1, max|x|)
        assert (2.0 ** -8 * xh.abs() >= 1e-6 * (amax * rr).unsqueeze(1)).all(), "an element sits on its row's mean"
    y, mean, rstd = C.layernorm_fwd(x, w, b, 1e-5)
    torch.cuda.synchronize()
    rs = [
        _ratio(f"{tag} mean", mean, mr, 1e-6 * amax),
        _ratio(f"{tag} rstd", rstd.double() / rr, torch.ones_like(rr), torch.full_like(rr, 1e-5)),
        _ratio(f"{tag} y", y, yr, 2.0 ** -8 * yr.abs() + 1e-6 * (w.double().abs() * xh.abs()
                                                                 + (b.double().abs() if b is not None else 0.0)) + R.FLOOR),
    ]
    assert y.dtype == BF and max(rs) <= 1.0, f"{tag}: forward ratios (mean, rstd, y) = {rs}"
    return mean, rstd


def _ln_stat_bounds(dy, x, w):
    _, _, rstd, xh = R.ln_ref(x, w)
    dyd = dy.double()
    return 1e-6 * (dyd * xh).abs().sum(0) + R.FLOOR, 1e-6 * dyd.abs().sum(0) + R.FLOOR, \
        1e-5 * (dyd * w.double()).abs().sum(1) * rstd + R.FLOOR


def _ln_bwd_check(C, x, w, b, dy, mean, rstd, tag):
    """The plain form: dx in x's dtype, dw / db accumulated into zeros."""
    D = x.shape[-1]
    dw = torch.zeros(D, device=dev)
    db = torch.zeros(D, device=dev) if b is not None else None
    dx = C.layernorm_bwd(dy, x, w, mean, rstd, dw, db, None)
    torch.cuda.synchronize()
    dxr, dwr, dbr = R.ln_bwd_ref(dy, x, w)
    bw, bb, bx32 = _ln_stat_bounds(dy, x, w)
    err = (dx.double() - dxr).abs().amax(1)
    err = torch.where(torch.isfinite(dx.double()).all(1), err, torch.full_like(err, float("inf")))
    # bf16 dx: one output rounding with 2x margin, relative to the row's largest element; fp32: the row's
    # sum |dy w| rstd (the size of the terms that cancel in g - mean(g) - xhat mean(g xhat))
    bx = 2.0 ** -8 * dxr.abs().amax(1) + R.FLOOR if x.dtype == BF else bx32
    rs = [(err / bx).max().item(), _ratio(f"{tag} dw", dw, dwr, bw)]
    print(f"  {tag} dx: worst row |err|/bound = {rs[0]:.3f}")
    if b is not None:
        rs.append(_ratio(f"{tag} db", db, dbr, bb))
    assert dx.dtype == x.dtype and max(rs) <= 1.0, f"{tag}: backward ratios (dx, dw, db) = {rs}"


@pytest.mark.parametrize("x_dt", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("D", [8, 520, 768, 1016, 3072, 8192])
def test_layernorm_grid(C, D, x_dt):
    """D = 8 and 8192 are the ends of the generic forward (1 and 16 chunks per lane); 520 / 1016 the ends of
    the lean forward's range (one chunk, and all but one, in its second round; clamped tail lanes); 3072 and
    8192 take the row-sums + column-slice backward.  Rows 5 (part of one block) and 333; with and without bias."""
    for rows in (5, 333):
        for bias in (True, False):
            tag = f"LN D={D} rows={rows} {'bf16' if x_dt == BF else 'f32'} bias={bias}"
            print(tag)
            x, w, b, dy = _ln_inputs(rows, D, x_dt, bias, seed=D + rows)
            mean, rstd = _ln_fwd_check(C, x, w, b, tag)
            _ln_bwd_check(C, x, w, b, dy, mean, rstd, tag)


@pytest.mark.parametrize("x_dt", [torch.float32, BF], ids=["f32", "bf16"])
def test_layernorm_many_rows(C, x_dt):
    """8200 rows at D = 64: dpe_layernorm_bwd_nblocks saturates at 1024 and a block walks more than 8 rows."""
    x, w, b, dy = _ln_inputs(8200, 64, x_dt, True, seed=8200)
    mean, rstd = _ln_fwd_check(C, x, w, b, "LN rows=8200")
    _ln_bwd_check(C, x, w, b, dy, mean, rstd, "LN rows=8200")


@pytest.mark.parametrize("D", [8, 768, 1016])
def test_layernorm_large_mean(C, D):
    """Per-row mean ~300, unit variance: cancellation in the variance.  fp32 x only -- bf16 has 8 significant
    bits, so its spacing near 300 is 2 and such a row cannot be stored."""
    for bias in (True, False):
        x, w, b, dy = _ln_inputs(37, D, torch.float32, bias, seed=300 + D, mean300=True)
        mean, rstd = _ln_fwd_check(C, x, w, b, f"LN mean300 D={D} bias={bias}", exact_mean=True)
        _ln_bwd_check(C, x, w, b, dy, mean, rstd, f"LN mean300 D={D} bias={bias}")


@pytest.mark.parametrize("x_dt", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("D", [768, 1016, 3072])
def test_layernorm_bwd_accumulate_and_residual(C, D, x_dt):
    """dx accumulated into a given fp32 tensor (dw / db into non-zero grads), and layernorm_bwd_residual
    (dx = res_in + dLN in fp32 plus its bf16 copy), lean (768, 1016) and generic (3072) kernels."""
    rows = 77
    x, w, b, dy = _ln_inputs(rows, D, x_dt, True, seed=D)
    mean, rstd = _ln_fwd_check(C, x, w, b, f"LN acc D={D}")
    dxr, dwr, dbr = R.ln_bwd_ref(dy, x, w)
    bw, bb, bx = _ln_stat_bounds(dy, x, w)
    g = torch.Generator().manual_seed(1)
    pre = torch.randn(rows, D, generator=g).to(dev)
    dw0, db0 = torch.randn(D, generator=g).to(dev), torch.randn(D, generator=g).to(dev)
    # accumulate form
    acc, dw, db = pre.clone(), dw0.clone(), db0.clone()
    ret = C.layernorm_bwd(dy, x, w, mean, rstd, dw, db, acc)
    torch.cuda.synchronize()
    assert ret.data_ptr() == acc.data_ptr()
    print(f"LN accumulate D={D} {x_dt}")
    # (the one extra fp32 rounding of pre + dLN, 2^-24 |sum|, is far inside the row budget; dw / db get it added)
    assert _ratio("dx_out", acc, pre.double() + dxr, bx.unsqueeze(1).expand_as(dxr)) <= 1.0
    assert _ratio("dw +=", dw, dw0.double() + dwr, bw + 2.0 ** -23 * (dw0.double() + dwr).abs()) <= 1.0
    assert _ratio("db +=", db, db0.double() + dbr, bb + 2.0 ** -23 * (db0.double() + dbr).abs()) <= 1.0
    # residual form
    dw, db = torch.zeros(D, device=dev), torch.zeros(D, device=dev)
    dx, dxb = C.layernorm_bwd_residual(dy, x, w, mean, rstd, dw, db, pre, False)
    torch.cuda.synchronize()
    assert dx.dtype == torch.float32 and dxb.dtype == BF
    assert _ratio("residual dx", dx, pre.double() + dxr, bx.unsqueeze(1).expand_as(dxr)) <= 1.0
    assert _same_bits(dxb, dx.to(BF)), "the bf16 copy must be the rounded fp32 dx"
    assert _ratio("residual dw", dw, dwr, bw) <= 1.0 and _ratio("residual db", db, dbr, bb) <= 1.0
    # deferred: dw / db untouched, the partials finalized later give the same sums
    dw2, db2 = torch.zeros(D, device=dev), torch.zeros(D, device=dev)
    dx2, dxb2, part = C.layernorm_bwd_residual(dy, x, w, mean, rstd, dw2, db2, pre, True)
    assert (dw2 == 0).all() and (db2 == 0).all() and _same_bits(dx2, dx) and _same_bits(dxb2, dxb)
    C.layernorm_bwd_finalize_group([part], [rows], [dw2], [db2])
    assert _same_bits(dw2, dw) and _same_bits(db2, db)


# ================================================== embedding and elementwise
def test_embedding_fwd_exact(C):
    """wte[idx] (+ wpe[t]) in fp32, bitwise: the sum of two bf16 values of similar size is exact in fp32 (and
    where it is not, fp32 addition rounds the same way in the reference)."""
    g = torch.Generator().manual_seed(1)
    Vn, T, D, B = 301, 48, 72, 3
    wte = (0.02 * torch.randn(Vn, D, generator=g)).to(BF).to(dev)
    wpe = (0.02 * torch.randn(T + 5, D, generator=g)).to(BF).to(dev)
    idx = torch.randint(0, Vn, (B, T), generator=g).to(dev)
    idx[0, 0], idx[0, 1] = 0, Vn - 1
    got = C.embedding_fwd(idx, wte, wpe)
    want = wte.float()[idx] + wpe.float()[:T].unsqueeze(0)
    assert got.dtype == torch.float32 and _same_bits(got, want)
    assert _same_bits(C.embedding_fwd(idx, wte, None), wte.float()[idx])
    assert _same_bits(C.embedding_fwd(idx, wte), wte.float()[idx])


@pytest.mark.parametrize("same_token", [True, False], ids=["one_token", "random"])
@pytest.mark.parametrize("with_pos", [False, True], ids=["no_dwpe", "dwpe"])
def test_embedding_bwd(C, same_token, with_pos):
    """Scatter-add into non-zero dwte (and dwpe): all 4 * 64 rows onto one token row (every atomic contends),
    and random tokens; fp32 sums in any order, so 1e-6 of the sum of |contributions| per element."""
    g = torch.Generator().manual_seed(2)
    Vn, B, T, D = 97, 4, 64, 64
    idx = torch.full((B, T), 13, dtype=torch.long) if same_token else torch.randint(0, Vn, (B, T), generator=g)
    idx = idx.to(dev)
    dout = torch.randn(B, T, D, generator=g).to(dev)
    dwte0 = torch.randn(Vn, D, generator=g).to(dev)
    dwpe0 = torch.randn(T, D, generator=g).to(dev)
    dwte, dwpe = dwte0.clone(), dwpe0.clone()
    C.embedding_bwd(idx, dout, dwte, dwpe if with_pos else None)
    torch.cuda.synchronize()
    flat, dd = idx.view(-1), dout.double().view(-1, D)
    want = dwte0.double().index_add(0, flat, dd)
    mag = dwte0.double().abs().index_add(0, flat, dd.abs())
    print(f"embedding_bwd same_token={same_token} with_pos={with_pos}")
    assert _ratio("dwte", dwte, want, 1e-6 * mag + R.FLOOR) <= 1.0
    if with_pos:
        wantp = dwpe0.double() + dd.view(B, T, D).sum(0)
        magp = dwpe0.double().abs() + dd.view(B, T, D).abs().sum(0)
        assert _ratio("dwpe", dwpe, wantp, 1e-6 * magp + R.FLOOR) <= 1.0
    else:
        assert _same_bits(dwpe, dwpe0)


N_ODD = 1000003  # not a multiple of 8: the bf16 calls take the scalar kernel


@pytest.mark.parametrize("dt", [torch.float32, BF], ids=["f32", "bf16"])
def test_add_alpha(C, dt):
    g = torch.Generator().manual_seed(3)
    a = torch.randn(N_ODD, generator=g).to(dt).to(dev)
    b = torch.randn(N_ODD, generator=g).to(dt).to(dev)
    got = C.add(a, b, -0.5)
    want = a.double() - 0.5 * b.double()
    mag = a.double().abs() + 0.5 * b.double().abs()
    # fp32 arithmetic on the terms (two roundings at most), bf16: plus the output rounding (at most 2^-8)
    bound = 2.0 ** -23 * mag + (2.0 ** -8 * want.abs() if dt == BF else 0.0) + R.FLOOR
    assert got.dtype == dt and _ratio(f"add {dt}", got, want, bound) <= 1.0


def test_cast_f32_exact(C):
    g = torch.Generator().manual_seed(4)
    for n in (N_ODD, 8, 7, 4096):
        x = (torch.randn(n, generator=g) * 100).to(BF).to(dev)
        assert _same_bits(C.cast_f32(x), x.float())


def _act_check(C, a, b, tag):
    """ops 0..3 on (a, b): relu, relu_bwd(dy = a, y = b), gelu, gelu_bwd(dy = a, x = b)."""
    ad, bd = a.double(), b.double()
    bf = a.dtype == BF
    print(tag)
    r0, r1 = C.act(a, None, 0), C.act(a, b, 1)
    assert torch.equal(r0, torch.clamp_min(a, 0)) and torch.equal(r1, torch.where(b > 0, a, torch.zeros_like(a)))
    r2, r3 = C.act(a, None, 2), C.act(a, b, 3)
    w2, w3 = R.gelu_ref(a), ad * R.gelu_grad_ref(b)
    if bf:  # the output rounding with 2x margin plus an absolute term (the derivative's scales with dy)
        b2, b3 = 2.0 ** -8 * w2.abs() + 1e-6, 2.0 ** -8 * w3.abs() + 1e-6 * ad.abs().clamp(min=1.0)
    else:   # GELU and its derivative to 1e-5 (the derivative is multiplied by dy)
        b2, b3 = torch.full_like(w2, 1e-5), 1e-5 * ad.abs().clamp(min=1.0)
    assert _ratio("gelu", r2, w2, b2) <= 1.0 and _ratio("gelu_bwd", r3, w3, b3) <= 1.0
    return r0, r1, r2, r3


@pytest.mark.parametrize("dt", [torch.float32, BF], ids=["f32", "bf16"])
def test_act_ops(C, dt):
    g = torch.Generator().manual_seed(5)
    a = (2.0 * torch.randn(N_ODD, generator=g)).to(dt).to(dev)
    b = (2.0 * torch.randn(N_ODD, generator=g)).to(dt).to(dev)
    a[:4] = torch.tensor([0.0, -0.0, 6.0, -6.0], dtype=dt)
    _act_check(C, a, b, f"act {dt} n={N_ODD}")


def test_act_bf16_misaligned_view(C):
    """A bf16 operand that starts 2 bytes into its buffer (contiguous, n % 8 == 0, not 16-byte aligned) takes
    the scalar kernel; the aligned copy takes the 8-wide one: same values, same bits."""
    g = torch.Generator().manual_seed(6)
    n = 8 * 4099
    big_a = (2.0 * torch.randn(n + 1, generator=g)).to(BF).to(dev)
    big_b = (2.0 * torch.randn(n + 1, generator=g)).to(BF).to(dev)
    a, b = big_a[1:], big_b[1:]
    assert a.is_contiguous() and a.data_ptr() % 16 == 2 and a.numel() % 8 == 0
    mis = _act_check(C, a, b, "act bf16 misaligned")
    ali = _act_check(C, a.clone(), b.clone(), "act bf16 aligned")
    assert a.clone().data_ptr() % 16 == 0
    for x, y in zip(mis, ali):
        assert _same_bits(x, y)
