"""Grouped-query attention (attn_fwd / attn_bwd with n_kv_head; the attn_*_gqa_kernel entry points of attn.hip) against
the fp64 references of _gpt2_ref.py / _packed_attn_ref.py: K and V are expanded to one head per query head, the
reference is evaluated on that, and dK, dV and their bounds are summed over each group.  The summed bound holds
because the kernel rounds the fp32 group sum to bf16 once: by the triangle inequality the summed 2^-9 |dK_h| terms
cover that one rounding.  Pass = max |err| / bound <= 1 per element, printed by every check.

Measured (MI355X, worst |err| / bound over the cases of the test):

                               out    lse2   dQ     dK     dV
    shapes                     0.582  0.364  0.134  0.153  0.461
    group independence         0.517  0.284  0.115  0.164  0.541
    packed                     0.551  0.275  0.169  0.263  0.531
    Fx fallback (T 100, D 32)  0.476  -      dqkv 0.462
"""
import math

import pytest
import torch

import _gpt2_ref as R
from _packed_attn_ref import doc_start_of, packed_attn_ref
from distributed_pytorch_example_amd.ops import functional as Fx
from test_gpt2_kernels_gpu import BF, SCALE, _Staged, _bits, _canary, _randn_case, _ratio, _same_bits, dev

pytestmark = pytest.mark.gpu


def _case(B, T, Hq, Hkv, seed, D=64):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, T, Hq + 2 * Hkv, D, generator=g).to(BF).to(dev)
    return qkv, torch.randn(B, T, Hq, D, generator=g).to(BF).to(dev)


def _ref(qkv, dout, Hq, Hkv, scale=SCALE, doc_start=None):
    """The fp64 reference on K / V expanded to Hq heads; dK, dV and their bounds summed over each group."""
    B, T, _, D = qkv.shape
    q, k, v = qkv.split([Hq, Hkv, Hkv], dim=2)
    G = Hq // Hkv
    qkv5 = torch.stack([q, k.repeat_interleave(G, dim=2), v.repeat_interleave(G, dim=2)], dim=2)
    r = R.attn_ref(qkv5, dout, scale) if doc_start is None else packed_attn_ref(qkv5, dout, scale, doc_start)

    def fold(a):  # [B, T, 3, Hq, D] -> [B, T, Hq + 2 Hkv, D]
        return torch.cat([a[:, :, 0]] + [a[:, :, i].reshape(B, T, Hkv, G, D).sum(3) for i in (1, 2)], dim=2)

    return dict(r, dqkv=fold(r["dqkv"]), b_dqkv=fold(r["b_dqkv"]))


def _run(C, qkv, dout, Hq, Hkv, doc_start=None):
    """attn_fwd + attn_bwd with n_kv_head into buffers followed by 128 canary rows, which must come back unchanged."""
    B, T, W, D = qkv.shape
    kw = dict(n_kv_head=Hkv)
    if doc_start is not None:
        kw["doc_start"], kw["doc_end"], _ = Fx.doc_bounds(doc_start.to(dev))
    bo, fo, co = _canary((B, T + 128, Hq, D), BF, B * T * Hq * D)
    bl, fl, cl = _canary((B, Hq, T + 128), torch.float32, B * Hq * T)
    bd, fd, cd = _canary((B, T + 128, W, D), BF, B * T * W * D)
    out, lse, dqkv = fo.view(B, T, Hq, D), fl.view(B, Hq, T), fd.view(B, T, W, D)
    C.attn_fwd(qkv, Hq, SCALE, True, out=out, lse=lse, **kw)
    C.attn_bwd(qkv, out, dout, lse, Hq, SCALE, True, dqkv=dqkv, **kw)
    torch.cuda.synchronize()
    assert torch.equal(_bits(bo.view(-1)[fo.numel():]), co), "attn_fwd stored past the end of out"
    assert torch.equal(_bits(bl.view(-1)[fl.numel():]), cl), "attn_fwd stored past the end of lse"
    assert torch.equal(_bits(bd.view(-1)[fd.numel():]), cd), "attn_bwd stored past the end of dqkv"
    return out, lse, dqkv


def _check(tag, got, ref, Hq, Hkv):
    out, lse, dqkv = got
    print(tag)
    parts = dict(zip(("dQ", "dK", "dV"), zip(dqkv.split([Hq, Hkv, Hkv], 2), ref["dqkv"].split([Hq, Hkv, Hkv], 2),
                                              ref["b_dqkv"].split([Hq, Hkv, Hkv], 2))))
    rs = {"out": _ratio("out", out, ref["out"], ref["b_out"]),
          "lse2": _ratio("lse2", lse, ref["lse2"], torch.full_like(ref["lse2"], ref["b_lse2"]))}
    rs.update({k: _ratio(k, *p) for k, p in parts.items()})
    for k, r in rs.items():
        assert r <= 1.0, f"{tag}: {k} exceeds its rounding budget, worst ratio {r:.3f}"


# one tile | MQA: one workgroup walks four heads | T % 128 == 64, two groups | G = 3: three key workgroups with a
# dead-wave tail, 5 / 3 / 1 query tiles per head, so the head change meets the ring at both parities
SHAPES = [(1, 64, 2, 1), (1, 128, 4, 1), (2, 192, 4, 2), (1, 320, 6, 2)]


@pytest.mark.parametrize("B,T,Hq,Hkv", SHAPES)
def test_gqa_shapes(C, B, T, Hq, Hkv):
    qkv, dout = _case(B, T, Hq, Hkv, 300 + T)
    _check(f"gqa B={B} T={T} Hq={Hq} Hkv={Hkv}", _run(C, qkv, dout, Hq, Hkv), _ref(qkv, dout, Hq, Hkv), Hq, Hkv)


def test_gqa_one_head_per_group_is_todays_call(C):
    """G = 1: the layout is today's byte for byte, and the GQA kernels give the bits of the call without n_kv_head."""
    qkv5, dout = _randn_case(2, 128, 2, 41)
    out0, lse0 = C.attn_fwd(qkv5, 2, SCALE, True)
    dq0 = C.attn_bwd(qkv5, out0, dout, lse0, 2, SCALE, True)
    out, lse, dqkv = _run(C, qkv5.view(2, 128, 6, 64), dout, 2, 2)
    assert _same_bits(out, out0) and _same_bits(lse, lse0) and _same_bits(dqkv, dq0.view(2, 128, 6, 64))


def test_gqa_group_independence(C):
    """(1, 128, 4, 2): group 1's inputs reach no output bit of group 0; swapping the two query heads of a group swaps
    their out / dQ bitwise and leaves dV bit-identical (P and dO only change places in the walk; dK's fp32 sum takes
    the heads in the other order, so it is held to the bound)."""
    Hq, Hkv = 4, 2
    qkv, dout = _case(1, 128, Hq, Hkv, 77)
    out, lse, dqkv = _run(C, qkv, dout, Hq, Hkv)
    g0 = [0, 1, 4, 6]  # group 0's rows of qkv / dqkv: query heads 0 and 1, K head 0, V head 0
    q2, d2 = _case(1, 128, Hq, Hkv, 78)
    q2[:, :, g0], d2[:, :, :2] = qkv[:, :, g0], dout[:, :, :2]
    out2, lse2, dqkv2 = _run(C, q2, d2, Hq, Hkv)
    assert _same_bits(out2[:, :, :2], out[:, :, :2]) and _same_bits(lse2[:, :2], lse[:, :2])
    assert _same_bits(dqkv2[:, :, g0], dqkv[:, :, g0])
    perm, hp = [1, 0, 2, 3, 4, 5, 6, 7], [1, 0, 2, 3]
    q3, d3 = qkv[:, :, perm].contiguous(), dout[:, :, hp].contiguous()
    got3 = _run(C, q3, d3, Hq, Hkv)
    assert _same_bits(got3[0], out[:, :, hp]) and _same_bits(got3[1], lse[:, hp])
    assert _same_bits(got3[2][:, :, :Hq], dqkv[:, :, hp]) and _same_bits(got3[2][:, :, 6:], dqkv[:, :, 6:])
    _check("gqa permuted heads", got3, _ref(q3, d3, Hq, Hkv), Hq, Hkv)


def test_gqa_packed(C):
    """Documents starting at 0, 70 (inside a tile) and 128 (on a tile edge), against the packed reference."""
    B, T, Hq, Hkv = 1, 256, 4, 2
    qkv, dout = _case(B, T, Hq, Hkv, 91)
    ds = doc_start_of(T, [70, 128]).unsqueeze(0)
    _check("gqa packed", _run(C, qkv, dout, Hq, Hkv, ds), _ref(qkv, dout, Hq, Hkv, doc_start=ds), Hq, Hkv)


@pytest.mark.parametrize("what", ["dropout", "seq_len", "staged", "indivisible"])
def test_gqa_refusals(C, what):
    """n_kv_head with dropout, with seq_len, under the staged switch, or not dividing H: an error, not a fallback."""
    Hkv = 4 if what == "indivisible" else 2
    qkv = torch.zeros(1, 64, 6 + 2 * Hkv, 64, dtype=BF, device=dev)
    kw = {"dropout": dict(dropout_p=0.1, rng=torch.zeros(2, dtype=torch.int64, device=dev)), "seq_len": dict(seq_len=32)}
    with _Staged(C, what == "staged"), pytest.raises(RuntimeError):
        C.attn_fwd(qkv, 6, SCALE, True, n_kv_head=Hkv, **kw.get(what, {}))
    out, lse = torch.zeros(1, 64, 6, 64, dtype=BF, device=dev), torch.zeros(1, 6, 64, device=dev)
    with _Staged(C, what == "staged"), pytest.raises(RuntimeError):
        C.attn_bwd(qkv, out, out, lse, 6, SCALE, True, n_kv_head=Hkv, **kw.get(what, {}))


def test_fx_causal_attention_n_kv_head(C):
    """Fx.causal_attention(n_kv_head=): the direct calls' bits at a kernel shape; at (T 100, D 32) the torch fallback
    (K / V expanded by repeat_interleave), inside the same bounds."""
    B, T, Hq, Hkv = 2, 128, 4, 2
    qkv, dout = _case(B, T, Hq, Hkv, 55)
    out, _, dqkv = _run(C, qkv, dout, Hq, Hkv)
    x = qkv.view(B, T, -1).clone().requires_grad_(True)
    y = Fx.causal_attention(x, Hq, n_kv_head=Hkv)
    y.backward(dout.view(B, T, -1))
    assert _same_bits(y.detach(), out.view(B, T, -1)) and _same_bits(x.grad, dqkv.view(B, T, -1))
    T, D = 100, 32
    qkv, dout = _case(B, T, Hq, Hkv, 56, D)
    x = qkv.view(B, T, -1).clone().requires_grad_(True)
    y = Fx.causal_attention(x, Hq, n_kv_head=Hkv)
    assert y.shape == (B, T, Hq * D) and y.dtype == BF
    y.backward(dout.view(B, T, -1))
    ref = _ref(qkv, dout, Hq, Hkv, 1.0 / math.sqrt(D))
    print("gqa fallback T=100 D=32")
    assert _ratio("out", y.detach().view(B, T, Hq, D), ref["out"], ref["b_out"]) <= 1.0
    assert _ratio("dqkv", x.grad.view(B, T, -1, D), ref["dqkv"], ref["b_dqkv"]) <= 1.0
