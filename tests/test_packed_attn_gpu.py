"""Packed-document causal attention on the GPU (attn.hip's packed LDS-DMA kernels, the embedding kernels with
position ids, the GPT-2 model with doc_start) against the fp64 reference of tests/_packed_attn_ref.py: per
element, max |err| / bound <= 1 under the rounding budgets of _gpt2_ref.py; every case prints its worst ratio.

Measured (MI355X, worst |err| / bound; 1.0 = at the bound):

    attention, packed LDS-DMA kernels   out    lse2   dQ     dK     dV
      T 128, boundary at 64             0.534  0.282  0.126  0.208  0.517
      T 128, boundary at 70             0.527  0.282  0.117  0.207  0.467
      T 128, boundaries at 1 and 127    0.673  0.252  0.106  0.188  0.535
      T 128, every token a document     0.000  0.000  0.000  0.000  0.000   (out == v, dV == dout bitwise;
                                                                             max |dQ|, |dK| 9.5e-07)
      T 192, boundaries at 100, 130     0.527  0.264  0.157  0.145  0.533
      T 256, B 2, geometric mean 24     0.629  0.359  0.175  0.219  0.579
      T 256, doc_start = 0              0.613  0.257  0.107  0.151  0.525   (bit-equal to the causal kernels:
                                                                             out, lse and dqkv)
      leak, base / perturbed            0.550  0.319  0.137  0.236  0.592   (the other documents bit-identical)
    torch fallback (T 100)              0.487  -      dqkv 0.326
    embedding_bwd with pos              dwte 0.114   dwpe 0.143
    graph replay of a packed training step: loss bit-equal to the eager step's (6.267364, 6.243253)
"""
import copy
import math

import pytest
import torch

import _gpt2_ref as R
import _packed_attn_ref as P
from distributed_pytorch_example_amd.models import get_model
from distributed_pytorch_example_amd.ops import functional as Fx

pytestmark = pytest.mark.gpu
dev = "cuda"
BF = torch.bfloat16
SCALE = 0.125  # 1 / sqrt(64)
H = 2


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


def _canary(shape, dtype, n_real):
    """A buffer of random bits; (buffer, its first n_real elements as a flat view, a copy of the rest)."""
    g = torch.Generator(device="cpu").manual_seed(12345)
    if dtype == BF:
        raw = torch.randint(-32768, 32767, shape, generator=g, dtype=torch.int16).to(dev).view(BF)
    else:
        raw = torch.randint(-2 ** 31, 2 ** 31 - 1, shape, generator=g, dtype=torch.int32).to(dev).view(torch.float32)
    flat = raw.view(-1)
    return raw, flat[:n_real], _bits(flat[n_real:]).clone()


def _packed_run(C, qkv, dout, ds, guard=True):
    """attn_fwd + attn_bwd with the document bounds of ``ds``; with ``guard`` the outputs are the leading part of
    larger buffers whose remaining 128 rows per batch entry must come back bit-unchanged."""
    B, T, _, Hh, D = qkv.shape
    s, e, _ = Fx.doc_bounds(ds.to(dev))
    if not guard:
        out, lse = C.attn_fwd(qkv, Hh, SCALE, True, doc_start=s, doc_end=e)
        dqkv = C.attn_bwd(qkv, out, dout, lse, Hh, SCALE, True, doc_start=s, doc_end=e)
        torch.cuda.synchronize()
        return out, lse, dqkv
    bo, fo, co = _canary((B, T + 128, Hh, D), BF, B * T * Hh * D)
    bl, fl, cl = _canary((B, Hh, T + 128), torch.float32, B * Hh * T)
    bd, fd, cd = _canary((B, T + 128, 3, Hh, D), BF, B * T * 3 * Hh * D)
    out, lse, dqkv = fo.view(B, T, Hh, D), fl.view(B, Hh, T), fd.view(B, T, 3, Hh, D)
    C.attn_fwd(qkv, Hh, SCALE, True, out=out, lse=lse, doc_start=s, doc_end=e)
    C.attn_bwd(qkv, out, dout, lse, Hh, SCALE, True, dqkv=dqkv, doc_start=s, doc_end=e)
    torch.cuda.synchronize()
    assert torch.equal(_bits(bo.view(-1)[fo.numel():]), co), "attn_fwd stored past the end of out"
    assert torch.equal(_bits(bl.view(-1)[fl.numel():]), cl), "attn_fwd stored past the end of lse"
    assert torch.equal(_bits(bd.view(-1)[fd.numel():]), cd), "attn_bwd stored past the end of dqkv"
    return out, lse, dqkv


def _check(tag, got, ref):
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


def _randn_case(B, T, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, T, 3, H, 64, generator=g).to(BF).to(dev)
    dout = torch.randn(B, T, H, 64, generator=g).to(BF).to(dev)
    return qkv, dout


# name -> (B, T, doc_start [B, T])
def _layouts():
    return {
        "T128_b64": (1, 128, P.doc_start_of(128, [64])[None]),            # whole-tile skip, no lower mask
        "T128_b70": (1, 128, P.doc_start_of(128, [70])[None]),            # a tile fully masked for rows with m = -inf
        "T128_b1_127": (1, 128, P.doc_start_of(128, [1, 127])[None]),     # one-token documents at both ends
        "T128_each": (1, 128, torch.arange(128, dtype=torch.int32)[None]),  # every token its own document
        "T192_b100_130": (1, 192, P.doc_start_of(192, [100, 130])[None]),  # odd tile count, half-live last workgroup,
        #                                                                    a document across the 128-row edge
        "T256_geo24": (2, 256, P.geometric_doc_start(2, 256, 24, seed=5)),  # general, rows differ
    }


@pytest.mark.parametrize("name", list(_layouts()))
def test_packed_layouts(C, name):
    B, T, ds = _layouts()[name]
    if name == "T256_geo24":
        assert not torch.equal(ds[0], ds[1])
    Fx.check_doc_start(ds)
    qkv, dout = _randn_case(B, T, 200 + T + len(name))
    ref = P.packed_attn_ref(qkv, dout, SCALE, ds)
    got = _packed_run(C, qkv, dout, ds)
    _check(f"packed {name}", got, ref)
    if name == "T128_each":
        # the reference itself: out = v, dV = dout, dQ = dK = 0 (softmax over one key)
        assert torch.equal(ref["out"], qkv[:, :, 2].double()) and torch.equal(ref["dqkv"][:, :, 2], dout.double())
        assert ref["dqkv"][:, :, :2].abs().max().item() < 1e-12
        print(f"  out == v bitwise: {_same_bits(got[0], qkv[:, :, 2])}, dV == dout bitwise: "
              f"{_same_bits(got[2][:, :, 2], dout)}, max |dQ|, |dK| = {got[2][:, :, :2].float().abs().max().item():.3g}")


def test_packed_doc_start_zero_is_causal(C):
    """doc_start = 0 everywhere is plain causal attention: under attn_ref's budgets; whether the packed kernels
    are bit-equal to the causal ones is printed."""
    B, T = 1, 256
    qkv, dout = _randn_case(B, T, 77)
    got = _packed_run(C, qkv, dout, torch.zeros(B, T, dtype=torch.int32))
    _check("packed doc_start=0 (T 256)", got, R.attn_ref(qkv, dout, SCALE))
    out, lse = C.attn_fwd(qkv, H, SCALE, True)
    dqkv = C.attn_bwd(qkv, out, dout, lse, H, SCALE, True)
    print(f"  bit-equal to the causal kernels: out {_same_bits(out, got[0])}, lse {_same_bits(lse, got[1])}, "
          f"dqkv {_same_bits(dqkv, got[2])}")


def test_packed_leak_exact(C):
    """Documents [0, 70), [70, 200), [200, 256): replacing the middle one's q, k, v, dout by fresh noise 16 times
    as large changes no bit of what the other two receive (a masked P is exactly 0 and the tile schedule depends
    on doc_start only), and the perturbed run is within budget."""
    T, lo, hi = 256, 70, 200
    ds = P.doc_start_of(T, [lo, hi])[None]
    qkv, dout = _randn_case(1, T, 91)
    got = _packed_run(C, qkv, dout, ds)
    _check("leak base", got, P.packed_attn_ref(qkv, dout, SCALE, ds))
    q2, d2 = _randn_case(1, T, 92)
    qkv2, dout2 = qkv.clone(), dout.clone()
    qkv2[:, lo:hi], dout2[:, lo:hi] = q2[:, lo:hi] * 16, d2[:, lo:hi] * 16
    got2 = _packed_run(C, qkv2, dout2, ds)
    for t in got2:
        assert torch.isfinite(t.float()).all()
    _check("leak perturbed", got2, P.packed_attn_ref(qkv2, dout2, SCALE, ds))
    for sl in (slice(0, lo), slice(hi, T)):
        assert _same_bits(got[0][:, sl], got2[0][:, sl]), "out of another document changed"
        assert _same_bits(got[1][..., sl], got2[1][..., sl]), "lse of another document changed"
        assert _same_bits(got[2][:, sl], got2[2][:, sl]), "dqkv of another document changed"
    assert not _same_bits(got[0][:, lo:hi], got2[0][:, lo:hi])


def test_packed_determinism(C):
    B, T, ds = _layouts()["T256_geo24"]
    qkv, dout = _randn_case(B, T, 51)
    a = _packed_run(C, qkv, dout, ds, guard=False)
    b = _packed_run(C, qkv, dout, ds, guard=False)
    for x, y in zip(a, b):
        assert _same_bits(x, y)


def test_packed_needs_the_dma_kernels(C):
    """The register-staged kernels have no packed variant: an error, not the plain causal result."""
    qkv, dout = _randn_case(1, 128, 3)
    s, e, _ = Fx.doc_bounds(P.doc_start_of(128, [70])[None].to(dev))
    prev = C.set_attn_staged(True)
    try:
        with pytest.raises(RuntimeError):
            C.attn_fwd(qkv, H, SCALE, True, doc_start=s, doc_end=e)
    finally:
        C.set_attn_staged(prev)
    with pytest.raises(RuntimeError):
        C.attn_fwd(qkv, H, SCALE, True, doc_start=s)  # doc_end goes with it


# ------------------------------------------------------------------ embedding
def test_embedding_fwd_with_pos_exact(C):
    g = torch.Generator().manual_seed(1)
    Vn, T, D, B = 301, 48, 72, 3
    wte = (0.02 * torch.randn(Vn, D, generator=g)).to(BF).to(dev)
    wpe = (0.02 * torch.randn(T + 5, D, generator=g)).to(BF).to(dev)
    idx = torch.randint(0, Vn, (B, T), generator=g).to(dev)
    ds = torch.stack([P.doc_start_of(T, [1, 20, 47]), P.doc_start_of(T, []), torch.arange(T, dtype=torch.int32)]).to(dev)
    pos = Fx.doc_bounds(ds)[2]
    got = C.embedding_fwd(idx, wte, wpe, pos)
    want = wte.float()[idx] + wpe.float()[pos.long()]
    assert got.dtype == torch.float32 and _same_bits(got, want)
    assert not _same_bits(got, C.embedding_fwd(idx, wte, wpe))
    assert _same_bits(C.embedding_fwd(idx, wte, wpe, pos=None), C.embedding_fwd(idx, wte, wpe))


def test_embedding_bwd_with_pos(C):
    """dwpe rows by position id; the budget of test_embedding_bwd (fp32 sums in any order: 1e-6 of the sum of
    |contributions| per element)."""
    g = torch.Generator().manual_seed(2)
    Vn, B, T, D = 97, 4, 64, 64
    idx = torch.randint(0, Vn, (B, T), generator=g).to(dev)
    dout = torch.randn(B, T, D, generator=g).to(dev)
    dwte0 = torch.randn(Vn, D, generator=g).to(dev)
    dwpe0 = torch.randn(T, D, generator=g).to(dev)
    ds = P.geometric_doc_start(B, T, 6, seed=3).to(dev)
    pos = Fx.doc_bounds(ds)[2]
    dwte, dwpe = dwte0.clone(), dwpe0.clone()
    C.embedding_bwd(idx, dout, dwte, dwpe, pos)
    torch.cuda.synchronize()
    dd = dout.double().view(-1, D)
    want = dwte0.double().index_add(0, idx.view(-1), dd)
    mag = dwte0.double().abs().index_add(0, idx.view(-1), dd.abs())
    print("embedding_bwd with pos")
    assert _ratio("dwte", dwte, want, 1e-6 * mag + R.FLOOR) <= 1.0
    wantp = dwpe0.double().index_add(0, pos.view(-1).long(), dd)
    magp = dwpe0.double().abs().index_add(0, pos.view(-1).long(), dd.abs())
    assert _ratio("dwpe", dwpe, wantp, 1e-6 * magp + R.FLOOR) <= 1.0


# ---------------------------------------------------------------------- model
def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


def _cos(a, b):
    a, b = a.float().flatten(), b.float().flatten()
    return (a @ b / (a.norm() * b.norm() + 1e-12)).item()


def _model_doc_start(T=128):
    return torch.stack([P.doc_start_of(T, [1, 40, 70, 127]), P.doc_start_of(T, [64])])


def test_gpt2_tiny_packed_gpu_vs_cpu(C):
    """Fused blocks, bf16, T 128, mixed boundaries against the CPU fp32 model with the same doc_start; the bounds
    of test_models_gpu.py::test_gpt2_tiny_gpu_vs_cpu."""
    torch.manual_seed(4)
    cpu = get_model("gpt2-tiny")
    gpu = copy.deepcopy(cpu).to(dev)
    assert all(b.fused for b in gpu.h)
    idx = torch.randint(0, 512, (2, 128))
    tgt = torch.randint(0, 512, (2, 128))
    ds = _model_doc_start()
    lc = Fx.cross_entropy(cpu(idx, None, ds), tgt)
    lc.backward()
    lg = Fx.cross_entropy(gpu(idx.to(dev), None, ds.to(dev)), tgt.to(dev))
    lg.backward()
    assert abs(lc.item() - lg.item()) < 2e-2 * abs(lc.item())
    gc = dict(cpu.named_parameters())
    for n, p in gpu.named_parameters():
        assert _cos(p.grad.cpu(), gc[n].grad) > 0.98, n
        assert _rel(p.grad.cpu(), gc[n].grad) < 0.1, n
    # and doc_start matters: the logits without it differ
    with torch.no_grad():
        a, b = gpu(idx.to(dev), None, ds.to(dev)), gpu(idx.to(dev))
    assert _rel(a, b) > 1e-2


def test_gpt2_packed_fused_block_matches_per_op(C):
    torch.manual_seed(8)
    m1 = get_model("gpt2-tiny", n_layer=3).to(dev)
    m2 = copy.deepcopy(m1)
    for b in m2.h:
        b.fused = False
    assert all(b.fused for b in m1.h)
    idx = torch.randint(0, 512, (2, 128), device=dev)
    tgt = torch.randint(0, 512, (2, 128), device=dev)
    ds = _model_doc_start().to(dev)
    l1, l2 = m1(idx, tgt, ds), m2(idx, tgt, ds)
    assert abs(l1.item() - l2.item()) < 1e-4 * abs(l2.item())
    l1.backward()
    l2.backward()
    g2 = dict(m2.named_parameters())
    for n, p in m1.named_parameters():
        assert _cos(p.grad, g2[n].grad) > 0.999, n
        assert _rel(p.grad, g2[n].grad) < 0.02, n


def test_packed_attention_T100_falls_back(C):
    """T % 64 != 0: the torch masked-softmax path with the document mask, under the budgets of the existing
    fallback test (its only roundings are the bf16 outputs)."""
    B, T, D = 2, 100, 64
    g = torch.Generator().manual_seed(170)
    qkv = torch.randn(B, T, 3 * H * D, generator=g).to(BF).to(dev).requires_grad_(True)
    dout = torch.randn(B, T, H * D, generator=g).to(BF).to(dev)
    ds = torch.stack([P.doc_start_of(T, [1, 33, 64, 99]), P.doc_start_of(T, [70])])
    out = Fx.causal_attention(qkv, H, Fx.doc_bounds(ds.to(dev)))
    assert out.shape == (B, T, H * D) and out.dtype == BF
    out.backward(dout)
    ref = P.packed_attn_ref(qkv.detach().view(B, T, 3, H, D), dout.view(B, T, H, D), 1.0 / math.sqrt(D), ds)
    print("packed fallback T=100")
    assert _ratio("out", out.detach().view(B, T, H, D), ref["out"], ref["b_out"]) <= 1.0
    assert _ratio("dqkv", qkv.grad.view(B, T, 3, H, D), ref["dqkv"], ref["b_dqkv"]) <= 1.0


def test_packed_training_step_replays_in_a_graph(C):
    """One packed GPT-2-tiny training step (forward, backward, AdamW) captured in a graph: a replay on a new
    batch and new doc_start gives, bit for bit, the loss of the eager step from the same parameters -- nothing
    in the step is derived on the host."""
    from distributed_pytorch_example_amd.optim import AdamW

    torch.manual_seed(12)
    m1 = get_model("gpt2-tiny").to(dev)
    m2 = copy.deepcopy(m1)
    o1, o2 = AdamW(m1.parameters(), lr=1e-4), AdamW(m2.parameters(), lr=1e-4)
    for m in (m1, m2):
        for p in m.parameters():
            p.grad = torch.zeros_like(p)
    xs = [torch.randint(0, 512, (2, 128), device=dev) for _ in range(3)]
    dss = [P.geometric_doc_start(2, 128, m, seed=s).to(dev) for m, s in ((16, 1), (40, 2), (5, 3))]
    ys = [x.roll(-1, 1) for x in xs]

    def step(model, opt, x, y, ds):
        loss = model(x, y, ds)
        loss.backward()
        opt.step()
        opt.zero_grad(set_to_none=False)
        return loss

    sx, sy, sd = xs[0].clone(), ys[0].clone(), dss[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step(m1, o1, sx, sy, sd)
    torch.cuda.current_stream().wait_stream(side)
    o1.graph_safe = True
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gl = step(m1, o1, sx, sy, sd)
    for i in (1, 2):
        with torch.no_grad():  # the eager model starts the step from the graph model's parameters
            for a, b in zip(m2.parameters(), m1.parameters()):
                a.copy_(b)
        sx.copy_(xs[i])
        sy.copy_(ys[i])
        sd.copy_(dss[i])
        g.replay()
        le = step(m2, o2, xs[i], ys[i], dss[i])
        torch.cuda.synchronize()
        print(f"  replay {i}: graph loss {gl.item():.6f}, eager loss {le.item():.6f}")
        assert _same_bits(gl.detach().float().reshape(1), le.detach().float().reshape(1))
    assert not torch.equal(dss[1], dss[2])
