"""Dropout on the GPU: the DROP instantiations of attn.hip's three LDS-DMA kernels, eltwise.hip's dropout_add /
dropout_cast and the GPT-2 model with cfg.dropout, against the numpy mask and the fp64 reference of
tests/_attn_dropout_ref.py: per element, max |err| / bound <= 1; every case prints its worst ratio.

Measured (MI355X, worst |err| / bound; 1.0 = at the bound):

    attention, DROP LDS-DMA kernels          out    lse2   dQ     dK     dV     fully dropped rows
      T 64, p 0.1                            0.478  0.276  0.133  0.176  0.579  0
      T 128, p 0.1                           0.718  0.307  0.095  0.208  0.528  0
      T 128, p 0.5                           0.633  0.307  0.186  0.335  0.458  2
      T 192, thr 230                         0.847  0.325  0.225  0.298  0.567  18
      T 256, B 2, offset 2^33 + 5, stream 7  0.520  0.444  0.127  0.175  0.493  1
      packed, T 128, boundary at 70          0.618  0.306  0.150  0.141  0.532  0
      packed, T 256, geometric mean 24       0.737  0.339  0.185  0.199  0.594  2
    dropout_add   0.957 / 0.904 (bf16 y, n 1027 / 8192), 0.892 / 0.956 (fp32 y)
    dropout_cast  0.929 / 0.981
    graph replay of a training step with dropout 0.1: loss bit-equal to the eager step's (6.275744, 6.238026);
    lr = 0 replays 6.078281, 6.070683, 6.072996
"""
import copy
import dataclasses

import numpy as np
import pytest
import torch

import _attn_dropout_ref as D
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


def _rng(seed, offset):
    return torch.tensor([seed, offset], dtype=torch.int64, device=dev)


def _randn_case(B, T, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, T, 3, H, 64, generator=g).to(BF).to(dev)
    dout = torch.randn(B, T, H, 64, generator=g).to(BF).to(dev)
    return qkv, dout


def _drop_run(C, qkv, dout, ds, p, rng, stream, guard=True):
    """attn_fwd + attn_bwd with dropout; with ``guard`` the outputs are the leading part of larger buffers whose
    remaining 128 rows per batch entry must come back bit-unchanged."""
    B, T, _, Hh, Dh = qkv.shape
    kw = dict(dropout_p=p, rng=rng, stream=stream)
    if ds is not None:
        s, e, _ = Fx.doc_bounds(ds.to(dev))
        kw.update(doc_start=s, doc_end=e)
    if not guard:
        out, lse = C.attn_fwd(qkv, Hh, SCALE, True, **kw)
        dqkv = C.attn_bwd(qkv, out, dout, lse, Hh, SCALE, True, **kw)
        torch.cuda.synchronize()
        return out, lse, dqkv
    bo, fo, co = _canary((B, T + 128, Hh, Dh), BF, B * T * Hh * Dh)
    bl, fl, cl = _canary((B, Hh, T + 128), torch.float32, B * Hh * T)
    bd, fd, cd = _canary((B, T + 128, 3, Hh, Dh), BF, B * T * 3 * Hh * Dh)
    out, lse, dqkv = fo.view(B, T, Hh, Dh), fl.view(B, Hh, T), fd.view(B, T, 3, Hh, Dh)
    C.attn_fwd(qkv, Hh, SCALE, True, out=out, lse=lse, **kw)
    C.attn_bwd(qkv, out, dout, lse, Hh, SCALE, True, dqkv=dqkv, **kw)
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


# ------------------------------------------------------------------- anchor
def test_numpy_philox_reproduces_the_existing_dropout(C):
    """The reference Philox against code older than the attention dropout: C.dropout's keep pattern."""
    n, p, seed, off = 4099, 0.5, 0x1234567 * 2 ** 20 + 89, 2 ** 33 + 77
    y = C.dropout(torch.ones(n, device=dev), p, seed, off)
    want = D.eltwise_keep(seed, off, 0, n, p)
    got = (y != 0).cpu()
    assert torch.equal(got, want)
    assert 0.4 < want.float().mean().item() < 0.6
    assert torch.equal(y.cpu()[want], torch.full((int(want.sum()),), 2.0))


# ---------------------------------------------------------------- attention
# name -> (B, T, p, seed, offset, stream, doc_start | None)
def _cases():
    return {
        "T64_p0.1": (1, 64, 0.1, 1234, 0, 3, None),                       # a single diagonal tile
        "T128_p0.1": (1, 128, 0.1, 1234, 0, 3, None),                     # full tile + diagonal tile
        "T128_p0.5": (1, 128, 0.5, 1234, 0, 3, None),                     # ... with dead rows
        "T192_thr230": (1, 192, 230 / 256, 99, 0, 3, None),               # odd tile count, half-live last workgroup
        "T256_B2_off2p33": (2, 256, 0.1, 1234, 2 ** 33 + 5, 7, None),     # two workgroups per kernel, 64-bit counter add
        "packed_T128_b70": (1, 128, 0.1, 1234, 0, 3, P.doc_start_of(128, [70])[None]),
        "packed_T256_geo24": (2, 256, 0.1, 1234, 0, 3, P.geometric_doc_start(2, 256, 24, seed=5)),
    }


_REF = {}


def _case(name):
    """(inputs, reference) of a case, computed once and shared by the tests that use it."""
    if name not in _REF:
        B, T, p, seed, off, stream, ds = _cases()[name]
        qkv, dout = _randn_case(B, T, 300 + T + len(name))
        thr = D.attn_threshold(p)
        keep = D.keep_mask(seed, off, stream, B, H, T, thr)
        _REF[name] = (qkv, dout, D.attn_dropout_ref(qkv.cpu(), dout.cpu(), SCALE, ds, keep, thr))
    return _REF[name]


@pytest.mark.parametrize("name", list(_cases()))
def test_attn_dropout_against_fp64(C, name):
    B, T, p, seed, off, stream, ds = _cases()[name]
    qkv, dout, ref = _case(name)
    refd = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in ref.items()}
    got = _drop_run(C, qkv, dout, ds, p, _rng(seed, off), stream)
    # (lse2 is checked against the UNDROPPED softmax's: the reference's lse2 ignores the mask)
    _check(f"attn dropout {name} (thr {D.attn_threshold(p)}, rate {Fx.attn_dropout_rate(p):.4f})", got, refd)
    dead = refd["dead"]  # [B, H, T]
    nd = int(dead.sum())
    print(f"  fully dropped rows: {nd}")
    if name in ("T128_p0.5", "T192_thr230"):
        assert nd > 0
    out, _, dqkv = got
    dead_bt = dead.permute(0, 2, 1)  # [B, T, H]
    if nd:
        assert out[dead_bt].float().abs().max().item() == 0.0, "a dead row's output is not exactly 0"
        assert dqkv[:, :, 0][dead_bt].float().abs().max().item() == 0.0, "a dead row's dQ is not exactly 0"


def test_attn_dropout_p0_is_the_plain_call(C):
    qkv, dout = _randn_case(2, 256, 11)
    out, lse = C.attn_fwd(qkv, H, SCALE, True)
    dqkv = C.attn_bwd(qkv, out, dout, lse, H, SCALE, True)
    for rng in (None, _rng(5, 6)):
        o2, l2 = C.attn_fwd(qkv, H, SCALE, True, dropout_p=0.0, rng=rng, stream=9)
        d2 = C.attn_bwd(qkv, o2, dout, l2, H, SCALE, True, dropout_p=0.0, rng=rng, stream=9)
        assert _same_bits(out, o2) and _same_bits(lse, l2) and _same_bits(dqkv, d2)


def test_attn_dropout_determinism_streams_and_offsets(C):
    qkv, dout = _randn_case(2, 256, 12)
    a = _drop_run(C, qkv, dout, None, 0.1, _rng(1234, 40), 3, guard=False)
    b = _drop_run(C, qkv, dout, None, 0.1, _rng(1234, 40), 3, guard=False)
    for x, y in zip(a, b):
        assert _same_bits(x, y)
    c = _drop_run(C, qkv, dout, None, 0.1, _rng(1234, 40), 4, guard=False)
    d = _drop_run(C, qkv, dout, None, 0.1, _rng(1234, 41), 3, guard=False)
    assert not _same_bits(a[0], c[0]), "another stream gives the same mask"
    assert not _same_bits(a[0], d[0]), "an advanced offset gives the same mask"
    assert _same_bits(a[1], c[1]) and _same_bits(a[1], d[1])  # lse2 does not see the mask


def test_attn_dropout_errors(C):
    qkv, dout = _randn_case(1, 128, 3)
    rng = _rng(1, 0)
    prev = C.set_attn_staged(True)
    try:
        with pytest.raises(RuntimeError):  # the register-staged kernels have no dropout variant
            C.attn_fwd(qkv, H, SCALE, True, dropout_p=0.1, rng=rng)
    finally:
        C.set_attn_staged(prev)
    with pytest.raises(RuntimeError):
        C.attn_fwd(qkv, H, SCALE, True, dropout_p=1.0, rng=rng)
    with pytest.raises(RuntimeError):
        C.attn_fwd(qkv, H, SCALE, True, dropout_p=-0.1, rng=rng)
    with pytest.raises(RuntimeError):
        C.attn_fwd(qkv, H, SCALE, True, dropout_p=0.1)  # rng missing
    with pytest.raises(RuntimeError):
        C.attn_fwd(qkv, H, SCALE, True, dropout_p=0.1, rng=rng.to(torch.int32))
    with pytest.raises(RuntimeError):
        C.attn_fwd(qkv, H, SCALE, True, dropout_p=0.1, rng=torch.zeros(3, dtype=torch.int64, device=dev))
    with pytest.raises(RuntimeError):
        C.attn_fwd(qkv, H, SCALE, True, dropout_p=0.1, rng=rng.cpu())
    out, lse = C.attn_fwd(qkv, H, SCALE, True, dropout_p=0.1, rng=rng)
    with pytest.raises(RuntimeError):
        C.attn_bwd(qkv, out, dout, lse, H, SCALE, True, dropout_p=0.1)


# --------------------------------------------------------------- elementwise
@pytest.mark.parametrize("n", [1027, 8192])
@pytest.mark.parametrize("ydt", [BF, torch.float32])
def test_dropout_add(C, n, ydt):
    """res + mask(y) s: the kept set is the numpy mask's, values within the roundings of one fp32 multiply and one
    fp32 add (2^-24 |y s| + 2^-24 |res + y s|, s the fp32 quotient 1 / (1 - p)); nothing stored past n."""
    p, stream = 0.25, 5
    g = torch.Generator().manual_seed(n)
    res = torch.randn(n, generator=g).to(dev)
    y = torch.randn(n, generator=g).to(ydt).to(dev)
    rng = _rng(0x5EED5EED5, 2 ** 32 + 9)
    seed, off = rng.tolist()  # read back from the device tensor
    buf, out, rest = _canary((n + 64,), torch.float32, n)
    C.dropout_add(res, y, p, rng, stream, out=out)
    torch.cuda.synchronize()
    assert torch.equal(_bits(buf.view(-1)[n:]), rest), "dropout_add stored past n"
    keep = D.eltwise_keep(seed, off, stream, n, p).to(dev)
    assert torch.equal(out != res, keep & (y != 0)), "kept set differs from the reference mask"
    assert _same_bits(out[~keep], res[~keep])
    s32 = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    ys = y.double() * s32
    want = res.double() + torch.where(keep, ys, torch.zeros_like(ys))
    bound = 2.0 ** -24 * (ys.abs() + want.abs()) * (1 + 2.0 ** -20) + 1e-30
    print(f"dropout_add n {n} {ydt}")
    assert _ratio("out", out, want, bound) <= 1.0
    assert _same_bits(C.dropout_add(res, y, p, rng, stream), out)
    assert not _same_bits(C.dropout_add(res, y, p, rng, stream + 1), out)


@pytest.mark.parametrize("n", [1027, 8192])
def test_dropout_cast(C, n):
    """bf16 mask(g) s: dropout_add's kept set, dropped elements exact zeros, kept ones within one fp32 rounding of
    the product plus one bf16 rounding; nothing stored past n."""
    p, stream = 0.25, 5
    g = torch.Generator().manual_seed(n + 1)
    x = torch.randn(n, generator=g).to(dev)
    rng = _rng(0x5EED5EED5, 2 ** 32 + 9)
    seed, off = rng.tolist()
    buf, out, rest = _canary((n + 64,), BF, n)
    C.dropout_cast(x, p, rng, stream, out=out)
    torch.cuda.synchronize()
    assert torch.equal(_bits(buf.view(-1)[n:]), rest), "dropout_cast stored past n"
    keep = D.eltwise_keep(seed, off, stream, n, p).to(dev)
    assert torch.equal(_bits(out[~keep]), torch.zeros(int((~keep).sum()), dtype=torch.int16, device=dev))
    assert torch.equal(out != 0, keep & (x != 0))
    s32 = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    want = torch.where(keep, x.double() * s32, torch.zeros(n, dtype=torch.float64, device=dev))
    bound = (2.0 ** -8 + 2.0 ** -24) * want.abs() * (1 + 2.0 ** -20) + 1e-30  # unit roundoffs: bf16 2^-8, fp32 2^-24
    print(f"dropout_cast n {n}")
    assert _ratio("out", out, want, bound) <= 1.0


def test_dropout_eltwise_errors(C):
    x = torch.randn(64, device=dev)
    with pytest.raises(RuntimeError):
        C.dropout_add(x, x, 1.0, _rng(1, 0), 0)
    with pytest.raises(RuntimeError):
        C.dropout_cast(x, 0.1, _rng(1, 0).cpu(), 0)
    with pytest.raises(RuntimeError):
        C.dropout_add(x, x[:32], 0.1, _rng(1, 0), 0)


# ---------------------------------------------------------------------- model
def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


def _cos(a, b):
    a, b = a.float().flatten(), b.float().flatten()
    return (a @ b / (a.norm() * b.norm() + 1e-12)).item()


def _model_doc_start(T=128):
    return torch.stack([P.doc_start_of(T, [1, 40, 70, 127]), P.doc_start_of(T, [64])])


def _models(n_layer=2):
    torch.manual_seed(21)
    m0 = get_model("gpt2-tiny", n_layer=n_layer).to(dev)
    m1 = get_model("gpt2-tiny", n_layer=n_layer, dropout=0.1).to(dev)
    m1.load_state_dict(m0.state_dict())
    idx = torch.randint(0, 512, (2, 128), device=dev)
    tgt = torch.randint(0, 512, (2, 128), device=dev)
    return m0, m1, idx, tgt


def test_gpt2_dropout_train_and_eval(C):
    m0, m1, idx, tgt = _models()
    assert all(b.fused for b in m1.h)
    Fx.manual_seed_dropout(1234)
    l0 = m0(idx, tgt)
    la = m1(idx, tgt)
    lb = m1(idx, tgt)
    print(f"  train loss: dropout 0 {l0.item():.6f}, dropout 0.1 {la.item():.6f}, next forward {lb.item():.6f}")
    assert abs(la.item() - l0.item()) > 1e-4, "GPT2Config(dropout=0.1) trains as if it were 0"
    assert la.item() != lb.item(), "two consecutive training forwards drew the same masks"
    Fx.manual_seed_dropout(1234)
    lc = m1(idx, tgt)
    assert _same_bits(la.detach().float().reshape(1), lc.detach().float().reshape(1)), "re-seeding does not reproduce"
    lc.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m1.parameters())
    m0.eval(), m1.eval()
    with torch.no_grad():
        e0, e1 = m0(idx, tgt), m1(idx, tgt)
    assert _same_bits(e0.float().reshape(1), e1.float().reshape(1))


@pytest.mark.parametrize("packed", [False, True])
def test_gpt2_dropout_fused_block_matches_per_op(C, packed):
    """The fused block and the per-op path draw the same masks from the same RNG state; the tolerances of
    test_gpt2_packed_fused_block_matches_per_op."""
    torch.manual_seed(8)
    m1 = get_model("gpt2-tiny", n_layer=3, dropout=0.1).to(dev)
    m2 = copy.deepcopy(m1)
    for b in m2.h:
        b.fused = False
    assert all(b.fused for b in m1.h)
    idx = torch.randint(0, 512, (2, 128), device=dev)
    tgt = torch.randint(0, 512, (2, 128), device=dev)
    ds = _model_doc_start().to(dev) if packed else None
    Fx.manual_seed_dropout(77)
    l1 = m1(idx, tgt, ds)
    Fx.manual_seed_dropout(77)
    l2 = m2(idx, tgt, ds)
    assert abs(l1.item() - l2.item()) < 1e-4 * abs(l2.item())
    l1.backward()
    l2.backward()
    g2 = dict(m2.named_parameters())
    for n, p in m1.named_parameters():
        assert _cos(p.grad, g2[n].grad) > 0.999, n
        assert _rel(p.grad, g2[n].grad) < 0.02, n
    # and the mask matters: the plain model's loss differs
    m3 = copy.deepcopy(m1)
    m3.cfg = dataclasses.replace(m3.cfg, dropout=0.0)
    assert abs(m3(idx, tgt, ds).item() - l1.item()) > 1e-4


def test_dropout_training_step_replays_in_a_graph(C):
    """One GPT-2-tiny training step with dropout captured in a graph: every replay's loss is bit-equal to an
    eager step from the same parameters and RNG state (the mask state is read on the device), and with lr = 0
    successive replays give different losses (the state advances under replay)."""
    from distributed_pytorch_example_amd.optim import AdamW

    torch.manual_seed(12)
    m1 = get_model("gpt2-tiny", dropout=0.1).to(dev)
    m2 = copy.deepcopy(m1)
    xs = [torch.randint(0, 512, (2, 128), device=dev) for _ in range(3)]
    ys = [x.roll(-1, 1) for x in xs]
    st = Fx.dropout_state(dev)
    Fx.manual_seed_dropout(2024)

    def step(model, opt, x, y):
        loss = model(x, y)
        loss.backward()
        opt.step()
        opt.zero_grad(set_to_none=False)
        return loss

    def capture(model, opt, sx, sy):
        for p in model.parameters():
            p.grad = torch.zeros_like(p)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                step(model, opt, sx, sy)
        torch.cuda.current_stream().wait_stream(side)
        opt.graph_safe = True
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            gl = step(model, opt, sx, sy)
        return g, gl

    o1, o2 = AdamW(m1.parameters(), lr=1e-4), AdamW(m2.parameters(), lr=1e-4)
    for p in m2.parameters():
        p.grad = torch.zeros_like(p)
    sx, sy = xs[0].clone(), ys[0].clone()
    g, gl = capture(m1, o1, sx, sy)
    for i in (1, 2):
        with torch.no_grad():  # the eager model starts the step from the graph model's parameters
            for a, b in zip(m2.parameters(), m1.parameters()):
                a.copy_(b)
        sx.copy_(xs[i])
        sy.copy_(ys[i])
        before = st.snapshot()
        g.replay()
        after = st.snapshot()
        st.tensor().copy_(before)  # ... and from the RNG state the replay started from
        le = step(m2, o2, xs[i], ys[i])
        torch.cuda.synchronize()
        print(f"  replay {i}: graph loss {gl.item():.6f}, eager loss {le.item():.6f}")
        assert _same_bits(gl.detach().float().reshape(1), le.detach().float().reshape(1))
        assert torch.equal(after, st.tensor()) and after[1].item() > before[1].item()
    # lr = 0: the parameters stand still, the masks do not
    m3 = copy.deepcopy(m1)
    g3, gl3 = capture(m3, AdamW(m3.parameters(), lr=0.0, weight_decay=0.0), xs[0].clone(), ys[0].clone())
    losses = []
    for _ in range(3):
        g3.replay()
        torch.cuda.synchronize()
        losses.append(gl3.item())
    print(f"  lr = 0 replays: {losses}")
    assert len(set(losses)) == 3, "replays of a captured step drew the same mask"
