"""Sliding-window causal attention (attn_fwd / attn_bwd / attn_decode_gqa with window=W: the WINDOW instantiations of the
LDS-DMA and GQA kernels of attn.hip, the windowed key range of decode_gqa.hip) against fp64.

Training kernels: _packed_attn_ref.packed_attn_ref takes any per-query lower bound, here max(doc_start[i], i - W + 1); GQA
expands K / V and sums dK, dV and their bounds per group (test_gqa_attn_gpu._ref).  Pass = max |err| / bound <= 1 per element
for out, lse2, dQ, dK, dV with the budgets of those references, printed by every case.  B 2, T 256: two query workgroups,
four key tiles.  Decode: the reference of test_attn_decode_gqa_gpu.py on the cache rows of the window; every cache row
outside lo .. len - 1 holds NaN, so a finite output also shows that no row outside the window reached the arithmetic.
"""
import copy

import pytest
import torch

from _decode_ref import attn_decode_ref
from _llama_ref import rope_ref
from _packed_attn_ref import doc_start_of, packed_attn_ref
from distributed_pytorch_example_amd.models import get_model
from distributed_pytorch_example_amd.ops import functional as Fx
from test_gpt2_kernels_gpu import BF, SCALE, _bits, _canary, _cos, _ratio, _rel, _same_bits, dev
from test_gqa_attn_gpu import _case, _check, _ref

pytestmark = pytest.mark.gpu

B, T = 2, 256
LAYOUTS = [(2, None), (4, 2), (3, 1)]  # the [3, H] layout | G = 2 | G = 3 on one KV head
DOCS = [40, 130, 131, 250]
_inputs = {}


def _data(H, Hkv):
    """(qkv [B, T, H + 2 Hkv, 64], dout) on the GPU, shared by the cases of a layout; [3, H] is the same bytes with Hkv = H."""
    if (H, Hkv) not in _inputs:
        _inputs[H, Hkv] = _case(B, T, H, Hkv or H, 900 + 10 * H + (Hkv or 0))
    return _inputs[H, Hkv]


def _lower(W, docs=None):
    """int32 [B, T]: the first key query i sees."""
    lo = (torch.arange(T, dtype=torch.int32) - W + 1).clamp_(min=0)
    if docs is not None:
        lo = torch.maximum(lo, doc_start_of(T, docs))
    return lo.expand(B, T).contiguous()


def _run(C, qkv, dout, H, Hkv, window, docs=None):
    """attn_fwd + attn_bwd into buffers followed by NaN canary rows, which must come back unchanged."""
    Wd = qkv.shape[2]
    x = qkv if Hkv else qkv.view(B, T, 3, H, 64)
    kw = dict(n_kv_head=Hkv) if Hkv else {}
    if window is not None:
        kw["window"] = window
    if docs is not None:
        kw["doc_start"], kw["doc_end"], _ = Fx.doc_bounds(doc_start_of(T, docs).expand(B, T).contiguous().to(dev))
    bo, fo, co = _canary((B, T + 128, H, 64), BF, B * T * H * 64)
    bl, fl, cl = _canary((B, H, T + 128), torch.float32, B * H * T)
    bd, fd, cd = _canary((B, T + 128, Wd, 64), BF, B * T * Wd * 64)
    out, lse, dqkv = fo.view(B, T, H, 64), fl.view(B, H, T), fd.view(x.shape)
    C.attn_fwd(x, H, SCALE, True, out=out, lse=lse, **kw)
    C.attn_bwd(x, out, dout, lse, H, SCALE, True, dqkv=dqkv, **kw)
    torch.cuda.synchronize()
    assert torch.equal(_bits(bo.view(-1)[fo.numel():]), co), "attn_fwd stored past the end of out"
    assert torch.equal(_bits(bl.view(-1)[fl.numel():]), cl), "attn_fwd stored past the end of lse"
    assert torch.equal(_bits(bd.view(-1)[fd.numel():]), cd), "attn_bwd stored past the end of dqkv"
    return out, lse, dqkv.view(B, T, Wd, 64)


def _reference(qkv, dout, H, Hkv, lower):
    if Hkv:
        return _ref(qkv, dout, H, Hkv, doc_start=lower)
    r = packed_attn_ref(qkv.view(B, T, 3, H, 64), dout, SCALE, lower)
    return dict(r, dqkv=r["dqkv"].reshape(B, T, 3 * H, 64), b_dqkv=r["b_dqkv"].reshape(B, T, 3 * H, 64))


# a row sees itself only | the edge inside a wave's diagonal tile | exactly one tile | the edge mid-tile | wider than a
# workgroup: the first tile is not the workgroup's own | one key masked in the whole problem
@pytest.mark.parametrize("H,Hkv", LAYOUTS)
@pytest.mark.parametrize("W", [1, 17, 64, 100, 192, 255])
def test_window(C, W, H, Hkv):
    qkv, dout = _data(H, Hkv)
    got = _run(C, qkv, dout, H, Hkv, W)
    _check(f"window W={W} H={H} Hkv={Hkv}", got, _reference(qkv, dout, H, Hkv, _lower(W)), H, Hkv or H)


@pytest.mark.parametrize("H,Hkv", [(2, None), (4, 2)])
@pytest.mark.parametrize("W", [17, 100])
def test_window_packed(C, W, H, Hkv):
    """Documents starting at 0, 40, 130, 131 and 250: window edges and document starts interleave inside one tile."""
    qkv, dout = _data(H, Hkv)
    got = _run(C, qkv, dout, H, Hkv, W, DOCS)
    _check(f"window packed W={W} H={H} Hkv={Hkv}", got, _reference(qkv, dout, H, Hkv, _lower(W, DOCS)), H, Hkv or H)


@pytest.mark.parametrize("H,Hkv", LAYOUTS)
@pytest.mark.parametrize("W", [256, 300])
def test_window_not_shorter_than_T_is_the_plain_call(C, W, H, Hkv):
    qkv, dout = _data(H, Hkv)
    assert all(_same_bits(a, b) for a, b in zip(_run(C, qkv, dout, H, Hkv, W), _run(C, qkv, dout, H, Hkv, None)))


# ------------------------------------------------------------------------------------------------------------ decode
HQ, HKV, TMAX, LENS = 8, 2, 256, (0, 5, 63, 200)
NAN_BITS = 0x7FC1


@pytest.mark.parametrize("S", [1, 4])
@pytest.mark.parametrize("W", [1, 32, 100, 256])
def test_decode_window(C, W, S):
    nb, G = len(LENS), HQ // HKV
    g = torch.Generator().manual_seed(50 + W)
    qkv = torch.randn(nb, HQ + 2 * HKV, 64, generator=g).to(BF)
    kc, vc = (torch.randn(nb, HKV, TMAX, 64, generator=g).to(BF) for _ in range(2))
    table = Fx.rope_table(TMAX)
    nan = torch.tensor(NAN_BITS, dtype=torch.int16).view(BF)
    # the reference: test_attn_decode_gqa_gpu.reference on each row's window, moved to the front of a cache of its own
    rot, rb = rope_ref(qkv.view(nb, 1, -1, 64), table[0], table[1], torch.tensor(LENS).view(nb, 1), HQ + HKV)
    q, bq = rot[:, 0, :HQ], rb[:, 0, :HQ]
    k, bk = rot[:, 0, HQ:].repeat_interleave(G, 1), rb[:, 0, HQ:].repeat_interleave(G, 1)
    step = torch.stack([q, k, qkv[:, HQ + HKV:].double().repeat_interleave(G, 1)], 1)
    kw, vw, wl = torch.zeros_like(kc), torch.zeros_like(vc), []
    for b, n in enumerate(LENS):
        lo = max(0, n - W + 1)
        kw[b, :, :n - lo], vw[b, :, :n - lo] = kc[b, :, lo:n], vc[b, :, lo:n]
        kc[b, :, :lo] = vc[b, :, :lo] = kc[b, :, n:] = vc[b, :, n:] = nan
        wl.append(n - lo)
    ke, ve = kw.repeat_interleave(G, 1), vw.repeat_interleave(G, 1)
    ref, b_out = attn_decode_ref(step, ke, ve, wl, SCALE)
    cached = torch.arange(TMAX)[None, None, :] < torch.tensor(wl)[:, None, None]
    eps = torch.einsum("bhd,bhtd->bht", bq, ke.double().abs()).masked_fill(~cached, 0.0).amax(-1)
    grow = torch.exp(2 * SCALE * torch.maximum(eps, (bq * k.abs() + q.abs() * bk + bq * bk).sum(-1)))
    bound = b_out * (grow + 2.0 ** 7 * (grow - 1)).repeat_interleave(64, 1)

    kd, vd = kc.to(dev), vc.to(dev)
    out = C.attn_decode_gqa(qkv.to(dev), kd, vd, torch.tensor(LENS, dtype=torch.int32, device=dev), table[0].to(dev),
                            table[1].to(dev), HKV, SCALE, S, window=W).cpu()
    assert torch.isfinite(out.float()).all(), "a key outside the window reached the arithmetic"
    ratio = ((out.double() - ref).abs() / bound).max().item()
    print(f"attn_decode_gqa window W={W} S={S}: worst |err| / bound = {ratio:.3f}")
    assert ratio <= 1.0
    ek, ev = kc.clone(), vc.clone()
    for b, n in enumerate(LENS):  # row len[b] is the step's; every other bit of the cache is unchanged
        ek[b, :, n], ev[b, :, n] = kd[b, :, n].cpu(), qkv[b, HQ + HKV:]
        assert torch.isfinite(kd[b, :, n].float()).all()
    assert torch.equal(kd.cpu().view(torch.int16), ek.view(torch.int16)) and torch.equal(vd.cpu().view(torch.int16), ev.view(torch.int16))


# -------------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("H,Hkv", [(2, None), (4, 2)])
def test_fx_causal_attention_window(C, H, Hkv):
    qkv, dout = _data(H, Hkv)
    out, _, dqkv = _run(C, qkv, dout, H, Hkv, 100)
    x = qkv.view(B, T, -1).clone().requires_grad_(True)
    y = Fx.causal_attention(x, H, n_kv_head=Hkv, window=100)
    y.backward(dout.view(B, T, -1))
    assert _same_bits(y.detach(), out.view(B, T, -1)) and _same_bits(x.grad, dqkv.view(B, T, -1))


def test_llama_tiny_sliding_window(C):
    """llama-tiny with sliding_window = 48 at T = 128 on the window kernels against its CPU copy on the masked-softmax
    fallback (the measures and thresholds of test_llama_gpu.py); greedy generation replayed from the graph gives the eager
    tokens, with the window shorter than the rows from the first decode step on."""
    torch.manual_seed(5)
    cpu = get_model("llama-tiny", sliding_window=48)
    gpu = copy.deepcopy(cpu).to(dev)
    idx, tgt = torch.randint(0, 512, (2, 128)), torch.randint(0, 512, (2, 128))
    lc, lg = cpu(idx, tgt), gpu(idx.to(dev), tgt.to(dev))
    lc.backward()
    lg.backward()
    print(f"llama-tiny sliding_window=48: loss cpu {lc.item():.4f} gpu {lg.item():.4f}")
    assert abs(lc.item() - lg.item()) < 2e-2 * abs(lc.item())
    gc = dict(cpu.named_parameters())
    for n, p in gpu.named_parameters():
        c, r = _cos(p.grad.cpu(), gc[n].grad), _rel(p.grad.cpu(), gc[n].grad)
        assert c > 0.98 and r < 0.1, (n, c, r)
    kw = dict(prompt_lens=[17, 70], temperature=0.0)
    assert torch.equal(gpu.generate(idx[:, :70].to(dev), 40, **kw), gpu.generate(idx[:, :70].to(dev), 40, graph=True, **kw))
