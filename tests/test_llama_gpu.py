"""The Llama ops under autograd and the llama-tiny model on the GPU against a deep copy on the CPU in fp32 (measures
and thresholds of test_gpt2_kernels_gpu.py::test_gpt2_tiny_T100_gpu_vs_cpu).

Measured (MI355X): loss cpu / gpu 6.3050 / 6.3050 (T 128), 6.2860 / 6.2862 (T 100), 6.2593 / 6.2594 (packed, T 192);
lowest per-parameter gradient cosine 0.99997 in all three (the gain of an ln_2).
"""
import copy

import pytest
import torch

from _packed_attn_ref import doc_start_of
from distributed_pytorch_example_amd.models import get_model
from distributed_pytorch_example_amd.ops import functional as Fx
from distributed_pytorch_example_amd.optim import build_optimizer
from test_gpt2_kernels_gpu import BF, _cos, _rel, _same_bits, dev

pytestmark = pytest.mark.gpu


def test_fx_ops_reproduce_the_direct_calls(C):
    g = torch.Generator().manual_seed(3)
    B, T, Hq, Hkv = 2, 70, 4, 2
    W = Hq + 2 * Hkv
    qkv = torch.randn(B, T, W * 64, generator=g).to(BF).to(dev)
    dout = torch.randn(B, T, W * 64, generator=g).to(BF).to(dev)
    table = Fx.rope_table(T, device=dev)
    pos = Fx.doc_bounds(doc_start_of(T, [3, 64]).expand(B, T).to(dev))[2]
    want = C.rope(qkv.view(B, T, W, 64), *table, pos, Hq + Hkv).view(B, T, -1)
    dwant = C.rope(dout.view(B, T, W, 64), *table, pos, Hq + Hkv, True).view(B, T, -1)
    for inplace in (False, True):
        x = qkv.clone().requires_grad_(True)
        y = Fx.rope(x * 1 if inplace else x, Hq, Hkv, table, pos, inplace=inplace)  # (in place: not on a leaf)
        y.backward(dout)
        assert _same_bits(y.detach(), want) and _same_bits(x.grad, dwant), f"Fx.rope inplace={inplace}"
    x = torch.randn(B * T, 256, generator=g).to(dev).requires_grad_(True)
    w = (1.0 + 0.5 * torch.randn(256, generator=g)).to(dev).requires_grad_(True)
    dy = torch.randn(B * T, 256, generator=g).to(BF).to(dev)
    y = Fx.rms_norm(x, w, 1e-5)
    y.backward(dy)
    y0, rstd = C.rmsnorm_fwd(x.detach(), w.detach(), 1e-5)
    dw0 = torch.zeros(256, device=dev)
    dx0 = C.rmsnorm_bwd(dy, x.detach(), w.detach(), rstd, dw0)
    assert _same_bits(y.detach(), y0) and _same_bits(x.grad, dx0) and _same_bits(w.grad, dw0)
    gu = torch.randn(B * T, 2 * 704, generator=g).to(BF).to(dev).requires_grad_(True)
    du = torch.randn(B * T, 704, generator=g).to(BF).to(dev)
    u = Fx.swiglu(gu)
    u.backward(du)
    assert _same_bits(u.detach(), C.swiglu_fwd(gu.detach())) and _same_bits(gu.grad, C.swiglu_bwd(du, gu.detach()))


@pytest.mark.parametrize("T,docs", [(128, None), (100, None), (192, [70, 128])], ids=["T128", "T100", "packed"])
def test_llama_tiny_gpu_vs_cpu(C, T, docs):
    """T = 128 takes the GQA flash kernels, T = 100 the attention fallback (RoPE, RMSNorm and SwiGLU stay on their
    kernels); the packed run has documents starting at 0, 70 (inside a tile) and 128 (on a tile edge)."""
    torch.manual_seed(5)
    cpu = get_model("llama-tiny", block_size=max(T, 128))
    gpu = copy.deepcopy(cpu).to(dev)
    idx, tgt = torch.randint(0, 512, (2, T)), torch.randint(0, 512, (2, T))
    ds = None if docs is None else doc_start_of(T, docs).expand(2, T).contiguous()
    lc = cpu(idx, tgt, ds)
    lc.backward()
    lg = gpu(idx.to(dev), tgt.to(dev), None if ds is None else ds.to(dev))
    lg.backward()
    assert abs(lc.item() - lg.item()) < 2e-2 * abs(lc.item())
    gc = dict(cpu.named_parameters())
    print(f"llama-tiny T={T} docs={docs}: loss cpu {lc.item():.4f} gpu {lg.item():.4f}")
    for n, p in gpu.named_parameters():
        c, r = _cos(p.grad.cpu(), gc[n].grad), _rel(p.grad.cpu(), gc[n].grad)
        print(f"  {n}: gradient cosine {c:.5f}, relative norm error {r:.4f}")
        assert c > 0.98 and r < 0.1, n


def test_llama_tiny_optimizer_step(C):
    torch.manual_seed(6)
    m = get_model("llama-tiny").to(dev)
    opt = build_optimizer("adamw", m.parameters(), lr=1e-3, weight_decay=0.01)
    before = [p.detach().clone() for p in m.parameters()]
    idx, tgt = torch.randint(0, 512, (2, 128), device=dev), torch.randint(0, 512, (2, 128), device=dev)
    loss = m(idx, tgt)
    loss.backward()
    opt.step()
    assert torch.isfinite(loss).item() and torch.isfinite(m(idx, tgt)).item()
    for (n, p), b in zip(m.named_parameters(), before):
        assert not torch.equal(p.detach(), b), f"{n} did not change"
