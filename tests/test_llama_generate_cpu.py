"""Llama.generate, Fx.attn_decode_gqa's torch path and the generate CLI with a Llama model, on the CPU in fp32."""
import contextlib
import io
import math

import pytest
import torch

from _decode_ref import attn_decode_ref, naive_generate
from _llama_ref import rope_ref
from distributed_pytorch_example_amd import generate as gen_cli
from distributed_pytorch_example_amd.models import get_model
from distributed_pytorch_example_amd.ops import functional as Fx
from distributed_pytorch_example_amd.optim import build_optimizer
from distributed_pytorch_example_amd.utils.checkpoint import make_checkpoint


def tiny(seed=0):
    torch.manual_seed(seed)
    m = get_model("llama-tiny")
    with torch.no_grad():
        for p in m.parameters():
            if p.ndim >= 2:
                p.mul_(4.0)
    return m.eval()


def test_greedy_equals_the_naive_loop_on_ragged_prompts():
    m, lens = tiny(), [3, 17, 64, 70]
    idx = torch.randint(0, 512, (4, 70), generator=torch.Generator().manual_seed(2))
    out, lgs = m.generate(idx, 6, prompt_lens=lens, temperature=0.0, return_logits=True)
    ref, ref_lgs = naive_generate(m, idx, lens, 6)
    assert torch.equal(out, ref)
    assert (lgs - ref_lgs).abs().max().item() < 1e-3 * ref_lgs.abs().max().item()


@pytest.mark.parametrize("Hq,Hkv", [(2, 2), (6, 2), (16, 1)])
def test_attn_decode_gqa_torch_path_against_fp64(Hq, Hkv):
    """fp32 sums of 64 products and 40 keys carry a few 2^-24 each: 1e-4 of the reference's P |v| (= 2^7 b_out) is
    generous.  Length 39 clamps onto the last row of a 24-row table; only cache row len[b] may change."""
    B, Tmax, D, G, lens = 3, 40, 64, Hq // Hkv, (0, 17, 39)
    g = torch.Generator().manual_seed(Hq)
    qkv = torch.randn(B, Hq + 2 * Hkv, D, generator=g)
    kc, vc = torch.randn(B, Hkv, Tmax, D, generator=g), torch.randn(B, Hkv, Tmax, D, generator=g)
    table = Fx.rope_table(24)
    rot, _ = rope_ref(qkv.view(B, 1, -1, D), table[0], table[1], torch.tensor(lens).clamp(0, 23).view(B, 1), Hq + Hkv)
    step = torch.stack([rot[:, 0, :Hq], rot[:, 0, Hq:].repeat_interleave(G, 1), qkv[:, Hq + Hkv:].double().repeat_interleave(G, 1)], 1)
    ref, b_out = attn_decode_ref(step, kc.repeat_interleave(G, 1), vc.repeat_interleave(G, 1), lens, 1.0 / math.sqrt(D))
    k2, v2 = kc.clone(), vc.clone()
    out = Fx.attn_decode_gqa(qkv.view(B, -1), k2, v2, torch.tensor(lens, dtype=torch.int32), Hq, Hkv, table)
    assert ((out.double() - ref).abs() <= 1e-4 * 2.0 ** 7 * b_out + 1e-6).all()
    for b, n in enumerate(lens):
        assert (k2[b, :, n].double() - rot[b, 0, Hq:]).abs().max().item() < 1e-5 and torch.equal(v2[b, :, n], qkv[b, Hq + Hkv:])
        k2[b, :, n], v2[b, :, n] = kc[b, :, n], vc[b, :, n]
    assert torch.equal(k2, kc) and torch.equal(v2, vc)


def test_cli_round_trips_a_llama_checkpoint(tmp_path):
    m = tiny(7).train()
    opt = build_optimizer("adamw", m.parameters(), lr=2e-2, ema={"decay": 0.5})
    x = torch.randint(0, 512, (2, 17), generator=torch.Generator().manual_seed(8))
    m(x[:, :-1], x[:, 1:]).backward()
    opt.step()
    path = str(tmp_path / "ckpt.pt")
    torch.save(make_checkpoint(m, opt, 0, 0.0, to_cpu=True), path)
    m.eval()
    idx = torch.tensor([[1, 2, 3, 0, 0], [7, 8, 9, 10, 11]])
    args = ["--model", "llama-tiny", "--checkpoint", path, "--prompt", "1,2,3", "--prompt", "7,8,9,10,11", "--max-new-tokens", "6",
            "--device", "cpu", "--temperature", "0"]

    def cli(a):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            assert gen_cli.main(a) == 0
        return [[int(t) for t in line.split(",")] for line in buf.getvalue().strip().splitlines()]

    assert cli(args) == m.generate(idx, 6, prompt_lens=[3, 5], temperature=0.0).tolist()
    with opt.ema_weights():
        want = m.generate(idx, 6, prompt_lens=[3, 5], temperature=0.0).tolist()
    assert cli(args + ["--ema"]) == want
