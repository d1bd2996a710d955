"""Sliding-window attention off the GPU: the routes of window= (C.attn_route, no tensor and no GPU call), the masked-softmax
fallbacks of Fx.causal_attention(window=) and Fx.attn_decode_gqa(window=) against fp64 at T = 96 (a shape the kernels
refuse), and train.py's parser.  Needs the built extension, not a GPU."""
import math

import pytest
import torch

from distributed_pytorch_example_amd import train
from distributed_pytorch_example_amd.ops import functional as Fx
from distributed_pytorch_example_amd.ops._ext import has_ext
from test_attn_route_cpu import T_OVER, _route

pytestmark = pytest.mark.skipif(not has_ext(), reason="native extension not built")

# (case, attn_route keywords, set_attn_staged, expected route)
ROUTES = [
    ("window", dict(window=100), False, "dma"),
    ("window_gqa", dict(window=100, n_kv_head=2), False, "gqa"),
    ("window_packed", dict(window=100, packed=True), False, "dma"),
    ("window_gqa_packed", dict(window=100, n_kv_head=2, packed=True), False, "gqa"),
    ("window_past_T", dict(window=10 ** 6), False, "dma"),
    ("window_dropout", dict(window=100, dropout=True), False, "none"),
    ("window_bidir", dict(window=100, causal=False), False, "none"),
    ("window_staged", dict(window=100), True, "none"),
    ("window_2GiB", dict(window=100, T=T_OVER, H=1), False, "none"),
    ("window_negative", dict(window=-1), False, "none"),
]


@pytest.mark.parametrize("case,kw,staged,route", ROUTES, ids=[r[0] for r in ROUTES])
def test_window_routes(case, kw, staged, route):
    got, why = _route(kw, staged)
    assert got == route, (got, why)
    assert ("window" in why and why.startswith("attn: ")) if route == "none" else why == ""


def _masked_softmax_ref(q, k, v, lower):
    """fp64 softmax(q k^T / sqrt(D)) v over the keys lower[i] <= j <= i; q, k, v [..., T, D]."""
    Tq = q.shape[-2]
    j = torch.arange(Tq)
    s = (q.double() @ k.double().transpose(-1, -2)) / math.sqrt(q.shape[-1])
    s = s.masked_fill((j[None, :] > j[:, None]) | (j[None, :] < lower[:, None]), float("-inf"))
    return torch.softmax(s, -1) @ v.double()


@pytest.mark.parametrize("Hkv", [None, 2])
@pytest.mark.parametrize("W", [1, 40, 96])
def test_causal_attention_fallback(W, Hkv):
    Bn, Tn, H, D = 2, 96, 4, 32
    g = torch.Generator().manual_seed(W)
    x = torch.randn(Bn, Tn, (H + 2 * Hkv if Hkv else 3 * H) * D, generator=g)
    y = Fx.causal_attention(x, H, n_kv_head=Hkv, window=W)
    q, k, v = (t.transpose(1, 2) for t in x.view(Bn, Tn, -1, D).split([H, Hkv or H, Hkv or H], dim=2))
    G = H // (Hkv or H)
    ref = _masked_softmax_ref(q, k.repeat_interleave(G, 1), v.repeat_interleave(G, 1), (torch.arange(Tn) - W + 1).clamp(min=0))
    assert (y.double() - ref.transpose(1, 2).reshape(Bn, Tn, H * D)).abs().max() < 1e-5  # fp32 softmax over <= 96 keys of N(0, 1) data


@pytest.mark.parametrize("W", [1, 40, 0])
def test_attn_decode_gqa_fallback(W):
    Hq, Hkv, Tmax, D, lens = 4, 2, 96, 64, [0, 5, 95]
    g = torch.Generator().manual_seed(7)
    step = torch.randn(3, (Hq + 2 * Hkv) * D, generator=g)
    kc, vc = torch.randn(3, Hkv, Tmax, D, generator=g), torch.randn(3, Hkv, Tmax, D, generator=g)
    table = (torch.ones(Tmax, D // 2), torch.zeros(Tmax, D // 2))  # the identity rotation: the step's key goes in as it is
    out = Fx.attn_decode_gqa(step, kc, vc, torch.tensor(lens, dtype=torch.int32), Hq, Hkv, table, window=W)
    for b, n in enumerate(lens):
        lo = max(0, n - W + 1) if W else 0
        q = step[b].view(-1, D)[:Hq].double()
        ke, ve = (c[b, :, lo:n + 1].double().repeat_interleave(Hq // Hkv, 0) for c in (kc, vc))  # row n: stored by the call
        p = torch.softmax(torch.einsum("hd,htd->ht", q, ke) / math.sqrt(D), -1)
        assert (out[b].double() - torch.einsum("ht,htd->hd", p, ve).reshape(-1)).abs().max() < 1e-5


@pytest.mark.parametrize("argv", [["--model", "gpt2-tiny", "--sliding-window", "64"], ["--model", "llama-tiny", "--sliding-window", "-1"]])
def test_train_parser_errors(argv, capsys):
    with pytest.raises(SystemExit):
        train.main(argv)
    assert "--sliding-window" in capsys.readouterr().err
