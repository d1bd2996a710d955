"""ViT off the GPU: the fp64 reference of the bidirectional attention against autograd, Fx.attention and Fx.patchify
on the CPU, the parameter counts, the vit-tiny forward against an independent torch implementation, and the CLI."""
import math
import os
import socket
import subprocess
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import _bidir_attn_ref as BR
import _gpt2_ref as R
from distributed_pytorch_example_amd.models import get_model
from distributed_pytorch_example_amd.ops import functional as Fx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- reference
@pytest.mark.parametrize("L", [1, 7, 23, 24])
def test_ref_closed_forms_equal_autograd(L):
    g = torch.Generator().manual_seed(3)
    B, T, H, D = 2, 24, 2, 8
    qkv = torch.randn(B, T, 3, H, D, generator=g, dtype=torch.float64)
    dout = torch.randn(B, T, H, D, generator=g, dtype=torch.float64)
    qkv[:, L:] *= 1e3  # padding rows: large and finite, and without influence
    dout[:, L:] *= 1e3
    ref = BR.bidir_attn_ref(qkv, dout, 0.3, L)
    O, dqkv = BR.bidir_attn_autograd(qkv, dout, 0.3, L)
    assert torch.allclose(ref["out"], O, rtol=1e-12, atol=1e-13)
    assert torch.allclose(ref["dqkv"], dqkv, rtol=1e-10, atol=1e-12)
    assert not ref["out"][:, L:].any() and not ref["dqkv"][:, L:].any() and not ref["lse2"][..., L:].any()
    # lse2 of the live rows, from the definition
    q, k = qkv[:, :L, 0].permute(0, 2, 1, 3), qkv[:, :L, 1].permute(0, 2, 1, 3)
    want = torch.logsumexp(0.3 * (q @ k.transpose(-1, -2)), -1) / math.log(2.0)
    assert torch.allclose(ref["lse2"][..., :L], want, rtol=1e-12, atol=1e-13)
    for key in ("b_out", "b_dqkv"):
        assert torch.isfinite(ref[key]).all() and (ref[key] > 0).all()


def test_ref_at_full_length_has_attn_refs_budgets():
    """L = T and no mask: the budgets are attn_ref's formulas (checked against attn_ref on a one-row causal case, where
    both masks coincide: T = 1)."""
    g = torch.Generator().manual_seed(4)
    qkv = torch.randn(3, 1, 3, 2, 8, generator=g, dtype=torch.float64)
    dout = torch.randn(3, 1, 2, 8, generator=g, dtype=torch.float64)
    a, b = R.attn_ref(qkv, dout, 0.5), BR.bidir_attn_ref(qkv, dout, 0.5, 1)
    for k in ("out", "lse2", "dqkv", "b_out", "b_dqkv"):
        assert torch.allclose(a[k], b[k], rtol=1e-13, atol=1e-300), k
    assert a["b_lse2"] == b["b_lse2"]


def test_tile_row_max_masks_keys_past_L():
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(1, 128, 3, 1, 8, generator=g, dtype=torch.float64)
    qkv[:, 70:, 1] *= 100
    tm = BR.bidir_tile_row_max(qkv, 0.5, 70)
    q, k = qkv[0, :, 0, 0], qkv[0, :70, 1, 0]
    s = 0.5 * R.LOG2E * (q @ k.T)
    assert torch.allclose(tm[0, 0, :, 0], s[:, :64].amax(-1)) and torch.allclose(tm[0, 0, :, 1], s[:, 64:].amax(-1))
    assert torch.isinf(BR.bidir_tile_row_max(qkv, 0.5, 64)[..., 1]).all()


# ------------------------------------------------------------- CPU functional
@pytest.mark.parametrize("T,D,L", [(24, 8, 24), (24, 8, 7), (64, 64, 17), (5, 16, 1)])
def test_cpu_attention_against_the_reference(T, D, L):
    g = torch.Generator().manual_seed(6)
    B, H = 2, 2
    qkv = torch.randn(B, T, 3 * H * D, generator=g).requires_grad_(True)
    dout = torch.randn(B, T, H * D, generator=g)
    out = Fx.attention(qkv, H, L) if L != T else Fx.attention(qkv, H)
    assert out.shape == (B, T, H * D) and out.dtype == qkv.dtype
    out.backward(dout)
    ref = BR.bidir_attn_ref(qkv.detach().view(B, T, 3, H, D), dout.view(B, T, H, D), 1.0 / math.sqrt(D), L)
    assert torch.allclose(out.detach().double().view(B, T, H, D), ref["out"], rtol=1e-4, atol=1e-5)
    assert torch.allclose(qkv.grad.double().view(B, T, 3, H, D), ref["dqkv"], rtol=1e-4, atol=1e-5)
    assert not out.detach()[:, L:].any() and not qkv.grad[:, L:].any()


def test_cpu_attention_is_not_causal_and_checks_seq_len():
    g = torch.Generator().manual_seed(7)
    qkv = torch.randn(1, 16, 3 * 2 * 8, generator=g)
    assert not torch.allclose(Fx.attention(qkv, 2), Fx.causal_attention(qkv, 2), rtol=1e-3, atol=1e-3)
    for bad in (0, 17, -1):
        with pytest.raises(ValueError):
            Fx.attention(qkv, 2, bad)


def test_cpu_patchify_is_the_conv_unfold():
    """A patch row times the flattened filter is the stride-p convolution."""
    g = torch.Generator().manual_seed(8)
    x = torch.randn(2, 3, 32, 32, generator=g)
    w = torch.randn(5, 3, 8, 8, generator=g)
    rows = Fx.patchify(x, 8)
    assert rows.shape == (2, 16, 192)
    want = F.conv2d(x, w, stride=8).flatten(2).transpose(1, 2)  # [B, N, D], patches row-major
    assert torch.allclose(rows @ w.view(5, -1).T, want, rtol=1e-4, atol=1e-4)
    with pytest.raises(ValueError):
        Fx.patchify(x, 12)


# -------------------------------------------------------------------- model
@pytest.mark.parametrize("name,count", [("vit-b16", 86567656), ("vit-s16", 22050664)])
def test_parameter_counts(name, count):
    with torch.device("meta"):
        m = get_model(name)
    assert sum(p.numel() for p in m.parameters()) == count
    cfg = m.cfg
    assert (cfg.seq_len, cfg.padded_len) == (197, 256)
    assert m.patch_embed.weight.shape == (cfg.n_embd, 3, 16, 16) and m.pos_embed.shape == (1, 197, cfg.n_embd)
    assert m.cls_token.shape == (1, 1, cfg.n_embd) and m.head.weight.shape == (1000, cfg.n_embd)


def test_vit_tiny_layout_and_marks():
    torch.manual_seed(1)
    m = get_model("vit-tiny")
    cfg = m.cfg
    assert (cfg.n_layer, cfg.n_head, cfg.n_embd, cfg.image_size, cfg.patch_size, cfg.num_classes) == (2, 2, 128, 32, 8, 10)
    assert (cfg.seq_len, cfg.padded_len) == (17, 64)
    for p in (m.pos_embed, m.cls_token, m.head.weight):
        assert p._dpe_muon is False
    for blk in m.blocks:
        assert blk.seq_len == 17
        for lin in (blk.c_attn, blk.attn_proj, blk.c_fc, blk.mlp_proj):
            assert lin.weight._dpe_overwrite_ok and not lin.bias.any()
            assert 0.018 < lin.weight.std().item() < 0.022  # trunc-normal(0.02), cut at +-2 as timm's default is
    assert [b._dpe_layer for b in m.blocks] == [0, 1]
    assert not m.patch_embed.bias.any() and not m.head.bias.any()
    # a causal Block is what it was: no seq_len
    assert get_model("gpt2-tiny").h[0].seq_len is None


class _TorchViT(nn.Module):
    """An independent pre-LN ViT in plain torch (conv patch embedding, nn.LayerNorm, SDPA over the real tokens)."""

    def __init__(self, m):
        super().__init__()
        self.m, self.cfg = m, m.cfg

    @staticmethod
    def _ln(src):
        ln = nn.LayerNorm(src.weight.shape[0], eps=src.eps)
        ln.weight, ln.bias = src.weight, src.bias  # the same Parameters: gradients land on the model's
        return ln

    def forward(self, x):
        m, cfg = self.m, self.cfg
        D, H = cfg.n_embd, cfg.n_head
        t = F.conv2d(x, m.patch_embed.weight, m.patch_embed.bias, stride=cfg.patch_size).flatten(2).transpose(1, 2)
        h = torch.cat([m.cls_token.expand(x.shape[0], -1, -1), t], 1) + m.pos_embed  # [B, 17, D]
        for blk in m.blocks:
            ln1, ln2 = self._ln(blk.ln_1), self._ln(blk.ln_2)
            B, N, _ = h.shape
            q, k, v = F.linear(ln1(h), blk.c_attn.weight, blk.c_attn.bias).view(B, N, 3, H, D // H).permute(2, 0, 3, 1, 4)
            a = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, N, D)
            h = h + F.linear(a, blk.attn_proj.weight, blk.attn_proj.bias)
            u = F.gelu(F.linear(ln2(h), blk.c_fc.weight, blk.c_fc.bias), approximate="tanh")
            h = h + F.linear(u, blk.mlp_proj.weight, blk.mlp_proj.bias)
        return F.linear(self._ln(m.ln_f)(h)[:, 0], m.head.weight, m.head.bias)


def test_vit_tiny_forward_against_plain_torch():
    torch.manual_seed(2)
    m = get_model("vit-tiny").eval()
    with torch.no_grad():  # biases and gains away from their 0 / 1 initial values: every term is exercised
        for n, p in m.named_parameters():
            if n.endswith("bias"):
                p.normal_(0, 0.05)
            elif p.ndim == 1:
                p.add_(0.1 * torch.randn_like(p))
    x = torch.randn(3, 3, 32, 32)
    with torch.no_grad():
        got, want = m(x), _TorchViT(m)(x)
    assert got.shape == (3, 10) and got.dtype == torch.float32
    assert torch.allclose(got, want, rtol=1e-4, atol=1e-5), (got - want).abs().max().item()
    # the gradients too: the padding rows pass nothing back
    m.train()
    loss = F.cross_entropy(m(x), torch.tensor([1, 2, 3]))
    loss.backward()
    gm = {n: p.grad.clone() for n, p in m.named_parameters()}
    m.zero_grad()
    F.cross_entropy(_TorchViT(m)(x), torch.tensor([1, 2, 3])).backward()
    for n, p in m.named_parameters():
        assert torch.allclose(gm[n], p.grad, rtol=1e-3, atol=1e-6), n


def test_bidirectional_block_refuses_dropout_and_documents():
    m = get_model("vit-tiny")
    x = torch.randn(1, 64, 128)
    with pytest.raises(ValueError):
        m.blocks[0](x, None, (0.1, None, 1))
    with pytest.raises(ValueError):
        m.blocks[0](x, Fx.doc_bounds(torch.zeros(1, 64, dtype=torch.int32)))


# ---------------------------------------------------------------------- CLI
def _train(tmp_path, extra):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, PYTHONPATH=ROOT, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
               MASTER_PORT=str(port), OMP_NUM_THREADS="2", CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--backend", "gloo", "--epochs", "1", "--max-steps", "2",
           "--num-samples", "16", "--batch-size", "4", "--seed", "1", "--checkpoint-dir", str(tmp_path / "ck"), *extra]
    return subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)


def test_train_cli_vit_tiny(tmp_path):
    r = _train(tmp_path, ["--model", "vit-tiny", "--label-smoothing", "0.1"])
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    log = r.stdout + r.stderr
    assert "Model parameters: 425,098" in log  # 2 blocks of 198,272 + patch 24,704 + cls 128 + pos 2,176 + ln_f 256 + head 1,290
    loss = float(log.split("Train Loss: ")[1].split()[0])
    assert math.isfinite(loss) and 1.8 < loss < 2.8  # ln(10) = 2.30 at initialisation


@pytest.mark.parametrize("flags,msg", [(["--mixup-alpha", "0.2"], "--mixup-alpha"), (["--cutmix-alpha", "1.0"], "--cutmix-alpha"),
                                       (["--dropout", "0.1"], "--dropout"), (["--doc-len-mean", "32"], "--doc-len-mean"),
                                       (["--image-size", "36"], "--image-size")])
def test_train_cli_parser_errors(capsys, flags, msg):
    """Parser errors leave before anything is initialised: checked in process."""
    from distributed_pytorch_example_amd.train import main

    with pytest.raises(SystemExit) as e:
        main(["--model", "vit-tiny", *flags])
    err = capsys.readouterr().err
    assert e.value.code == 2 and msg in err and "vit" in err, err[-2000:]
