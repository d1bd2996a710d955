"""The fp64 references of tests/_gpt2_ref.py checked where no GPU exists: the closed-form attention gradients
against fp64 autograd, the LayerNorm backward and the GELU derivative likewise, the cross-entropy gradient
against torch, and the input builders' claims."""
import math

import torch
import torch.nn.functional as F

import _gpt2_ref as R


def _close(a, b, tol=1e-11):
    assert (a - b).abs().max().item() <= tol * max(1.0, b.abs().max().item()), (a - b).abs().max().item()


def test_attention_closed_form_matches_autograd():
    torch.manual_seed(0)
    for (B, T, H, D) in ((2, 64, 3, 64), (1, 40, 2, 32)):
        qkv = torch.randn(B, T, 3, H, D).to(torch.bfloat16)
        dout = torch.randn(B, T, H, D).to(torch.bfloat16)
        scale = 1.0 / math.sqrt(D)
        ref = R.attn_ref(qkv, dout, scale)
        O, g = R.attn_autograd(qkv, dout, scale)
        _close(ref["out"], O)
        _close(ref["dqkv"], g)
        # lse2 against a direct evaluation, and softmax rows summing to one through it
        q, k, _ = qkv.double().permute(2, 0, 3, 1, 4)
        S = scale * (q @ k.transpose(-1, -2))
        for i in (0, T // 2, T - 1):
            want = torch.logsumexp(S[..., i, :i + 1], -1) / math.log(2.0)
            _close(ref["lse2"][..., i], want)
        assert (ref["b_out"] > 0).all() and (ref["b_dqkv"] > 0).all()


def test_emulation_within_budgets():
    """attn_emulate (the kernels' roundings in torch) stays inside attn_ref's budgets on randn inputs."""
    torch.manual_seed(1)
    qkv = torch.randn(1, 128, 3, 2, 64).to(torch.bfloat16)
    dout = torch.randn(1, 128, 2, 64).to(torch.bfloat16)
    ref = R.attn_ref(qkv, dout, 0.125)
    out, lse2, dqkv = R.attn_emulate(qkv, dout, 0.125)
    assert ((out.double() - ref["out"]).abs() / ref["b_out"]).max().item() <= 1.0
    assert (lse2.double() - ref["lse2"]).abs().max().item() <= ref["b_lse2"]
    assert ((dqkv.double() - ref["dqkv"]).abs() / ref["b_dqkv"]).max().item() <= 1.0


def test_staircase_moves_the_row_max():
    qkv, a = R.staircase_qkv(256, (12.0, 6.5))
    tm = R.tile_row_max(qkv, 0.125)[0]  # [H, T, 4]
    hi = a > 0
    jump = tm[..., 1:] - tm[..., :-1]
    fin = torch.isfinite(tm[..., 1:])
    j0, j1 = jump[0], jump[1]
    assert ((j0[hi] > 8) & fin[0][hi]).sum(-1).max().item() >= 2
    assert not ((j0[~hi] > 8) & fin[0][~hi]).any()
    assert ((j1[hi] > 4) & (j1[hi] < 8) & fin[1][hi]).any() and not ((j1 > 8) & fin[1]).any()
    later, defer, dist = R.deferred_max_trace(tm)
    assert later[0][hi].max().item() >= 2 and later[0][~hi].max().item() == 0
    assert defer[1][hi].max().item() > 4 and dist.min().item() > 0.25


def test_layernorm_and_gelu_refs_match_autograd():
    torch.manual_seed(2)
    x = torch.randn(7, 24, dtype=torch.float64, requires_grad=True)
    w = torch.randn(24, dtype=torch.float64, requires_grad=True)
    b = torch.randn(24, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(7, 24, dtype=torch.float64)
    y = F.layer_norm(x, (24,), w, b, 1e-5)
    y.backward(dy)
    yr, mean, rstd, _ = R.ln_ref(x.detach(), w.detach(), b.detach())
    dx, dw, db = R.ln_bwd_ref(dy, x.detach(), w.detach())
    _close(yr, y.detach()); _close(dx, x.grad); _close(dw, w.grad); _close(db, b.grad)
    _close(mean, x.detach().mean(-1))
    t = torch.linspace(-6, 6, 101, dtype=torch.float64, requires_grad=True)
    g = F.gelu(t, approximate="tanh")
    g.sum().backward()
    _close(R.gelu_ref(t.detach()), g.detach()); _close(R.gelu_grad_ref(t.detach()), t.grad)


def test_cross_entropy_ref_matches_torch():
    torch.manual_seed(3)
    z = torch.randn(9, 40, dtype=torch.float64, requires_grad=True)
    V, ign = 37, 5
    lab = torch.tensor([0, 36, 29, 5, 5, 7, 1, 5, 36])
    loss = F.cross_entropy(z[:, :V], lab, ignore_index=ign, reduction="sum")
    loss.backward()
    rows, g, am, valid = R.ce_ref(z.detach(), lab, V, 1.0, ign)
    _close(rows.sum(), loss.detach()); _close(g, z.grad)
    assert valid.sum().item() == 6 and (rows[~valid] == 0).all() and (g[:, V:] == 0).all()
    assert (am == z.detach()[:, :V].argmax(1)).all()
