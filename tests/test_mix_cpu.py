"""Mixup / CutMix without a GPU: BatchMixer's CPU path against the fp64 references, the two-label CE identity,
the Beta CDF quadrature, the distribution checks the GPU draw is held to (on a torch Beta sample), flag validation and
a one-epoch train.py run."""
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import _mix_ref as R
from distributed_pytorch_example_amd.data import BatchMixer
from distributed_pytorch_example_amd.ops import functional as Fx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_quadrature_matches_scipy_betainc():
    sp = pytest.importorskip("scipy.special")
    x = np.linspace(0.0, 1.0, 201)
    for alpha in (0.2, 0.5, 1.0, 2.0, 5.0):
        err = np.max(np.abs(R.betainc_quad(alpha, x) - sp.betainc(alpha, alpha, x)))
        print(f"alpha {alpha}: quadrature max error {err:.2e}")
        assert err < 1e-4


def test_quadrature_closed_forms():
    x = np.linspace(0.0, 1.0, 101)
    assert np.max(np.abs(R.betainc_quad(1.0, x) - x)) < 1e-9                        # uniform
    assert np.max(np.abs(R.betainc_quad(2.0, x) - (3 * x ** 2 - 2 * x ** 3))) < 1e-4
    assert np.max(np.abs(R.betainc_quad(0.5, x) - 2 / np.pi * np.arcsin(np.sqrt(x)))) < 1e-4  # arcsine law


@pytest.mark.parametrize("alpha", [0.2, 1.0, 2.0])
def test_the_distribution_check_is_satisfiable(alpha):
    """A torch fp64 Beta sample of the GPU test's size passes the very check the GPU draw is held to, and a sample
    of a neighbouring alpha misses it: the bound is neither impossible nor blind."""
    g = torch.Generator().manual_seed(5)
    n = 8192

    def beta(a):
        ga = torch._standard_gamma(torch.full((n, 2), a, dtype=torch.float64), generator=g)
        return (ga[:, 0] / ga.sum(1)).numpy()

    d = R.check_lam_sample(beta(alpha), alpha)
    print(f"alpha {alpha}: sup |F_n - F| = {d:.4f}")
    for other in (alpha * 0.5, alpha * 2.0):
        with pytest.raises(AssertionError):
            R.check_lam_sample(beta(other), alpha)
    u = torch.randint(0, 160, (n,), generator=g).numpy()
    assert R.ks_sup_discrete(u, 160) <= 0.03


def test_batchmixer_cpu_rows_and_pixels():
    torch.manual_seed(0)
    mixer = BatchMixer(mixup_alpha=0.2, cutmix_alpha=1.0, prob=0.8, switch_prob=0.5)
    x = torch.randn(3, 3, 6, 10)
    y = torch.tensor([1, 7, 4])
    seen = set()
    for _ in range(40):
        rows = mixer.draw(6, 10)
        assert rows.shape == (1, 8) and rows.dtype == torch.float32
        row = rows[0]
        mode = int(row[6])
        seen.add(mode)
        x1, y1, x2, y2 = (int(v) for v in row[2:6])
        if mode == 0:
            assert row[:7].tolist() == [1, 1, 0, 0, 0, 0, 0]
        elif mode == 1:
            assert row[0] == row[1] == row[7] and (x1, y1, x2, y2) == (0, 0, 0, 0)
        else:
            assert row[0] == 1 and 0 <= x1 <= x2 <= 10 and 0 <= y1 <= y2 <= 6
            assert abs(float(row[1]) - (1 - (x2 - x1) * (y2 - y1) / 60)) < 1e-6
            hw, hh = R.half_sizes(float(row[7]), 6, 10)
            assert x2 - x1 <= 2 * hw and y2 - y1 <= 2 * hh
        out = BatchMixer.mix_torch(x, row)
        assert torch.allclose(out.double(), R.mix_pixels(x, row), atol=1e-6, rtol=0)
    assert seen == {0, 1, 2}
    xo, (t, t2, w) = mixer(x, y)
    assert xo.shape == x.shape and torch.equal(t, y) and torch.equal(t2, y.roll(1, 0)) and w.shape == (1,)
    assert 0.0 <= float(w) <= 1.0


def test_batchmixer_box_rule_is_torchvisions():
    assert R.cutmix_box(0.75, 5, 3, 6, 10) == (3, 2, 7, 4)   # half sizes int(0.25 * 10), int(0.25 * 6)
    assert R.cutmix_box(0.0, 0, 0, 6, 10) == (0, 0, 5, 3)    # clamped at two borders
    assert R.cutmix_box(1.0, 9, 5, 6, 10) == (9, 5, 9, 5)    # empty
    from distributed_pytorch_example_amd.data.mix import cutmix_box

    for lam in (0.0, 0.3, 0.75, 1.0):
        for c in ((0, 0), (5, 3), (9, 5)):
            assert cutmix_box(lam, *c, 6, 10) == R.cutmix_box(lam, *c, 6, 10)


def test_batchmixer_features_and_errors():
    torch.manual_seed(1)
    x = torch.randn(4, 784)
    y = torch.tensor([0, 1, 2, 3])
    xo, (t, t2, w) = BatchMixer(mixup_alpha=1.0)(x, y)
    lam = float(w)
    assert torch.allclose(xo, lam * x + (1 - lam) * x.roll(1, 0), atol=1e-6)
    with pytest.raises(ValueError):
        BatchMixer(cutmix_alpha=1.0)(x, y)
    for kw in (dict(mixup_alpha=-1.0), dict(prob=1.5), dict(switch_prob=-0.1)):
        with pytest.raises(ValueError):
            BatchMixer(**kw)
    off = BatchMixer()
    assert not off.enabled and off.draw(4, 4)[0].tolist() == [1, 1, 0, 0, 0, 0, 0, 1]
    with pytest.raises(ValueError):
        Fx.mix_pack(torch.randn(2, 3, 4, 4), off.draw(4, 4)[0])          # GPU only
    with pytest.raises(ValueError):
        Fx.mix_pack(torch.randn(2, 3, 4, 4, requires_grad=True), off.draw(4, 4)[0])


@pytest.mark.parametrize("eps,zl", [(0.0, 0.0), (0.1, 0.0), (0.1, 1e-4)])
def test_two_label_ce_identity_fp64(eps, zl):
    """w CE(y) + (1 - w) CE(y2) == the two-label CE (per-row w, y == y2, ignored rows, a row without partner), for
    the formula, the autograd reference and Fx.cross_entropy's CPU branch."""
    import _ce_reg_ref as P

    g = torch.Generator().manual_seed(3)
    B, V = 8, 10
    z = 3.0 * torch.randn(B, V, generator=g, dtype=torch.float64)
    y = torch.randint(0, V, (B,), generator=g)
    y2 = y.roll(1, 0).clone()
    y[0], y[1], y2[2], y2[3], y[4], y2[5] = V - 1, -100, -100, y[3], 0, 0
    for w in (torch.tensor([0.3]), torch.rand(B, generator=g)):
        la, ga = R.ce_autograd_ref(z, y, y2, w, V, eps, zl)
        lf, gf = R.ce_formula_ref(z, y, y2, w, V, eps, zl)
        assert abs(la - lf) < 1e-12 and (ga - gf).abs().max() < 1e-12
        # the convex combination of two plain CEs, row by row
        yy2, ww = R._second(y, y2, w, -100)
        tot = 0.0
        for i in range(B):
            if y[i] == -100:
                assert ga[i].abs().max() == 0
                continue
            a, _ = P.formula_ref(z[i:i + 1], y[i:i + 1], V, eps, zl)
            b, _ = P.formula_ref(z[i:i + 1], yy2[i:i + 1], V, eps, zl)
            tot += float(ww[i]) * a + (1 - float(ww[i])) * b
        assert abs(tot / int((y != -100).sum()) - la) < 1e-12
        fx = Fx.cross_entropy(z.float(), y, V, label_smoothing=eps, z_loss=zl, labels2=y2, mix_w=w.float())
        assert abs(fx.item() - la) < 1e-5 * abs(la)
    # w = 1 is the one-label loss; dropping the partner term is visible
    l1, g1 = R.ce_formula_ref(z, y, y2, torch.tensor([1.0]), V, eps, zl)
    lp, gp = P.formula_ref(z, y, V, eps, zl)
    assert abs(l1 - lp) < 1e-12 and (g1 - gp).abs().max() < 1e-12
    _, gd = R.ce_formula_ref(z, y, y2, torch.tensor([0.5]), V, eps, zl, drop="partner")
    _, g5 = R.ce_formula_ref(z, y, y2, torch.tensor([0.5]), V, eps, zl)
    assert (gd - g5).abs().max() > 0.4 * (1 - eps)
    with pytest.raises(ValueError):
        Fx.cross_entropy(z.float(), y, V, labels2=y2)


def test_bf16_rounding_reference():
    v = torch.tensor([1.0, 1.00390625, 1.01171875, -3.3, 1e-3, 0.0], dtype=torch.float64)  # 1 + 2^-8: a tie, to even
    assert torch.equal(R.bf16_round(v), v.float().to(torch.bfloat16).double())
    # a value whose fp32 rounding lands on a bf16 tie: rounding twice would go the other way
    t = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -30], dtype=torch.float64)
    assert R.bf16_round(t).item() == 1.0 + 2.0 ** -7


@pytest.mark.parametrize("flags,needle", [
    (["--mixup-alpha", "-0.1"], "--mixup-alpha"),
    (["--cutmix-alpha", "-1"], "--cutmix-alpha"),
    (["--mix-prob", "0.5"], "--mix-prob"),
    (["--mixup-alpha", "0.2", "--mix-prob", "1.5"], "--mix-prob"),
    (["--mixup-alpha", "0.2", "--mix-switch-prob", "-0.5"], "--mix-switch-prob"),
    (["--cutmix-alpha", "1.0"], "--cutmix-alpha"),                       # simplenet has no images
    (["--model", "gpt2-tiny", "--mixup-alpha", "0.2"], "gpt2"),
])
def test_train_rejects_mix_flags_before_it_starts(flags, needle, capsys):
    from distributed_pytorch_example_amd.train import main

    with pytest.raises(SystemExit) as e:
        main(flags)
    assert e.value.code == 2
    assert needle in capsys.readouterr().err


def test_train_resnet_tiny_one_epoch_with_mixing(tmp_path):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, PYTHONPATH=ROOT, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
               MASTER_PORT=str(port), OMP_NUM_THREADS="2", CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--backend", "gloo", "--model", "resnet_tiny", "--epochs", "1",
           "--max-steps", "3", "--num-samples", "64", "--batch-size", "8", "--image-size", "32", "--seed", "3",
           "--mixup-alpha", "0.2", "--cutmix-alpha", "1.0", "--label-smoothing", "0.1", "--checkpoint-dir", str(tmp_path)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    m = re.search(r"Train Loss: ([0-9.eE+-]+|nan|inf)", r.stdout + r.stderr)
    assert m, (r.stdout + r.stderr)[-2000:]
    assert np.isfinite(float(m.group(1))) and float(m.group(1)) > 0
