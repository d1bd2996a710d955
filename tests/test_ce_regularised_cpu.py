"""Label smoothing and z-loss without a GPU: the references themselves, the CPU branches of the public functions
against the fp64 formula, argument validation, the train.py flags, and validation staying the plain CE."""
import os
import socket
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import _ce_reg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REGS = [(0.1, 0.0), (0.0, 1e-4), (0.0, 1e-2), (0.1, 1e-4), (0.1, 1e-2)]


def _inputs(B, V, ld, seed=0):
    g = torch.Generator().manual_seed(1234 + seed + V)
    z = 3.0 * torch.randn(B, ld, generator=g)
    y = torch.randint(0, V, (B,), generator=g)
    y[0] = V - 1
    y[1] = -100
    if B > 5:
        y[5] = -100
    return z, y


@pytest.mark.parametrize("B,V,ld", [(8, 16, 16), (8, 1000, 1000), (8, 1003, 1008)])
def test_formula_is_the_autograd_reference(B, V, ld):
    z, y = _inputs(B, V, ld)
    for eps, lam in REGS + [(0.0, 0.0)]:
        la, ga = R.autograd_ref(z.double(), y, V, eps, lam)
        lf, gf = R.formula_ref(z.double(), y, V, eps, lam)
        assert abs(la - lf) <= 1e-13 * abs(la)
        assert (ga - gf).abs().max().item() <= 1e-14
        assert gf[:, V:].abs().sum().item() == 0.0 and gf[y == -100].abs().sum().item() == 0.0


@pytest.mark.parametrize("B,V,ld", [(8, 16, 16), (8, 1000, 1000)])
def test_the_bound_sees_each_term(B, V, ld):
    """With E0 taken from an fp32 evaluation of the plain CE (here torch's on the CPU, standing in for the plain
    kernel: the GPU test repeats this with the kernel's own E0), every crippled reference misses the gradient
    bound and the loss bound by 3x at least."""
    z, y = _inputs(B, V, ld)
    zf = z.clone().requires_grad_(True)
    n = int((y != -100).sum())
    (g32,) = torch.autograd.grad(F.cross_entropy(zf[:, :V], y, ignore_index=-100) * n, zf)
    _, g64 = R.autograd_ref(z.double(), y, V, 0.0, 0.0)
    E0 = (g32.double() - g64).abs().max().item()
    assert 0.0 < E0 < 1e-6
    bound = R.f32_bound(E0)
    seen = set()
    for eps, lam in REGS:
        for drop, (gr, lr) in R.sensitivity(z.double(), y, V, eps, lam, bound).items():
            seen.add(drop)
            assert gr >= 3.0 and lr >= 3.0, (drop, eps, lam, gr, lr)
    assert seen == set(R.DROPS)


def test_cpu_branches_match_the_formula():
    from distributed_pytorch_example_amd.ops import functional as Fx
    from distributed_pytorch_example_amd.ops.layers import CrossEntropyLoss

    z, y = _inputs(8, 1003, 1008)
    n = int((y != -100).sum())
    for eps, lam in REGS + [(0.0, 0.0)]:
        loss_ref, g_ref = R.formula_ref(z.double(), y, 1003, eps, lam)
        zz = z.clone().requires_grad_(True)
        loss = Fx.cross_entropy(zz, y, 1003, label_smoothing=eps, z_loss=lam)
        loss.backward()
        assert abs(loss.item() - loss_ref) < 1e-5 * abs(loss_ref)
        assert (zz.grad.double() - g_ref / n).abs().max().item() < 1e-6
        assert zz.grad[:, 1003:].abs().max().item() == 0.0
        mod = CrossEntropyLoss(label_smoothing=eps, z_loss=lam)
        assert abs(mod(z[:, :1003], y).item() - loss_ref) < 1e-5 * abs(loss_ref)
        # the tied LM head: logits = x @ wte^T
        g = torch.Generator().manual_seed(5)
        x, wte = torch.randn(2, 4, 32, generator=g), torch.randn(50, 32, generator=g, requires_grad=True)
        yy = torch.randint(0, 50, (2, 4), generator=g)
        yy[0, 0] = -100
        lr, _ = R.formula_ref((x.reshape(-1, 32) @ wte.detach().T).double(), yy.reshape(-1), 50, eps, lam)
        assert abs(Fx.lm_head_ce(x, wte, yy, label_smoothing=eps, z_loss=lam).item() - lr) < 1e-5 * abs(lr)


def test_argument_validation():
    from distributed_pytorch_example_amd.ops import functional as Fx
    from distributed_pytorch_example_amd.ops.layers import CrossEntropyLoss

    z, y = _inputs(8, 16, 16)
    for kw in (dict(label_smoothing=1.0), dict(label_smoothing=-0.1), dict(z_loss=-1e-3)):
        with pytest.raises(ValueError):
            Fx.cross_entropy(z, y, **kw)
        with pytest.raises(ValueError):
            Fx.lm_head_ce(z[:, None, :], torch.randn(5, 16), y[:, None].clamp(0, 4), **kw)
        with pytest.raises(ValueError):
            CrossEntropyLoss(**kw)
    m = CrossEntropyLoss()
    assert (m.ignore_index, m.label_smoothing, m.z_loss) == (-100, 0.0, 0.0)


def test_gpt2_config_carries_the_regularisers():
    from distributed_pytorch_example_amd.models import get_model
    from distributed_pytorch_example_amd.models.gpt2 import GPT2Config

    assert (GPT2Config().label_smoothing, GPT2Config().z_loss) == (0.0, 0.0)
    torch.manual_seed(0)
    m = get_model("gpt2-tiny", label_smoothing=0.1, z_loss=1e-2, n_layer=1)
    assert (m.cfg.label_smoothing, m.cfg.z_loss) == (0.1, 1e-2)
    idx = torch.randint(0, 512, (2, 16))
    tgt = torch.randint(0, 512, (2, 16))
    logits = m(idx)
    want, _ = R.formula_ref(logits.double().reshape(-1, 512), tgt.reshape(-1), 512, 0.1, 1e-2)
    assert abs(m(idx, tgt).item() - want) < 1e-5 * abs(want)


def test_parser_flags():
    from distributed_pytorch_example_amd.train import build_parser, main

    a = build_parser().parse_args([])
    assert a.label_smoothing == 0.0 and a.z_loss == 0.0
    a = build_parser().parse_args(["--label-smoothing", "0.1", "--z-loss", "1e-4"])
    assert a.label_smoothing == 0.1 and a.z_loss == 1e-4
    help_text = build_parser().format_help()
    assert "validation" in help_text and "plain" in help_text
    for bad in (["--label-smoothing", "1.0"], ["--z-loss", "-1"]):
        with pytest.raises(SystemExit) as e:
            main(bad)
        assert e.value.code == 2


def test_validation_loss_is_the_plain_ce():
    """train.validate goes through Fx.cross_entropy_eval, whatever the training criterion is."""
    from distributed_pytorch_example_amd.models import get_model
    from distributed_pytorch_example_amd.train import validate

    torch.manual_seed(1)
    model = get_model("simplenet")
    data = [(torch.randn(16, 784), torch.randint(0, 10, (16,))) for _ in range(3)]

    def criterion(out, tgt):
        raise AssertionError("validate must not use the training criterion")

    loss, acc = validate(model, data, criterion, torch.device("cpu"), 10)
    with torch.no_grad():
        want = sum(F.cross_entropy(model(x).float(), y).item() for x, y in data) / 3
    assert abs(loss - want) < 1e-5 * want and 0.0 <= acc <= 100.0


def test_train_cli_with_regularisers(tmp_path):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, PYTHONPATH=ROOT, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
               MASTER_PORT=str(port), OMP_NUM_THREADS="2", CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--backend", "gloo", "--model", "simplenet", "--epochs", "1",
           "--max-steps", "3", "--num-samples", "256", "--lr", "0", "--checkpoint-dir", str(tmp_path / "ck"),
           "--label-smoothing", "0.1", "--z-loss", "0.05"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-3000:]
    train = float(log.split("  Train Loss: ")[1].split()[0])
    val = float(log.split("  Val Loss: ")[1].split(",")[0])
    # lr 0: one model for both losses, on random 10-class data (plain CE about ln 10 on either split); the train
    # loss carries the regularisers (z-loss alone: 0.05 * lse^2 >= 0.05 * ln(10)^2 = 0.26), the val loss does not
    assert train > val + 0.1, (train, val)
