"""ConvNeXt on the CPU path: the parameter count, the model against the same graph in plain torch ops, the depthwise
op against F.conv2d, and the train.py command line."""
import math
import os
import socket
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from distributed_pytorch_example_amd.models import get_model
from distributed_pytorch_example_amd.ops import functional as Fx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_convnext_tiny_parameter_count():
    assert get_model("convnext-tiny").num_params() == 28_589_128  # torchvision's convnext_tiny


def _plain(m, x):
    """The convnext-test graph in NCHW torch ops on m's parameters."""
    def ln(mod, t):  # channels-last LayerNorm of an NCHW tensor
        return F.layer_norm(t.permute(0, 2, 3, 1), (t.shape[1],), mod.weight, mod.bias, 1e-6).permute(0, 3, 1, 2)

    h = ln(m.stem_norm, F.conv2d(x, m.stem.weight, m.stem.bias, stride=4))
    for i, stage in enumerate(m.stages):
        if i:
            d = m.downs[i - 1]
            h = F.conv2d(ln(m.down_norms[i - 1], h), d.weight, d.bias, stride=2)
        for b in stage:
            t = F.conv2d(h, b.dwconv.weight, b.dwconv.bias, padding=3, groups=h.shape[1])
            t = F.layer_norm(t.permute(0, 2, 3, 1), (h.shape[1],), b.norm.weight, b.norm.bias, 1e-6)
            t = F.linear(F.gelu(F.linear(t, b.fc1.weight, b.fc1.bias), approximate="tanh"), b.fc2.weight, b.fc2.bias)
            h = h + (b.gamma * t).permute(0, 3, 1, 2)
    h = F.layer_norm(h.mean(dim=(2, 3)), (h.shape[1],), m.head_norm.weight, m.head_norm.bias, 1e-6)
    return F.linear(h, m.head.weight, m.head.bias)


def test_convnext_test_model_matches_plain_torch():
    torch.manual_seed(2)
    m = get_model("convnext-test", layer_scale_init=0.5)  # a layer scale at which the blocks carry signal
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("bias"):
                p.normal_(0, 0.05)
    x = torch.randn(4, 3, 32, 32)
    tgt = torch.randint(0, 10, (4,))
    params = list(m.parameters())
    la = F.cross_entropy(m(x), tgt)
    ga = torch.autograd.grad(la, params)
    lb = F.cross_entropy(_plain(m, x), tgt)
    gb = torch.autograd.grad(lb, params)
    torch.testing.assert_close(la, lb, rtol=1e-5, atol=1e-6)
    for (n, _), a, b in zip(m.named_parameters(), ga, gb):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6 * b.abs().max().item(), msg=lambda s, n=n: f"{n}: {s}")


def test_depthwise_op_cpu_matches_conv2d():
    torch.manual_seed(3)
    x = torch.randn(2, 9, 5, 16, requires_grad=True)
    w = torch.randn(16, 1, 7, 7, requires_grad=True)
    b = torch.randn(16, requires_grad=True)
    dy = torch.randn(2, 9, 5, 16)
    got = torch.autograd.grad(Fx.depthwise_conv2d_nhwc(x, w, b), (x, w, b), dy)
    y = F.conv2d(x.permute(0, 3, 1, 2), w, b, padding=3, groups=16).permute(0, 2, 3, 1)
    torch.testing.assert_close(Fx.depthwise_conv2d_nhwc(x, w, b), y)
    for a, r in zip(got, torch.autograd.grad(y, (x, w, b), dy)):
        torch.testing.assert_close(a, r)
    with pytest.raises(ValueError):
        Fx.depthwise_conv2d_nhwc(x, torch.randn(16, 1, 3, 3))


def test_train_cli_convnext_test(tmp_path):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, PYTHONPATH=ROOT, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
               MASTER_PORT=str(port), OMP_NUM_THREADS="2", CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--backend", "gloo", "--epochs", "1", "--max-steps", "2",
           "--num-samples", "16", "--batch-size", "4", "--seed", "1", "--checkpoint-dir", str(tmp_path / "ck"),
           "--model", "convnext-test"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-3000:]
    loss = float(log.split("Train Loss: ")[1].split()[0])
    assert math.isfinite(loss) and 1.8 < loss < 2.8  # ln(10) = 2.30 at initialisation


@pytest.mark.parametrize("flags,msg", [(["--mixup-alpha", "0.2"], "--mixup-alpha"), (["--cutmix-alpha", "1.0"], "--cutmix-alpha"),
                                       (["--dropout", "0.1"], "--dropout"), (["--doc-len-mean", "32"], "--doc-len-mean")])
def test_train_cli_parser_errors(capsys, flags, msg):
    from distributed_pytorch_example_amd.train import main

    with pytest.raises(SystemExit) as e:
        main(["--model", "convnext-test", *flags])
    err = capsys.readouterr().err
    assert e.value.code == 2 and f"{msg} is not available for the convnext models" in err, err[-2000:]
