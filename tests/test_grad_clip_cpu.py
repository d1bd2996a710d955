"""Gradient clipping without a GPU: the CPU path of set_grad_clip is the stock torch sequence, the argument
checks, the unchanged state_dict schema, and the train.py flags end to end on gloo at world 1."""
import copy
import os
import socket
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(37, 5, generator=g).requires_grad_(True), torch.randn(1025, generator=g).requires_grad_(True)]


def _set_grads(ps, seed):
    g = torch.Generator().manual_seed(100 + seed)
    for p in ps:
        p.grad = torch.randn(p.shape, generator=g)


def _pair(kind, a, b):
    from distributed_pytorch_example_amd import optim

    if kind == "adam":
        return optim.Adam(a, lr=1e-2), torch.optim.Adam(b, lr=1e-2)
    if kind == "adamw":
        return optim.AdamW(a, lr=1e-2, weight_decay=1e-2), torch.optim.AdamW(b, lr=1e-2, weight_decay=1e-2)
    return optim.SGD(a, lr=0.05, momentum=0.9), torch.optim.SGD(b, lr=0.05, momentum=0.9)


@pytest.mark.parametrize("kind", ["adam", "adamw", "sgd"])
@pytest.mark.parametrize("max_norm", [0.5, 1e4])
def test_cpu_path_is_the_stock_sequence(kind, max_norm):
    ours_p, ref_p = _params(), _params()
    ours, ref = _pair(kind, ours_p, ref_p)
    ours.set_grad_clip(max_norm)
    assert ours.grad_norm is None
    for s in range(3):
        _set_grads(ours_p, s)
        ours.step()
        _set_grads(ref_p, s)
        n = torch.nn.utils.clip_grad_norm_(ref_p, max_norm)
        ref.step()
        assert torch.equal(ours.grad_norm, n)
        for a, b in zip(ours_p, ref_p):
            assert torch.equal(a.grad, b.grad)  # torch's clip scales the gradients in place
    for a, b in zip(ours_p, ref_p):
        assert torch.equal(a, b)
    assert float(ours.skipped_steps) == 0.0


def test_cpu_skip_nonfinite():
    from distributed_pytorch_example_amd.optim import SGD

    ps = _params()
    opt = SGD(ps, lr=0.05, momentum=0.9)
    opt.set_grad_clip(1.0, skip_nonfinite=True)
    _set_grads(ps, 0)
    opt.step()
    before = [p.detach().clone() for p in ps]
    _set_grads(ps, 1)
    ps[-1].grad[-1] = float("inf")
    opt.step()
    for a, b in zip(ps, before):
        assert torch.equal(a, b)
    assert float(opt.skipped_steps) == 1.0 and torch.isinf(opt.grad_norm)


@pytest.mark.parametrize("bad", [0, 0.0, -1.0, float("nan")])
def test_set_grad_clip_rejects_non_positive(bad):
    from distributed_pytorch_example_amd.optim import Adam, build_optimizer

    with pytest.raises(ValueError):
        Adam(_params(), lr=1e-3).set_grad_clip(bad)
    with pytest.raises(ValueError):
        build_optimizer("sgd", _params(), lr=0.1, clip_grad_norm=bad)


def test_state_dict_unchanged_by_clip():
    a_p, b_p = _params(), _params()
    from distributed_pytorch_example_amd.optim import build_optimizer

    a = build_optimizer("adamw", a_p, lr=1e-2, weight_decay=1e-2)
    b = build_optimizer("adamw", b_p, lr=1e-2, weight_decay=1e-2, clip_grad_norm=1e4)  # never clips
    for s in range(2):
        _set_grads(a_p, s); a.step()
        _set_grads(b_p, s); b.step()
    sa, sb = a.state_dict(), b.state_dict()
    assert [sorted(g) for g in sa["param_groups"]] == [sorted(g) for g in sb["param_groups"]]
    assert sa["param_groups"] == sb["param_groups"]
    assert sa["state"].keys() == sb["state"].keys()
    for k in sa["state"]:
        assert sa["state"][k].keys() == sb["state"][k].keys()
        for name in sa["state"][k]:
            assert torch.equal(torch.as_tensor(sa["state"][k][name]), torch.as_tensor(sb["state"][k][name]))
    # a checkpoint taken with clipping loads into an optimizer without it, and back
    a.load_state_dict(copy.deepcopy(sb))
    b.load_state_dict(copy.deepcopy(sa))
    assert b._clip_max == 1e4  # the setting is the optimizer's, not the checkpoint's


def test_parser_defaults():
    from distributed_pytorch_example_amd.train import build_parser

    args = build_parser().parse_args([])
    assert args.clip_grad_norm is None and args.skip_nonfinite_steps is False
    args = build_parser().parse_args(["--clip-grad-norm", "1.0", "--skip-nonfinite-steps"])
    assert args.clip_grad_norm == 1.0 and args.skip_nonfinite_steps is True


def _train(tmp_path, extra):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, PYTHONPATH=ROOT, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
               MASTER_PORT=str(port), OMP_NUM_THREADS="2", CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--backend", "gloo", "--model", "simplenet", "--epochs", "1",
           "--max-steps", "3", "--num-samples", "256", "--checkpoint-dir", str(tmp_path / "ck"), *extra]
    return subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)


def test_train_cli_logs_grad_norm_only_with_the_flag(tmp_path):
    r = _train(tmp_path, ["--clip-grad-norm", "0.5"])
    assert r.returncode == 0, r.stderr[-3000:]
    log = r.stdout + r.stderr
    lines = [ln for ln in log.splitlines() if "Grad norm (last step): " in ln]
    assert len(lines) == 1, log[-3000:]
    tail = lines[0].split("Grad norm (last step): ")[1]
    norm, skipped = tail.split(", skipped steps: ")
    assert float(norm) > 0.0 and int(skipped) == 0
    assert log.index("  Throughput: ") < log.index("  Grad norm (last step): ")

    r = _train(tmp_path, [])
    assert r.returncode == 0, r.stderr[-3000:]
    assert "Grad norm" not in r.stdout + r.stderr
