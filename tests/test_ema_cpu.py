"""The weight EMA (set_ema) without a GPU: the CPU path against torch.optim.swa_utils.AveragedModel bit for bit,
the warm-up sequence, state_dict interchange, ema_weights(), argument handling and a resumed end-to-end run."""
import copy
import io
import os
import socket
import subprocess
import sys

import pytest
import torch
from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["adam", "adamw", "sgd", "lars", "lamb", "muon"]


class _Net(torch.nn.Module):
    """Three parameters: a matrix Muon takes (16 x 8), a bias, and a 3-D tensor it does not."""

    def __init__(self, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.w = torch.nn.Parameter(torch.randn(16, 8, generator=g))
        self.b = torch.nn.Parameter(torch.randn(16, generator=g))
        self.k = torch.nn.Parameter(torch.randn(3, 5, 7, generator=g))


def _make(name, net, ngroups):
    from distributed_pytorch_example_amd import optim

    cls = {"adam": optim.Adam, "adamw": optim.AdamW, "sgd": optim.SGD, "lars": optim.LARS, "lamb": optim.LAMB,
           "muon": optim.Muon}[name]
    if ngroups == 1:
        groups = [{"params": [net.w] if name == "muon" else [net.w, net.b, net.k]}]
        if name == "muon":  # its one-group form: a Muon group; the others go to an AdamW group of the same optimizer
            groups.append({"params": [net.b, net.k], "use_muon": False})
    else:
        groups = [{"params": [net.w], "lr": 0.02}, {"params": [net.b], "lr": 0.01}, {"params": [net.k], "lr": 0.005}]
        if name == "muon":
            groups[1]["use_muon"] = groups[2]["use_muon"] = False
    return cls(groups, lr=0.01, weight_decay=1e-2)


def _set(net, seed):
    g = torch.Generator().manual_seed(1000 + seed)
    for p in net.parameters():
        p.grad = torch.randn(p.shape, generator=g)


def _params(opt):
    return [p for g in opt.param_groups for p in g["params"]]


@pytest.mark.parametrize("ngroups", [3, 1])
@pytest.mark.parametrize("name", NAMES)
def test_equals_averaged_model_bitwise(name, ngroups):
    """5 steps: the average is AveragedModel's EMA bit for bit, and the weights are those of a twin optimizer
    without an EMA."""
    net, twin = _Net(), _Net()
    opt, plain = _make(name, net, ngroups), _make(name, twin, ngroups)
    opt.set_ema(0.9)
    assert opt.ema_decay_now is None and float(opt.ema_num_updates) == 0.0
    avg = AveragedModel(net, multi_avg_fn=get_ema_multi_avg_fn(0.9))
    for s in range(5):
        _set(net, s); _set(twin, s)
        opt.step(); plain.step()
        avg.update_parameters(net)
        for p, q in zip(net.parameters(), twin.parameters()):
            assert torch.equal(p, q), (name, s)
        for p, a in zip(net.parameters(), avg.module.parameters()):
            assert torch.equal(opt.state[p]["ema"], a), (name, s)
        if s == 0:  # the first update copies
            assert all(torch.equal(e, p) for e, p in zip(opt.ema_parameters(), _params(opt)))
    assert float(opt.ema_num_updates) == 5.0
    assert opt.ema_decay_now.dtype == torch.float32 and float(opt.ema_decay_now) == float(torch.tensor(0.9))
    assert [e.data_ptr() for e in opt.ema_parameters()] == [opt.state[p]["ema"].data_ptr() for p in _params(opt)]
    assert "ema" not in plain.state_dict() and all("ema" not in st for st in plain.state.values())


@pytest.mark.parametrize("name", NAMES)
def test_warmup_sequence(name):
    """d_0 = 0, d_n = min(decay, (1 + n) / (10 + n)): 0.2 at n = 1 up to the cap 0.5 from n = 8 on; each update is
    the lerp by 1 - d_n of the weights the step wrote."""
    from distributed_pytorch_example_amd.optim import ema_decay_at

    net = _Net(1)
    opt = _make(name, net, 3)
    opt.set_ema(0.5, warmup=True)
    seen = []
    for n in range(11):
        before = [e.clone() for e in opt.ema_parameters()]
        _set(net, n)
        opt.step()
        want = 0.0 if n == 0 else min(0.5, (1.0 + n) / (10.0 + n))
        assert ema_decay_at(n, 0.5, True) == want
        assert float(opt.ema_decay_now) == float(torch.tensor(want, dtype=torch.float32)), n
        seen.append(want)
        for e, e0, p in zip(opt.ema_parameters(), before, _params(opt)):
            ref = p.detach().clone() if n == 0 else torch.lerp(e0, p.detach(), 1.0 - want)
            assert torch.equal(e, ref), (name, n)
    assert seen[1] == 2.0 / 11.0 and seen[7] < 0.5 and seen[8] == 0.5 == seen[10]
    assert ema_decay_at(3, 0.999, False) == 0.999 and ema_decay_at(0, 0.999, False) == 0.0


@pytest.mark.parametrize("name", ["adamw", "sgd", "lamb", "muon"])
def test_state_dict_round_trip(name):
    """Saved after 3 steps (through torch.save / torch.load(weights_only=True)) and loaded into a fresh optimizer
    whose own EMA flags differ: the checkpoint's settings win, and 4 more steps are bitwise the uninterrupted run."""
    a_net = _Net(2)
    a = _make(name, a_net, 3)
    a.set_ema(0.8, warmup=True)
    for s in range(3):
        _set(a_net, s); a.step()
    sd = a.state_dict()
    assert sd["ema"] == {"decay": 0.8, "warmup": True, "num_updates": 3}
    assert all(type(v) in (bool, int, float) for v in sd["ema"].values())
    assert all(torch.equal(st["ema"], a.state[p]["ema"]) for st, p in zip(sd["state"].values(), _params(a)))
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    sd = torch.load(buf, weights_only=True)
    b_net = copy.deepcopy(a_net)
    b = _make(name, b_net, 3)
    b.set_ema(0.3)
    b.load_state_dict(sd)
    assert b.ema_config == {"decay": 0.8, "warmup": True} and float(b.ema_num_updates) == 3.0
    for s in range(3, 7):
        _set(a_net, s); _set(b_net, s)
        a.step(); b.step()
        assert float(a.ema_decay_now) == float(b.ema_decay_now)
        for x, y in zip(a.ema_parameters(), b.ema_parameters()):
            assert torch.equal(x, y), (name, s)
        for x, y in zip(a_net.parameters(), b_net.parameters()):
            assert torch.equal(x, y), (name, s)
    assert float(b.ema_num_updates) == 7.0


def test_state_without_ema_starts_a_fresh_average():
    a_net, b_net = _Net(3), _Net(3)
    a, b = _make("sgd", a_net, 3), _make("sgd", b_net, 3)
    b.set_ema(0.9)
    for s in range(2):
        _set(a_net, s); _set(b_net, s)
        a.step(); b.step()
    assert float(b.ema_num_updates) == 2.0
    b.load_state_dict(a.state_dict())  # no "ema" entry
    assert b.ema_config == {"decay": 0.9, "warmup": False} and float(b.ema_num_updates) == 0.0
    _set(b_net, 5); b.step()
    assert float(b.ema_decay_now) == 0.0 and float(b.ema_num_updates) == 1.0
    assert all(torch.equal(e, p) for e, p in zip(b.ema_parameters(), b_net.parameters()))  # n = 0 copies


def test_stock_adamw_loads_the_dict():
    net = _Net(4)
    opt = _make("adamw", net, 3)
    opt.set_ema(0.9)
    for s in range(2):
        _set(net, s); opt.step()
    sd = copy.deepcopy(opt.state_dict())
    twin = copy.deepcopy(net)
    stock = torch.optim.AdamW([{"params": [twin.w], "lr": 0.02}, {"params": [twin.b], "lr": 0.01}, {"params": [twin.k], "lr": 0.005}],
                              lr=0.01, weight_decay=1e-2)
    stock.load_state_dict(sd)
    _set(net, 9); _set(twin, 9)
    opt.step(); stock.step()
    for p, q in zip(net.parameters(), twin.parameters()):
        assert torch.equal(p, q)


def test_set_ema_off_drops_the_state():
    net = _Net(5)
    opt = _make("adam", net, 1)
    opt.set_ema(0.9)
    _set(net, 0); opt.step()
    opt.set_ema(None)
    assert opt.ema_config is None and opt.ema_decay_now is None and float(opt.ema_num_updates) == 0.0
    assert all("ema" not in st for st in opt.state.values()) and "ema" not in opt.state_dict()
    with pytest.raises(RuntimeError):
        opt.ema_parameters()
    _set(net, 1); opt.step()
    assert all("ema" not in st for st in opt.state.values())


def test_argument_errors():
    from distributed_pytorch_example_amd.optim import build_optimizer

    net = _Net(6)
    opt = _make("sgd", net, 1)
    for bad in (1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            opt.set_ema(bad)
    with pytest.raises(ValueError):
        opt.set_ema(None, warmup=True)
    with pytest.raises(RuntimeError):  # no EMA set
        opt.swap_ema()
    opt.set_ema(0.0)  # 0 is allowed: the average is the last weights
    with pytest.raises(RuntimeError):  # no update yet
        opt.swap_ema()
    with pytest.raises(RuntimeError):
        with opt.ema_weights():
            pass
    for bad in ({"warmup": True}, {"decay": 0.9, "steps": 3}):
        with pytest.raises(ValueError):
            build_optimizer("sgd", list(net.parameters()), lr=0.1, ema=bad)
    with pytest.raises(ValueError):
        build_optimizer("sgd", list(net.parameters()), lr=0.1, ema={"decay": 1.0})
    o = build_optimizer("lamb", list(net.parameters()), lr=0.1, ema={"decay": 0.99, "warmup": True})
    assert o.ema_config == {"decay": 0.99, "warmup": True}
    assert build_optimizer("sgd", list(net.parameters()), lr=0.1).ema_config is None


def test_ema_weights_swaps_and_restores():
    net = _Net(7)
    opt = _make("adamw", net, 3)
    opt.set_ema(0.5)
    for s in range(3):
        _set(net, s); opt.step()
    w = [p.detach().clone() for p in net.parameters()]
    e = [t.clone() for t in opt.ema_parameters()]
    assert not any(torch.equal(a, b) for a, b in zip(w, e))
    with opt.ema_weights() as o:
        assert o is opt
        assert all(torch.equal(p, b) for p, b in zip(net.parameters(), e))
        assert all(torch.equal(t, a) for t, a in zip(opt.ema_parameters(), w))
        with pytest.raises(RuntimeError):  # no step on the averaged weights
            opt.step()
    assert all(torch.equal(p, a) for p, a in zip(net.parameters(), w))
    assert all(torch.equal(t, b) for t, b in zip(opt.ema_parameters(), e))
    with pytest.raises(ZeroDivisionError):  # restored when the body raises, too
        with opt.ema_weights():
            1 / 0
    assert all(torch.equal(p, a) for p, a in zip(net.parameters(), w))
    opt.swap_ema(); opt.swap_ema()
    assert all(torch.equal(p, a) for p, a in zip(net.parameters(), w))


@pytest.mark.parametrize("flags", [["--ema-warmup"], ["--ema-decay", "1.0"], ["--ema-decay", "-0.5"]])
def test_train_rejects_ema_flags_before_it_starts(flags, capsys):
    from distributed_pytorch_example_amd.train import main

    with pytest.raises(SystemExit) as e:
        main(flags)
    assert e.value.code == 2
    assert "--ema-" in capsys.readouterr().err


def _train(ckdir, extra, epochs):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, PYTHONPATH=ROOT, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
               MASTER_PORT=str(port), OMP_NUM_THREADS="2", CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--backend", "gloo", "--model", "simplenet", "--epochs", str(epochs),
           "--max-steps", "5", "--num-samples", "640", "--seed", "3", "--checkpoint-dir", str(ckdir), *extra]
    return subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)


def _continue_from(src, dst, freeze=False):
    """The reference's resume runs the checkpoint's own epoch again; a copy whose epoch is one later continues after
    it, as an uninterrupted run does.  ``freeze``: lr 0 in the saved param groups (a resume takes them from the file)."""
    ck = torch.load(src, weights_only=True)
    ck["epoch"] += 1
    if freeze:
        for g in ck["optimizer_state_dict"]["param_groups"]:
            g["lr"] = 0.0
    torch.save(ck, dst)
    return ck


def test_train_cli_ema_and_resume(tmp_path):
    """train.py --ema-decay 0.9 --ema-warmup, 2 epochs x 5 steps: the EMA line after every epoch and the average in
    the checkpoint.  Then epochs 2 and 3 from that checkpoint in one run, and as two runs with a resume (without
    EMA flags, then with other ones) between them: the same EMA tensors, bit for bit.

    SimpleNet's initialisation and its dropout masks are not seeded, so no two training runs have the same weights.
    The continuation therefore starts from one file and runs at lr 0: the weights W stay the checkpoint's whatever
    the masks are, while the average keeps moving towards them, ema += (1 - d_n) (W - ema) with n = 10 .. 19 -- equal
    only if the resume restored the tensors and the counter and the warm-up went on where it was."""
    ema = ["--ema-decay", "0.9", "--ema-warmup"]
    r = _train(tmp_path / "a", ema, 2)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-3000:]
    lines = [ln for ln in log.splitlines() if "  EMA Val Loss: " in ln]
    assert len(lines) == 2, log[-3000:]
    for ln, n in zip(lines, (5, 10)):
        tail = ln.split("  EMA Val Loss: ")[1]
        loss, rest = tail.split(", EMA Val Accuracy: ")
        acc, d = rest.split("% (decay ")
        assert float(loss) > 0.0 and 0.0 <= float(acc) <= 100.0
        assert float(d.rstrip(")")) == pytest.approx(min(0.9, n / (9.0 + n)), rel=1e-5)  # d_(n-1): the epoch's last step
    assert log.index("  Val Loss: ") < log.index("  EMA Val Loss: ")
    start = tmp_path / "start.pt"
    ck = _continue_from(tmp_path / "a" / "latest_model.pt", start, freeze=True)
    sd = ck["optimizer_state_dict"]
    assert sd["ema"] == {"decay": 0.9, "warmup": True, "num_updates": 10}
    assert len(sd["state"]) == 6
    assert all(st["ema"].dtype == torch.float32 and st["ema"].shape == st["exp_avg"].shape for st in sd["state"].values())
    weights = list(ck["model_state_dict"].values())
    assert not any(torch.equal(st["ema"], w) for st, w in zip(sd["state"].values(), weights))

    def load(path):
        ck = torch.load(path, weights_only=True)
        sd = ck["optimizer_state_dict"]
        return sd["ema"], [st["ema"] for st in sd["state"].values()], list(ck["model_state_dict"].values())

    r = _train(tmp_path / "whole", ema + ["--resume", str(start)], 4)  # epochs 2 and 3
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    r = _train(tmp_path / "part1", ["--resume", str(start)], 3)  # epoch 2; no EMA flag: the checkpoint's EMA goes on
    log = r.stdout + r.stderr
    assert r.returncode == 0 and log.count("  EMA Val Loss: ") == 1, log[-3000:]
    _continue_from(tmp_path / "part1" / "latest_model.pt", tmp_path / "mid.pt")
    r = _train(tmp_path / "part2", ["--ema-decay", "0.5", "--resume", str(tmp_path / "mid.pt")], 4)  # epoch 3; not the flag's
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    cfg_w, ema_w, w_w = load(tmp_path / "whole" / "latest_model.pt")
    cfg_p, ema_p, w_p = load(tmp_path / "part2" / "latest_model.pt")
    assert cfg_w == cfg_p == {"decay": 0.9, "warmup": True, "num_updates": 20}
    for x, y, w in zip(w_w, w_p, weights):
        assert torch.equal(x, w) and torch.equal(y, w)  # lr 0
    for x, y, e0, w in zip(ema_w, ema_p, (st["ema"] for st in sd["state"].values()), weights):
        assert torch.equal(x, y)
        assert not torch.equal(x, e0) and not torch.equal(x, w)  # it moved, and is no copy of the weights
        # the 10 updates contract the gap by prod d_n, n = 10 .. 19 (about 2e-2)
        shrink = 1.0
        for n in range(10, 20):
            shrink *= min(0.9, (1.0 + n) / (10.0 + n))
        assert torch.allclose(x - w, (e0 - w) * shrink, rtol=1e-3, atol=1e-7)

    # no flag, no line, no state
    r = _train(tmp_path / "plain", [], 1)
    assert r.returncode == 0 and "EMA Val" not in r.stdout + r.stderr
    assert "ema" not in torch.load(tmp_path / "plain" / "latest_model.pt", weights_only=True)["optimizer_state_dict"]
