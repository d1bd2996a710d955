"""optim.Muon on the CPU (the same formulas in torch ops) against the fp64 reference tests/_muon_ref.py, and the
plumbing around it: build_optimizer's three-way split, hand-made groups, the state dict, clipping and schedules,
argument checks and train.py.

The Newton-Schulz bound.  ns_emulated is the chain of the definition with its bf16 roundings and exact products;
e_emu = |ns_emulated - ns_ref64|_F / |ns_ref64|_F is what those roundings cost.  An implementation differs from
the emulation only in the order its fp32 sums are taken (and in rounding u before or after the normalisation),
which moves it by a fraction of e_emu, so it is held to 2 e_emu of the fp64 chain:

    |dW - dW_ref64|_F <= 2 e_emu lr gamma |O_ref64|_F + 4 * 2^-24 |W|_F

per step, the last term being the fp32 rounding of W on both sides of the difference.

The momentum buffer is a running average of the gradients: a step rounds g - buf, its product with 1 - momentum and
the sum, each within 2^-24 of a value no larger than |g| + |buf| <= |g_t| + (1 - momentum) sum_s |g_s|, and earlier
errors only shrink, so after t steps |buf - buf_ref64| <= 4 * 2^-24 sum_s |g_s| element by element.
"""
import io
import math
import os
import socket
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
try:
    from _muon_ref import MuonRef, ns_blocks, ns_emulated, ns_ref64
finally:
    sys.path.pop(0)

MATS = [((72, 200), 1), ((384, 128), 3), ((128, 128), 1)]  # wide, tall blocks of a split parameter, square
SMALL = [(1,), (1025,), (33,)]
KW = dict(lr=0.02, momentum=0.9375, weight_decay=0.01)  # (1 - momentum is exact in fp32)
u32 = 2.0 ** -24


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    mats = [torch.nn.Parameter(torch.randn(s, generator=g) * 0.05) for s, _ in MATS]
    for p, (_, split) in zip(mats, MATS):
        if split > 1:
            p._dpe_muon_split = split
    small = [torch.nn.Parameter(torch.randn(s, generator=g)) for s in SMALL]
    return mats, small


def _grads(ps, seed):
    g = torch.Generator().manual_seed(1000 + seed)
    return [torch.randn(p.shape, generator=g) for p in ps]


def _set(ps, gs):
    for p, g in zip(ps, gs):
        p.grad = g.clone()


def _muon(mats, small, **kw):
    from distributed_pytorch_example_amd.optim import Muon

    return Muon([{"params": mats}, {"params": small, "use_muon": False, "weight_decay": 0.0}], **{**KW, **kw})


def test_cpu_matches_the_fp64_reference():
    from distributed_pytorch_example_amd.optim import AdamW

    mats, small = _params()
    twin = [torch.nn.Parameter(p.detach().clone()) for p in small]
    opt, adamw = _muon(mats, small), AdamW(twin, lr=KW["lr"], weight_decay=0.0)
    ref = MuonRef(mats, splits=[s for _, s in MATS], **KW)
    gsum = [torch.zeros(s, dtype=torch.float64) for s, _ in MATS]
    for step in range(3):
        gs = _grads(mats + small, step)
        _set(mats + small, gs)
        _set(twin, gs[len(mats):])
        before = [p.detach().double().clone() for p in mats]
        ref_before = [w.clone() for w in ref.w]
        opt.step()
        adamw.step()
        uo = ref.step(gs[:len(mats)])
        for i, p in enumerate(mats):
            buf = opt.state[p]["momentum_buffer"].double()
            gsum[i] += gs[i].double().abs()
            assert ((buf - ref.buf[i]).abs() <= 4 * u32 * gsum[i]).all(), ("buf", i, step)
            u, O = uo[i]
            split = MATS[i][1]
            e_emu = ((ns_blocks(ns_emulated, u, split) - O).norm() / O.norm()).item()
            gm = 0.2 * math.sqrt(max(p.shape[0] // split, p.shape[1]))
            bound = 2 * e_emu * KW["lr"] * gm * O.norm().item() + 4 * u32 * ref.w[i].norm().item()
            err = ((p.detach().double() - before[i]) - (ref.w[i] - ref_before[i])).norm().item()
            print(f"step {step} matrix {i}: e_emu {e_emu:.4f}  err / bound {err / bound:.3f}")
            assert err <= bound, (i, step, err, bound)
        for a, b in zip(small, twin):
            assert torch.equal(a, b)
            assert torch.equal(opt.state[a]["exp_avg_sq"], adamw.state[b]["exp_avg_sq"])


def test_newton_schulz_orthogonalises():
    from distributed_pytorch_example_amd.optim import newton_schulz

    torch.manual_seed(3)
    for shape in ((72, 200), (136, 40)):
        O = newton_schulz(torch.randn(shape))
        assert O.dtype == torch.bfloat16 and O.shape == shape
        sv = torch.linalg.svdvals(O.double())
        assert 0.5 <= sv.min() and sv.max() <= 1.3, (shape, sv.min(), sv.max())


def test_build_optimizer_splits_gpt2_tiny_three_ways():
    from distributed_pytorch_example_amd.models import get_model
    from distributed_pytorch_example_amd.optim import Muon, build_optimizer

    model = get_model("gpt2-tiny")
    names = {id(p): n for n, p in model.named_parameters()}
    opt = build_optimizer("muon", model.parameters(), lr=0.02, weight_decay=0.1)
    assert isinstance(opt, Muon) and len(opt.param_groups) == 3
    mu, wd, nowd = opt.param_groups
    assert mu["use_muon"] and not wd["use_muon"] and not nowd["use_muon"]
    assert mu["momentum"] == 0.95 and mu["ns_steps"] == 5 and mu["scale"] == "match_rms" and mu["nesterov"]
    assert mu["weight_decay"] == 0.1 and wd["weight_decay"] == 0.1 and nowd["weight_decay"] == 0.0
    n_layer = model.cfg.n_layer
    got = sorted(names[id(p)] for p in mu["params"])
    want = sorted(f"h.{i}.{m}.weight" for i in range(n_layer) for m in ("c_attn", "attn_proj", "c_fc", "mlp_proj"))
    assert got == want
    assert sorted(names[id(p)] for p in wd["params"]) == ["wpe", "wte"]
    assert all(p.ndim <= 1 for p in nowd["params"])
    assert len(mu["params"]) + 2 + len(nowd["params"]) == len(list(model.parameters()))
    for blk in model.h:
        assert blk.c_attn.weight._dpe_muon_split == 3
    assert build_optimizer("muon", model.parameters(), lr=0.02, momentum=0.9, ns_steps=3).param_groups[0]["ns_steps"] == 3
    # a matrix with a dimension that is no multiple of 8 (outside the MFMA envelope the issue fixes) goes to AdamW
    odd = [torch.nn.Parameter(torch.zeros(16, 12)), torch.nn.Parameter(torch.zeros(16, 24))]
    g = build_optimizer("muon", odd, lr=0.1).param_groups
    assert [(x["use_muon"], x["params"][0].shape[1]) for x in g] == [(True, 24), (False, 12)]


def test_other_models_keep_their_output_layers_on_adamw():
    from distributed_pytorch_example_amd.models import get_model
    from distributed_pytorch_example_amd.optim import build_optimizer

    for name, out in (("simplenet", "layers.6.weight"), ("resnet_tiny", "fc.weight")):
        model = get_model(name)
        names = {id(p): n for n, p in model.named_parameters()}
        groups = build_optimizer("muon", model.parameters(), lr=0.02).param_groups
        mu = [names[id(p)] for g in groups if g["use_muon"] for p in g["params"]]
        assert out not in mu and out in names.values()
        assert all(p.ndim == 2 for g in groups if g["use_muon"] for p in g["params"])  # conv filters stay on AdamW


def test_hand_made_groups_are_kept():
    from distributed_pytorch_example_amd.optim import build_optimizer

    mats, small = _params()
    groups = [{"params": mats[:1], "scale": "spectral", "ns_steps": 3}, {"params": mats[1:], "momentum": 0.9},
              {"params": small, "use_muon": False, "lr": 1e-3}]
    opt = build_optimizer("muon", groups, lr=0.02, weight_decay=0.1)
    g0, g1, g2 = opt.param_groups
    assert (g0["scale"], g0["ns_steps"], g0["use_muon"], g0["momentum"]) == ("spectral", 3, True, 0.95)
    assert (g1["scale"], g1["ns_steps"], g1["momentum"]) == ("match_rms", 5, 0.9)
    assert not g2["use_muon"] and g2["lr"] == 1e-3 and g2["weight_decay"] == 0.1
    assert [len(g["params"]) for g in opt.param_groups] == [1, 2, 3]


def test_spectral_scale_and_plain_momentum():
    mats, small = _params()
    kw = dict(scale="spectral", nesterov=False)
    opt = _muon(mats, small, **kw)
    ref = MuonRef(mats, splits=[s for _, s in MATS], ns=ns_emulated, **{**KW, **kw})
    gs = _grads(mats + small, 0)
    _set(mats + small, gs)
    before = [p.detach().double().clone() for p in mats]
    opt.step()
    uo = ref.step(gs[:len(mats)])
    for i, p in enumerate(mats):
        split = MATS[i][1]
        rows = p.shape[0] // split
        gm = math.sqrt(max(1.0, rows / p.shape[1]))
        O64 = ns_blocks(ns_ref64, uo[i][0], split)
        e_emu = ((uo[i][1] - O64).norm() / O64.norm()).item()
        want = before[i] * (1.0 - KW["lr"] * KW["weight_decay"]) - KW["lr"] * gm * O64
        bound = 2 * e_emu * KW["lr"] * gm * O64.norm().item() + 4 * u32 * want.norm().item()
        assert (p.detach().double() - want).norm().item() <= bound


def test_state_dict_round_trip_continues_bitwise():
    mats, small = _params()
    a = _muon(mats, small)
    a.set_lr_schedule("cosine", warmup_steps=1, total_steps=6)
    for step in range(2):
        _set(mats + small, _grads(mats + small, step))
        a.step()
    f = io.BytesIO()
    torch.save(a.state_dict(), f)
    f.seek(0)
    sd = torch.load(f, weights_only=True)
    assert set(sd["state"][0]) == {"step", "momentum_buffer"} and set(sd["state"][len(mats)]) == {"step", "exp_avg", "exp_avg_sq"}
    assert sd["param_groups"][0]["use_muon"] and sd["param_groups"][0]["scale"] == "match_rms"
    mats2 = [torch.nn.Parameter(p.detach().clone()) for p in mats]
    for p, (_, split) in zip(mats2, MATS):
        if split > 1:
            p._dpe_muon_split = split
    small2 = [torch.nn.Parameter(p.detach().clone()) for p in small]
    b = _muon(mats2, small2)
    b.load_state_dict(sd)
    for step in range(2, 4):
        gs = _grads(mats + small, step)
        _set(mats + small, gs)
        _set(mats2 + small2, gs)
        a.step()
        b.step()
    for p, q in zip(mats + small, mats2 + small2):
        assert torch.equal(p, q)
    assert torch.equal(a.state[mats[0]]["momentum_buffer"], b.state[mats2[0]]["momentum_buffer"])


def test_clipping_and_a_cosine_schedule_compose():
    """One global norm over both kinds of group, then the scheduled lr: equal to clipping by hand and setting the lr."""
    from distributed_pytorch_example_amd.optim import lr_factor

    mats, small = _params()
    mats2, small2 = _params()
    for p, q in zip(mats, mats2):
        if hasattr(p, "_dpe_muon_split"):
            q._dpe_muon_split = p._dpe_muon_split
    a, b = _muon(mats, small), _muon(mats2, small2)
    a.set_grad_clip(1.0)
    a.set_lr_schedule("cosine", warmup_steps=1, total_steps=4, min_ratio=0.1)
    for step in range(3):
        gs = _grads(mats + small, step)
        _set(mats + small, gs)
        _set(mats2 + small2, gs)
        norm = torch.nn.utils.clip_grad_norm_(mats2 + small2, 1.0)
        f = lr_factor(step, "cosine", 1, 4, 0.1)
        for g in b.param_groups:
            g["lr"] = KW["lr"] * f
        a.step()
        b.step()
        assert float(a.grad_norm) == pytest.approx(float(norm), rel=1e-6) and float(norm) > 1.0
        assert float(a.current_lr[0]) == pytest.approx(KW["lr"] * f, rel=1e-6)
    for p, q in zip(mats + small, mats2 + small2):
        assert torch.equal(p, q)
    assert a.param_groups[0]["lr"] == KW["lr"]  # the base lr stays


def test_argument_checks():
    from distributed_pytorch_example_amd import train
    from distributed_pytorch_example_amd.optim import Muon, build_optimizer

    mats, small = _params()
    for bad in (dict(momentum=1.0), dict(momentum=-0.1), dict(ns_steps=0), dict(ns_steps=2.5), dict(scale="rms"),
                dict(ns_coefficients=(1.0, 2.0)), dict(lr=-1.0), dict(weight_decay=-0.1)):
        with pytest.raises(ValueError):
            Muon(mats, **bad)
    with pytest.raises(ValueError):
        Muon(small)  # 1-D tensors in a Muon group
    with pytest.raises(ValueError):
        build_optimizer("adamw", small, lr=0.1, ns_steps=5)
    with pytest.raises(RuntimeError, match="Muon"):
        Muon(mats)._ov_attach(None)  # what DDP.overlap_optimizer calls
    assert Muon._whole_matrix
    p = train.build_parser()
    args = p.parse_args(["--optimizer", "muon", "--muon-momentum", "0.9", "--muon-ns-steps", "3"])
    assert (args.optimizer, args.muon_momentum, args.muon_ns_steps) == ("muon", 0.9, 3)
    assert p.parse_args([]).muon_momentum is None and p.parse_args([]).muon_ns_steps is None
    for bad in (["--optimizer", "adamw", "--muon-momentum", "0.9"], ["--muon-ns-steps", "3"],
                ["--optimizer", "muon", "--muon-momentum", "1.0"], ["--optimizer", "muon", "--muon-ns-steps", "0"]):
        with pytest.raises(SystemExit):
            train.main(bad)


def test_train_cli_muon(tmp_path):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, PYTHONPATH=ROOT, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
               MASTER_PORT=str(port), OMP_NUM_THREADS="2", CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--backend", "gloo", "--model", "gpt2-tiny", "--optimizer", "muon",
           "--epochs", "3", "--num-samples", "16", "--batch-size", "4", "--seq-len", "64", "--seed", "1", "--lr", "0.01",
           "--weight-decay", "0.01", "--checkpoint-dir", str(tmp_path / "ck")]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    log = r.stdout + r.stderr
    losses = [float(x.split()[0]) for x in log.split("Train Loss: ")[1:]]
    assert len(losses) == 3 and all(math.isfinite(v) for v in losses)
    assert losses[-1] < losses[0], losses
