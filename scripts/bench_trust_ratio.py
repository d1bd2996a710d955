"""Cost of the layer-wise trust ratios of optim.LARS / optim.LAMB (docs/perf_notes.md, "LARS and LAMB").

Real parameter lists (ResNet-50 with LARS against fused SGD-momentum, GPT-2-small with LAMB against fused
AdamW), gradients as views of one flat fp32 buffer (the DDP bucket layout).  Three arms alternate in one process
after warm-up, each timed with device events over ``--iters`` steps per round:

  trust    fused LARS (partials + ratio + update: 3 launches) / LAMB (phase 1 + ratio + phase 2: 3 launches)
  plain    fused SGD / AdamW                                   (1 launch)
  foreach  the same LARS / LAMB formula in torch._foreach ops

and every kernel of the trust step on its own, next to the plain update kernel measured in the same run, with
the bytes each must move (no bf16 shadows here: no forward has run).

    python scripts/bench_trust_ratio.py [--models resnet50,gpt2] [--iters 50] [--rounds 5]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / iters  # ms per call


def foreach_lars(params, grads, lr, mom, wd, tc, te):
    bufs = [torch.zeros_like(p) for p in params]

    @torch.no_grad()
    def step():
        wn = torch.stack(torch._foreach_norm(params))
        gn = torch.stack(torch._foreach_norm(grads))
        ratio = torch.where((wn > 0) & (gn > 0), tc * wn / (gn + wd * wn + te), torch.ones_like(wn))
        d = torch._foreach_add(grads, params, alpha=wd)
        torch._foreach_mul_(d, list(ratio.unbind()))
        torch._foreach_mul_(bufs, mom)
        torch._foreach_add_(bufs, d)
        torch._foreach_add_(params, bufs, alpha=-lr)

    return step


def foreach_lamb(params, grads, lr, b1, b2, eps, wd):
    m = [torch.zeros_like(p) for p in params]
    v = [torch.zeros_like(p) for p in params]
    t = [0]

    @torch.no_grad()
    def step():
        t[0] += 1
        bc1, bc2 = 1.0 - b1 ** t[0], 1.0 - b2 ** t[0]
        torch._foreach_lerp_(m, grads, 1.0 - b1)
        torch._foreach_mul_(v, b2)
        torch._foreach_addcmul_(v, grads, grads, value=1.0 - b2)
        den = torch._foreach_sqrt(v)
        torch._foreach_div_(den, bc2 ** 0.5)
        torch._foreach_add_(den, eps)
        u = torch._foreach_div(m, den)
        torch._foreach_div_(u, bc1)
        torch._foreach_add_(u, params, alpha=wd)
        wn = torch.stack(torch._foreach_norm(params))
        un = torch.stack(torch._foreach_norm(u))
        ratio = torch.where((wn > 0) & (un > 0), wn / un, torch.ones_like(wn))
        torch._foreach_mul_(u, list(ratio.unbind()))
        torch._foreach_add_(params, u, alpha=-lr)

    return step


def bench(model_name, iters, rounds):
    from distributed_pytorch_example_amd.models import get_model
    from distributed_pytorch_example_amd.ops import ext
    from distributed_pytorch_example_amd.optim import LAMB, LARS, SGD, AdamW

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = get_model(model_name).to(dev)
    params = [p for p in model.parameters() if p.requires_grad]
    n = sum(p.numel() for p in params)
    flat = torch.randn(n, device=dev) * 1e-2
    off = 0
    for p in params:
        p.grad = flat[off:off + p.numel()].view_as(p)
        off += p.numel()
    grads = [p.grad for p in params]
    lamb = model_name.startswith("gpt2")

    # the arms share the parameters but own their states: each arm is a complete step (tiny lr: no drift)
    if lamb:
        trust, plain = LAMB(params, lr=1e-6, weight_decay=1e-2), AdamW(params, lr=1e-6, weight_decay=1e-2)
        foreach = foreach_lamb(params, grads, 1e-6, 0.9, 0.999, 1e-6, 1e-2)
    else:
        trust, plain = LARS(params, lr=1e-4, momentum=0.9, weight_decay=1e-4), SGD(params, lr=1e-4, momentum=0.9,
                                                                                    weight_decay=1e-4)
        foreach = foreach_lars(params, grads, 1e-4, 0.9, 1e-4, 1e-3, 1e-8)
    arms = {"trust": trust.step, "plain": plain.step, "foreach": foreach}
    for fn in arms.values():  # warm-up: tables, states, code objects
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    series = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            series[k].append(timed(fn, iters))

    C = ext()
    kind = trust._trust
    d, ck = trust._tab
    first, pw, px = trust._trust_tab
    nck = ck.size(0)
    passes = {  # name: (call, bytes per element)
        "partials" if not lamb else "phase1": (lambda: C.optim_trust_partials(kind, d, ck, trust._hp, trust._steps, pw, px),
                                               24 if lamb else 8),
        "ratio": (lambda: C.optim_trust_ratio(kind, d, first, nck, pw, px, trust._hp, trust._trust_stats), 0),
        "update" if not lamb else "phase2": (lambda: C.optim_trust_step(kind, d, ck, trust._hp, trust._steps, trust._trust_stats),
                                             16 if lamb else 20),
        "plain_update": (lambda: C.optim_step(plain._kind, plain._tab[0], plain._tab[1], plain._hp, plain._steps),
                         28 if lamb else 20),
    }
    t_pass = {k: [] for k in passes}
    for _ in range(rounds):  # alternating, as the arms
        for k, (fn, _) in passes.items():
            t_pass[k].append(timed(fn, iters))
    torch.cuda.synchronize()
    med = {k: statistics.median(v) for k, v in series.items()}
    res = {
        "model": model_name, "optimizer": "lamb" if lamb else "lars", "params": n, "tensors": len(params),
        "chunks": int(nck), "iters": iters, "rounds": rounds,
        "step_ms": {k: {"median": round(med[k], 4), "min": round(min(v), 4), "max": round(max(v), 4)}
                    for k, v in series.items()},
        "trust_minus_plain_ms": round(med["trust"] - med["plain"], 4),
        "foreach_over_trust": round(med["foreach"] / med["trust"], 2),
        "passes": {k: {"ms": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4),
                       "bytes": passes[k][1] * n,
                       "GBps": round(passes[k][1] * n / statistics.median(v) / 1e6, 1)} for k, v in t_pass.items()},
        "ratio_min_median_max": [round(x, 5) for x in (trust.trust_stats[:, 2].min().item(),
                                                       trust.trust_stats[:, 2].median().item(),
                                                       trust.trust_stats[:, 2].max().item())],
    }
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="resnet50,gpt2")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_trust_ratio.py measures on the GPU; none found")
    for m in args.models.split(","):
        bench(m, args.iters, args.rounds)


if __name__ == "__main__":
    main()
