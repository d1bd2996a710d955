"""Cost of label smoothing + z-loss in the fused cross-entropy (docs/perf_notes.md, "Label smoothing and z-loss").

The mean-CE kernel pair (``cross_entropy_mean``: per-row pass + fixed-order reduction), bf16 logits, gradient
written in place, at the GPT-2 LM-head shape (8192 x 50257, rows padded to 50304) and at the ResNet-50 shape
(512 x 1000).  Two arms alternate in one process after warm-up, each timed with device events over ``--iters``
calls per round:

  plain   label_smoothing = z_loss = 0           (the default instantiation)
  reg     label_smoothing = 0.1, z_loss = 1e-4   (the REG instantiation)

Both move the same bytes: one read and one write of the logits.

    python scripts/bench_ce_regularised.py [--iters 20] [--rounds 7]
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
    return s.elapsed_time(e) / iters * 1e3  # us per call


def bench(C, B, V, ld, iters, rounds):
    # in place: after the first call the buffer holds gradients, which are as good as logits for timing
    # (|values| < 1: no overflow, and the kernel's work does not depend on the values)
    z = (torch.randn(B, ld, device="cuda") * 3).to(torch.bfloat16)
    y = torch.randint(0, V, (B,), device="cuda")
    y[::17] = -100
    arms = {"plain": lambda: C.cross_entropy_mean(z, y, V, True, -100, True),
            "reg": lambda: C.cross_entropy_mean(z, y, V, True, -100, True, label_smoothing=0.1, z_loss=1e-4)}
    for fn in arms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    series = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            series[k].append(timed(fn, iters))
    med = {k: statistics.median(v) for k, v in series.items()}
    res = {"shape": [B, V, ld], "iters": iters, "rounds": rounds, "bytes": 2 * B * ld * 2,
           "us": {k: {"median": round(med[k], 2), "min": round(min(v), 2), "max": round(max(v), 2)} for k, v in series.items()},
           "TBps": {k: round(2 * B * ld * 2 / med[k] / 1e6, 3) for k in arms},
           "reg_over_plain": round(med["reg"] / med["plain"], 4)}
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ce_regularised.py measures on the GPU; none found")
    from distributed_pytorch_example_amd.ops import ext

    C = ext()
    bench(C, 8192, 50257, 50304, args.iters, args.rounds)
    bench(C, 512, 1000, 1000, args.iters * 10, args.rounds)


if __name__ == "__main__":
    main()
