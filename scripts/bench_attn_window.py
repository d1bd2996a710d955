#!/usr/bin/env python3
"""Sliding-window attention against the same call without a window, timed with HIP events in one process with the arms
alternating (every round visits every arm once; the plain arm is visited twice a round, as "plain" and "plain_again", so
the spread between two runs of the same code is measured beside the differences).

  training: (B, T, Hq, Hkv) = (4, 4096, 32, 4), forward and backward (dQ + dK/dV, one attn_bwd call) for W in
            {256, 1024, 4096 = off: dispatched to the plain instantiations}
  decode:   attn_decode_gqa at Tmax 4096, len 3991 .. 4000, W in {512, 0}

usage: bench_attn_window.py [--reps 100] [--rounds 5]
Prints one JSON line per arm and round as it is measured, then one summary line per arm (the minimum and the median over
the rounds, us per call)."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--B", type=int, default=4)
    ap.add_argument("--T", type=int, default=4096)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_attn_window.py measures on the GPU; there is none")
    from distributed_pytorch_example_amd.ops import ext

    C = ext()
    B, T, Hq, Hkv, D = a.B, a.T, 32, 4, 64
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    qkv = torch.randn(B, T, Hq + 2 * Hkv, D, device=dev).to(torch.bfloat16)
    do = torch.randn(B, T, Hq, D, device=dev).to(torch.bfloat16)
    scale = 1.0 / math.sqrt(D)
    arms = [("plain", None), ("W256", 256), ("W1024", 1024), (f"W{T}", T), ("plain_again", None)]
    res = {}

    def record(name, what, us):
        res.setdefault((name, what), []).append(us)
        print(json.dumps({"arm": name, "pass": what, "us": round(us, 2)}), flush=True)

    state = {}
    for name, W in arms:  # warm-up of every arm, and the forward results its backward reads
        kw = dict(n_kv_head=Hkv, **({} if W is None else {"window": W}))
        out, lse = C.attn_fwd(qkv, Hq, scale, True, **kw)
        C.attn_bwd(qkv, out, do, lse, Hq, scale, True, **kw)
        state[name] = (kw, out, lse)
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for name, _ in arms:
            kw, out, lse = state[name]
            record(name, "fwd", timed(lambda: C.attn_fwd(qkv, Hq, scale, True, out=out, lse=lse, **kw), a.reps))
            record(name, "bwd", timed(lambda: C.attn_bwd(qkv, out, do, lse, Hq, scale, True, **kw), a.reps))

    # decode: one step of 4 rows near the end of a 4096-row cache
    Tmax = 4096
    step = torch.randn(B, Hq + 2 * Hkv, D, device=dev).to(torch.bfloat16)
    kc, vc = (torch.randn(B, Hkv, Tmax, D, device=dev).to(torch.bfloat16) for _ in range(2))
    lens = torch.tensor([4000 - 3 * b for b in range(B)], dtype=torch.int32, device=dev)
    ang = torch.arange(Tmax, device=dev, dtype=torch.float32)[:, None] * torch.logspace(0, -4, 32, base=10.0, device=dev)[None]
    cos, sin = ang.cos().contiguous(), ang.sin().contiguous()
    darms = [("decode_plain", 0), ("decode_W512", 512), ("decode_plain_again", 0)]
    for name, W in darms:
        C.attn_decode_gqa(step, kc, vc, lens, cos, sin, Hkv, scale, window=W)
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for name, W in darms:
            record(name, "decode", timed(lambda: C.attn_decode_gqa(step, kc, vc, lens, cos, sin, Hkv, scale, window=W), 10 * a.reps))

    for (name, what), v in res.items():
        print(json.dumps({"arm": name, "pass": what, "min_us": round(min(v), 2), "median_us": round(statistics.median(v), 2),
                          "max_us": round(max(v), 2), "rounds": len(v)}), flush=True)


if __name__ == "__main__":
    main()
