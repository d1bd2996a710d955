#!/usr/bin/env python3
"""Bidirectional attention with a key-length bound against two yardsticks, forward and backward, at the ViT-B/16
batch-256 shapes (B, Tp, H, L) = (256, 256, 12, 197) and (256, 256, 12, 256), D = 64:

    bidir     attn_fwd / attn_bwd with causal=False, seq_len=L on the padded [B, Tp, 3, H, 64] tensor
    sdpa      F.scaled_dot_product_attention without a mask over the L real rows only ([B, H, L, 64] contiguous
              q, k, v made outside the timed window: no padding, no layout work), backward through autograd
    causal    this project's causal kernels at the same Tp (half the score tiles: a different function, shown as the
              neighbouring point of the same code)

usage: bench_attn_bidir.py [--reps 50] [--rounds 5] [--B 256 --H 12] [--limit 120]

Device events around ``reps`` calls per window, ``rounds`` windows per arm, the arms alternating inside one process;
one JSON line is printed and flushed after every window and a min / median / max line per arm at the end.  Every
window runs under its own time limit: SIGALRM with its default action ends the process if a window does not return
within ``--limit`` seconds, and the line printed before the window names it.  The useful work of an arm is the
4 B H L^2 D (forward) and 10 B H L^2 D (backward) flops of the L x L problem, whatever the arm computes.
"""
import argparse
import json
import math
import os
import signal
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def say(**kw):
    print(json.dumps(kw), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--H", type=int, default=12)
    ap.add_argument("--limit", type=int, default=120, help="seconds one window may take before the process is ended")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attn_bidir.py needs a GPU: nothing is measured without one")
    from distributed_pytorch_example_amd.ops import ext

    C = ext()
    B, H, D, Tp = a.B, a.H, 64, 256
    dev = torch.device("cuda", 0)
    scale = 1.0 / math.sqrt(D)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]

    def window(fwd, bwd):
        ev[0].record()
        for _ in range(a.reps):
            fwd()
        ev[1].record()
        for _ in range(a.reps):
            bwd()
        ev[2].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) * 1e3 / a.reps, ev[1].elapsed_time(ev[2]) * 1e3 / a.reps

    for L in (197, 256):
        torch.manual_seed(L)
        qkv = torch.randn(B, Tp, 3, H, D, device=dev).to(torch.bfloat16)
        do = torch.randn(B, Tp, H, D, device=dev).to(torch.bfloat16)
        arms = {}

        out, lse = C.attn_fwd(qkv, H, scale, False, seq_len=L)
        arms["bidir"] = (lambda: C.attn_fwd(qkv, H, scale, False, seq_len=L),
                         lambda o=out, l=lse: C.attn_bwd(qkv, o, do, l, H, scale, False, seq_len=L))
        outc, lsec = C.attn_fwd(qkv, H, scale, True)
        arms["causal"] = (lambda: C.attn_fwd(qkv, H, scale, True),
                          lambda o=outc, l=lsec: C.attn_bwd(qkv, o, do, l, H, scale, True))
        q, k, v = (qkv[:, :L, i].transpose(1, 2).contiguous().requires_grad_(True) for i in range(3))
        dos = do[:, :L].transpose(1, 2).contiguous()
        so = F.scaled_dot_product_attention(q, k, v)
        # the same function: sdpa over the real rows against the kernel's rows < L
        err = (so.detach().transpose(1, 2).float() - out[:, :L].float()).abs().max().item()

        def sdpa_bwd(so=so):
            q.grad = k.grad = v.grad = None
            so.backward(dos, retain_graph=True)

        arms["sdpa"] = (lambda: F.scaled_dot_product_attention(q, k, v), sdpa_bwd)
        res = {n: {"fwd": [], "bwd": []} for n in arms}
        for rnd in range(a.rounds + 1):  # round 0 warms every arm up and is not kept
            for n, (fw, bw) in arms.items():
                say(start=n, L=L, round=rnd, limit_s=a.limit)
                signal.alarm(a.limit)
                f_us, b_us = window(fw, bw)
                signal.alarm(0)
                say(arm=n, L=L, round=rnd, fwd_us=round(f_us, 2), bwd_us=round(b_us, 2), kept=rnd > 0)
                if rnd > 0:
                    res[n]["fwd"].append(f_us)
                    res[n]["bwd"].append(b_us)

        def mmm(x):
            return [round(min(x), 2), round(statistics.median(x), 2), round(max(x), 2)]

        flop = B * H * L * L * D
        for n, r in res.items():
            fm, bm = statistics.median(r["fwd"]), statistics.median(r["bwd"])
            say(summary=n, shape=[B, Tp, H, L], fwd_us_min_med_max=mmm(r["fwd"]), bwd_us_min_med_max=mmm(r["bwd"]),
                fwd_tflops_of_LxL=round(4 * flop / fm * 1e-6, 1), bwd_tflops_of_LxL=round(10 * flop / bm * 1e-6, 1),
                **({"sdpa_vs_bidir_max_abs_diff": round(err, 5)} if n == "sdpa" else {}))


if __name__ == "__main__":
    main()
