#!/usr/bin/env python3
"""Depthwise 7x7 kernels at the four ConvNeXt-T stage shapes [256, 56|28|14|7, same, 96|192|384|768], bf16:
forward, data gradient and weight gradient, against ``F.conv2d(groups=C)`` in channels-last bf16 (forward, and its
autograd backward, which yields both gradients in one call) and against each call's byte bound: the compulsory bytes
(every activation operand read once, the output written once: 4 B per element for all three calls) over the 5.9 TB/s
streaming rate measured by scripts/stream_probe.hip.

usage: bench_dwconv.py [--batch 256] [--window-s 0.2] [--warmup 20] [--rounds 5] [--limit 120] [--no-torch]

Device events around one window of calls, ``rounds`` windows per arm; the calls per window are sized from a pilot of
``warmup`` calls so that a window lasts about ``--window-s`` seconds (at least 3 calls); one JSON line is printed and
flushed after every arm.  Every arm runs under its own time limit: SIGALRM with its default action ends the process
if an arm does not return within ``--limit`` seconds.  The torch arms run last, so that a stall in the vendor library
cannot cost an arm of ours.
"""
import argparse
import json
import os
import signal
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STAGES = [(56, 96), (28, 192), (14, 384), (7, 768)]
STREAM_BYTES_PER_S = 5.9e12


def say(**kw):
    print(json.dumps(kw), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--window-s", type=float, default=0.2, help="seconds of calls per timed window")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=int, default=120, help="seconds one arm may take before the process is ended")
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dwconv.py needs a GPU: nothing is measured without one")
    from distributed_pytorch_example_amd.ops import functional as Fx
    from distributed_pytorch_example_amd.ops._ext import ext

    C_ = ext()
    dev = torch.device("cuda", 0)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(name, shape, fn, bound_us, ours_us=None):
        say(start=name, shape=shape, limit_s=a.limit)
        signal.alarm(a.limit)
        fn()
        ev[0].record()
        for _ in range(a.warmup):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        iters = max(3, int(a.window_s * 1e3 / (ev[0].elapsed_time(ev[1]) / a.warmup)))
        us = []
        for _ in range(a.rounds):
            ev[0].record()
            for _ in range(iters):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            us.append(ev[0].elapsed_time(ev[1]) * 1e3 / iters)
        signal.alarm(0)
        med = statistics.median(us)
        say(arm=name, shape=shape, calls_per_window=iters, us_min_med_max=[round(min(us), 1), round(med, 1), round(max(us), 1)],
            byte_bound_us=round(bound_us, 1), fraction_of_byte_bound=round(bound_us / med, 3),
            **({"ours_over_torch": round(ours_us / med, 3)} if ours_us is not None else {}))
        return med

    ours = {}
    cases = []
    for hw, ch in STAGES:
        torch.manual_seed(hw)
        shape = [a.batch, hw, hw, ch]
        x = torch.randn(shape, device=dev).to(torch.bfloat16)
        dy = torch.randn(shape, device=dev).to(torch.bfloat16)
        w = torch.randn(ch, 1, 7, 7, device=dev) * 0.1
        b = torch.randn(ch, device=dev)
        cases.append((shape, x, dy, w, b))
        w49, w49f = Fx._dw_taps(w), Fx._dw_taps_flipped(w)
        dw, db = torch.empty_like(w), torch.empty_like(b)
        bound = 4.0 * x.numel() / STREAM_BYTES_PER_S * 1e6
        ours[hw, "fwd"] = timed("dwconv7_fwd", shape, lambda: C_.dwconv7_fwd(x, w49, b), bound)
        ours[hw, "dgrad"] = timed("dwconv7_dgrad", shape, lambda: C_.dwconv7_dgrad(dy, w49f), bound)
        ours[hw, "wgrad"] = timed("dwconv7_wgrad", shape, lambda: C_.dwconv7_wgrad(dy, x, dw, db, False), bound)
    if a.no_torch:
        return
    for shape, x, dy, w, b in cases:
        hw, ch = shape[1], shape[3]
        xt = x.permute(0, 3, 1, 2).requires_grad_()  # NCHW view of NHWC storage = channels-last
        dyt = dy.permute(0, 3, 1, 2)
        wt, bt = w.to(torch.bfloat16).requires_grad_(), b.to(torch.bfloat16).requires_grad_()
        bound = 4.0 * x.numel() / STREAM_BYTES_PER_S * 1e6
        with torch.no_grad():
            timed("torch_conv2d_fwd", shape, lambda: F.conv2d(xt, wt, bt, padding=3, groups=ch), bound, ours[hw, "fwd"])
        y = F.conv2d(xt, wt, bt, padding=3, groups=ch)
        timed("torch_conv2d_bwd(dgrad+wgrad)", shape,
              lambda: torch.autograd.grad(y, (xt, wt, bt), dyt, retain_graph=True), 2 * bound,
              ours[hw, "dgrad"] + ours[hw, "wgrad"])


if __name__ == "__main__":
    main()
