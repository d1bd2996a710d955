#!/usr/bin/env python3
"""The Llama kernels (csrc/kernels/llama.hip) at TinyLlama-1.1B's shapes -- M = batch * 2048 tokens, D = 2048, F = 5632,
32 query / 4 KV heads of 64 -- each against the eager torch composition it replaces, and one tinyllama-1.1b training
step (forward, backward, AdamW) in tok/s.

usage: bench_llama.py [--batch 4] [--window-s 0.2] [--warmup 10] [--rounds 5] [--limit 120] [--no-step]

Device events around windows of calls after a warm-up; the two arms of a pair alternate window by window in the same
process, ``rounds`` windows each, and the median is reported.  A kernel's rate is its compulsory bytes (every operand
read once, every result written once, computed from the shapes below) over its time, next to the 5.9 TB/s streaming
rate of scripts/stream_probe.hip.  One JSON line per pair; SIGALRM ends the process if a pair takes over ``--limit`` s.
No rate is a pass / fail threshold.
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

STREAM_BYTES_PER_S = 5.9e12
T, D, FF, HQ, HKV = 2048, 2048, 5632, 32, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--window-s", type=float, default=0.2, help="seconds of calls per timed window")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=int, default=120, help="seconds one pair may take before the process is ended")
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_llama.py needs a GPU: nothing is measured without one")
    from distributed_pytorch_example_amd.models import get_model
    from distributed_pytorch_example_amd.ops import functional as Fx
    from distributed_pytorch_example_amd.ops._ext import ext
    from distributed_pytorch_example_amd.optim import build_optimizer

    C = ext()
    dev = torch.device("cuda", 0)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    B, M, W, NR = a.batch, a.batch * T, HQ + 2 * HKV, HQ + HKV
    bf = torch.bfloat16

    def window(fn, iters):
        ev[0].record()
        for _ in range(iters):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) * 1e3 / iters

    def pair(name, nbytes, ours, eager):
        signal.alarm(a.limit)
        ours(), eager()  # (first launches load code objects)
        it = [max(3, int(a.window_s * 1e6 / window(f, a.warmup))) for f in (ours, eager)]
        us = ([], [])
        for _ in range(a.rounds):
            for k, f in enumerate((ours, eager)):
                us[k].append(window(f, it[k]))
        signal.alarm(0)
        mo, me = statistics.median(us[0]), statistics.median(us[1])
        print(json.dumps({"kernel": name, "tokens": M, "compulsory_MB": round(nbytes / 1e6, 1),
                          "ours_us_min_med_max": [round(min(us[0]), 1), round(mo, 1), round(max(us[0]), 1)],
                          "eager_us_min_med_max": [round(min(us[1]), 1), round(me, 1), round(max(us[1]), 1)],
                          "ours_TB_per_s": round(nbytes / mo / 1e6, 2), "stream_probe_TB_per_s": STREAM_BYTES_PER_S / 1e12,
                          "eager_over_ours": round(me / mo, 2)}), flush=True)

    torch.manual_seed(0)
    # ---- RoPE: in place on the 36 rotated heads (read + write), backward out of place over all 40 (read + write)
    qkv = torch.randn(B, T, W, 64, device=dev).to(bf)
    cos, sin = Fx.rope_table(T, device=dev)
    c4 = torch.cat([cos, cos], -1).to(bf)[None, :, None, :]
    s4 = torch.cat([sin, sin], -1).to(bf)[None, :, None, :]

    def rope_eager():  # HF: q * cos + rotate_half(q) * sin on q and k, then the packed row again
        x = qkv[:, :, :NR]
        r = x * c4 + torch.cat([-x[..., 32:], x[..., :32]], -1) * s4
        return torch.cat([r, qkv[:, :, NR:]], 2)

    pair("rope_fwd_inplace", 2 * M * NR * 128, lambda: C.rope(qkv, cos, sin, None, NR, False, qkv), rope_eager)
    pair("rope_bwd", 2 * M * W * 128, lambda: C.rope(qkv, cos, sin, None, NR, True), rope_eager)
    # ---- RMSNorm: fp32 residual stream in, bf16 out; backward reads dy (bf16) and x, writes fp32 dx
    x = torch.randn(M, D, device=dev)
    w = torch.rand(D, device=dev) + 0.5
    dy = torch.randn(M, D, device=dev).to(bf)
    dw = torch.zeros(D, device=dev)
    _, rstd = C.rmsnorm_fwd(x, w, 1e-5)

    def rms_eager(xx=x):
        return (xx * torch.rsqrt(xx.pow(2).mean(-1, keepdim=True) + 1e-5) * w).to(bf)

    xg = x.clone().requires_grad_(True)
    yg = rms_eager(xg)
    pair("rmsnorm_fwd", M * D * 6, lambda: C.rmsnorm_fwd(x, w, 1e-5), rms_eager)
    pair("rmsnorm_bwd", M * D * 10, lambda: C.rmsnorm_bwd(dy, x, w, rstd, dw),
         lambda: torch.autograd.grad(yg, xg, dy, retain_graph=True))
    del xg, yg
    # ---- SwiGLU: gu [M, 2F] -> u [M, F]; backward reads du and gu, writes dgu
    gu = torch.randn(M, 2 * FF, device=dev).to(bf)
    du = torch.randn(M, FF, device=dev).to(bf)

    def swiglu_eager(g=gu):
        return F.silu(g[:, :FF]) * g[:, FF:]

    gg = gu.clone().requires_grad_(True)
    ug = swiglu_eager(gg)
    pair("swiglu_fwd", M * FF * 6, lambda: C.swiglu_fwd(gu), swiglu_eager)
    pair("swiglu_bwd", M * FF * 10, lambda: C.swiglu_bwd(du, gu), lambda: torch.autograd.grad(ug, gg, du, retain_graph=True))
    del gg, ug, gu, du, x, dy, qkv
    if a.no_step:
        return
    # ---- one training step of tinyllama-1.1b
    signal.alarm(4 * a.limit)
    model = get_model("tinyllama-1.1b").to(dev)
    opt = build_optimizer("adamw", model.parameters(), lr=1e-4, weight_decay=0.1)
    idx = torch.randint(0, 32000, (B, T), device=dev)
    tgt = torch.randint(0, 32000, (B, T), device=dev)

    def step():
        loss = model(idx, tgt)
        loss.backward()
        opt.step()
        opt.zero_grad()
        return loss

    ms = [window(step, 2) / 1e3 for _ in range(2 + a.rounds)][2:]  # (the first two windows are the warm-up)
    loss = step()
    signal.alarm(0)
    med = statistics.median(ms)
    print(json.dumps({"model": "tinyllama-1.1b", "batch": B, "seq_len": T, "params": model.num_params(),
                      "step_ms_min_med_max": [round(min(ms), 1), round(med, 1), round(max(ms), 1)],
                      "tok_per_s": round(M / med * 1e3), "loss": round(loss.item(), 4)}), flush=True)


if __name__ == "__main__":
    main()
