#!/usr/bin/env python
"""GPT-2 decoding: ms per token of four arms at B in {1, 8, 16} and context 128 / 512 / 1000,

  a  re-running GPT2.forward on the whole prefix for every token (all a user could do before the KV cache)
  b  KV cache + the training GEMMs (Fx.linear / Fx.linear_residual) on the single-token rows
  c  KV cache + Fx.linear_skinny
  d  arm c with the decode step replayed from a captured HIP graph

then (arm k) the kernels of one arm-c step timed in place with events between the ops, and (arm s) every projection
shape of the step on linear_skinny against Fx.linear at M = 1, 8, 16 -- the table behind Fx.SKINNY_SLOWER.  For arm c
the weight bytes a step must read (every block matrix and the padded LM head in bf16, once) over the step time are
set against 6.29 TB/s, the measured HBM streaming rate of the MI355X.

Every arm runs in a child process under its own time limit, and every result is one JSON line printed and flushed
as soon as it exists: a hang is attributable to the arm and shape that printed last.

    python scripts/bench_decode.py [--model gpt2] [--arms a,b,c,d,k,s] [--steps 20] [--timeout 240]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BATCHES = (1, 8, 16)
CONTEXTS = (128, 512, 1000)
HBM_STREAM = 6.29e12  # bytes / s, float4 copy


def emit(**kw):
    print(json.dumps(kw), flush=True)


def step_weight_bytes(model):
    """bf16 bytes of every matrix one decode step reads once: the blocks' four projections and the padded LM head."""
    cfg = model.cfg
    d, vp = cfg.n_embd, (cfg.vocab_size + 63) // 64 * 64
    return 2 * (cfg.n_layer * 12 * d * d + vp * d)


def child(args):
    import torch

    from distributed_pytorch_example_amd.models import get_model
    from distributed_pytorch_example_amd.models.gpt2 import KVCache
    from distributed_pytorch_example_amd.ops import ext, functional as Fx

    if not torch.cuda.is_available():
        raise SystemExit("bench_decode.py measures on the GPU; there is none here")
    ext()
    dev = torch.device("cuda")
    torch.manual_seed(0)
    model = get_model(args.model).to(dev).eval()
    cfg = model.cfg
    V = cfg.vocab_size
    contexts = [c for c in CONTEXTS if c + args.steps + 4 <= cfg.block_size]

    def sync_time(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    with torch.no_grad():
        if args.arm == "a":
            for B in BATCHES:
                for ctx in contexts:
                    idx = torch.randint(0, V, (B, ctx), device=dev)
                    fn = lambda: model(idx)[:, -1, :V].argmax(-1)
                    sync_time(fn, 2)
                    emit(arm="a", B=B, context=ctx, ms_per_token=round(sync_time(fn, 5), 4))
        elif args.arm in ("b", "c", "d"):
            model.decode_skinny = args.arm != "b"
            state = Fx.DropoutState(dev).manual_seed(1)
            for B in BATCHES:
                for ctx in contexts:
                    cache = KVCache(model, B, cfg.block_size)
                    cache.buf.normal_()
                    tok = torch.randint(0, V, (B,), device=dev)

                    def step():
                        logits = model._decode_step(tok, cache)
                        cache.len.add_(1)
                        tok.copy_(Fx.sample_logits(logits, V, 0.9, 50, 0.95, state))

                    def run(n, fn):
                        cache.len.fill_(ctx)
                        return sync_time(fn, n)

                    run(3, step)
                    if args.arm == "d":
                        g = torch.cuda.CUDAGraph()
                        cache.len.fill_(ctx)
                        with torch.cuda.graph(g):
                            step()
                        run(3, g.replay)
                        ms = run(args.steps, g.replay)
                    else:
                        ms = run(args.steps, step)
                    row = dict(arm=args.arm, B=B, context=ctx, ms_per_token=round(ms, 4))
                    if args.arm == "c":
                        wb = step_weight_bytes(model)
                        row.update(weight_mb=round(wb / 1e6, 1), weight_tb_s=round(wb / (ms * 1e-3) / 1e12, 3),
                                   share_of_stream=round(wb / (ms * 1e-3) / HBM_STREAM, 3))
                    emit(**row)
        elif args.arm == "k":
            # one arm-c step with an event after every op: per-kind totals over the layers, mean of `steps` steps
            B, ctx = 8, contexts[-1]
            cache = KVCache(model, B, cfg.block_size)
            cache.buf.normal_()
            tok = torch.randint(0, V, (B,), device=dev)
            state = Fx.DropoutState(dev).manual_seed(1)
            H = cfg.n_head
            tot = {}

            def timed_step(marks):
                def mark(name):
                    e = torch.cuda.Event(enable_timing=True)
                    e.record()
                    marks.append((name, e))

                mark("start")
                x = Fx.embedding(tok.view(B, 1), model.wte, model.wpe, cache.len.view(B, 1)).view(B, -1)
                mark("embedding")
                for l, blk in enumerate(model.h):
                    h = blk.ln_1(x); mark("layernorm")
                    qkv = model._proj(h, blk.c_attn); mark("c_attn")
                    a = Fx.attn_decode(qkv, cache.buf[l, 0], cache.buf[l, 1], cache.len, H); mark("attn_decode")
                    x = model._proj(a, blk.attn_proj, residual=x); mark("attn_proj")
                    h = blk.ln_2(x); mark("layernorm")
                    u = model._proj(h, blk.c_fc, Fx.ACT_GELU); mark("c_fc")
                    x = model._proj(u, blk.mlp_proj, residual=x); mark("mlp_proj")
                h = model.ln_f(x); mark("layernorm")
                logits = model._head(h); mark("lm_head")
                Fx.sample_logits(logits, V, 0.9, 50, 0.95, state); mark("sample_logits")

            for it in range(3 + args.steps):
                cache.len.fill_(ctx)
                marks = []
                timed_step(marks)
                torch.cuda.synchronize()
                if it >= 3:
                    for (_, e0), (name, e1) in zip(marks[:-1], marks[1:]):
                        tot[name] = tot.get(name, 0.0) + e0.elapsed_time(e1)
            emit(arm="k", B=B, context=ctx, note="event-to-event ms per step (launch gaps included), summed over layers",
                 **{k: round(v / args.steps, 4) for k, v in tot.items()}, total=round(sum(tot.values()) / args.steps, 4))
        elif args.arm == "s":
            # every projection shape on linear_skinny (the default plan and without the K split over blocks) and on
            # Fx.linear.  Each arm is one captured graph of 4 rounds over `copies` different weights (no host launch
            # cost in the figure, and no arm finds its weight in the L2 from the call before); the graphs alternate.
            d = cfg.n_embd
            vp = (V + 63) // 64 * 64
            shapes = [("c_attn", 3 * d, d, 12), ("attn_proj", d, d, 12), ("c_fc", 4 * d, d, 12), ("mlp_proj", d, 4 * d, 12),
                      ("lm_head", vp, d, 2)]
            for name, N, K, copies in shapes:
                ws = [torch.nn.Parameter(torch.randn(N, K, device=dev) * 0.02) for _ in range(copies)]
                bias = torch.zeros(N, device=dev)
                for M in (1, 8, 16):
                    x = torch.randn(M, K, device=dev).to(torch.bfloat16)
                    calls = {"skinny": lambda w: Fx.linear_skinny(x, w, bias),
                             "skinny_k1": lambda w: Fx.linear_skinny(x, w, bias, ksplit=1),
                             "linear": lambda w: Fx.linear(x, w, bias)}
                    graphs = {}
                    for arm, fn in calls.items():
                        for w in ws:
                            fn(w)  # warm-up: shadows, code objects
                        torch.cuda.synchronize()
                        g = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(g):
                            for _ in range(4):
                                for w in ws:
                                    fn(w)
                        graphs[arm] = g
                    res = {arm: [] for arm in calls}
                    for rnd in range(4):
                        for arm, g in graphs.items():
                            res[arm].append(sync_time(g.replay, 10) / (4 * copies) * 1e3)
                    us = {arm: round(min(v[1:]), 2) for arm, v in res.items()}
                    best = min(us, key=us.get)
                    emit(arm="s", shape=name, N=N, K=K, M=M, **{k + "_us": v for k, v in us.items()},
                         default_splits=ext().linear_skinny_splits(M, N, K), fastest=best,
                         skinny_tb_s=round(2 * N * K / (us["skinny"] * 1e-6) / 1e12, 3))
        else:
            raise SystemExit(f"unknown arm {args.arm!r}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", default="gpt2", choices=["gpt2", "gpt2-tiny"])
    ap.add_argument("--arms", default="a,b,c,d,k,s")
    ap.add_argument("--steps", type=int, default=20, help="timed decode steps per shape")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per arm (child process)")
    ap.add_argument("--arm", default=None, help=argparse.SUPPRESS)  # child mode
    args = ap.parse_args()
    if args.arm is not None:
        return child(args)
    for arm in args.arms.split(","):
        emit(event="arm_start", arm=arm)
        cmd = [sys.executable, os.path.abspath(__file__), "--model", args.model, "--steps", str(args.steps), "--arm", arm]
        try:
            rc = subprocess.run(cmd, timeout=args.timeout).returncode
        except subprocess.TimeoutExpired:
            emit(event="arm_timeout", arm=arm, seconds=args.timeout)
            return 124  # nothing more is started on a device that may be hung
        emit(event="arm_end", arm=arm, rc=rc)
        if rc != 0:
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
