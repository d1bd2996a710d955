#!/usr/bin/env python3
"""Packed-document attention against the causal kernels at the GPT-2-small training shape (B=8, T=1024, H=12,
D=64), four arms and a diagnostic one, alternated inside one process:

    causal      today's causal kernels (the yardstick: unchanged code)
    packed0     the packed kernels with doc_start = 0 (the same mask, two extra loads per lane)
    packed128   the packed kernels, 128-token documents
    packedgeo   the packed kernels, seeded geometric document lengths of mean 256
    packed96    (diagnostic) 96-token documents: as short as packed128's, but every document start lies inside a
                64-key tile, so each wave's first tile takes the path with both masks

usage: bench_attn_packed.py [--reps 200] [--rounds 7] [--B 8 --T 1024 --H 12] [--no-kernels]

Forward and backward (dQ + dK/dV, two kernels behind one call) are timed with device events over ``reps`` calls
per window, ``rounds`` windows per arm, arms alternating; min / median / max over the windows are printed, so
the causal arm's own spread stands beside every difference.  The dQ / dK-dV split comes from a separate pass
under torch.profiler (kernel durations by name, profiler off during the event timing).  Outputs of packed0 are
compared with the causal arm's first.  One JSON line per arm.
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def geometric_doc_start(B, T, mean, seed):
    g = torch.Generator().manual_seed(seed)
    first = torch.rand(B, T, generator=g) < 1.0 / mean
    first[:, 0] = True
    t = torch.arange(T).expand(B, -1)
    return torch.cummax(torch.where(first, t, torch.zeros_like(t)), dim=1).values.to(torch.int32)


def visible_pairs(ds):
    """Number of (query, key) pairs the mask keeps: sum over tokens of t - doc_start + 1."""
    t = torch.arange(ds.shape[1]).expand_as(ds)
    return int((t - ds.long() + 1).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--T", type=int, default=1024)
    ap.add_argument("--H", type=int, default=12)
    ap.add_argument("--no-kernels", action="store_true", help="skip the torch.profiler pass (dQ / dK-dV split)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attn_packed.py needs a GPU: nothing is measured without one")
    from distributed_pytorch_example_amd.ops import ext
    from distributed_pytorch_example_amd.ops import functional as Fx

    C = ext()
    B, T, H, D = a.B, a.T, a.H, 64
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    qkv = torch.randn(B, T, 3, H, D, device=dev).to(torch.bfloat16)
    do = torch.randn(B, T, H, D, device=dev).to(torch.bfloat16)
    scale = 1.0 / math.sqrt(D)
    t = torch.arange(T, dtype=torch.int32)
    layouts = {"causal": None, "packed0": torch.zeros(B, T, dtype=torch.int32),
               "packed128": ((t // 128) * 128).expand(B, -1).contiguous(),
               "packedgeo": geometric_doc_start(B, T, 256, seed=0),
               "packed96": ((t // 96) * 96).expand(B, -1).contiguous()}
    arms = {}
    for n, ds in layouts.items():
        kw = {}
        if ds is not None:
            s, e, _ = Fx.doc_bounds(ds.to(dev))
            kw = {"doc_start": s, "doc_end": e}
        pairs = visible_pairs(ds if ds is not None else torch.zeros(B, T, dtype=torch.int32))
        arms[n] = {"kw": kw, "pairs": pairs, "fwd": [], "bwd": []}
    outs = {}
    for n, arm in arms.items():  # warm-up of every arm, outputs kept for the backward and the check
        out, lse = C.attn_fwd(qkv, H, scale, True, **arm["kw"])
        dq = C.attn_bwd(qkv, out, do, lse, H, scale, True, **arm["kw"])
        outs[n] = (out, lse, dq)
    torch.cuda.synchronize()
    same = all(torch.equal(x.view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32),
                           y.view(torch.int16 if y.dtype == torch.bfloat16 else torch.int32))
               for x, y in zip(outs["causal"], outs["packed0"]))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    for _ in range(a.rounds):
        for n, arm in arms.items():
            out, lse, _ = outs[n]
            ev[0].record()
            for _ in range(a.reps):
                C.attn_fwd(qkv, H, scale, True, **arm["kw"])
            ev[1].record()
            for _ in range(a.reps):
                C.attn_bwd(qkv, out, do, lse, H, scale, True, **arm["kw"])
            ev[2].record()
            torch.cuda.synchronize()
            arm["fwd"].append(ev[0].elapsed_time(ev[1]) * 1e3 / a.reps)
            arm["bwd"].append(ev[1].elapsed_time(ev[2]) * 1e3 / a.reps)
    split = {n: None for n in arms}
    if not a.no_kernels:
        from torch.profiler import ProfilerActivity, profile

        for n, arm in arms.items():
            out, lse, _ = outs[n]
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                for _ in range(20):
                    C.attn_bwd(qkv, out, do, lse, H, scale, True, **arm["kw"])
                torch.cuda.synchronize()
            k = {}
            for e in prof.events():
                for key in ("attn_bwd_dq_dma_kernel", "attn_bwd_dma_kernel"):
                    if key in e.name:
                        k.setdefault(key, []).append(e.device_time if hasattr(e, "device_time") else e.cuda_time)
            if len(k) == 2:
                split[n] = {"dq_us": round(statistics.median(k["attn_bwd_dq_dma_kernel"]), 2),
                            "dkdv_us": round(statistics.median(k["attn_bwd_dma_kernel"]), 2)}

    def mmm(v):
        return [round(min(v), 2), round(statistics.median(v), 2), round(max(v), 2)]

    for n, arm in arms.items():
        print(json.dumps({"arm": n, "shape": [B, T, H, D], "visible_pairs_share": round(arm["pairs"] / (B * T * (T + 1) / 2), 4),
                          "fwd_us_min_med_max": mmm(arm["fwd"]), "bwd_us_min_med_max": mmm(arm["bwd"]),
                          "bwd_split_us": split[n] if split[n] is not None else "not measured",
                          **({"bit_equal_to_causal": same} if n == "packed0" else {})}))


if __name__ == "__main__":
    main()
