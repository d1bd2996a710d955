#!/usr/bin/env python
"""Fx.attn_decode_gqa against the only path there was before it: Fx.rope on the step row, then Fx.attn_decode on a cache
whose K / V heads are expanded G times by repeat_interleave.  (B, Hq, Hkv, Tmax) = (8, 32, 4, 2048), len near 2000.

Each arm is one captured graph of one call per layer over ``--layers`` separate caches (TinyLlama's 22: no call finds
its cache in the L2 or the Infinity Cache from the call before, and no host launch cost is in the figure); the two graphs
alternate in one process, the first round is dropped, the minimum and the spread of the rest are printed.  The bytes are
the K and V rows a call must read, from the shapes; the rate is set against 6.29 TB/s, the measured HBM streaming rate.
One JSON line per arm.

    python scripts/bench_attn_decode_gqa.py [--layers 22] [--rounds 6] [--reps 10]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_STREAM = 6.29e12  # bytes / s, float4 copy


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--layers", type=int, default=22)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    import torch

    from distributed_pytorch_example_amd.ops import ext, functional as Fx

    if not torch.cuda.is_available():
        raise SystemExit("bench_attn_decode_gqa.py measures on the GPU; there is none here")
    ext()
    dev = torch.device("cuda")
    torch.manual_seed(0)
    B, Hq, Hkv, Tmax, D = 8, 32, 4, 2048, 64
    G, W = Hq // Hkv, Hq + 2 * Hkv
    lens = torch.randint(1990, 2010, (B,), dtype=torch.int32, device=dev)
    table = tuple(t.to(dev) for t in Fx.rope_table(Tmax))
    qkv = torch.randn(B, W * D, device=dev).to(torch.bfloat16)
    caches = [torch.randn(2, B, Hkv, Tmax, D, device=dev).to(torch.bfloat16) for _ in range(args.layers)]
    wide = [c.repeat_interleave(G, dim=2) for c in caches]

    def new(l):
        return Fx.attn_decode_gqa(qkv, caches[l][0], caches[l][1], lens, Hq, Hkv, table)

    def old(l):
        r = Fx.rope(qkv.view(B, 1, -1), Hq, Hkv, table, lens.view(B, 1)).view(B, W, D)
        step = torch.stack([r[:, :Hq], r[:, Hq:Hq + Hkv].repeat_interleave(G, 1), r[:, Hq + Hkv:].repeat_interleave(G, 1)], 1)
        return Fx.attn_decode(step.reshape(B, -1), wide[l][0], wide[l][1], lens, Hq)

    # the two paths compute the same thing: bf16 outputs of differently ordered sums
    diff = (new(0).float() - old(0).float()).abs().max().item()
    graphs = {}
    for name, fn in (("attn_decode_gqa", new), ("rope+attn_decode_expanded", old)):
        for l in range(args.layers):
            fn(l)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for l in range(args.layers):
                fn(l)
        graphs[name] = g
    res = {k: [] for k in graphs}
    for _ in range(args.rounds):
        for name, g in graphs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.reps):
                g.replay()
            torch.cuda.synchronize()
            res[name].append((time.perf_counter() - t0) / (args.reps * args.layers) * 1e6)
    kv = 2 * 2 * D * Hkv * int(lens.sum().item())  # K and V rows 0 .. len - 1 of every (row, KV head), bf16
    for name, us in res.items():
        nbytes = kv * (G if "expanded" in name else 1)
        best = min(us[1:])
        print(json.dumps(dict(arm=name, us_per_call=round(best, 2), us_spread=[round(min(us[1:]), 2), round(max(us[1:]), 2)],
                              kv_mb=round(nbytes / 1e6, 2), tb_s=round(nbytes / (best * 1e-6) / 1e12, 3),
                              share_of_stream=round(nbytes / (best * 1e-6) / HBM_STREAM, 3),
                              default_splits=ext().attn_decode_splits(B * (Hq if "expanded" in name else Hkv), Tmax),
                              max_abs_diff_between_arms=diff)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
