"""Worker of tests/test_trust_ratio_rccl_world2_gpu.py: a small SimpleNet under DDP over real RCCL, rank-local
data, 3 LAMB steps and 3 LARS steps.  The per-tensor norms are taken over the all-reduced (averaged) bucket
views with a fixed summation order, so every rank must print the same trust_stats bits and the same parameter
hash.  ``reference()`` is the single-process run on the concatenated batch (imported by the test)."""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WORLD = 2
STEPS = 3
BATCH = 8  # per rank
OPTIMIZERS = (("lamb", dict(lr=1e-2, weight_decay=1e-2)), ("lars", dict(lr=5e-2, weight_decay=1e-4, trust_coefficient=0.02)))


def make_model(dev):
    from distributed_pytorch_example_amd.models import get_model

    torch.manual_seed(300)
    return get_model("simplenet", input_size=64, hidden_size=128).to(dev).eval()  # eval: no dropout masks


def rank_data(rank, step):
    g = torch.Generator().manual_seed(1000 * (rank + 1) + step)
    return torch.randn(BATCH, 64, generator=g), torch.randint(0, 10, (BATCH,), generator=g)


def run(model, fwd, batches, dev):
    """STEPS steps of each optimizer in turn on the same model; returns every step's trust_stats [n, 3]."""
    from distributed_pytorch_example_amd.ops import functional as Fx
    from distributed_pytorch_example_amd.optim import build_optimizer

    stats = []
    for name, kw in OPTIMIZERS:
        opt = build_optimizer(name, model.parameters(), **kw)
        for step in range(STEPS):
            x, y = batches(step)
            loss = Fx.cross_entropy(fwd(x.to(dev)), y.to(dev), 10)
            loss.backward()
            opt.step()
            stats.append(opt.trust_stats.clone())
            opt.zero_grad()
    torch.cuda.synchronize()
    return [s.cpu() for s in stats]


def reference(dev):
    """One process, every rank's batch concatenated (the mean loss over it has the averaged gradient)."""
    model = make_model(dev)

    def batches(step):
        xs, ys = zip(*(rank_data(r, step) for r in range(WORLD)))
        return torch.cat(xs), torch.cat(ys)

    return run(model, model, batches, dev)


def main():
    from distributed_pytorch_example_amd.parallel import DDP
    from distributed_pytorch_example_amd.parallel import dist as pdist

    rank, world, _ = pdist.init_process_group("rccl")
    assert world == WORLD
    dev = torch.device("cuda", 0)
    model = make_model(dev)
    ddp = DDP(model, bucket_cap_mb=0.25, first_bucket_mb=0.05)
    assert ddp._native and ddp.reducer.world == world
    stats = run(model, ddp, lambda step: rank_data(rank, step), dev)
    h = hashlib.sha1()
    for p in model.parameters():
        h.update(p.detach().cpu().numpy().tobytes())
    bits = torch.stack(stats).view(torch.int32).flatten().tolist()
    print(f"rank {rank} trust-ratio result: params={h.hexdigest()} stats={','.join(f'{b & 0xFFFFFFFF:08x}' for b in bits)}",
          flush=True)
    pdist.destroy_process_group()


if __name__ == "__main__":
    main()
