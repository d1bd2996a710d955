"""Token ids in, token ids out: continue prompts with a GPT-2 checkpoint written by train.py.

    python -m distributed_pytorch_example_amd.generate --model gpt2-tiny --checkpoint ckpt.pt \\
        --prompt 1,2,3 --prompt 7,8 --max-new-tokens 16 --temperature 0.8 --top-k 40 --top-p 0.95 --seed 0

Prints one line of comma-separated token ids per prompt (the new tokens only).  There is no tokenizer here.
``--ema`` generates from the averaged weights the optimizer state holds (train.py --ema-decay).
"""
from __future__ import annotations

import argparse
import sys

import torch

from .models import get_model
from .optim import _muon_groups, _trust_groups


def _parse_prompt(text: str):
    try:
        ids = [int(t) for t in text.split(",") if t.strip() != ""]
    except ValueError:
        raise argparse.ArgumentTypeError(f"--prompt takes comma-separated token ids, got {text!r}")
    if not ids:
        raise argparse.ArgumentTypeError("--prompt must hold at least one token id")
    return ids


def ema_state_dict(model, opt_state: dict):
    """{parameter name: averaged tensor} from an optimizer state_dict's ``state[i]["ema"]`` tensors, or None where it
    holds none.  The state is indexed by position in the optimizer's param groups; the grouping is one of the three
    build_optimizer makes from model.parameters() (one group; matrices / vectors; Muon's three), told apart by the
    group sizes and checked by every tensor's shape."""
    state, groups = opt_state.get("state", {}), opt_state.get("param_groups", [])
    if not state or not all("ema" in st for st in state.values()):
        return None
    named = list(model.named_parameters())
    by_id = {id(p): n for n, p in named}
    params = [p for _, p in named]
    sizes = [len(g["params"]) for g in groups]
    for cand in ([{"params": params}], _trust_groups(params, 0.0, {}), _muon_groups(params, 0.0)):
        if [len(g["params"]) for g in cand] != sizes:
            continue
        flat = [p for g in cand for p in g["params"]]
        ids = [i for g in groups for i in g["params"]]
        if all(i in state and tuple(state[i]["ema"].shape) == tuple(p.shape) for i, p in zip(ids, flat)):
            return {by_id[id(p)]: state[i]["ema"] for i, p in zip(ids, flat)}
    raise ValueError("the optimizer state's param groups match none of build_optimizer's groupings of this model")


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m distributed_pytorch_example_amd.generate", description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", choices=["gpt2", "gpt2-tiny"], default="gpt2")
    ap.add_argument("--checkpoint", required=True, help="a train.py checkpoint (model_state_dict, optimizer_state_dict)")
    ap.add_argument("--prompt", type=_parse_prompt, action="append", required=True, help="comma-separated token ids; repeat for a batch")
    ap.add_argument("--max-new-tokens", type=int, default=16)
    ap.add_argument("--temperature", type=float, default=1.0, help="0 = greedy")
    ap.add_argument("--top-k", type=int, default=0, help="0 = off")
    ap.add_argument("--top-p", type=float, default=1.0, help="1 = off")
    ap.add_argument("--eos-id", type=int, default=None)
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--graph", action="store_true", help="replay the decode step from a captured HIP graph (GPU)")
    ap.add_argument("--ema", action="store_true", help="generate from the optimizer state's averaged weights")
    ap.add_argument("--device", default=None, help="default: cuda when there is one")
    args = ap.parse_args(argv)

    dev = torch.device(args.device or ("cuda" if torch.cuda.is_available() else "cpu"))
    ckpt = torch.load(args.checkpoint, map_location="cpu", weights_only=True)
    model = get_model(args.model)
    model.load_state_dict(ckpt["model_state_dict"])
    if args.ema:
        ema = ema_state_dict(model, ckpt.get("optimizer_state_dict") or {})
        if ema is None:
            ap.error("--ema: the checkpoint's optimizer state holds no averaged weights (train with --ema-decay)")
        model.load_state_dict(ema)
    vocab = model.cfg.vocab_size
    for p in args.prompt:
        if min(p) < 0 or max(p) >= vocab:
            ap.error(f"--prompt: token ids must lie in [0, {vocab})")
    if args.graph and dev.type != "cuda":
        ap.error("--graph needs the GPU")
    model = model.to(dev)
    lens = [len(p) for p in args.prompt]
    idx = torch.zeros(len(lens), max(lens), dtype=torch.int64)
    for b, p in enumerate(args.prompt):
        idx[b, :len(p)] = torch.tensor(p)
    try:
        out = model.generate(idx.to(dev), args.max_new_tokens, prompt_lens=lens, temperature=args.temperature, top_k=args.top_k,
                             top_p=args.top_p, eos_id=args.eos_id, seed=args.seed, graph=args.graph)
    except ValueError as e:
        ap.error(str(e))
    for row in out.tolist():
        print(",".join(str(t) for t in row))
    return 0


if __name__ == "__main__":
    sys.exit(main())
