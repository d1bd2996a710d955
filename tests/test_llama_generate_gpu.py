"""Llama.generate on the GPU (llama-tiny: 4 query / 2 KV heads of 64, block 128, vocab 512; the matrices scaled x4 so the
logits spread): GQA KV cache + Fx.attn_decode_gqa against a CPU fp32 twin with the same weights.

B 4, ragged prompts of 3, 17, 64 and 70 tokens, 24 new tokens.  Teacher-forced parity as test_generate_gpu.py: the
generated sequence is fed to the twin; e_cache = worst |returned logits - twin|, e_full = worst |existing GPU forward on
the full prefix - twin| at the same positions (the training path, not the code under test); e_cache <= 2 e_full.
"""
import copy

import pytest
import torch

from distributed_pytorch_example_amd.models import get_model

pytestmark = pytest.mark.gpu

LENS = [3, 17, 64, 70]
NEW = 24
_state = {}


def setup():
    """(GPU model, CPU twin, idx [4, 70] on the GPU), built once."""
    if not _state:
        torch.manual_seed(4321)
        twin = get_model("llama-tiny")
        with torch.no_grad():
            for p in twin.parameters():
                if p.ndim >= 2:
                    p.mul_(4.0)
        twin.eval()
        idx = torch.randint(0, twin.cfg.vocab_size, (len(LENS), max(LENS)), generator=torch.Generator().manual_seed(5))
        _state.update(model=copy.deepcopy(twin).cuda(), twin=twin, idx=idx)
    return _state["model"], _state["twin"], _state["idx"].cuda()


@torch.no_grad()
def parity(model, twin, idx, out, lgs):
    V = twin.cfg.vocab_size
    e_cache = e_full = 0.0
    for b, n in enumerate(LENS):
        seq = torch.cat([idx[b, :n], out[b, :-1]]).unsqueeze(0)  # the tokens whose next-token logits were drawn from
        ref = twin(seq.cpu())[0, n - 1:, :V].float()
        e_cache = max(e_cache, (lgs[b].cpu() - ref).abs().max().item())
        e_full = max(e_full, (model(seq)[0, n - 1:, :V].float().cpu() - ref).abs().max().item())
    return e_cache, e_full


@pytest.mark.parametrize("skinny", [True, False])
def test_teacher_forced_parity_and_greedy(skinny):
    model, twin, idx = setup()
    model.decode_skinny = skinny
    try:
        out, lgs = model.generate(idx, NEW, prompt_lens=LENS, temperature=0.0, return_logits=True)
    finally:
        model.decode_skinny = True
    assert out.shape == (4, NEW) and lgs.shape == (4, NEW, 512) and lgs.dtype == torch.float32
    e_cache, e_full = parity(model, twin, idx, out, lgs)
    print(f"llama generate skinny={skinny}: e_cache = {e_cache:.4g}, e_full = {e_full:.4g}, spread of the logits = {lgs.std().item():.3g}")
    assert e_cache <= 2.0 * e_full
    col = torch.arange(512, device=lgs.device).expand_as(lgs)
    low = torch.where(lgs == lgs.max(-1, keepdim=True).values, col, torch.full_like(col, 512)).min(-1).values
    assert torch.equal(out, low)


def test_seed_graph_and_eos():
    model, _, idx = setup()
    kw = dict(prompt_lens=LENS, temperature=0.9, top_k=50, top_p=0.95, seed=7, return_logits=True, eos_id=3)
    out, lgs = model.generate(idx, NEW, **kw)
    out2, lgs2 = model.generate(idx, NEW, **kw)
    assert torch.equal(out, out2) and torch.equal(lgs, lgs2), "the same seed must give the same tokens"
    assert not torch.equal(out, model.generate(idx, NEW, **{**kw, "seed": 8, "return_logits": False}))
    gout, glgs = model.generate(idx, NEW, graph=True, **kw)  # the captured step, replayed: bit for bit the eager run
    assert torch.equal(out, gout) and torch.equal(lgs, glgs)
    base = model.generate(idx, NEW, prompt_lens=LENS, temperature=0.0)
    eos = int(base[0, 5])
    rep = model.generate(idx, NEW, prompt_lens=LENS, temperature=0.0, eos_id=eos)
    for row, ref in zip(rep.tolist(), base.tolist()):
        first = ref.index(eos) if eos in ref else NEW
        assert row[:first] == ref[:first] and all(t == eos for t in row[first:]), "a row that has emitted eos repeats it"
