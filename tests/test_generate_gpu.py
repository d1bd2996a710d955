"""GPT2.generate on the GPU (gpt2-tiny: 2 heads of 64, block 128, vocab 512; the matrices scaled up so the logits
spread): KV cache + single-token kernels against a CPU fp32 twin with the same weights.

B 4, ragged prompts of 3, 17, 64 and 70 tokens, 24 new tokens.  Teacher-forced parity: the generated sequence is fed
to the twin; e_cache = worst |returned logits - twin| and e_full = worst |existing GPU forward on the full prefix -
twin| at the same positions (the parent commit's path, not the code under test); e_cache <= 2 e_full, the factor
test_model_parity_gpu.py uses for a second bf16 pipeline.  Both are printed.
"""
import copy

import pytest
import torch

from distributed_pytorch_example_amd.models import get_model
from distributed_pytorch_example_amd.optim import build_optimizer

pytestmark = pytest.mark.gpu

LENS = [3, 17, 64, 70]
NEW = 24
_state = {}


def setup():
    """(GPU model, CPU twin, idx [4, 70] on the GPU); built once, the weights never change."""
    if not _state:
        torch.manual_seed(1234)
        twin = get_model("gpt2-tiny")
        with torch.no_grad():
            for p in twin.parameters():
                if p.ndim >= 2:
                    p.mul_(4.0)
        twin.eval()
        model = copy.deepcopy(twin).cuda()
        g = torch.Generator().manual_seed(5)
        idx = torch.randint(0, twin.cfg.vocab_size, (len(LENS), max(LENS)), generator=g)
        _state.update(model=model, twin=twin, idx=idx)
    return _state["model"], _state["twin"], _state["idx"].cuda()


@torch.no_grad()
def parity(model, twin, idx, out, lgs):
    """(e_cache, e_full) of the returned logits and of the existing GPU forward, both against the twin fed the
    generated sequence."""
    V = twin.cfg.vocab_size
    e_cache = e_full = 0.0
    was = model.training
    model.eval()
    for b, n in enumerate(LENS):
        seq = torch.cat([idx[b, :n], out[b, :-1]]).unsqueeze(0)  # the tokens whose next-token logits were drawn from
        ref = twin(seq.cpu())[0, n - 1:, :V].float()
        full = model(seq)[0, n - 1:, :V].float().cpu()
        e_cache = max(e_cache, (lgs[b].cpu() - ref).abs().max().item())
        e_full = max(e_full, (full - ref).abs().max().item())
    model.train(was)
    return e_cache, e_full


@pytest.mark.parametrize("skinny", [True, False])
def test_teacher_forced_parity_and_greedy(skinny):
    model, twin, idx = setup()
    model.decode_skinny = skinny
    try:
        model.train()
        out, lgs = model.generate(idx, NEW, prompt_lens=LENS, temperature=0.0, return_logits=True)
        assert model.training, "generate must restore the mode"
    finally:
        model.decode_skinny = True
        model.eval()
    assert out.shape == (4, NEW) and out.dtype == torch.int64 and lgs.shape == (4, NEW, 512) and lgs.dtype == torch.float32
    e_cache, e_full = parity(model, twin, idx, out, lgs)
    print(f"generate skinny={skinny}: e_cache = {e_cache:.4g}, e_full = {e_full:.4g}, spread of the logits = {lgs.std().item():.3g}")
    assert e_cache <= 2.0 * e_full
    # greedy tokens are the lowest-index argmax of the returned logits, exactly
    V = lgs.shape[-1]
    col = torch.arange(V, device=lgs.device).expand_as(lgs)
    low = torch.where(lgs == lgs.max(-1, keepdim=True).values, col, torch.full_like(col, V)).min(-1).values
    assert torch.equal(out, low)


def test_sampled_parity_and_seed():
    model, twin, idx = setup()
    kw = dict(prompt_lens=LENS, temperature=0.9, top_k=50, top_p=0.95, seed=7, return_logits=True)
    out, lgs = model.generate(idx, NEW, **kw)
    e_cache, e_full = parity(model, twin, idx, out, lgs)
    print(f"generate sampled: e_cache = {e_cache:.4g}, e_full = {e_full:.4g}")
    assert e_cache <= 2.0 * e_full
    out2, lgs2 = model.generate(idx, NEW, **kw)
    assert torch.equal(out, out2) and torch.equal(lgs, lgs2), "the same seed must give the same tokens"
    out3 = model.generate(idx, NEW, **{**kw, "seed": 8, "return_logits": False})
    assert not torch.equal(out, out3)


def test_graph_equals_eager():
    """One decode step captured after a warm-up step and replayed: tokens and logits equal the eager run bit for bit
    over 24 steps with sampling on, so the RNG offset and len advance under replay."""
    model, _, idx = setup()
    kw = dict(prompt_lens=LENS, temperature=0.9, top_k=50, top_p=0.95, seed=11, return_logits=True, eos_id=3)
    out, lgs = model.generate(idx, NEW, **kw)
    gout, glgs = model.generate(idx, NEW, graph=True, **kw)
    assert torch.equal(out, gout)
    assert torch.equal(lgs, glgs)


def test_eos_repeats():
    model, _, idx = setup()
    base = model.generate(idx, NEW, prompt_lens=LENS, temperature=0.0)
    eos = int(base[0, 5])
    out = model.generate(idx, NEW, prompt_lens=LENS, temperature=0.0, eos_id=eos)
    for b in range(out.shape[0]):
        row, ref = out[b].tolist(), base[b].tolist()
        first = ref.index(eos) if eos in ref else NEW
        assert row[:first] == ref[:first], "a row that has not drawn eos is unaffected"
        assert all(t == eos for t in row[first:]), "once a row has emitted eos_id it repeats it"
    assert out[0, 5:].eq(eos).all()


def test_inside_ema_weights():
    """Inside optimizer.ema_weights() the logits are those of the averaged weights: they differ from the live ones and
    match the twin loaded with the ``ema`` tensors."""
    torch.manual_seed(99)
    model = get_model("gpt2-tiny").cuda()
    with torch.no_grad():
        for p in model.parameters():
            if p.ndim >= 2:
                p.mul_(4.0)
    opt = build_optimizer("adamw", model.parameters(), lr=3e-3, ema={"decay": 0.5})
    g = torch.Generator().manual_seed(6)
    for _ in range(3):
        x = torch.randint(0, 512, (4, 65), generator=g).cuda()
        model(x[:, :-1], x[:, 1:]).backward()
        opt.step()
        opt.zero_grad()
    idx = _state["idx"].cuda() if _state else setup()[2]
    live, live_lgs = model.generate(idx, NEW, prompt_lens=LENS, temperature=0.0, return_logits=True)
    twin = get_model("gpt2-tiny")  # (the averages are read before the swap: inside, the state holds the live weights)
    twin.load_state_dict({n: opt.state[p]["ema"].detach().cpu().clone() for n, p in model.named_parameters()})
    twin.eval()
    with opt.ema_weights():
        out, lgs = model.generate(idx, NEW, prompt_lens=LENS, temperature=0.0, return_logits=True)
        e_cache, e_full = parity(model, twin, idx, out, lgs)
    print(f"generate inside ema_weights: e_cache = {e_cache:.4g}, e_full = {e_full:.4g}, "
          f"|ema - live| logits = {(lgs[:, 0] - live_lgs[:, 0]).abs().max().item():.4g}")
    assert e_cache <= 2.0 * e_full
    assert (lgs[:, 0] - live_lgs[:, 0]).abs().max().item() > 4.0 * e_full, "the averaged weights must give other logits"
    after = model.generate(idx, NEW, prompt_lens=LENS, temperature=0.0)
    assert torch.equal(after, live), "the live weights are back afterwards"


def test_length_check_raises_on_the_host():
    model, _, idx = setup()
    with pytest.raises(ValueError, match="block_size"):
        model.generate(idx, 128 - 70 + 1, prompt_lens=LENS)
    model.generate(idx, 2, prompt_lens=LENS)  # (and the model still works)
