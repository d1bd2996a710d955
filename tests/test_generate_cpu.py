"""GPT2.generate, the sampler's torch path and the generate CLI on the CPU (fp32 throughout), and the proof of the
sampler's Python reference that test_sample_gpu.py relies on."""
import contextlib
import io

import numpy as np
import pytest
import torch

from _attn_dropout_ref import philox4x32
from _decode_ref import SAMPLE_C3, gumbel_ref, head_tail_row, keep_ref, naive_generate, philox
from distributed_pytorch_example_amd import generate as gen_cli
from distributed_pytorch_example_amd.models import get_model
from distributed_pytorch_example_amd.ops import functional as Fx
from distributed_pytorch_example_amd.optim import build_optimizer
from distributed_pytorch_example_amd.utils.checkpoint import make_checkpoint


def tiny(seed=0):
    torch.manual_seed(seed)
    m = get_model("gpt2-tiny")
    with torch.no_grad():
        for p in m.parameters():
            if p.ndim >= 2:
                p.mul_(4.0)
    return m.eval()


def test_greedy_equals_the_naive_loop():
    m = tiny()
    idx = torch.randint(0, 512, (2, 9), generator=torch.Generator().manual_seed(1))
    out, lgs = m.generate(idx, 7, temperature=0.0, return_logits=True)
    ref, ref_lgs = naive_generate(m, idx, [9, 9], 7)
    assert torch.equal(out, ref)
    assert (lgs - ref_lgs).abs().max().item() < 1e-3 * ref_lgs.abs().max().item()


def test_greedy_ragged_prompts_and_mode():
    m = tiny(1)
    lens = [3, 17, 64, 70]
    idx = torch.randint(0, 512, (4, 70), generator=torch.Generator().manual_seed(2))
    m.train()
    out = m.generate(idx, 6, prompt_lens=lens, temperature=0.0)
    assert m.training, "generate must restore the mode"
    m.eval()
    ref, _ = naive_generate(m, idx, lens, 6)
    assert torch.equal(out, ref)
    # the padding behind a short prompt is never read
    idx2 = idx.clone()
    for b, n in enumerate(lens):
        idx2[b, n:] = 511
    assert torch.equal(m.generate(idx2, 6, prompt_lens=lens, temperature=0.0), out)


def test_top_k_1_equals_greedy_and_seed_repeats():
    m = tiny(2)
    idx = torch.randint(0, 512, (3, 12), generator=torch.Generator().manual_seed(3))
    greedy = m.generate(idx, 8, temperature=0.0)
    assert torch.equal(m.generate(idx, 8, temperature=0.8, top_k=1, seed=4), greedy)
    a = m.generate(idx, 8, temperature=1.0, top_k=40, top_p=0.9, seed=5)
    assert torch.equal(a, m.generate(idx, 8, temperature=1.0, top_k=40, top_p=0.9, seed=5))
    assert not torch.equal(a, m.generate(idx, 8, temperature=1.0, top_k=40, top_p=0.9, seed=6))


def test_eos_repeats_and_length_check():
    m = tiny(3)
    idx = torch.randint(0, 512, (2, 10), generator=torch.Generator().manual_seed(4))
    base = m.generate(idx, 10, temperature=0.0)
    eos = int(base[1, 3])
    out = m.generate(idx, 10, temperature=0.0, eos_id=eos)
    assert out[1, 3:].eq(eos).all() and torch.equal(out[1, :3], base[1, :3])
    with pytest.raises(ValueError, match="block_size"):
        m.generate(idx, 128 - 10 + 1)
    with pytest.raises(ValueError, match="graph"):
        m.generate(idx, 4, graph=True)


@pytest.mark.parametrize("V", [8, 100, 50257])
@pytest.mark.parametrize("ties,top_k,top_p,n_keep", [(0, 1, 1.0, 1), (0, 0, 0.3, 1), (2, 5, 1.0, 6), (0, 0, 0.92, 4), (0, 3, 0.97, 3)])
def test_cpu_sampler_kept_sets(V, ties, top_k, top_p, n_keep):
    """Fx.sample_keep (the CPU sampler's filters) keeps what _decode_ref.keep_ref keeps on the constructed rows, and
    every draw of the CPU sampler lies in that set."""
    z, pos = head_tail_row(V, 6, ties=ties, seed=V + 6)
    keep, margin = keep_ref(z.unsqueeze(0), top_k, top_p)
    assert margin.item() >= V * 2.0 ** -22
    assert set(torch.where(keep[0])[0].tolist()) == set(pos[:n_keep].tolist())
    _, got = Fx.sample_keep(z.unsqueeze(0), 1.0, top_k, top_p)
    assert torch.equal(got, keep)
    R = 64 if V > 1000 else 512
    tok = Fx.sample_logits(z.unsqueeze(0).expand(R, V), V, 1.0, top_k, top_p, generator=torch.Generator().manual_seed(V))
    assert set(tok.tolist()) <= set(pos[:n_keep].tolist())


def test_cpu_sampler_greedy_ties_padding_and_done():
    z = torch.zeros(3, 8)
    z[0, 2] = z[0, 5] = 1.0
    z[1, 4] = 1.0
    z[:, 6:] = 9.0  # padding: V = 6
    assert Fx.sample_logits(z, 6, 0.0).tolist() == [2, 4, 0]
    done = torch.tensor([0, 1, 0], dtype=torch.int32)
    tok = Fx.sample_logits(z, 6, 0.0, eos_id=2, done=done)
    assert tok.tolist() == [2, 2, 0] and done.tolist() == [1, 1, 0]
    draws = Fx.sample_logits(torch.zeros(2000, 8), 5, 1.0, generator=torch.Generator().manual_seed(0))
    assert draws.max() < 5 and draws.unique().numel() == 5


def test_reference_philox_is_the_kernels_philox():
    """_decode_ref.philox with the dropout kernels' c3 reproduces tests/_attn_dropout_ref.philox4x32 (which the
    dropout GPU tests hold the kernels to); with the sampler's c3 every block differs."""
    ctr = np.array([0, 1, 2, 2 ** 32 - 1, 2 ** 32, 2 ** 63 + 12345], dtype=np.uint64)
    for seed, stream in ((0, 0), (0x1234_5678_9ABC_DEF0, 7), (2 ** 63 - 1, 2 ** 32 - 1)):
        a = philox(seed, ctr, stream, c3=0x9E3779B9)
        b = philox4x32(seed, ctr, stream)
        assert a.dtype == np.uint32 and np.array_equal(a, b)
        assert not (philox(seed, ctr, stream) == b).all(axis=-1).any()
    assert SAMPLE_C3 != 0x9E3779B9 and SAMPLE_C3 > 2 ** 16  # mix_draw's fourth word is a small trip count
    g = gumbel_ref(1, 0, 0, 4, 10)
    assert g.shape == (4, 10) and torch.isfinite(g).all()
    assert torch.equal(gumbel_ref(1, 3, 0, 1, 10), gumbel_ref(1, 0, 0, 2, 10)[1:])  # row r starts ceil(V / 4) r blocks in


def _checkpoint(tmp_path, ema):
    m = tiny(7)
    m.train()
    opt = build_optimizer("adamw", m.parameters(), lr=2e-2, ema={"decay": 0.5} if ema else None)
    x = torch.randint(0, 512, (2, 17), generator=torch.Generator().manual_seed(8))
    for _ in range(2):
        m(x[:, :-1], x[:, 1:]).backward()
        opt.step()
        opt.zero_grad()
    path = str(tmp_path / "ckpt.pt")
    torch.save(make_checkpoint(m, opt, 0, 0.0, to_cpu=True), path)
    return m.eval(), opt, path


def _cli(args):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        assert gen_cli.main(args) == 0
    return [[int(t) for t in line.split(",")] for line in buf.getvalue().strip().splitlines()]


def test_cli_prints_what_generate_returns(tmp_path):
    m, opt, path = _checkpoint(tmp_path, ema=True)
    prompts = [[1, 2, 3], [7, 8, 9, 10, 11]]
    idx = torch.zeros(2, 5, dtype=torch.int64)
    for b, p in enumerate(prompts):
        idx[b, :len(p)] = torch.tensor(p)
    args = ["--model", "gpt2-tiny", "--checkpoint", path, "--prompt", "1,2,3", "--prompt", "7,8,9,10,11", "--max-new-tokens", "6",
            "--device", "cpu"]
    assert _cli(args + ["--temperature", "0"]) == m.generate(idx, 6, prompt_lens=[3, 5], temperature=0.0).tolist()
    kw = dict(temperature=0.8, top_k=30, top_p=0.9, eos_id=5, seed=3)
    assert _cli(args + ["--temperature", "0.8", "--top-k", "30", "--top-p", "0.9", "--eos-id", "5", "--seed", "3"]) == \
        m.generate(idx, 6, prompt_lens=[3, 5], **kw).tolist()
    # --ema: the averaged weights of the optimizer state
    with opt.ema_weights():
        want = m.generate(idx, 6, prompt_lens=[3, 5], temperature=0.0).tolist()
    assert _cli(args + ["--temperature", "0", "--ema"]) == want


def test_cli_ema_without_averaged_weights_is_a_parser_error(tmp_path, capsys):
    _, _, path = _checkpoint(tmp_path, ema=False)
    with pytest.raises(SystemExit) as e:
        gen_cli.main(["--model", "gpt2-tiny", "--checkpoint", path, "--prompt", "1,2", "--ema", "--device", "cpu"])
    assert e.value.code == 2
    assert "--ema" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        gen_cli.main(["--model", "gpt2-tiny", "--checkpoint", path, "--prompt", "1,x", "--device", "cpu"])
