"""The Llama model off the GPU: llama-tiny against the independent Hugging-Face-style reference of _llama_ref.py, the
parameter count of tinyllama-1.1b, the rope table, and the train.py names.

Measured: relative norm error of the fp32 logits against the fp64 reference 5.6e-07 (plain and packed)."""
import copy
import math
import os
import socket
import subprocess
import sys

import pytest
import torch

import _llama_ref as R
from _packed_attn_ref import doc_start_of
from distributed_pytorch_example_amd.models import get_model
from distributed_pytorch_example_amd.ops import functional as Fx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("packed", [False, True], ids=["plain", "packed"])
def test_llama_tiny_vs_hf_style_reference(packed):
    torch.manual_seed(11)
    m = get_model("llama-tiny")
    for p in m.parameters():
        p.data.add_(0.1 * torch.randn_like(p) if p.dim() == 1 else 0)  # (norm gains off 1: they are checked too)
    idx = torch.randint(0, 512, (2, 100))
    ds = torch.stack([doc_start_of(100, [70]), doc_start_of(100, [3, 64])]) if packed else None
    with torch.no_grad():
        got = m(idx, None, ds)
        ref = R.llama_ref(copy.deepcopy(m).double(), idx, ds)
    rel = ((got.double() - ref).norm() / ref.norm()).item()
    print(f"llama-tiny logits vs fp64 reference, packed={packed}: relative norm error {rel:.6e}")
    assert got.shape == (2, 100, 512) and rel < 1e-4


def test_tinyllama_parameter_count():
    with torch.device("meta"):
        m = get_model("tinyllama-1.1b")
    assert m.num_params() == 1_100_048_384
    assert m.h[0].c_attn.weight.shape == (40 * 64, 2048) and m.h[0].c_fc.weight.shape == (2 * 5632, 2048)


@pytest.mark.parametrize("p,i", [(0, 0), (1, 31), (2047, 0), (2047, 31)])
def test_rope_table_entries(p, i):
    cos, sin = Fx.rope_table(2048)
    ang = p * 10000.0 ** (-2.0 * i / 64.0)
    assert cos.shape == sin.shape == (2048, 32) and cos.dtype == torch.float32
    assert abs(cos[p, i].item() - math.cos(ang)) <= 2.0 ** -24 and abs(sin[p, i].item() - math.sin(ang)) <= 2.0 ** -24


def _train(tmp_path, extra):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, PYTHONPATH=ROOT, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
               MASTER_PORT=str(port), OMP_NUM_THREADS="2", CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--backend", "gloo", "--model", "llama-tiny", "--epochs", "1",
           "--num-samples", "16", "--batch-size", "4", "--seq-len", "64", "--seed", "1", "--doc-len-mean", "32",
           "--checkpoint-dir", str(tmp_path / "ck"), *extra]
    return subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)


def test_train_cli_llama_tiny(tmp_path):
    r = _train(tmp_path, [])
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    loss = float((r.stdout + r.stderr).split("Train Loss: ")[1].split()[0])
    assert math.isfinite(loss) and 5.0 < loss < 8.0  # ln(512) = 6.24 at initialisation
    r = _train(tmp_path, ["--dropout", "0.1"])
    assert r.returncode == 2 and "--dropout" in r.stderr
