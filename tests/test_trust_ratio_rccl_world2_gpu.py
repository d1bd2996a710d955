"""LARS / LAMB under DDP at world 2 over real RCCL (two processes on GPU 0, socket transport, launched as
tests/test_grad_clip_rccl_world2_gpu.py does): the per-tensor norms are taken over the averaged buckets with a
fixed summation order, so both ranks derive the same trust_stats bits and end with the same parameters, and the
stats equal the single-process run on the concatenated batch."""
import os
import re
import socket
import struct
import subprocess
import sys
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run_world(n, args, extra_env=None, timeout=100):
    port = _port()
    procs = []
    for r in range(n):
        env = dict(os.environ)
        env.update({"RANK": str(r), "WORLD_SIZE": str(n), "LOCAL_RANK": "0", "LOCAL_WORLD_SIZE": str(n),
                    "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "PYTHONPATH": ROOT,
                    "NCCL_HOSTID": f"dpe-test-host-{r}", "NCCL_SOCKET_IFNAME": "lo", "NCCL_IB_DISABLE": "1",
                    "HSA_ENABLE_IPC_MODE_LEGACY": "0", "OMP_NUM_THREADS": "1",
                    "DPE_RCCL_MAX_CHANNELS": "4"})
        env.update(extra_env or {})
        procs.append(subprocess.Popen([sys.executable, "-u", *args], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True))
    outs = [None] * n
    deadline = time.time() + timeout
    try:
        for i, p in enumerate(procs):
            try:
                outs[i] = p.communicate(timeout=max(1.0, deadline - time.time()))[0]
            except subprocess.TimeoutExpired:
                break  # (every process still running is killed below; its output is kept for the report)
    finally:
        for i, p in enumerate(procs):
            if p.poll() is None:
                p.kill()
            if outs[i] is None:
                outs[i] = (p.communicate()[0] or "") + f"\n[killed by the test after {timeout}s]"
    return [p.returncode for p in procs], outs


def _f32(bits):
    return struct.unpack("<f", struct.pack("<I", bits))[0]


def test_trust_ratio_ddp_step_world2_rccl():
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    try:
        import _trust_ratio_world2_worker as worker
    finally:
        sys.path.pop(0)

    codes, outs = _run_world(2, [os.path.join(ROOT, "tests", "_trust_ratio_world2_worker.py")], timeout=100)
    assert codes == [0, 0], "\n".join(o[-3000:] for o in outs)
    res = []
    for o in outs:
        m = re.search(r"trust-ratio result: params=([0-9a-f]{40}) stats=([0-9a-f,]+)", o)
        assert m, o[-3000:]
        res.append((m.group(1), [int(b, 16) for b in m.group(2).split(",")]))
        print(m.group(0)[:200])
    assert res[0][0] == res[1][0], "parameters diverged across ranks"
    assert res[0][1] == res[1][1], "ranks derived different trust stats"

    ref = torch.stack(worker.reference(torch.device("cuda", 0))).double()  # [optimizers * STEPS, n_tensors, 3]
    got = torch.tensor([_f32(b) for b in res[0][1]], dtype=torch.float64).reshape(ref.shape)
    assert ref.shape[0] == len(worker.OPTIMIZERS) * worker.STEPS and ref.shape[2] == 3
    assert torch.isfinite(got).all() and (got[:, :, :2] > 0).all()
    assert (got[:, :, 2] != 1.0).any(dim=1).all()  # every step scaled some tensor
    rel = ((got - ref).abs() / ref.abs()).amax(dim=(1, 2))
    for step, r in enumerate(rel.tolist()):
        print(f"step {step}: worst rel diff of the trust stats, world 2 vs single process: {r:.2e}")
    assert (rel <= 1e-5).all()
