"""Gradient clipping under DDP at world 2 over real RCCL (two processes on GPU 0, socket transport, launched
as tests/test_ddp_rccl_world2_gpu.py does): the norm is taken over the averaged buckets with a fixed summation
order, so both ranks derive the same norm bits and end with the same parameters, and the norm equals the
single-process run on the concatenated batch."""
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


def test_clipped_ddp_step_world2_rccl():
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    try:
        import _grad_clip_world2_worker as worker
    finally:
        sys.path.pop(0)

    codes, outs = _run_world(2, [os.path.join(ROOT, "tests", "_grad_clip_world2_worker.py")], timeout=100)
    assert codes == [0, 0], "\n".join(o[-3000:] for o in outs)
    res = []
    for o in outs:
        m = re.search(r"grad-clip result: params=([0-9a-f]{40}) norms=([0-9a-f,]+)", o)
        assert m, o[-3000:]
        res.append((m.group(1), [int(b, 16) for b in m.group(2).split(",")]))
        print(m.group(0))
    assert res[0][0] == res[1][0], "parameters diverged across ranks"
    assert res[0][1] == res[1][1], "ranks derived different gradient norms"
    norms = [_f32(b) for b in res[0][1]]
    assert len(norms) == worker.STEPS and all(n > worker.MAX_NORM for n in norms), norms  # it clipped on every step

    ref = [_f32(b) for b in worker.reference(torch.device("cuda", 0))]
    for step, (a, b) in enumerate(zip(norms, ref)):
        rel = abs(a - b) / b
        print(f"step {step}: world-2 norm {a:.8g}, single-process {b:.8g}, rel diff {rel:.2e}")
        assert rel <= 1e-5
