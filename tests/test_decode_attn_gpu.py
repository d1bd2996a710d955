"""attn_decode (csrc/kernels/decode.hip) against the fp64 reference of tests/_decode_ref.py: one query per (row, head)
against a head-major KV cache, the key range split over S workgroups and merged by attn_decode_combine.

B 3, H 2, Tmax 192; the rows' lengths come from {0, 1, 63, 64, 65, 127, 191} (the first token, both sides of a
64-key boundary, the last slot, rows that differ within a batch); S forced to 1, 2, 3 and 8 (S = 8 with len = 1
leaves six splits without a key).  Cache rows beyond len hold NaN bit patterns and so does a guard region behind the
output.  Per element |err| <= b_out = 2^-7 (P |v|), the flash kernels' budget (attn_decode keeps P in fp32, which only
makes it easier); every case prints its worst ratio.  No test passes a len outside [0, Tmax - 1].
"""
import math

import pytest
import torch

from _decode_ref import attn_decode_ref
from _gpt2_ref import staircase_qkv

pytestmark = pytest.mark.gpu

B, H, TMAX, D = 3, 2, 192, 64
SCALE = 1.0 / math.sqrt(D)
LENS = [(0, 1, 63), (64, 65, 127), (191, 0, 64), (1, 1, 1), (127, 191, 65)]
SPLITS = [1, 2, 3, 8]
NAN_BITS = 0x7FC1  # a bf16 quiet NaN
_cases = {}


def case(lens):
    """(qkv_step, kc, vc) bf16 on the CPU with NaN beyond each row's length, and the fp64 (out, bound); shared,
    never modified."""
    if lens not in _cases:
        g = torch.Generator().manual_seed(100 + sum(lens))
        qkv = torch.randn(B, 3, H, D, generator=g).to(torch.bfloat16)
        kc = torch.randn(B, H, TMAX, D, generator=g).to(torch.bfloat16)
        vc = torch.randn(B, H, TMAX, D, generator=g).to(torch.bfloat16)
        nan = torch.tensor(NAN_BITS, dtype=torch.int16).view(torch.bfloat16)
        for b, n in enumerate(lens):
            kc[b, :, n:] = nan
            vc[b, :, n:] = nan
        _cases[lens] = (qkv, kc, vc) + attn_decode_ref(qkv, kc, vc, lens, SCALE)
    return _cases[lens]


def run(C, qkv, kc, vc, lens, S):
    """The kernel on device copies -> (out, kc, vc) back on the CPU."""
    dev = torch.device("cuda")
    q, k, v = qkv.to(dev), kc.to(dev).clone(), vc.to(dev).clone()
    nb = qkv.shape[0]
    obuf = torch.full((nb + 1, H * D), NAN_BITS, dtype=torch.int16, device=dev).view(torch.bfloat16)  # last row: guard
    out = C.attn_decode(q, k, v, torch.tensor(lens, dtype=torch.int32, device=dev), SCALE, S, obuf[:nb])
    torch.cuda.synchronize()
    assert out.data_ptr() == obuf.data_ptr()
    assert (obuf[nb].view(torch.int16) == NAN_BITS).all(), "the guard behind the output was written"
    return out.cpu(), k.cpu(), v.cpu()


def bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("S", SPLITS)
@pytest.mark.parametrize("lens", LENS)
def test_attn_decode(C, lens, S):
    qkv, kc, vc, ref, bound = case(lens)
    out, k2, v2 = run(C, qkv, kc, vc, lens, S)
    assert out.shape == (B, H * D) and out.dtype == torch.bfloat16
    assert torch.isfinite(out.float()).all(), "a masked key reached the arithmetic"
    ratio = ((out.double() - ref).abs() / bound).max().item()
    print(f"attn_decode lens={lens} S={S}: worst |err| / b_out = {ratio:.3f}")
    assert ratio <= 1.0
    # cache row len[b] is the step's K / V bit for bit; every other row is unchanged bit for bit
    ek, ev = kc.clone(), vc.clone()
    for b, n in enumerate(lens):
        ek[b, :, n] = qkv[b, 1]
        ev[b, :, n] = qkv[b, 2]
    assert torch.equal(bits(k2), bits(ek)) and torch.equal(bits(v2), bits(ev))


def test_default_splits_and_guard(C):
    """The default S is a function of (B H, Tmax) only, and nothing is written behind the output or the cache: the
    output of a larger batch's first rows and the cache of its last row stay as they were."""
    assert C.attn_decode_splits(B * H, TMAX) == C.attn_decode_splits(B * H, TMAX) >= 1
    lens = LENS[0]
    qkv, kc, vc, ref, bound = case(lens)
    dev = torch.device("cuda")
    # one extra (guard) batch row in the cache buffers behind the B real ones
    kbuf = torch.full((B + 1, H, TMAX, D), NAN_BITS, dtype=torch.int16, device=dev).view(torch.bfloat16)
    vbuf = kbuf.clone()
    kbuf[:B], vbuf[:B] = kc.to(dev), vc.to(dev)
    out = C.attn_decode(qkv.to(dev), kbuf[:B], vbuf[:B], torch.tensor(lens, dtype=torch.int32, device=dev), SCALE, 0)
    torch.cuda.synchronize()
    assert ((out.cpu().double() - ref).abs() / bound).max().item() <= 1.0
    assert (bits(kbuf[B].cpu()) == NAN_BITS).all() and (bits(vbuf[B].cpu()) == NAN_BITS).all()


def test_staircase_moves_the_max_between_splits(C):
    """_gpt2_ref.staircase_qkv with 24-key tiles: the score of an a_hi query rises by 6 (head 0) and 12 (head 1) log2
    units every 24 keys, and S = 8 over 192 keys gives every split 24 keys, so each split's maximum is above the one
    before it and the combine rescales at every split.  S = 1 and S = 8 meet the same bound."""
    T = TMAX
    qkv_full, _ = staircase_qkv(T, (6.0, 12.0), tile=24)  # [1, T, 3, 2, 64]; row 0 is an a_hi row (block 0)
    # the query of row 0 (a_hi) against all T keys: the step is token T - 1 with row 0's query
    step = qkv_full[0, T - 1].clone()
    step[0] = qkv_full[0, 0, 0]
    qkv = step.unsqueeze(0).contiguous()  # [1, 3, 2, 64]
    kc = qkv_full[0, :, 1].transpose(0, 1).unsqueeze(0).contiguous()  # [1, 2, T, 64]
    vc = qkv_full[0, :, 2].transpose(0, 1).unsqueeze(0).contiguous()
    lens = (T - 1,)
    ref, bound = attn_decode_ref(qkv, kc, vc, lens, SCALE)
    for S in (1, 8):
        out, _, _ = run(C, qkv, kc, vc, lens, S)
        ratio = ((out.double() - ref).abs() / bound).max().item()
        print(f"staircase S={S}: worst |err| / b_out = {ratio:.3f}")
        assert torch.isfinite(out.float()).all() and ratio <= 1.0


@pytest.mark.parametrize("S", [1, 3])
def test_bitwise_repeatable(C, S):
    lens = LENS[1]
    qkv, kc, vc, _, _ = case(lens)
    a, ka, va = run(C, qkv, kc, vc, lens, S)
    b, kb, vb = run(C, qkv, kc, vc, lens, S)
    assert torch.equal(bits(a), bits(b)) and torch.equal(bits(ka), bits(kb)) and torch.equal(bits(va), bits(vb))


def test_wrapper_matches_cpu_path():
    """Fx.attn_decode on the GPU and its torch path on the CPU (fp32 cache) agree within the bf16 budget."""
    from distributed_pytorch_example_amd.ops import functional as Fx

    lens = LENS[4]
    qkv, kc, vc, ref, bound = case(lens)
    dev = torch.device("cuda")
    out = Fx.attn_decode(qkv.reshape(B, -1).to(dev), kc.to(dev).clone(), vc.to(dev).clone(),
                         torch.tensor(lens, dtype=torch.int32, device=dev), H)
    kf, vf = kc.float(), vc.float()
    cpu = Fx.attn_decode(qkv.reshape(B, -1).float(), kf, vf, torch.tensor(lens, dtype=torch.int32), H)
    assert ((out.cpu().double() - ref).abs() / bound).max().item() <= 1.0
    assert ((cpu.double() - ref).abs() / bound).max().item() <= 1.0
    for b, n in enumerate(lens):
        assert torch.equal(kf[b, :, n], qkv[b, 1].float()) and torch.equal(vf[b, :, n], qkv[b, 2].float())
