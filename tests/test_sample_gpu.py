"""sample_logits (csrc/kernels/decode.hip) against the fp64 references of tests/_decode_ref.py.

The sampler is defined on values: temperature 0 is the argmax (lowest index on ties); otherwise s = z / temperature in
fp32, top-k keeps s >= the k-th largest value (ties stay), top-p keeps j iff the softmax mass of the strictly larger kept
values is < top_p, and the token is the arg max over the kept j of s_j + g_j with g the Gumbel noise of the Philox
words the reference recomputes.

  1 / 2  greedy = lowest-index argmax on planted exact ties and with the maximum in the last real column; padding
         columns holding +large values are never drawn (greedy and sampled)
  3      constructed rows (geometric head tokens at permuted positions over a tail of mass < 2^-10), V in {8, 100,
         50257 with ld 50304}: the fp64 kept set is first asserted unambiguous (no |M_>(j) - top_p| < V 2^-22, the crude
         bound of a sequential fp32 sum of V probabilities plus their exp), then every one of 4096 draws lies in it
  4      exact draw, 4096 distinct rows with 8 - 100 kept tokens: the kernel's token scores within 2^-14 max(1, |score|)
         of the fp64 maximum (fp32 evaluation with few-ulp functions on magnitudes <= 64 errs below 2^-17; the factor 8
         is slack for the division by temperature) and equals the reference token wherever the top-two gap exceeds
         that; the reference alone shows <= 1 % of the rows under the gap
  5      65536 rows of one 8-token distribution: sup |empirical CDF - exact CDF| <= 0.01 at temperature 1, 0.5 and 2
         (DKW: a correct sampler exceeds it with probability 2 exp(-2 65536 10^-4) ~ 4e-6)
  6      the same state gives the same tokens, the advanced state different ones, rows of one call differ
  7      a row whose done flag is set emits eos_id; a row that draws eos_id sets its flag; other rows are unaffected

fp32 rows wider than 32768 columns are outside the kernel (they would not fit the registers of one workgroup): the
50257-column cases run on bf16 logits, the LM head's dtype.
"""
import pytest
import torch

from _decode_ref import gumbel_ref, head_tail_row, keep_ref

pytestmark = pytest.mark.gpu

BIG = 1.0e4
DT = {"bf16": torch.bfloat16, "f32": torch.float32}


def dev():
    return torch.device("cuda")


def rng(seed, offset=0):
    return torch.tensor([seed, offset], dtype=torch.int64, device=dev())


def padded(z, ld, dtype, rows=None, fill=BIG):
    """z [R, V] fp32 (bf16-representable values) -> [R, ld] of ``dtype`` on the GPU, the pad columns = ``fill``;
    ``rows``: z is one row, repeated that often (on the device)."""
    R, V = z.shape
    zt = z.to(dev()).to(dtype)
    if rows is not None:
        zt, R = zt.expand(rows, V), rows
    out = torch.full((R, ld), fill, dtype=dtype, device=dev())
    out[:, :V] = zt
    return out


def bf(t):
    return t.to(torch.bfloat16).float()


# ----------------------------------------------------------------- 1, 2: greedy
@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_greedy_ties_last_column_and_padding(C, dt):
    V, ld = 100, 104
    g = torch.Generator().manual_seed(1)
    z = bf(torch.randn(6, V, generator=g))
    z[0, 17] = z[0, 60] = 9.0           # exact tie: the lower index
    z[1, V - 1] = 9.0                   # the maximum in the last real column
    z[2, V - 1] = z[2, 3] = 9.0         # tie between the last real column and an early one
    z[3, 0] = 9.0
    z[4] = -3.0                         # every column ties
    z[5, 96:] = 9.0                     # ties inside the tail chunk, next to the padding
    tok = C.sample_logits(padded(z, ld, DT[dt]), V, 0.0, 0, 1.0, rng(0)).cpu()
    assert tok.tolist() == [17, V - 1, 3, 0, 0, 96]


def test_greedy_wide_row(C):
    V, ld = 50257, 50304
    z = bf(torch.randn(3, V, generator=torch.Generator().manual_seed(2)))
    z[0, V - 1] = 9.0
    z[1, 40000] = z[1, 12345] = 9.0
    z[2, 50256] = z[2, 50255] = 9.0
    tok = C.sample_logits(padded(z, ld, torch.bfloat16), V, 0.0, 0, 1.0, rng(0)).cpu()
    assert tok.tolist() == [V - 1, 12345, 50255]


@pytest.mark.parametrize("dt,V,ld", [("bf16", 100, 104), ("f32", 100, 104), ("bf16", 50257, 50304), ("f32", 5, 8)])
def test_padding_is_never_drawn(C, dt, V, ld):
    R = 4096 if V < 1000 else 256
    z = torch.zeros(1, V)  # flat: every real column is as likely as any other
    tok = C.sample_logits(padded(z, ld, DT[dt], rows=R), V, 1.0, 0, 1.0, rng(3)).cpu()
    assert tok.min() >= 0 and tok.max() < V
    assert tok.unique().numel() > min(V, R) // 4


# ------------------------------------------------------------------ 3: filters
FILTERS = [  # (name, n_head, ties, top_k, top_p, expected number kept or None)
    ("top_k=1", 6, 0, 1, 1.0, 1),
    ("top_p below the largest head", 6, 0, 0, 0.3, 1),
    ("ties on the top-k threshold", 6, 2, 5, 1.0, 6),
    ("top_p", 6, 0, 0, 0.92, 4),
    ("top_k and top_p", 6, 0, 3, 0.97, 3),
]


@pytest.mark.parametrize("dt,V,ld", [("bf16", 8, 8), ("f32", 8, 8), ("bf16", 100, 104), ("f32", 100, 104), ("bf16", 50257, 50304)])
@pytest.mark.parametrize("name,n_head,ties,top_k,top_p,n_keep", FILTERS)
def test_filters(C, dt, V, ld, name, n_head, ties, top_k, top_p, n_keep):
    temperature = 1.0
    z, pos = head_tail_row(V, n_head, ties=ties, seed=V + n_head)
    s = (z / temperature).unsqueeze(0)
    keep, margin = keep_ref(s, top_k, top_p)
    # the input's own condition: the fp64 kept set is not within fp32 summation error of another one
    assert margin.item() >= V * 2.0 ** -22, (name, V, margin.item())
    kept = set(torch.where(keep[0])[0].tolist())
    assert kept == set(pos[:n_keep].tolist()), (name, V, sorted(kept), pos.tolist())
    R = 4096
    logits = padded(z.unsqueeze(0), ld, DT[dt], rows=R)
    tok = C.sample_logits(logits, V, temperature, top_k, top_p, rng(11 + V)).cpu()
    drawn = set(tok.tolist())
    assert drawn <= kept, (name, V, sorted(drawn - kept))
    if len(kept) > 1:
        assert len(drawn) > 1, "4096 draws from several kept tokens gave one"


# --------------------------------------------------------------- 4: exact draw
def _exact_rows(V, temperature, top_k, top_p, R=4096):
    """R rows of bf16-representable randn logits whose fp64 kept set is unambiguous (the first R of 2 R candidates
    that meet the margin), with between 8 and 100 kept tokens each."""
    g = torch.Generator().manual_seed(4)
    z = bf(torch.randn(2 * R, V, generator=g))
    s = z / temperature  # fp32 division: the kernel's s_j
    keep, margin = keep_ref(s, top_k, top_p)
    ok = margin >= V * 2.0 ** -22
    assert ok.sum() >= R
    z, s, keep = z[ok][:R], s[ok][:R], keep[ok][:R]
    n = keep.sum(-1)
    assert n.min() >= 8 and n.max() <= 100, (n.min().item(), n.max().item())
    return z, s, keep


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("top_k,top_p", [(40, 1.0), (0, 0.9), (60, 0.95)])
def test_exact_draw(C, dt, top_k, top_p):
    V, ld, temperature, seed, offset, stream = 100, 104, 0.7, 0x1234_5678_9ABC, 10 ** 10, 5
    z, s, keep = _exact_rows(V, temperature, top_k, top_p)
    R = z.shape[0]
    score = torch.where(keep, s.double() + gumbel_ref(seed, offset, stream, R, V), torch.full((R, V), float("-inf"), dtype=torch.float64))
    top2 = torch.topk(score, 2, dim=-1).values
    tol = 2.0 ** -14 * top2[:, 0].abs().clamp(min=1.0)
    clear = (top2[:, 0] - top2[:, 1]) > tol
    assert (~clear).float().mean().item() <= 0.01, "the reference alone must leave <= 1 % of the rows under the gap"
    ref_tok = score.argmax(-1)
    tok = C.sample_logits(padded(z, ld, DT[dt]), V, temperature, top_k, top_p, rng(seed, offset), stream).cpu()
    assert keep[torch.arange(R), tok].all(), "a token outside the kept set"
    got = score[torch.arange(R), tok]
    worst = ((top2[:, 0] - got) / tol).max().item()
    print(f"exact draw {dt} top_k={top_k} top_p={top_p}: worst (max score - drawn score) / tol = {worst:.3g}; "
          f"{int((~clear).sum())} of {R} rows under the gap")
    assert worst <= 1.0
    assert torch.equal(tok[clear], ref_tok[clear])


# ------------------------------------------------------------- 5: distribution
@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("temperature", [1.0, 0.5, 2.0])
def test_distribution(C, dt, temperature):
    V, R = 8, 65536
    z = bf(torch.tensor([0.0, -0.5, 1.0, -2.0, 0.25, -1.0, 0.75, -3.0]))
    tok = C.sample_logits(padded(z.unsqueeze(0), V, DT[dt], rows=R), V, temperature, 0, 1.0, rng(77, 123)).cpu()
    emp = torch.bincount(tok, minlength=V).double().cumsum(0) / R
    exact = torch.softmax((z / temperature).double(), dim=-1).cumsum(0)
    sup = (emp - exact).abs().max().item()
    print(f"distribution {dt} T={temperature}: sup |CDF - exact| = {sup:.5f}")
    assert sup <= 0.01


# -------------------------------------------------------------------- 6: state
def test_state(C):
    from distributed_pytorch_example_amd.ops import functional as Fx

    V, ld, R = 100, 104, 512
    logits = padded(torch.zeros(R, V), ld, torch.bfloat16)
    st = Fx.DropoutState(dev()).manual_seed(99, 1000)
    snap = st.snapshot()
    a = Fx.sample_logits(logits, V, 1.0, state=st)
    assert st.tensor().tolist() == [99, 1000 + R * 25], "the state advances by B ceil(V / 4)"
    b = Fx.sample_logits(logits, V, 1.0, state=st)
    again = C.sample_logits(logits, V, 1.0, 0, 1.0, snap)
    assert torch.equal(a, again), "the same state must give the same tokens"
    assert not torch.equal(a, b), "the advanced state must give other tokens"
    assert a.unique().numel() > 50, "the rows of one call must differ"
    # rows are told apart by the counter only: row r of a call at offset o is row 0 of a call at offset o + r * 25
    one = C.sample_logits(logits[:1], V, 1.0, 0, 1.0, rng(99, 1000 + 7 * 25))
    assert one.item() == a[7].item()


# --------------------------------------------------------------- 7: done / eos
def test_done_and_eos(C):
    V, eos = 8, 3
    first = torch.full((6, V), -5.0)
    for r, t in enumerate([3, 5, 3, 1, 0, 7]):
        first[r, t] = 5.0
    second = torch.full((6, V), -5.0)
    for r, t in enumerate([1, 2, 4, 3, 6, 6]):
        second[r, t] = 5.0
    done = torch.zeros(6, dtype=torch.int32, device=dev())
    t1 = C.sample_logits(padded(first, V, torch.bfloat16), V, 0.0, 0, 1.0, rng(0), 0, eos, done).cpu()
    assert t1.tolist() == [3, 5, 3, 1, 0, 7] and done.cpu().tolist() == [1, 0, 1, 0, 0, 0]
    t2 = C.sample_logits(padded(second, V, torch.bfloat16), V, 0.0, 0, 1.0, rng(0), 0, eos, done).cpu()
    assert t2.tolist() == [3, 2, 3, 3, 6, 6] and done.cpu().tolist() == [1, 0, 1, 1, 0, 0]
    # sampled, not greedy: the finished rows still emit eos, the others draw from their own rows
    t3 = C.sample_logits(padded(second, V, torch.float32), V, 0.25, 0, 1.0, rng(5), 0, eos, done).cpu()
    assert t3.tolist()[:4] == [3, 2, 3, 3] and done.cpu().tolist()[:4] == [1, 0, 1, 1]
    # without eos_id the flags are neither read nor written
    t4 = C.sample_logits(padded(second, V, torch.bfloat16), V, 0.0, 0, 1.0, rng(0), 0, -1, done).cpu()
    assert t4.tolist() == [1, 2, 4, 3, 6, 6] and done.cpu().tolist()[:4] == [1, 0, 1, 1]
