"""linear_skinny (csrc/kernels/decode.hip): y[M, N] = x[M, K] w[N, K]^T for M <= 16 on v_mfma_f32_16x16x32_bf16 with the
weights streamed straight into the B fragments, against the fp64 references of tests/_gemm_ref.py.

Shapes: M in {1, 5, 16} x (N, K) in {(16, 32), (48, 160), (528, 64), (272, 800)} and one GPT-2 row, (768, 3072) at
M = 8 (the only one whose default plan splits K over blocks; (272, 800) is also forced to 2 and 3 block splits).
Tier A (_gemm_ref.int_case, exact integers): bf16 and fp32 outputs equal the fp64 result bit for bit, with bias and
with residual (also aliasing the output).  Tier B (randn_case): per element |err| <= b_bf16 / b_f32 / b_gelu with the
binding's ``splits`` (K partials added per output); every case prints its worst ratio.  x is a view with a padded row
stride into a buffer of NaN (behind every row and behind row M), and the output is the head of a buffer whose tail row
must come back bit-unchanged.  K = 40 and N = 24 are outside the envelope: the binding raises, the wrapper falls back.
"""
import pytest
import torch

from _gemm_ref import b_bf16, b_f32, b_gelu, gemm_ref, int_case, randn_case

pytestmark = pytest.mark.gpu

MS = [1, 5, 16]
NK = [(16, 32), (48, 160), (528, 64), (272, 800)]
SHAPES = [(M, N, K, 0) for M in MS for N, K in NK] + [(8, 768, 3072, 0), (5, 272, 800, 2), (16, 272, 800, 3)]


def dev():
    return torch.device("cuda")


def padded_x(A):
    """A [M, K] as a view with row stride K + 8 into a [M + 1, K + 8] buffer of NaN."""
    M, K = A.shape
    buf = torch.full((M + 1, K + 8), float("nan"), dtype=torch.bfloat16, device=dev())
    buf[:M, :K] = A.to(dev())
    return buf[:M, :K]


def run(C, c, *, bias=False, gelu=False, out_f32=False, res=None, alias=False, ksplit=0):
    """-> the [M, N] result on the CPU; checks the guard row behind the output."""
    M, N = c["M"], c["N"]
    dt = torch.float32 if out_f32 else torch.bfloat16
    obuf = torch.full((M + 1, N), float("nan"), dtype=dt, device=dev())
    r = None
    if res is not None:
        if alias:
            obuf[:M] = res.to(dev())
            r = obuf[:M]
        else:
            r = res.to(dev())
    y = C.linear_skinny(padded_x(c["A"]), c["B"].to(dev()), c["bias"].to(dev()) if bias else None, gelu, out_f32, r, obuf[:M],
                        ksplit)
    torch.cuda.synchronize()
    assert y.data_ptr() == obuf.data_ptr()
    assert torch.isnan(obuf[M]).all(), "the guard row behind the output was written"
    return y.cpu()


@pytest.mark.parametrize("M,N,K,ks", SHAPES)
def test_tier_a_exact(C, M, N, K, ks):
    c = int_case(M, N, K, "nt", "f32")
    ref = gemm_ref(c["A"], c["B"], "nt", bias=c["bias"], residual=c["res"])["y"]
    for alias in (False, True):
        y = run(C, c, bias=True, out_f32=True, res=c["res"], alias=alias, ksplit=ks)
        assert torch.equal(y.double(), ref), (M, N, K, "fp32 + bias + residual", alias)
    y = run(C, c, out_f32=True, ksplit=ks)
    assert torch.equal(y.double(), gemm_ref(c["A"], c["B"], "nt")["y"])
    cb = int_case(M, N, K, "nt", "bf16")
    for bias in (False, True):
        y = run(C, cb, bias=bias, ksplit=ks)
        assert torch.equal(y.double(), gemm_ref(cb["A"], cb["B"], "nt", bias=cb["bias"] if bias else None)["y"]), (M, N, K, bias)


@pytest.mark.parametrize("M,N,K,ks", SHAPES)
def test_tier_b_budgets(C, M, N, K, ks):
    c = randn_case(M, N, K, "nt")
    splits = C.linear_skinny_splits(M, N, K, ks)
    assert splits >= 4 and splits % 4 == 0
    worst = {}
    r = gemm_ref(c["A"], c["B"], "nt", bias=c["bias"])
    y = run(C, c, bias=True, ksplit=ks)
    worst["bf16"] = ((y.double() - r["y"]).abs() / b_bf16(r["y"], r["mag"], K, splits)).max().item()
    g, bound = b_gelu(r["y"], r["mag"], K, splits)
    y = run(C, c, bias=True, gelu=True, ksplit=ks)
    worst["gelu"] = ((y.double() - g).abs() / bound).max().item()
    r = gemm_ref(c["A"], c["B"], "nt", bias=c["bias"], residual=c["res"])
    y = run(C, c, bias=True, out_f32=True, res=c["res"], alias=True, ksplit=ks)
    worst["f32"] = ((y.double() - r["y"]).abs() / b_f32(r["mag"], K, splits)).max().item()
    print(f"linear_skinny M={M} N={N} K={K} splits={splits}: " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst


def test_default_plan_splits_k_on_the_gpt2_row(C):
    assert C.linear_skinny_splits(8, 768, 3072) > 4      # blocks along K: 48 column tiles alone leave most CUs idle
    assert C.linear_skinny_splits(8, 50304, 768) == 4    # the LM head has tiles enough


@pytest.mark.parametrize("N,K", [(16, 40), (24, 32)])
def test_envelope(C, N, K):
    """Outside the envelope the binding raises; Fx.linear_skinny then runs Fx.linear / Fx.linear_residual."""
    from distributed_pytorch_example_amd.ops import functional as Fx

    c = randn_case(5, N, K, "nt")
    with pytest.raises(RuntimeError, match="envelope"):
        C.linear_skinny(c["A"].to(dev()), c["B"].to(dev()))
    with pytest.raises(RuntimeError, match="envelope"):
        C.linear_skinny(torch.zeros(17, 32, dtype=torch.bfloat16, device=dev()), torch.zeros(16, 32, dtype=torch.bfloat16, device=dev()))
    w = torch.nn.Parameter(c["B"].float().to(dev()))
    bias = c["bias"].to(dev())
    r = gemm_ref(c["A"], c["B"], "nt", bias=c["bias"])
    y = Fx.linear_skinny(c["A"].to(dev()), w, bias)
    assert y.dtype == torch.bfloat16
    assert ((y.cpu().double() - r["y"]).abs() / b_bf16(r["y"], r["mag"], K, 4)).max().item() <= 1.0
    r = gemm_ref(c["A"], c["B"], "nt", bias=c["bias"], residual=c["res"])
    y = Fx.linear_skinny(c["A"].to(dev()), w, bias, residual=c["res"].to(dev()))
    assert y.dtype == torch.float32
    assert ((y.cpu().double() - r["y"]).abs() / b_f32(r["mag"], K, 4)).max().item() <= 1.0


def test_wrapper_in_envelope_uses_the_kernel_and_updates_the_residual_in_place(C):
    from distributed_pytorch_example_amd.ops import functional as Fx

    c = int_case(5, 48, 160, "nt", "f32")
    w = torch.nn.Parameter(c["B"].float().to(dev()))
    res = c["res"].to(dev()).clone()
    y = Fx.linear_skinny(c["A"].to(dev()), w, c["bias"].to(dev()), residual=res)
    assert y.data_ptr() == res.data_ptr()
    assert torch.equal(y.cpu().double(), gemm_ref(c["A"], c["B"], "nt", bias=c["bias"], residual=c["res"])["y"])
    # the LM head's zero pad rows: 48 real rows padded to 64
    y = Fx.linear_skinny(c["A"].to(dev()), w, pad_rows=16)
    assert y.shape == (5, 64) and (y[:, 48:] == 0).all()


@pytest.mark.parametrize("M", [5, 9, 16])
def test_wide_n_four_tiles_per_block(C, M):
    """N / 64 >= 512 with M >= 8 takes the kernel with four column tiles per block (the LM head's plan; M = 5 stays on
    one tile per block at the same width): N = 64 * 513, K = 96 (three
    K chunks: one wave of the four has none).  Small integers, so fp32 and bf16 outputs are exact; then randn under
    the Tier B budgets."""
    N, K = 64 * 513, 96
    g = torch.Generator().manual_seed(M)
    c = dict(M=M, N=N, K=K, A=torch.randint(-1, 2, (M, K), generator=g).to(torch.bfloat16),
             B=torch.randint(-2, 3, (N, K), generator=g).to(torch.bfloat16), bias=torch.randint(-4, 5, (N,), generator=g).float(),
             res=torch.randint(-64, 65, (M, N), generator=g).float())
    assert C.linear_skinny_splits(M, N, K) == 4
    ref = gemm_ref(c["A"], c["B"], "nt", bias=c["bias"])
    assert ref["y"].abs().max().item() <= 256 and len(torch.unique(ref["y"])) > 50
    assert torch.equal(run(C, c, bias=True).double(), ref["y"])
    assert torch.equal(run(C, c, bias=True, out_f32=True, res=c["res"], alias=True).double(), ref["y"] + c["res"].double())
    c = dict(randn_case(M, 48, K, "nt"))  # (the cached case's x and bias shape; a wide w of its own)
    c.update(N=N, B=(torch.randn(N, K, generator=g) / K ** 0.5).to(torch.bfloat16), bias=torch.randn(N, generator=g))
    r = gemm_ref(c["A"], c["B"], "nt", bias=c["bias"])
    worst = ((run(C, c, bias=True).double() - r["y"]).abs() / b_bf16(r["y"], r["mag"], K, 4)).max().item()
    gref, gb = b_gelu(r["y"], r["mag"], K, 4)
    worst_g = ((run(C, c, bias=True, gelu=True).double() - gref).abs() / gb).max().item()
    print(f"linear_skinny wide N={N} M={M}: bf16 {worst:.3f}  gelu {worst_g:.3f}")
    assert worst <= 1.0 and worst_g <= 1.0
