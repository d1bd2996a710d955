"""The attention mode matrix as one table over C.attn_route (dpe_attn_route, csrc/kernels/attn.hip): which kernel
family -- 'dma' (LDS-DMA), 'staged' (register-staged), 'gqa' -- serves a call, and which calls are refused ('none', with
a reason that names the offending argument).  The route is integer arithmetic on the host: no tensor, no GPU call, so
the 2^31-byte boundary between the LDS-DMA and the register-staged kernels is tested here without a 2 GiB tensor.
Needs the built extension, not a GPU."""
import pytest

from distributed_pytorch_example_amd.ops._ext import ext, has_ext

pytestmark = pytest.mark.skipif(not has_ext(), reason="native extension not built")

T, H = 256, 4

# (case, attn_route keywords besides T and H, set_attn_staged, expected route, what the reason names)
MATRIX = [
    ("plain", {}, False, "dma", ""),
    ("plain_staged", {}, True, "staged", ""),
    ("packed", dict(packed=True), False, "dma", ""),
    ("dropout", dict(dropout=True), False, "dma", ""),
    ("dropout_packed", dict(dropout=True, packed=True), False, "dma", ""),
    ("bidir", dict(causal=False), False, "dma", ""),
    ("bidir_seq_len", dict(causal=False, seq_len=100), False, "dma", ""),
    ("bidir_seq_len_T", dict(causal=False, seq_len=T), False, "dma", ""),
    ("gqa", dict(n_kv_head=2), False, "gqa", ""),
    ("gqa_packed", dict(n_kv_head=2, packed=True), False, "gqa", ""),
    ("gqa_one_kv_head", dict(n_kv_head=1), False, "gqa", ""),
    ("gqa_all_heads", dict(n_kv_head=H), False, "gqa", ""),
    # the register-staged kernels are plain causal only
    ("packed_staged", dict(packed=True), True, "none", "doc_start"),
    ("dropout_staged", dict(dropout=True), True, "none", "dropout"),
    ("bidir_staged", dict(causal=False), True, "none", "causal=False"),
    ("gqa_staged", dict(n_kv_head=2), True, "none", "n_kv_head"),
    # shapes
    ("D_32", dict(D=32), False, "none", "head dim"),
    ("D_128_gqa", dict(D=128, n_kv_head=2), False, "none", "head dim"),
    ("T_100", dict(T=100), False, "none", "T "),
    ("T_65_bidir", dict(T=65, causal=False), False, "none", "T "),
    ("T_96_gqa", dict(T=96, n_kv_head=2), False, "none", "T "),
    # seq_len
    ("seq_len_causal", dict(seq_len=100), False, "none", "seq_len"),
    ("seq_len_negative", dict(causal=False, seq_len=-1), False, "none", "seq_len"),
    ("seq_len_past_T", dict(causal=False, seq_len=T + 1), False, "none", "seq_len"),
    # the bidirectional mask combines with nothing
    ("bidir_packed", dict(causal=False, packed=True), False, "none", "doc_start"),
    ("bidir_dropout", dict(causal=False, dropout=True), False, "none", "dropout"),
    # grouped K / V heads: causal, with or without packed documents
    ("gqa_not_dividing", dict(n_kv_head=3), False, "none", "n_kv_head"),
    ("gqa_more_than_H", dict(n_kv_head=2 * H), False, "none", "n_kv_head"),
    ("gqa_negative", dict(n_kv_head=-1), False, "none", "n_kv_head"),
    ("gqa_dropout", dict(n_kv_head=2, dropout=True), False, "none", "dropout"),
    ("gqa_seq_len", dict(n_kv_head=2, seq_len=100), False, "none", "seq_len"),
    ("gqa_bidir", dict(n_kv_head=2, causal=False), False, "none", "causal"),
]


def _route(kw, staged=False):
    C = ext()
    kw = dict(kw)
    prev = C.set_attn_staged(staged)
    try:
        return C.attn_route(kw.pop("T", T), kw.pop("H", H), **kw)
    finally:
        C.set_attn_staged(prev)


@pytest.mark.parametrize("case,kw,staged,route,names", MATRIX, ids=[m[0] for m in MATRIX])
def test_mode_matrix(case, kw, staged, route, names):
    got, why = _route(kw, staged)
    assert got == route, f"{case}: {got} ({why})"
    if route == "none":
        assert why.startswith("attn: ") and names in why, why
    else:
        assert why == ""


# One sequence's qkv rows, T * row width * 64 * 2 bytes, must stay below 2^31 for the LDS-DMA kernels' 32-bit buffer
# range.  With H = 1 the row width is 3 in both layouts ([3, H] and H + 2 * n_kv_head with one K / V head).
T_FITS, T_OVER = 5592384, 5592448
MODES = [("plain", {}), ("packed", dict(packed=True)), ("dropout", dict(dropout=True)), ("bidir", dict(causal=False)),
         ("gqa", dict(n_kv_head=1))]


def test_boundary_arithmetic():
    assert T_FITS % 64 == 0 and T_OVER == T_FITS + 64
    assert T_FITS * 3 * 64 * 2 == 2147475456 < 2 ** 31 <= T_OVER * 3 * 64 * 2 == 2147500032


@pytest.mark.parametrize("mode,kw", MODES, ids=[m[0] for m in MODES])
def test_last_T_below_2GiB_takes_the_dma_kernels(mode, kw):
    assert _route(dict(kw, T=T_FITS, H=1)) == ("gqa" if mode == "gqa" else "dma", "")


@pytest.mark.parametrize("mode,kw", MODES, ids=[m[0] for m in MODES])
def test_first_T_at_2GiB_is_staged_or_refused(mode, kw):
    got, why = _route(dict(kw, T=T_OVER, H=1))
    if mode == "plain":
        assert (got, why) == ("staged", "")
    else:
        assert got == "none" and "LDS-DMA kernels only" in why, (got, why)


def test_row_width_counts_the_kv_heads():
    """GQA rows are H + 2 * n_kv_head heads wide, not 3 * H: at a T where 8 + 2 * 2 = 12 heads fit, 3 * 8 = 24 do not."""
    T12 = (2 ** 31 // (12 * 128)) // 64 * 64
    assert T12 * 12 * 128 < 2 ** 31 <= T12 * 24 * 128
    assert _route(dict(T=T12, H=8, n_kv_head=2))[0] == "gqa"
    assert _route(dict(T=T12, H=8, n_kv_head=8))[0] == "none"
    assert _route(dict(T=T12, H=8))[0] == "staged"


def test_route_leaves_the_staged_switch_alone():
    C = ext()
    prev = C.set_attn_staged(False)
    try:
        C.attn_route(T, H)
        assert C.set_attn_staged(False) is False
    finally:
        C.set_attn_staged(prev)
