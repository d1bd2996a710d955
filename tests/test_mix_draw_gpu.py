"""mix_draw_kernel: continuity of the counter, the box invariants, the distributions of everything it draws, and
the draw + mix_pack pair under graph replay."""
import numpy as np
import pytest
import torch

import _mix_ref as R
from distributed_pytorch_example_amd.data import BatchMixer
from distributed_pytorch_example_amd.ops import functional as Fx

pytestmark = pytest.mark.gpu
dev = "cuda"
N = 8192
H, W = 224, 160


def _mixer(seed, **kw):
    return BatchMixer(device=dev, **kw).manual_seed(seed)


def test_count_rows_are_consecutive_single_draws():
    kw = dict(mixup_alpha=0.2, cutmix_alpha=1.0, prob=0.9)
    a, b = _mixer(11, **kw), _mixer(11, **kw)
    four = a.draw(H, W, count=4)
    singles = torch.cat([b.draw(H, W) for _ in range(4)])
    assert four.shape == (4, 8) and torch.equal(four, singles)
    assert a.rng.tensor().tolist() == [11, 4] == b.rng.tensor().tolist()
    assert torch.equal(a.draw(H, W, count=3), torch.cat([b.draw(H, W) for _ in range(3)]))  # and from offset 4 on
    assert len({tuple(r) for r in four.tolist()}) == 4
    # more rows than the block has threads, and another stream: other rows
    big = _mixer(11, **kw).draw(H, W, count=600)
    assert torch.equal(big[:4], four) and torch.equal(big[597:], _mixer(11, **kw).manual_seed(11, 597).draw(H, W, count=3))
    assert not torch.equal(BatchMixer(device=dev, stream=5, **kw).manual_seed(11).draw(H, W, count=4), four)


@pytest.fixture(scope="module")
def rows():
    """8192 rows at prob 0.7, switch_prob 0.25, both modes on (one launch, shared by the tests below)."""
    return _mixer(2024, mixup_alpha=0.2, cutmix_alpha=1.0, prob=0.7, switch_prob=0.25).draw(H, W, count=N).cpu()


def test_box_invariants(rows):
    r = rows.double().numpy()
    mode = r[:, 6]
    assert set(np.unique(mode)) == {0.0, 1.0, 2.0}
    lam = r[:, 7]
    assert np.all((lam >= 0) & (lam <= 1))
    x1, y1, x2, y2 = r[:, 2], r[:, 3], r[:, 4], r[:, 5]
    assert np.all(r[:, 2:6] == np.floor(r[:, 2:6]))
    assert np.all((0 <= x1) & (x1 <= x2) & (x2 <= W) & (0 <= y1) & (y1 <= y2) & (y2 <= H))
    none, mixup, cut = mode == 0, mode == 1, mode == 2
    assert np.all(r[none][:, :7] == np.array([1, 1, 0, 0, 0, 0, 0.0]))
    assert np.all(r[mixup][:, 2:6] == 0) and np.all(r[mixup, 0] == lam[mixup]) and np.all(r[mixup, 1] == lam[mixup])
    assert np.all(r[cut, 0] == 1)
    # w_lab = 1 - area / (H W) to one fp32 ulp of the value
    want = 1.0 - (x2 - x1) * (y2 - y1) / float(H * W)
    ulp = np.spacing(np.abs(want[cut]).astype(np.float32)).astype(np.float64)
    assert np.all(np.abs(r[cut, 1] - want[cut]) <= ulp)
    # half sizes within one pixel of the fp64 formula on the row's lam_raw (an unclamped side shows the half size)
    hw, hh = R.half_sizes(lam, H, W)
    both_x = cut & (x1 > 0) & (x2 < W)
    both_y = cut & (y1 > 0) & (y2 < H)
    assert both_x.sum() > 100 and both_y.sum() > 100
    assert np.all(np.abs((x2 - x1)[both_x] / 2 - hw[both_x]) <= 1) and np.all((x2 - x1)[both_x] % 2 == 0)
    assert np.all(np.abs((y2 - y1)[both_y] / 2 - hh[both_y]) <= 1) and np.all((y2 - y1)[both_y] % 2 == 0)
    assert np.all((x2 - x1)[cut] <= 2 * hw[cut] + 2) and np.all((y2 - y1)[cut] <= 2 * hh[cut] + 2)


def test_mode_frequencies(rows):
    mode = rows[:, 6].numpy()
    for m, p in ((0, 0.3), (1, 0.7 * 0.75), (2, 0.7 * 0.25)):
        f = float((mode == m).mean())
        print(f"mode {m}: frequency {f:.4f}, expected {p:.4f}")
        assert abs(f - p) <= 0.03


@pytest.mark.parametrize("alpha", [0.2, 1.0, 2.0])
def test_lam_is_beta(alpha):
    lam = _mixer(77, mixup_alpha=alpha).draw(H, W, count=N)[:, 7].double().cpu().numpy()
    d = R.check_lam_sample(lam, alpha)  # sup |F_n - F| <= 0.03 against the exact Beta(alpha, alpha) CDF
    print(f"alpha {alpha}: sup |F_n - F| = {d:.4f}, mean {lam.mean():.4f}")


def test_box_centres_are_uniform():
    """r_x and r_y, recovered from the rows: the midpoint of a box no side of which is clamped, else the unclamped side
    minus / plus the half size (cutmix_alpha = 1: lam uniform, independent of the centre)."""
    r = _mixer(78, cutmix_alpha=1.0).draw(H, W, count=N).double().cpu().numpy()
    assert np.all(r[:, 6] == 2)
    hw, hh = R.half_sizes(r[:, 7], H, W)

    def centre(lo, hi, half, size):
        c = np.where(lo > 0, lo + half, hi - half)          # one side clamped: from the other one
        c = np.where((lo > 0) & (hi < size), (lo + hi) / 2, c)
        known = (lo > 0) | (hi < size)
        return c[known], known.mean()

    for lo, hi, half, size, name in ((r[:, 2], r[:, 4], hw, W, "r_x"), (r[:, 3], r[:, 5], hh, H, "r_y")):
        c, share = centre(lo, hi, half, size)
        assert share > 0.999
        c = np.clip(np.rint(c), 0, size - 1)
        d = R.ks_sup_discrete(c, size)
        print(f"{name}: sup |F_n - F| = {d:.4f} over {len(c)} rows")
        assert d <= 0.03


def test_graph_replay_draws_anew():
    """draw + mix_pack captured once (one stream) and replayed three times: three different rows, bitwise the rows and
    the packed batches of three eager calls from the same seed."""
    kw = dict(mixup_alpha=1.0, cutmix_alpha=1.0)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(3, 3, 8, 12, generator=g).to(dev)

    def step(m):
        row = m.draw(8, 12)[0]
        return row, Fx.mix_pack(x, row, "s2d")

    eager = _mixer(5, **kw)
    want = [tuple(t.clone() for t in step(eager)) for _ in range(4)]  # the warm-up call and three steps
    m = _mixer(5, **kw)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step(m)  # warm-up outside the capture: want[0]
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        row, xo = step(m)
    got = []
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        got.append((row.clone(), xo.clone()))
    for (gr, gx), (wr, wx) in zip(got, want[1:]):
        assert torch.equal(gr, wr) and torch.equal(gx, wx)
    assert len({tuple(gr.tolist()) for gr, _ in got}) == 3
    assert m.rng.tensor().tolist() == [5, 4]
    assert got[0][1].shape == Fx.to_s2d_input(x).shape
