"""A training step with the BatchMixer: the fused path (device draw, mix inside the pack, two-label CE) against
torch-mixed images through the plain path, and train_epoch without a mixer against the step as it was."""
import copy

import pytest
import torch

from distributed_pytorch_example_amd.data import BatchMixer
from distributed_pytorch_example_amd.models import get_model
from distributed_pytorch_example_amd.ops import functional as Fx
from distributed_pytorch_example_amd.optim import SGD
from distributed_pytorch_example_amd.train import train_epoch

pytestmark = pytest.mark.gpu
dev = "cuda"


def _tiny(seed=1):
    """resnet_tiny with the classifier's weights scaled by 8: at initialisation every loss is ln 10 otherwise, and a
    mixed and an unmixed loss could not be told apart."""
    torch.manual_seed(seed)
    m = get_model("resnet_tiny")
    with torch.no_grad():
        m.fc.weight.mul_(8.0)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(8, 3, 32, 32, generator=g)
    y = torch.randint(0, 10, (8,), generator=g)
    return m.to(dev), x.to(dev), y.to(dev)


@pytest.mark.parametrize("kw", [dict(mixup_alpha=50.0), dict(cutmix_alpha=50.0)], ids=["mixup", "cutmix"])
def test_fused_mixed_step_matches_torch_mixed_plain_path(C, kw):
    """alpha = 50: lam is 0.5 +- 0.05, whatever the seed, so the mixed loss is far from the unmixed one."""
    model, x, y = _tiny()
    ref = copy.deepcopy(model)
    a, b = (BatchMixer(device=dev, **kw).manual_seed(21) for _ in range(2))
    # the fused path, as train_epoch runs it
    data, (t, t2, w) = a(x, y)
    assert data.dtype == torch.bfloat16 and data.shape == (8, 16, 16, 16) and w.shape == (1,)
    loss = Fx.cross_entropy(model(data), t, 10, label_smoothing=0.1, labels2=t2, mix_w=w)
    loss.backward()
    # the comparison: the same row, torch-mixed fp32 images, two plain losses combined
    row = b.draw(32, 32)[0]
    assert torch.equal(row[1:2], w) and int(row[6]) in (1, 2)
    out = ref(BatchMixer.mix_torch(x, row))
    lw = row[1]
    loss_ref = lw * Fx.cross_entropy(out, y, 10, label_smoothing=0.1) + (1 - lw) * Fx.cross_entropy(out, y.roll(1, 0), 10,
                                                                                                  label_smoothing=0.1)
    loss_ref.backward()
    plain = Fx.cross_entropy(copy.deepcopy(ref)(x), y, 10, label_smoothing=0.1)
    rel = abs(loss.item() - loss_ref.item()) / abs(loss_ref.item())
    gap = abs(plain.item() - loss_ref.item()) / abs(loss_ref.item())
    print(f"{kw}: row {row.tolist()} fused {loss.item():.6f} torch-mixed {loss_ref.item():.6f} (rel {rel:.2e}) "
          f"unmixed {plain.item():.6f} (gap {gap:.2e})")
    assert rel < 1e-3
    assert gap > 1e-2
    gf, gr = model.fc.weight.grad.float(), ref.fc.weight.grad.float()
    assert ((gf - gr).norm() / gr.norm()).item() < 2e-2  # the same gradient through both loss forms


def _loader(x, y, steps):
    return [(x, y)] * steps


def test_train_epoch_with_mixer_runs_and_differs(C):
    model, x, y = _tiny()
    base = copy.deepcopy(model)
    opt = SGD(model.parameters(), lr=0.01, momentum=0.9)

    def criterion(out, tgt):
        if isinstance(tgt, tuple):
            return Fx.cross_entropy(out, tgt[0], 10, labels2=tgt[1], mix_w=tgt[2])
        return Fx.cross_entropy(out, tgt, 10)

    mixer = BatchMixer(mixup_alpha=50.0, device=dev).manual_seed(3)
    loss = train_epoch(model, _loader(x, y, 2), opt, criterion, torch.device(dev), 0, 1, mixer=mixer)
    assert loss == loss and loss > 0
    assert mixer.rng.tensor().tolist() == [3, 2]  # one draw per step, on the device
    assert any(not torch.equal(p, q) for p, q in zip(model.parameters(), base.parameters()))


def _manual_step(model, opt, x, y, num_classes):
    """train_epoch's step as it was before it took a mixer."""
    model.train()
    loss = Fx.cross_entropy(model(x), y, num_classes)
    loss.backward()
    opt.step()
    opt.zero_grad()
    return loss.detach().double().item()


def test_without_a_mixer_the_step_is_what_it_was(C):
    """mixer=None: loss and updated weights bitwise those of the step written out by hand.  Weights are compared on
    SimpleNet, whose kernels sum in a fixed order; ResNet's weight gradients go through float atomics, so there the
    loss (forward only) is the bitwise check."""
    from distributed_pytorch_example_amd.optim import Adam

    def crit(nc):
        return lambda out, tgt: Fx.cross_entropy(out, tgt, nc)

    torch.manual_seed(4)
    s1 = get_model("simplenet").to(dev)
    s1.layers[2].p = s1.layers[5].p = 0.0  # no dropout: the two steps would draw different masks
    s2 = copy.deepcopy(s1)
    xs, ys = torch.randn(64, 784, device=dev), torch.randint(0, 10, (64,), device=dev)
    o1, o2 = Adam(s1.parameters(), lr=1e-3), Adam(s2.parameters(), lr=1e-3)
    l1 = train_epoch(s1, _loader(xs, ys, 1), o1, crit(10), torch.device(dev), 0, 1, mixer=None)
    l2 = _manual_step(s2, o2, xs, ys, 10)
    assert l1 == l2
    for p, q in zip(s1.parameters(), s2.parameters()):
        assert torch.equal(p, q)

    model, x, y = _tiny()
    ref = copy.deepcopy(model)
    l1 = train_epoch(model, _loader(x, y, 1), SGD(model.parameters(), lr=0.01), crit(10), torch.device(dev), 0, 1, mixer=None)
    l2 = _manual_step(ref, SGD(ref.parameters(), lr=0.01), x, y, 10)
    assert l1 == l2
