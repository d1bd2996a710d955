"""Mixup / CutMix with the mixing decision drawn on the device (README, "Batch mixing").

One decision per batch, as torchvision's ``v2.MixUp`` / ``v2.CutMix``: a device fp32 row
``[w_pix, w_lab, x1, y1, x2, y2, mode, lam_raw]`` (mode 0 none, 1 mixup, 2 cutmix; box ``[y1:y2, x1:x2]``).
On the GPU the row comes from ``mix_draw_kernel`` and is only ever read by kernels -- the mix itself happens inside
the pass that packs the batch for the stem (``Fx.mix_pack``) and the loss takes the label weight as a view of the
row -- so a step captured in a HIP graph draws anew on every replay.
"""
from __future__ import annotations

import math

import torch

from ..ops import functional as Fx
from ..ops._ext import ext

MODE_NONE, MODE_MIXUP, MODE_CUTMIX = 0, 1, 2
# Philox counter_lo of the draws: no dropout call site uses it (they count up from 0)
MIX_STREAM = 0x4D495800


def cutmix_box(lam: float, r_x: int, r_y: int, H: int, W: int):
    """torchvision's box for a centre ``(r_x, r_y)``: half sizes ``int(0.5 sqrt(1 - lam) W)`` and ``... H``, clamped
    to the image.  Returns ``(x1, y1, x2, y2)``."""
    r = 0.5 * math.sqrt(max(0.0, 1.0 - lam))
    hw, hh = int(r * W), int(r * H)
    return max(r_x - hw, 0), max(r_y - hh, 0), min(r_x + hw, W), min(r_y + hh, H)


class BatchMixer:
    """``x, (y, y2, w) = mixer(x, y)``: the batch mixed with ``x.roll(1, 0)``, the partner's labels and the weight of
    ``y`` (a one-element view of the decision row), for ``Fx.cross_entropy(out, y, ..., labels2=y2, mix_w=w)``.

    ``mixup_alpha`` / ``cutmix_alpha``: the Beta parameters (0: that mode is off); ``prob``: the probability of mixing
    a batch at all; ``switch_prob``: the probability of cutmix when both modes are on.  The RNG state is a
    ``DropoutState`` of the mixer's own (seeded by ``DropoutState.default_seed()``: DDP ranks draw differently;
    ``manual_seed`` reseeds it; it is not checkpointed) that advances by one per drawn row, on the device.  On the CPU
    torch's generator draws instead."""

    def __init__(self, mixup_alpha: float = 0.0, cutmix_alpha: float = 0.0, prob: float = 1.0, switch_prob: float = 0.5,
                 device="cpu", stream: int = MIX_STREAM):
        if not (mixup_alpha >= 0.0 and cutmix_alpha >= 0.0):
            raise ValueError(f"mixup_alpha and cutmix_alpha must be >= 0, got {mixup_alpha}, {cutmix_alpha}")
        if not (0.0 <= prob <= 1.0 and 0.0 <= switch_prob <= 1.0):
            raise ValueError(f"prob and switch_prob must be in [0, 1], got {prob}, {switch_prob}")
        if not 0 <= int(stream) <= 0xFFFFFFFF:
            raise ValueError("stream must fit 32 bits")
        self.mixup_alpha, self.cutmix_alpha = float(mixup_alpha), float(cutmix_alpha)
        self.prob, self.switch_prob = float(prob), float(switch_prob)
        self.device = torch.device(device)
        self.stream = int(stream)
        self.rng = Fx.DropoutState(self.device)

    @property
    def enabled(self) -> bool:
        return (self.mixup_alpha > 0.0 or self.cutmix_alpha > 0.0) and self.prob > 0.0

    def manual_seed(self, seed: int, offset: int = 0) -> "BatchMixer":
        self.rng.manual_seed(seed, offset)
        return self

    # ------------------------------------------------------------------ draw
    def draw(self, H: int, W: int, count: int = 1) -> torch.Tensor:
        """``count`` decision rows ``[count, 8]`` for ``H x W`` images (``H = W = 1`` for non-image inputs, whose rows
        are only valid in the modes none and mixup).  Row ``i`` of one call is the row of the ``i``-th of ``count``
        single draws: the state advances by ``count``."""
        if self.device.type == "cuda":
            out = ext().mix_draw(self.rng.tensor(), self.stream, int(H), int(W), self.mixup_alpha, self.cutmix_alpha,
                                 self.prob, self.switch_prob, int(count))
            self.rng.advance(int(count))
            return out
        return torch.stack([self._draw_cpu(int(H), int(W)) for _ in range(int(count))])

    def _draw_cpu(self, H: int, W: int) -> torch.Tensor:
        row = torch.tensor([1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])
        if not self.enabled or not float(torch.rand(())) < self.prob:
            return row
        if self.mixup_alpha > 0.0 and self.cutmix_alpha > 0.0:
            mode = MODE_CUTMIX if float(torch.rand(())) < self.switch_prob else MODE_MIXUP
        else:
            mode = MODE_MIXUP if self.mixup_alpha > 0.0 else MODE_CUTMIX
        alpha = self.cutmix_alpha if mode == MODE_CUTMIX else self.mixup_alpha
        a = torch.tensor(alpha, dtype=torch.float64)
        lam = float(torch.distributions.Beta(a, a).sample())
        row[6], row[7] = float(mode), lam
        if mode == MODE_MIXUP:
            row[0] = row[1] = lam
        else:
            r_x, r_y = int(torch.randint(W, ())), int(torch.randint(H, ()))
            x1, y1, x2, y2 = cutmix_box(lam, r_x, r_y, H, W)
            row[1] = 1.0 - (x2 - x1) * (y2 - y1) / float(H * W)
            row[2], row[3], row[4], row[5] = float(x1), float(y1), float(x2), float(y2)
        return row

    # ------------------------------------------------------------------- mix
    @staticmethod
    def mix_torch(x: torch.Tensor, row: torch.Tensor) -> torch.Tensor:
        """The pixel rule in torch ops that read the row where it lives (no host copy of it): for 4-D image batches
        the box as a mask, for everything else the blend alone."""
        xp = x.roll(1, 0)
        w = row[0].to(x.dtype if x.is_floating_point() else torch.float32)
        out = torch.lerp(xp, x, w)  # w x + (1 - w) x_partner
        if x.dim() == 4:
            H, W = x.shape[-2:]
            ys = torch.arange(H, device=x.device, dtype=row.dtype)[:, None]
            xs = torch.arange(W, device=x.device, dtype=row.dtype)[None, :]
            inside = (ys >= row[3]) & (ys < row[5]) & (xs >= row[2]) & (xs < row[4])
            out = torch.where(inside, xp, torch.where(w == 1, x, out))
        return out

    def __call__(self, x: torch.Tensor, target: torch.Tensor, layout: str = "s2d", cpad: int = 8):
        """``(x_out, (target, target.roll(1, 0), w_lab))``.  A 4-D NCHW fp32 batch on the GPU comes back packed for the
        stem (``layout`` "s2d": ``Fx.to_s2d_input``'s form, "nhwc": ``Fx.to_nhwc_input``'s with ``cpad``) by the one
        kernel that also mixes; any other input is mixed by torch ops (mixup only unless it is an image batch)."""
        image = x.dim() == 4
        if not image and self.cutmix_alpha > 0.0:
            raise ValueError("cutmix needs an NCHW image batch; use mixup (cutmix_alpha = 0) for other inputs")
        H, W = (x.shape[-2], x.shape[-1]) if image else (1, 1)
        row = self.draw(H, W)[0].to(x.device)
        if x.is_cuda and image and x.dtype == torch.float32 and (layout != "s2d" or (x.shape[1] <= 4 and H % 2 == 0 and W % 2 == 0)):
            x_out = Fx.mix_pack(x, row, layout, cpad)
        else:
            x_out = self.mix_torch(x, row)
        return x_out, (target, target.roll(1, 0), row[1:2])
