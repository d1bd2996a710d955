"""Autograd-level ops.  GPU tensors -> hand-written gfx950 kernels (``_C``);
CPU tensors -> torch reference math with identical semantics (the CPU/gloo
configuration of the reference, and the reference used by the numerics tests).

Activation layout convention: convolutional activations are NHWC
(``[N, H, W, C]``); on the GPU they are bf16.  Conv weights are stored
``[Cout, R, S, Cin]`` (OHWI) so the forward implicit GEMM reads them K-contiguous.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import torch
import torch.nn.functional as F
from torch.autograd import Function

from ._ext import ext
from ._state import grad_done, grad_fresh, grad_sink, note_use, shadow

ACT_NONE, ACT_RELU, ACT_GELU = 0, 1, 2

# CPU reference path: optionally round activations (forward) and their
# gradients (backward) to bf16 at the same points the GPU kernels do, so the
# GPU path can be validated against a reference with identical rounding
# points (tests) instead of against pure fp32.
EMULATE_BF16 = False


class _RoundBF16(Function):
    @staticmethod
    def forward(ctx, x):
        return x.to(torch.bfloat16).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).to(g.dtype)


def _emu(x):
    return _RoundBF16.apply(x) if EMULATE_BF16 else x


def _emu_w(w):
    return w.to(torch.bfloat16).to(w.dtype) if EMULATE_BF16 else w


def _pad8(n: int) -> int:
    return (n + 7) // 8 * 8


# ===================================================================== Linear
class _LinearFn(Function):
    """bf16 Linear on the MFMA GEMMs.  Output widths that are not a multiple of 8 (SimpleNet's
    10-class head) run on the bf16 shadow padded to Np = pad8(N) rows: bias (zero-padded) and ReLU
    stay in the GEMM epilogue, the backward pads dy once (F.pad, one kernel) and the weight grad
    writes only the N real rows into the gradient buffer, with the bias grad from the same launch."""

    @staticmethod
    def forward(ctx, x, weight, bias, act: int, out_f32: bool):
        C = ext()
        N = weight.shape[0]
        Np = _pad8(N)
        w16 = shadow(weight, Np - N)
        xb = x if x.dtype == torch.bfloat16 else x.to(torch.bfloat16)
        xb = xb.contiguous()
        if Np != N:
            bpad = F.pad(bias.detach(), (0, Np - N)) if bias is not None else None
            y = C.linear_fwd(xb, w16, bpad, act, out_f32)[..., :N].contiguous()
        else:
            y = C.linear_fwd(xb, w16, bias.detach() if bias is not None else None, act, out_f32)
        ctx.save_for_backward(xb, y if act != ACT_NONE else None)
        ctx.weight, ctx.bias, ctx.act, ctx.N, ctx.Np = weight, bias, act, N, Np
        ctx.x_dtype = x.dtype
        note_use(weight)
        if bias is not None:
            note_use(bias)
        return y

    @staticmethod
    def backward(ctx, dy):
        C = ext()
        xb, y = ctx.saved_tensors
        weight, bias, act, N, Np = ctx.weight, ctx.bias, ctx.act, ctx.N, ctx.Np
        dy = dy.to(torch.bfloat16) if dy.dtype != torch.bfloat16 else dy
        if act == ACT_RELU:
            dy = C.act(dy.contiguous(), y.to(torch.bfloat16).contiguous() if y.dtype != torch.bfloat16 else y.contiguous(), 1)
        dy = dy.contiguous()
        dyp = F.pad(dy, (0, Np - N)) if Np != N else dy  # zero pad columns: the GEMMs' 16-B rows
        dx = None
        if ctx.needs_input_grad[0]:
            dx = C.linear_dgrad(dyp, shadow(weight, Np - N))
            if ctx.x_dtype != torch.bfloat16:
                dx = dx.to(ctx.x_dtype)
        want_b = bias is not None and ctx.needs_input_grad[2]
        bbuf, bdirect = grad_sink(bias) if want_b else (None, False)
        gw = None
        if ctx.needs_input_grad[1]:
            buf, direct = grad_sink(weight)
            # column-padded dy: only the N real rows of dW (and of db) are written
            C.linear_wgrad(dyp, xb, buf, 1.0, None, bbuf, 0, direct and grad_fresh(weight))
            grad_done(weight, direct)
            gw = None if direct else buf
        elif want_b:
            C.colsum(dy, bbuf, True)
        gb = None
        if want_b:
            grad_done(bias, bdirect)
            gb = None if bdirect else bbuf
        return dx, gw, gb, None, None


def linear(x, weight, bias=None, act: int = ACT_NONE, out_f32: bool = False):
    if not x.is_cuda:
        xin = _emu(x.float() if x.dtype != weight.dtype else x)
        w = weight + (_emu_w(weight) - weight).detach() if EMULATE_BF16 else weight
        y = F.linear(xin, w, bias)
        if act == ACT_RELU:
            y = F.relu(y)
        elif act == ACT_GELU:
            y = F.gelu(y, approximate="tanh")
        return y if out_f32 else _emu(y)
    if act == ACT_GELU:
        return gelu(_LinearFn.apply(x, weight, bias, ACT_NONE, out_f32))
    return _LinearFn.apply(x, weight, bias, act, out_f32)


# ============================================================ activations
class _ActFn(Function):
    @staticmethod
    def forward(ctx, x, op: int):
        C = ext()
        xc = x.contiguous()
        y = C.act(xc, None, op)
        ctx.op = op
        ctx.save_for_backward(y if op == 0 else xc)
        return y

    @staticmethod
    def backward(ctx, dy):
        (s,) = ctx.saved_tensors
        dy = dy.contiguous().to(s.dtype)
        return ext().act(dy, s, 1 if ctx.op == 0 else 3), None


def relu(x):
    if not x.is_cuda:
        return F.relu(x)
    return _ActFn.apply(x, 0)


def gelu(x):
    if not x.is_cuda:
        return F.gelu(x, approximate="tanh")
    return _ActFn.apply(x, 2)


class _RNG:
    """Counter-based dropout RNG stream: (seed, offset) -> Philox; mask regenerated in backward."""

    seed = None
    offset = 0

    @classmethod
    def next(cls, n: int):
        if cls.seed is None:
            cls.seed = int(torch.initial_seed()) & 0xFFFFFFFFFFFF
        off = cls.offset
        cls.offset += (n + 3) // 4
        return cls.seed, off


class _DropoutFn(Function):
    @staticmethod
    def forward(ctx, x, p: float):
        seed, off = _RNG.next(x.numel())
        ctx.p, ctx.seed, ctx.off = p, seed, off
        return ext().dropout(x.contiguous(), p, seed, off)

    @staticmethod
    def backward(ctx, dy):
        return ext().dropout(dy.contiguous(), ctx.p, ctx.seed, ctx.off), None


def dropout(x, p: float, training: bool):
    if not training or p == 0.0:
        return x
    if not x.is_cuda:
        return F.dropout(x, p, True)
    return _DropoutFn.apply(x, p)


# ---- dropout whose per-step state lives on the device (GPT-2: attention, residual and embedding dropout)
# _RNG above advances a Python integer that is baked into kernel arguments, so a captured step would replay one mask
# for ever.  Here (seed, offset) is a device int64[2] tensor that the kernels read; advancing it is one in-place
# device op, which a graph captures and replays like the optimizer's device-side lr and step counters.
class DropoutState:
    """The dropout RNG state of one device.  ``snapshot()`` is taken once per forward and handed to every kernel
    of that forward and to its backward (autograd nodes save the snapshot, so another forward in between does not
    change the masks the backward regenerates); ``advance(stride)`` then moves the live state past the counters
    that forward can use.  Call sites are told apart by their ``stream`` (Philox counter_lo), not by the offset."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.state = None

    @staticmethod
    def default_seed() -> int:
        """torch.initial_seed() mixed with the process rank: DDP ranks draw different masks."""
        import os

        rank = 0
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            rank = torch.distributed.get_rank()
        else:
            rank = int(os.environ.get("RANK", "0") or 0)
        return (int(torch.initial_seed()) + 0x9E3779B97F4A7C15 * (rank + 1)) & 0x7FFFFFFFFFFFFFFF

    def manual_seed(self, seed: int, offset: int = 0) -> "DropoutState":
        """(Re)start the state at ``(seed, offset)``; in place once the tensor exists, so captured graphs follow."""
        new = torch.tensor([int(seed) & 0x7FFFFFFFFFFFFFFF, int(offset)], dtype=torch.int64)
        if self.state is None:
            self.state = new.to(self.device)
        else:
            self.state.copy_(new)
        return self

    def tensor(self) -> torch.Tensor:
        if self.state is None:
            self.manual_seed(self.default_seed())
        return self.state

    def advance(self, stride: int) -> None:
        """offset += stride: one in-place device op (capturable)."""
        self.tensor()[1:].add_(int(stride))

    def snapshot(self) -> torch.Tensor:
        """A fresh device copy of (seed, offset) for one forward and its backward."""
        return self.tensor().clone()


_dropout_states: dict = {}


def dropout_state(device) -> DropoutState:
    """The DropoutState of ``device`` (created on first use, seeded by DropoutState.default_seed())."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    st = _dropout_states.get(device)
    if st is None:
        st = _dropout_states[device] = DropoutState(device)
    return st


def manual_seed_dropout(seed: int, device=None, offset: int = 0) -> None:
    """Reseed the device-side dropout state (of ``device``; default: every state created so far, and cuda's current
    device when there is one)."""
    if device is not None:
        dropout_state(device).manual_seed(seed, offset)
        return
    if torch.cuda.is_available():
        dropout_state("cuda")
    for st in _dropout_states.values():
        st.manual_seed(seed, offset)


def attn_dropout_threshold(p: float) -> int:
    """The attention kernels compare one byte of Philox output per element of P: an element is dropped iff its
    byte is below thr = clamp(round(256 p), 1, 255)."""
    if not 0.0 <= p < 1.0:
        raise ValueError(f"dropout p must be in [0, 1), got {p}")
    return min(255, max(1, int(math.floor(256.0 * p + 0.5))))


def attn_dropout_rate(p: float) -> float:
    """The rate the attention kernels apply for a requested ``p`` > 0: thr / 256 (8-bit quantisation; kept
    probabilities are scaled by 256 / (256 - thr), the inverse of this rate's keep probability, so the expectation
    is exact).  0 stays 0."""
    return 0.0 if p == 0.0 else attn_dropout_threshold(p) / 256.0


class _DropoutAddFn(Function):
    """res (fp32) + dropout(y): mask from the device state ``rng`` and ``stream``, regenerated in backward."""

    @staticmethod
    def forward(ctx, res, y, p: float, rng, stream: int):
        ctx.p, ctx.rng, ctx.stream, ctx.ydtype = p, rng, stream, y.dtype
        return ext().dropout_add(res.contiguous(), y.contiguous(), p, rng, stream)

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        gy = None
        if ctx.needs_input_grad[1]:
            if ctx.ydtype == torch.bfloat16:
                gy = ext().dropout_cast(g, ctx.p, ctx.rng, ctx.stream)
            else:
                gy = ext().dropout_add(torch.zeros_like(g), g, ctx.p, ctx.rng, ctx.stream)
        return g, gy, None, None, None


def dropout_add(res, y, p: float, rng=None, stream: int = 0):
    """res + dropout(y) in training (fp32 residual stream ``res``; ``y`` bf16 or fp32).  On the GPU ``rng`` is the
    forward's DropoutState snapshot and ``stream`` the call site; off it torch's generator draws the mask."""
    if not res.is_cuda:
        return res + F.dropout(y.float(), p, True)
    if rng is None:
        raise ValueError("dropout_add on the GPU needs the forward's rng snapshot")
    return _DropoutAddFn.apply(res.float(), y, p, rng, stream)


def dropout_rng(x, p: float, rng=None, stream: int = 0):
    """dropout(x) of an fp32 ``x`` with the device-side state (dropout_add onto zeros)."""
    if not x.is_cuda:
        return F.dropout(x, p, True)
    return dropout_add(torch.zeros_like(x, dtype=torch.float32), x, p, rng, stream)


# ====================================================================== Conv
def _conv_out(h, k, s, p, d):
    return (h + 2 * p - d * (k - 1) - 1) // s + 1


class _ConvFn(Function):
    @staticmethod
    def forward(ctx, x, weight, w16, stride, padding, dilation, want_stats):
        C = ext()
        y, st = C.conv_fwd(x, w16, list(stride), list(padding), list(dilation), want_stats, None)
        ctx.save_for_backward(x)
        ctx.w16, ctx.weight = w16, weight
        ctx.conf = (list(stride), list(padding), list(dilation))
        note_use(weight)
        if want_stats:
            ctx.mark_non_differentiable(st)
            return y, st
        return y

    @staticmethod
    def backward(ctx, dy, *unused):
        C = ext()
        (x,) = ctx.saved_tensors
        stride, padding, dilation = ctx.conf
        dy = dy.contiguous()
        dx = None
        if ctx.needs_input_grad[0]:
            dx = C.conv_dgrad(dy, ctx.w16, list(x.shape), stride, padding, dilation, None)
        gw = None
        weight = ctx.weight
        if ctx.needs_input_grad[1]:
            if tuple(ctx.w16.shape) == tuple(weight.shape):
                buf, direct = grad_sink(weight)
                C.conv_wgrad(dy, x, buf, stride, padding, dilation, 1.0)
            else:  # channel-padded filter (stem): reduce in padded layout, keep the real channels
                tmp = torch.zeros(ctx.w16.shape, dtype=torch.float32, device=dy.device)
                C.conv_wgrad(dy, x, tmp, stride, padding, dilation, 1.0)
                buf, direct = grad_sink(weight)
                buf.add_(tmp[..., : weight.shape[-1]])
            grad_done(weight, direct)
            gw = None if direct else buf
        return dx, gw, None, None, None, None, None


def _pad_filter_channels(cp: int):
    def fn(w):
        out = torch.zeros((*w.shape[:-1], cp), dtype=torch.bfloat16, device=w.device)
        out[..., : w.shape[-1]] = w
        return out

    return fn


def conv2d_nhwc(x, weight, stride=(1, 1), padding=(0, 0), dilation=(1, 1), want_stats: bool = False):
    """x: [N,H,W,Cin'] (Cin' >= Cin, zero-padded channels allowed), weight: [Cout,R,S,Cin] fp32 master.

    With ``want_stats`` (GPU) returns ``(y, stats)`` where ``stats`` holds per-channel
    partial (sum, sum^2) of y from the GEMM epilogue, consumed by ``batch_norm_nhwc``."""
    stride, padding, dilation = _pair(stride), _pair(padding), _pair(dilation)
    if not x.is_cuda:
        cin = weight.shape[-1]
        xc = _emu(x[..., :cin].permute(0, 3, 1, 2).float())
        w = weight + (_emu_w(weight) - weight).detach() if EMULATE_BF16 else weight
        y = F.conv2d(xc, w.permute(0, 3, 1, 2), None, stride, padding, dilation)
        y = _emu(y.permute(0, 2, 3, 1).contiguous())
        return (y, None) if want_stats else y
    from ._state import derived_shadow

    if x.shape[-1] != weight.shape[-1]:
        w16 = derived_shadow(weight, f"cpad{x.shape[-1]}", _pad_filter_channels(x.shape[-1]))
    else:
        w16 = shadow(weight)
    return _ConvFn.apply(x.contiguous(), weight, w16, stride, padding, dilation, want_stats)


# ================================================ space-to-depth ResNet stem
# A 7x7/s2/p3 conv over x equals a 4x4/s1 conv over the space-to-depth image
# x'[q][p][(ay,ax,c)] = x[2q+ay][2p+ax][c], padded 2 (top/left) and 1
# (bottom/right), with filter w'[o][dy][dx][(ay,ax,c)] = w[o][2dy+ay-1][2dx+ax-1][c]
# (zero outside 7x7).  Each 7x7 tap appears exactly once in w', so the weight
# gradient maps back by a gather.
_S2D_IDX: dict = {}


def _s2d_index(cin: int, device):
    key = (cin, str(device))
    if key not in _S2D_IDX:
        dst, src = [], []
        for dy in range(4):
            for dx in range(4):
                for ay in range(2):
                    for ax in range(2):
                        for c in range(4):
                            r, s_ = 2 * dy + ay - 1, 2 * dx + ax - 1
                            if 0 <= r < 7 and 0 <= s_ < 7 and c < cin:
                                dst.append(((dy * 4 + dx) * 4 + ay * 2 + ax) * 4 + c)
                                src.append((r * 7 + s_) * cin + c)
        order = sorted(range(len(src)), key=lambda i: src[i])
        inv = torch.tensor([dst[i] for i in order], dtype=torch.long, device=device)  # w-flat index -> w'-flat index
        _S2D_IDX[key] = (torch.tensor(dst, dtype=torch.long, device=device),
                         torch.tensor(src, dtype=torch.long, device=device), inv)
    return _S2D_IDX[key]


def _s2d_filter(w):
    co, cin = w.shape[0], w.shape[-1]
    dst, src, _ = _s2d_index(cin, w.device)
    out = torch.zeros((co, 256), dtype=torch.bfloat16, device=w.device)
    out[:, dst] = w.reshape(co, -1)[:, src].to(torch.bfloat16)
    return out.view(co, 4, 4, 16)


class _S2DStemFn(Function):
    @staticmethod
    def forward(ctx, xs, weight, w16, want_stats):
        y, st = ext().conv_fwd(xs, w16, [1, 1], [2, 2, 1, 1], [1, 1], want_stats, None)
        ctx.save_for_backward(xs)
        ctx.weight = weight
        note_use(weight)
        if want_stats:
            ctx.mark_non_differentiable(st)
            return y, st
        return y

    @staticmethod
    def backward(ctx, dy, *unused):
        (xs,) = ctx.saved_tensors
        weight = ctx.weight
        co = weight.shape[0]
        tmp = torch.zeros((co, 4, 4, 16), dtype=torch.float32, device=dy.device)
        ext().conv_wgrad(dy.contiguous(), xs, tmp, [1, 1], [2, 2], [1, 1], 1.0)
        buf, direct = grad_sink(weight)
        buf.view(co, -1).add_(tmp.view(co, 256)[:, _s2d_index(weight.shape[-1], dy.device)[2]])
        grad_done(weight, direct)
        return None, (None if direct else buf), None, None


def to_s2d_input(x: torch.Tensor) -> torch.Tensor:
    """NCHW fp32 images [N,3,H,W] -> space-to-depth NHWC bf16 [N,H/2,W/2,16] (GPU stem input)."""
    return ext().nchw_to_s2d(x.float().contiguous())


def stem_conv_s2d(xs, weight, want_stats: bool = False):
    """7x7/s2/p3 conv (filter ``weight`` [Co,7,7,Cin<=4]) over a space-to-depth input ``xs``."""
    from ._state import derived_shadow

    assert tuple(weight.shape[1:3]) == (7, 7) and weight.shape[-1] <= 4 and xs.shape[-1] == 16
    w16 = derived_shadow(weight, "s2d", _s2d_filter)
    return _S2DStemFn.apply(xs.contiguous(), weight, w16, want_stats)


def _pair(v) -> tuple:
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


# ================================================================ BatchNorm
class _BNFn(Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, residual, rmean, rvar, momentum, eps, relu_, stats):
        C = ext()
        y, coef = C.bn_fwd_train(x, gamma.detach(), beta.detach(), rmean, rvar, momentum, eps, relu_, residual, stats)
        ctx.save_for_backward(x, y if relu_ else None, coef)
        ctx.gamma, ctx.beta, ctx.has_res = gamma, beta, residual is not None
        note_use(gamma)
        note_use(beta)
        return y

    @staticmethod
    def backward(ctx, dy):
        C = ext()
        x, y, coef = ctx.saved_tensors
        gbuf, gdirect = grad_sink(ctx.gamma)
        bbuf, bdirect = grad_sink(ctx.beta)
        dx, dz = C.bn_bwd(dy.contiguous(), y, x, ctx.gamma.detach(), coef, gbuf, bbuf, ctx.has_res)
        grad_done(ctx.gamma, gdirect)
        grad_done(ctx.beta, bdirect)
        return (dx, None if gdirect else gbuf, None if bdirect else bbuf, dz if ctx.has_res else None,
                None, None, None, None, None, None)


def batch_norm_nhwc(x, gamma, beta, running_mean, running_var, training: bool, momentum: float = 0.1,
                    eps: float = 1e-5, relu: bool = False, residual=None, stats=None, num_batches_tracked=None):
    """y = act(BN(x) [+ residual]) over the channel (last) dim of an NHWC tensor."""
    if not x.is_cuda:
        C_ = x.shape[-1]
        xf = x.reshape(-1, C_).float()
        yf = F.batch_norm(xf, running_mean, running_var, gamma, beta, training, momentum, eps)
        y = yf.reshape(x.shape)
        if residual is not None:
            y = y + residual.float()
        if relu:
            y = F.relu(y)
        if training and num_batches_tracked is not None:
            num_batches_tracked.add_(1)
        return _emu(y)
    if training:
        if num_batches_tracked is not None:
            num_batches_tracked.add_(1)
        return _BNFn.apply(x.contiguous(), gamma, beta, residual.contiguous() if residual is not None else None,
                           running_mean, running_var, momentum, eps, relu, stats)
    return ext().bn_fwd_eval(x.contiguous(), gamma.detach(), beta.detach(), running_mean, running_var, eps, relu,
                             residual.contiguous() if residual is not None else None)


class _StemBNReluPoolFn(Function):
    """maxpool(relu(BN(h))) for the ResNet stem with training-mode BN whose
    statistics came from the conv epilogue: the BN+ReLU output (the largest
    activation of the network) is never written or re-read; the backward
    gathers the pooled gradient per element inside the BN-backward passes."""

    @staticmethod
    def forward(ctx, h, gamma, beta, rmean, rvar, momentum, eps, stats, k, s, p):
        C = ext()
        M = h.numel() // h.shape[-1]
        coef = C.bn_coef(stats, M, gamma.detach(), beta.detach(), rmean, rvar, momentum, eps)
        y, idx = C.bnrelu_maxpool_fwd(h, coef, k, s, p)
        ctx.save_for_backward(h, idx, coef)
        ctx.gamma, ctx.beta, ctx.conf = gamma, beta, (k, s, p)
        note_use(gamma)
        note_use(beta)
        return y

    @staticmethod
    def backward(ctx, dy):
        h, idx, coef = ctx.saved_tensors
        gbuf, gdirect = grad_sink(ctx.gamma)
        bbuf, bdirect = grad_sink(ctx.beta)
        dh = ext().maxpool_bn_bwd(dy.contiguous(), idx, h, ctx.gamma.detach(), coef, gbuf, bbuf, *ctx.conf)
        grad_done(ctx.gamma, gdirect)
        grad_done(ctx.beta, bdirect)
        return (dh, None if gdirect else gbuf, None if bdirect else bbuf) + (None,) * 8


def stem_bn_relu_maxpool(h, bn, stats, kernel_size=3, stride=2, padding=1):
    """max_pool2d(relu(bn(h))) in training mode from conv-epilogue statistics (GPU)."""
    if bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
    return _StemBNReluPoolFn.apply(h.contiguous(), bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.momentum, bn.eps,
                                   stats, kernel_size, stride, padding)


class _StemFusedFn(Function):
    """The whole training-mode ResNet stem -- s2d 7x7/s2 conv, BN (statistics from the conv epilogue), ReLU,
    3x3/s2 max-pool -- as one node.  Backward: the BN-backward reduction over the pooled gradient, then the
    stem weight grad computing dL/dh on the fly (csrc stem_bwd_fused): neither the BN+ReLU output nor dL/dh
    is ever written (the standalone apply pass moved 1.95 GB per batch-512 step)."""

    @staticmethod
    def forward(ctx, xs, weight, w16, gamma, beta, rmean, rvar, momentum, eps):
        C = ext()
        h, st = C.conv_fwd(xs, w16, [1, 1], [2, 2, 1, 1], [1, 1], True, None)
        coef = C.bn_coef(st, h.numel() // h.shape[-1], gamma.detach(), beta.detach(), rmean, rvar, momentum, eps)
        y, idx = C.bnrelu_maxpool_fwd(h, coef, 3, 2, 1)
        ctx.save_for_backward(xs, h, idx, coef)
        ctx.weight, ctx.gamma, ctx.beta = weight, gamma, beta
        for p in (weight, gamma, beta):
            note_use(p)
        return y

    @staticmethod
    def backward(ctx, dy):
        xs, h, idx, coef = ctx.saved_tensors
        weight, gamma, beta = ctx.weight, ctx.gamma, ctx.beta
        co = weight.shape[0]
        gbuf, gdirect = grad_sink(gamma)
        bbuf, bdirect = grad_sink(beta)
        tmp = torch.zeros((co, 4, 4, 16), dtype=torch.float32, device=dy.device)
        ext().stem_bwd_fused(dy.contiguous(), idx, h, xs, gamma.detach(), coef, gbuf, bbuf, tmp)
        grad_done(gamma, gdirect)
        grad_done(beta, bdirect)
        buf, direct = grad_sink(weight)
        buf.view(co, -1).add_(tmp.view(co, 256)[:, _s2d_index(weight.shape[-1], dy.device)[2]])
        grad_done(weight, direct)
        return (None, None if direct else buf, None, None if gdirect else gbuf, None if bdirect else bbuf,
                None, None, None, None)


def stem_fused_ok(xs) -> bool:
    """The fused stem path's envelope: s2d input [N, H, W, 16] on the GPU with even H, W <= 112."""
    return (xs.is_cuda and xs.dim() == 4 and xs.shape[-1] == 16 and xs.shape[1] % 2 == 0 and xs.shape[2] % 2 == 0
            and 97 <= xs.shape[2] <= 112 and xs.shape[1] >= 8)


def stem_fused(xs, weight, bn):
    """maxpool(relu(bn(conv_s2d(xs, weight)))) in training mode, one autograd node (see _StemFusedFn)."""
    from ._state import derived_shadow

    if bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
    w16 = derived_shadow(weight, "s2d", _s2d_filter)
    return _StemFusedFn.apply(xs.contiguous(), weight, w16, bn.weight, bn.bias, bn.running_mean, bn.running_var,
                              bn.momentum, bn.eps)


# ================================================================== pooling
class _MaxPoolFn(Function):
    @staticmethod
    def forward(ctx, x, k, s, p):
        y, idx = ext().maxpool_fwd(x, k, s, p)
        ctx.save_for_backward(idx)
        ctx.conf = (list(x.shape), k, s, p)
        return y

    @staticmethod
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        xs, k, s, p = ctx.conf
        return ext().maxpool_bwd(dy.contiguous(), idx, xs, k, s, p), None, None, None


def max_pool2d_nhwc(x, kernel_size=3, stride=2, padding=1):
    if not x.is_cuda:
        return _emu(F.max_pool2d(x.permute(0, 3, 1, 2), kernel_size, stride, padding).permute(0, 2, 3, 1).contiguous())
    return _MaxPoolFn.apply(x.contiguous(), kernel_size, stride, padding)


class _GAvgPoolFn(Function):
    @staticmethod
    def forward(ctx, x):
        ctx.shape = list(x.shape)
        return ext().gavgpool_fwd(x)

    @staticmethod
    def backward(ctx, dy):
        return ext().gavgpool_bwd(dy.contiguous(), ctx.shape)


def global_avg_pool_nhwc(x):
    if not x.is_cuda:
        return _emu(x.float().mean(dim=(1, 2)))
    return _GAvgPoolFn.apply(x.contiguous())


# ===================================================================== loss
class _CEFn(Function):
    """Mean CE: the kernel pair (per-row pass + fixed-order reduction) also yields the mean over the
    non-ignored rows and 1 / their count, and backward is one scaling pass -- no torch-level count /
    clamp / divide / cast kernels at the launch-bound forward -> backward seam."""

    @staticmethod
    def forward(ctx, logits, labels, num_classes: int, ignore_index: int, label_smoothing: float = 0.0, z_loss: float = 0.0,
                labels2=None, mix_w=None):
        mix = {} if labels2 is None else {"labels2": labels2.contiguous(), "mix_w": mix_w}
        out4, d = ext().cross_entropy_mean(logits.contiguous(), labels.contiguous(), num_classes,
                                           logits.dtype == torch.bfloat16, ignore_index,
                                           label_smoothing=label_smoothing, z_loss=z_loss, **mix)
        ctx.save_for_backward(d, out4)
        return out4[2:3].reshape(())

    @staticmethod
    def backward(ctx, g):
        d, out4 = ctx.saved_tensors
        return ext().ce_grad_scale(d, g.float().reshape(1), out4[3:4]), None, None, None, None, None, None, None


def _check_ce_reg(label_smoothing: float, z_loss: float):
    if not 0.0 <= label_smoothing < 1.0:
        raise ValueError(f"label_smoothing must be in [0, 1), got {label_smoothing}")
    if not z_loss >= 0.0:
        raise ValueError(f"z_loss must be >= 0, got {z_loss}")


def _ce_reference(logits, labels, ignore_index: int, label_smoothing: float, z_loss: float):
    """The CPU branch: the regularised mean CE in plain torch ops (``logits``: [rows, classes])."""
    loss = F.cross_entropy(logits, labels, ignore_index=ignore_index, label_smoothing=label_smoothing)
    if z_loss != 0.0:
        keep = labels != ignore_index
        lse2 = torch.logsumexp(logits, dim=-1).square() * keep
        loss = loss + z_loss * lse2.sum() / keep.sum().clamp(min=1)
    return loss


def _ce_mix_reference(logits, labels, labels2, mix_w, ignore_index: int, label_smoothing: float, z_loss: float):
    """The CPU branch with two labels per row: F.cross_entropy on the soft target w onehot(y) + (1 - w) onehot(y2)
    over the rows whose ``labels`` entry is not ignored (a row whose ``labels2`` entry is ignored has w = 1)."""
    keep = labels != ignore_index
    n = keep.sum().clamp(min=1)
    V = logits.shape[-1]
    w = mix_w.to(logits.dtype).reshape(-1).expand(labels.numel()) if mix_w.numel() == 1 else mix_w.to(logits.dtype).reshape(-1)
    w = torch.where(labels2 == ignore_index, torch.ones_like(w), w)
    y2 = torch.where(labels2 == ignore_index, labels, labels2)
    tgt = w[:, None] * F.one_hot(labels.clamp(min=0), V) + (1.0 - w)[:, None] * F.one_hot(y2.clamp(min=0), V)
    rows = F.cross_entropy(logits, tgt.to(logits.dtype), reduction="none", label_smoothing=label_smoothing)
    if z_loss != 0.0:
        rows = rows + z_loss * torch.logsumexp(logits, dim=-1).square()
    return (rows * keep).sum() / n


def cross_entropy(logits, labels, num_classes: Optional[int] = None, ignore_index: int = -100,
                  label_smoothing: float = 0.0, z_loss: float = 0.0, labels2=None, mix_w=None):
    """Mean softmax cross-entropy over rows (torch.nn.CrossEntropyLoss semantics, ``label_smoothing`` included),
    plus ``z_loss * mean(logsumexp^2)`` over the non-ignored rows.

    ``labels2`` / ``mix_w`` (together; mixup / cutmix targets): a second label per row and the weight ``w`` of the
    first one, a tensor of one element (the batch's) or one per row -- on the GPU a device fp32 tensor the kernel
    reads, never a host number.  The row's target is ``w onehot(y) + (1 - w) onehot(y2)``; a row is ignored iff
    ``labels`` says so, and ``labels2 == ignore_index`` marks a row without partner (``w = 1``)."""
    if num_classes is None:
        num_classes = logits.shape[-1]
    _check_ce_reg(label_smoothing, z_loss)
    if (labels2 is None) != (mix_w is None):
        raise ValueError("cross_entropy: labels2 and mix_w go together")
    if labels2 is not None and not torch.is_tensor(mix_w):
        raise TypeError("cross_entropy: mix_w must be a tensor (one weight, or one per row)")
    if not logits.is_cuda:
        lf = logits.reshape(-1, logits.shape[-1])[:, :num_classes].float()
        if labels2 is not None:
            return _ce_mix_reference(lf, labels.reshape(-1), labels2.reshape(-1), mix_w, ignore_index, label_smoothing, z_loss)
        return _ce_reference(lf, labels.reshape(-1), ignore_index, label_smoothing, z_loss)
    if labels2 is not None:
        return _CEFn.apply(logits.reshape(-1, logits.shape[-1]), labels.reshape(-1), num_classes, ignore_index,
                           float(label_smoothing), float(z_loss), labels2.reshape(-1), mix_w.detach().float())
    return _CEFn.apply(logits.reshape(-1, logits.shape[-1]), labels.reshape(-1), num_classes, ignore_index,
                       float(label_smoothing), float(z_loss))


def cross_entropy_eval(logits, labels, num_classes: Optional[int] = None):
    """(loss_sum, correct_count) as device scalars, one fused pass (no grad)."""
    if num_classes is None:
        num_classes = logits.shape[-1]
    if not logits.is_cuda:
        lf = logits.reshape(-1, logits.shape[-1])[:, :num_classes].float()
        loss = F.cross_entropy(lf, labels.reshape(-1), reduction="sum")
        return loss, (lf.argmax(1) == labels.reshape(-1)).sum().float()
    _, s, correct, _ = ext().cross_entropy(logits.reshape(-1, logits.shape[-1]).contiguous(), labels.reshape(-1).contiguous(),
                                           num_classes, 1.0, False, False, -100)
    return s.reshape(()), correct.reshape(())


# ================================================================ LayerNorm
class _LNFn(Function):
    @staticmethod
    def forward(ctx, x, w, b, eps):
        y, mean, rstd = ext().layernorm_fwd(x.contiguous(), w.detach(), b.detach() if b is not None else None, eps)
        ctx.save_for_backward(x, mean, rstd)
        ctx.w, ctx.b = w, b
        note_use(w)
        if b is not None:
            note_use(b)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mean, rstd = ctx.saved_tensors
        wbuf, wd = grad_sink(ctx.w)
        bbuf, bd = (grad_sink(ctx.b) if ctx.b is not None else (None, False))
        dx = ext().layernorm_bwd(dy.contiguous().to(torch.bfloat16), x.contiguous(), ctx.w.detach(), mean, rstd, wbuf, bbuf,
                                 None)
        grad_done(ctx.w, wd)
        if ctx.b is not None:
            grad_done(ctx.b, bd)
        return dx, (None if wd else wbuf), (None if (bd or ctx.b is None) else bbuf), None


def layer_norm(x, weight, bias=None, eps: float = 1e-5):
    """LayerNorm over the last dim. GPU: f32/bf16 in -> bf16 out."""
    if not x.is_cuda:
        return F.layer_norm(x.float(), (x.shape[-1],), weight, bias, eps)
    return _LNFn.apply(x, weight, bias, eps)


# ================================================================ Embedding
class _EmbFn(Function):
    @staticmethod
    def forward(ctx, idx, wte, wpe, wte16, wpe16, pos=None):
        out = ext().embedding_fwd(idx, wte16, wpe16, pos)
        ctx.save_for_backward(idx)
        ctx.wte, ctx.wpe, ctx.pos = wte, wpe, pos
        note_use(wte)
        if wpe is not None:
            note_use(wpe)
        return out

    @staticmethod
    def backward(ctx, dout):
        (idx,) = ctx.saved_tensors
        tb, td = grad_sink(ctx.wte)
        pb, pd = grad_sink(ctx.wpe) if ctx.wpe is not None else (None, False)
        for p, buf, d in ((ctx.wte, tb, td), (ctx.wpe, pb, pd)):  # the scatter-add needs a zeroed start
            if p is not None and d and grad_fresh(p):
                buf.zero_()
        ext().embedding_bwd(idx, dout.contiguous().float(), tb, pb, ctx.pos)
        grad_done(ctx.wte, td)
        if ctx.wpe is not None:
            grad_done(ctx.wpe, pd)
        return None, (None if td else tb), (None if (pd or ctx.wpe is None) else pb), None, None, None


def embedding(idx, wte, wpe=None, pos=None):
    """tok + pos embedding -> f32 [B,T,D] residual stream.  ``pos`` (int32 [B, T], from doc_bounds): the position
    id of every token in place of its index in the row."""
    if not idx.is_cuda:
        T = idx.shape[1]
        x = F.embedding(idx, wte)
        if wpe is not None:
            x = x + (wpe[:T].unsqueeze(0) if pos is None else F.embedding(pos.long(), wpe))
        return x
    # (a loader's x = tokens[:, :-1] is a strided view; the kernels index idx as one flat array)
    return _EmbFn.apply(idx.contiguous(), wte, wpe, shadow(wte), shadow(wpe) if wpe is not None else None,
                        pos.to(torch.int32).contiguous() if pos is not None else None)


# ================================================================ Attention
# ---- packed documents: several documents end to end in one row, block-diagonal causal mask.
# doc_start [B, T]: the index within the row of the first token of token t's document.  Valid iff
# doc_start[b, 0] == 0 and doc_start[b, t] is doc_start[b, t - 1] or t.  Query i sees key j iff
# doc_start[b, i] <= j <= i; token t's position id is t - doc_start[b, t]; all zeros = plain causal attention.
def doc_bounds(doc_start):
    """doc_start [B, T] (any integer dtype) -> (doc_start, doc_end, pos), int32 [B, T] each: doc_end is the
    exclusive end of the token's document, pos its position id.  Device ops only, no host sync (graph-safe);
    call it once per batch and hand the result to every layer."""
    ds = doc_start.to(torch.int32).contiguous()
    T = ds.shape[-1]
    t = torch.arange(T, device=ds.device, dtype=torch.int32).expand_as(ds)
    # the next document start at or after t + 1: a reverse running minimum over "t where a document starts, else T"
    nxt = torch.where(ds == t, t, torch.full_like(t, T))
    nxt = torch.cat([nxt[..., 1:], torch.full_like(nxt[..., :1], T)], dim=-1)
    de = torch.flip(torch.cummin(torch.flip(nxt, (-1,)), dim=-1).values, (-1,)).to(torch.int32).contiguous()
    # (clamped: an invalid doc_start may give wrong numbers, never a position outside the table)
    return ds, de, (t - ds).clamp_(0, T - 1).contiguous()


def doc_start_from_lengths(lengths, T: int):
    """Document lengths of one row (a sequence of positive ints; the last one is cut at, or extended to, T) ->
    doc_start int32 [T]."""
    out = torch.zeros(T, dtype=torch.int32)
    s = 0
    for n in lengths:
        n = int(n)
        if n < 1:
            raise ValueError("document lengths must be at least 1")
        if s >= T:
            break
        out[s:] = s
        s += n
    return out


def doc_start_from_eos(idx, eos_id: int):
    """idx [B, T] -> doc_start int32 [B, T]: the token after an EOS starts a document.  Device ops, no sync."""
    T = idx.shape[-1]
    t = torch.arange(T, device=idx.device, dtype=torch.int32).expand(idx.shape)
    first = torch.ones_like(idx, dtype=torch.bool)
    first[..., 1:] = idx[..., :-1] == eos_id
    return torch.cummax(torch.where(first, t, torch.zeros_like(t)), dim=-1).values.to(torch.int32)


def check_doc_start(doc_start) -> None:
    """Raise ValueError unless doc_start [B, T] is valid (see above).  Synchronises: opt-in, outside the step."""
    if doc_start.dim() != 2:
        raise ValueError("doc_start must be [B, T]")
    ds = doc_start.long()
    t = torch.arange(ds.shape[1], device=ds.device).expand_as(ds)
    if bool((ds[:, 0] != 0).any()):
        raise ValueError("doc_start[:, 0] must be 0")
    if bool((ds > t).any()) or bool((ds < 0).any()):
        raise ValueError("doc_start[b, t] must lie in [0, t]")
    if bool((ds[:, 1:] < ds[:, :-1]).any()):
        raise ValueError("doc_start must be non-decreasing")
    if bool(((ds[:, 1:] != ds[:, :-1]) & (ds[:, 1:] != t[:, 1:])).any()):
        raise ValueError("doc_start[b, t] must be doc_start[b, t - 1] or t")


class _AttnFn(Function):
    @staticmethod
    def forward(ctx, qkv, H: int, scale: float, doc_start=None, doc_end=None, dropout_p: float = 0.0, rng=None,
                stream: int = 0):
        ctx.drop = None
        if dropout_p > 0.0:  # dropout on P inside the kernels; rng is the forward's snapshot, kept for backward
            ctx.drop = dict(dropout_p=dropout_p, rng=rng, stream=stream)
            out, lse = ext().attn_fwd(qkv.contiguous(), H, scale, True, doc_start=doc_start, doc_end=doc_end, **ctx.drop)
        elif doc_start is None:
            out, lse = ext().attn_fwd(qkv.contiguous(), H, scale, True)
        else:
            out, lse = ext().attn_fwd(qkv.contiguous(), H, scale, True, doc_start=doc_start, doc_end=doc_end)
        ctx.save_for_backward(qkv, out, lse)
        ctx.H, ctx.scale, ctx.doc = H, scale, (doc_start, doc_end)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse = ctx.saved_tensors
        ds, de = ctx.doc
        if ctx.drop is not None:
            dqkv = ext().attn_bwd(qkv, out, dout.contiguous().to(torch.bfloat16), lse, ctx.H, ctx.scale, True,
                                  doc_start=ds, doc_end=de, **ctx.drop)
        elif ds is None:
            dqkv = ext().attn_bwd(qkv, out, dout.contiguous().to(torch.bfloat16), lse, ctx.H, ctx.scale, True)
        else:
            dqkv = ext().attn_bwd(qkv, out, dout.contiguous().to(torch.bfloat16), lse, ctx.H, ctx.scale, True,
                                  doc_start=ds, doc_end=de)
        return dqkv, None, None, None, None, None, None, None


def attn_kernel_ok(T: int, D: int) -> bool:
    """The shapes the flash-attention kernels take (csrc/kernels/attn.hip): head dim 64, whole 64-key tiles."""
    return D == 64 and T % 64 == 0


def _causal_attention_torch(qkv5, scale: float, doc_start=None, dropout_p: float = 0.0):
    """Shapes outside the kernels' range (and every packed-document or dropout call off the GPU): explicit masked
    softmax(Q K^T) V in fp32 torch ops (autograd differentiates it), result in qkv's dtype like the kernel's.
    ``doc_start`` [B, T]: keys before the query's document are masked too.  ``dropout_p``: F.dropout on P (torch's
    generator and the true p, not the kernels' Philox mask and 8-bit rate: the same distribution up to that)."""
    q, k, v = qkv5.float().permute(2, 0, 3, 1, 4)  # each [B, H, T, D]
    T = q.shape[-2]
    s = (q @ k.transpose(-1, -2)) * scale
    s = s.masked_fill(torch.ones(T, T, dtype=torch.bool, device=s.device).triu(1), float("-inf"))
    if doc_start is not None:
        j = torch.arange(T, device=s.device)
        s = s.masked_fill((j[None, None, :] < doc_start.long()[:, :, None]).unsqueeze(1), float("-inf"))
    pr = torch.softmax(s, dim=-1)
    if dropout_p > 0.0:
        pr = F.dropout(pr, dropout_p, True)
    o = pr @ v
    return o.transpose(1, 2).to(qkv5.dtype)  # [B, T, H, D]


def causal_attention(qkv, n_head: int, doc_bounds=None, dropout_p: float = 0.0, rng=None, stream: int = 0):
    """qkv: [B, T, 3*H*D] -> [B, T, H*D] causal softmax attention.  ``doc_bounds`` (the tuple doc_bounds()
    returns): attention stays inside each packed document.  ``dropout_p`` > 0 (training; the caller decides):
    dropout on the attention probabilities -- inside the flash kernels at the rate attn_dropout_rate(dropout_p),
    with the mask drawn from ``rng`` (a DropoutState snapshot, default: a fresh one, after which the state is
    advanced) and ``stream``; off the GPU or for other shapes an explicit softmax with F.dropout on P."""
    B, T, three_hd = qkv.shape
    D = three_hd // (3 * n_head)
    scale = 1.0 / math.sqrt(D)
    if dropout_p != 0.0:
        if not 0.0 < dropout_p < 1.0:
            raise ValueError(f"dropout_p must be in [0, 1), got {dropout_p}")
        ds, de = (doc_bounds[0], doc_bounds[1]) if doc_bounds is not None else (None, None)
        if not qkv.is_cuda or not attn_kernel_ok(T, D):
            return _causal_attention_torch(qkv.reshape(B, T, 3, n_head, D), scale, ds, dropout_p).reshape(B, T, n_head * D)
        if rng is None:
            st = dropout_state(qkv.device)
            rng = st.snapshot()
            st.advance(B * n_head * (T // 4) ** 2)
        out = _AttnFn.apply(qkv.reshape(B, T, 3, n_head, D), n_head, scale, ds, de, dropout_p, rng, stream)
        return out.reshape(B, T, n_head * D)
    if doc_bounds is not None:
        ds, de = doc_bounds[0], doc_bounds[1]
        if not qkv.is_cuda or not attn_kernel_ok(T, D):
            return _causal_attention_torch(qkv.reshape(B, T, 3, n_head, D), scale, ds).reshape(B, T, n_head * D)
        out = _AttnFn.apply(qkv.reshape(B, T, 3, n_head, D), n_head, scale, ds, de)
        return out.reshape(B, T, n_head * D)
    if not qkv.is_cuda:
        q, k, v = qkv.float().view(B, T, 3, n_head, D).permute(2, 0, 3, 1, 4)
        o = F.scaled_dot_product_attention(q, k, v, is_causal=True)
        return o.transpose(1, 2).reshape(B, T, n_head * D)
    if not attn_kernel_ok(T, D):
        return _causal_attention_torch(qkv.reshape(B, T, 3, n_head, D), scale).reshape(B, T, n_head * D)
    out = _AttnFn.apply(qkv.reshape(B, T, 3, n_head, D), n_head, scale, None, None)
    return out.reshape(B, T, n_head * D)


class _BidirAttnFn(Function):
    """Bidirectional attention over the first ``seq_len`` rows on the LDS-DMA kernels (causal=False); the rows from
    ``seq_len`` on are padding: zeros in the output and in all three parts of the gradient."""

    @staticmethod
    def forward(ctx, qkv, H: int, scale: float, seq_len: int):
        out, lse = ext().attn_fwd(qkv.contiguous(), H, scale, False, seq_len=seq_len)
        ctx.save_for_backward(qkv, out, lse)
        ctx.H, ctx.scale, ctx.seq_len = H, scale, seq_len
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse = ctx.saved_tensors
        dqkv = ext().attn_bwd(qkv, out, dout.contiguous().to(torch.bfloat16), lse, ctx.H, ctx.scale, False,
                              seq_len=ctx.seq_len)
        return dqkv, None, None, None


def _attention_torch(qkv5, scale: float, seq_len: int):
    """The bidirectional form of _causal_attention_torch: query i < seq_len sees the keys j < seq_len, the rows from
    seq_len on are zeros (and pass no gradient); fp32 softmax, result in qkv's dtype."""
    T = qkv5.shape[1]
    q, k, v = qkv5[:, :seq_len].float().permute(2, 0, 3, 1, 4)  # each [B, H, L, D]: the padding rows never enter
    o = torch.softmax((q @ k.transpose(-1, -2)) * scale, dim=-1) @ v
    o = F.pad(o.transpose(1, 2), (0, 0, 0, 0, 0, T - seq_len))  # [B, T, H, D], zeros from seq_len on
    return o.to(qkv5.dtype)


def attention(qkv, n_head: int, seq_len: Optional[int] = None):
    """qkv: [B, Tp, 3*H*D] -> [B, Tp, H*D] softmax attention without the causal mask over the first ``seq_len`` rows
    (default Tp): query i < seq_len sees the keys j < seq_len; the rows from seq_len on are padding and come back as
    zeros, in the output and in the gradient.  On the GPU with attn_kernel_ok(Tp, D) the flash kernels run; elsewhere
    an explicit fp32 masked softmax in torch ops with the same semantics."""
    B, T, three_hd = qkv.shape
    D = three_hd // (3 * n_head)
    L = T if seq_len is None else int(seq_len)
    if not 1 <= L <= T:
        raise ValueError(f"seq_len must be in [1, {T}], got {seq_len}")
    scale = 1.0 / math.sqrt(D)
    if not qkv.is_cuda or not attn_kernel_ok(T, D):
        return _attention_torch(qkv.reshape(B, T, 3, n_head, D), scale, L).reshape(B, T, n_head * D)
    return _BidirAttnFn.apply(qkv.reshape(B, T, 3, n_head, D), n_head, scale, L).reshape(B, T, n_head * D)


def patchify(x: torch.Tensor, patch: int) -> torch.Tensor:
    """NCHW fp32 image batch [B, C, H, W] -> patch rows [B, (H/p)(W/p), C*p*p], each row ordered (c, py, px), so a
    patch-embedding filter [D, C, p, p] flattened is the ``linear`` weight.  bf16 from one kernel on the GPU (one RNE
    rounding); on the CPU unfold / reshape in x's dtype, like to_nhwc_input.  The input has no gradient."""
    B, C, H, W = x.shape
    p = int(patch)
    if H % p or W % p:
        raise ValueError(f"patch {p} must divide the image size {H} x {W}")
    if not x.is_cuda:
        y = x.detach().reshape(B, C, H // p, p, W // p, p).permute(0, 2, 4, 1, 3, 5)
        return y.reshape(B, (H // p) * (W // p), C * p * p).contiguous()
    return ext().patchify(x.detach().float().contiguous(), p)


def add(a, b):
    if not a.is_cuda:
        return a + b
    return _AddFn.apply(a, b)


class _AddFn(Function):
    @staticmethod
    def forward(ctx, a, b):
        return ext().add(a.contiguous(), b.contiguous(), 1.0)

    @staticmethod
    def backward(ctx, g):
        return g, g


def to_nhwc_input(x: torch.Tensor, cpad: int = 8) -> torch.Tensor:
    """NCHW fp32 image batch -> NHWC (bf16 on GPU, channel-padded to ``cpad``)."""
    if not x.is_cuda:
        y = x.permute(0, 2, 3, 1).float()
        if y.shape[-1] < cpad:
            y = F.pad(y, (0, cpad - y.shape[-1]))
        return y.contiguous()
    return ext().nchw_to_nhwc(x.float().contiguous(), cpad)


MIX_LAYOUTS = {"s2d": 0, "nhwc": 1}


def mix_pack(x: torch.Tensor, params: torch.Tensor, layout: str = "s2d", cpad: int = 8) -> torch.Tensor:
    """``to_s2d_input`` / ``to_nhwc_input`` of the batch mixed with ``x.roll(1, 0)`` by one device row ``params``
    (``[w_pix, w_lab, x1, y1, x2, y2, mode, lam_raw]``, ``data.BatchMixer.draw``): inside the box the partner's
    pixel, outside ``w_pix * x + (1 - w_pix) * partner`` in fp32, rounded once to bf16.  One pass over the NCHW fp32
    batch, GPU only, not differentiable."""
    if layout not in MIX_LAYOUTS:
        raise ValueError(f"mix_pack: layout must be one of {sorted(MIX_LAYOUTS)}, got {layout!r}")
    if x.requires_grad:
        raise ValueError("mix_pack is not differentiable: the input batch must not require grad")
    if not x.is_cuda:
        raise ValueError("mix_pack runs on the GPU (on the CPU BatchMixer mixes with torch ops)")
    if x.dim() != 4 or x.dtype != torch.float32:
        raise ValueError("mix_pack: x must be an NCHW fp32 batch")
    return ext().mix_pack(x.contiguous(), params.reshape(8), MIX_LAYOUTS[layout], cpad)


# ====================================================== residual-stream linear
class _LinearResidualFn(Function):
    """y = x_res + a @ W^T + b  with a bf16 activations and x_res the fp32 residual stream,
    one GEMM launch (fp32-residual epilogue)."""

    @staticmethod
    def forward(ctx, a, weight, bias, x_res):
        C = ext()
        w16 = shadow(weight)
        ab = a.contiguous() if a.dtype == torch.bfloat16 else a.to(torch.bfloat16).contiguous()
        y = C.linear_fwd(ab, w16, bias.detach() if bias is not None else None, 0, True, x_res.contiguous(), None)
        ctx.save_for_backward(ab)
        ctx.weight, ctx.bias = weight, bias
        note_use(weight)
        if bias is not None:
            note_use(bias)
        return y

    @staticmethod
    def backward(ctx, dy):
        C = ext()
        (ab,) = ctx.saved_tensors
        weight, bias = ctx.weight, ctx.bias
        dyb = dy.to(torch.bfloat16).contiguous()
        da = C.linear_dgrad(dyb, shadow(weight)) if ctx.needs_input_grad[0] else None
        buf, direct = grad_sink(weight)
        bb, bd = grad_sink(bias) if bias is not None else (None, False)
        C.linear_wgrad(dyb, ab, buf, 1.0, None, bb, 0, direct and grad_fresh(weight))  # bias grad: row sums of dy^T in the same launch
        grad_done(weight, direct)
        gb = None
        if bias is not None:
            grad_done(bias, bd)
            gb = None if bd else bb
        return da, (None if direct else buf), gb, dy


def linear_residual(a, weight, bias, x_res):
    """x_res (fp32) + linear(a)."""
    if not a.is_cuda:
        return x_res + F.linear(a.float(), weight, bias)
    return _LinearResidualFn.apply(a, weight, bias, x_res)


# ================================================================ LM head
class _LMHeadFn(Function):
    """logits[.., Vp] = x @ wte_pad^T, wte tied with the token embedding; the
    vocab is padded to a multiple of 64 inside the bf16 shadow only (zero pad
    rows), the fp32 master keeps the canonical [V, D] shape."""

    @staticmethod
    def forward(ctx, x, wte, pad_rows: int):
        C = ext()
        w16 = shadow(wte, pad_rows)
        xb = x.contiguous() if x.dtype == torch.bfloat16 else x.to(torch.bfloat16).contiguous()
        y = C.linear_fwd(xb, w16, None, 0, False, None, None)
        ctx.save_for_backward(xb)
        ctx.wte, ctx.pad = wte, pad_rows
        note_use(wte)
        return y

    @staticmethod
    def backward(ctx, dlogits):
        C = ext()
        (xb,) = ctx.saved_tensors
        d = dlogits.to(torch.bfloat16).contiguous()
        dx = C.linear_dgrad(d, shadow(ctx.wte, ctx.pad))
        buf, direct = grad_sink(ctx.wte)
        C.linear_wgrad(d, xb, buf, 1.0, None, None, 0, direct and grad_fresh(ctx.wte))  # padded leading dim, only the V real rows are produced
        grad_done(ctx.wte, direct)
        return dx, (None if direct else buf), None


class _LMHeadCEFn(Function):
    """Fused tied LM head + mean cross-entropy (GPT-2 training path).

    The logits never leave the op: the CE kernel holds each row in registers
    and overwrites the logits with (softmax - onehot) in place (one HBM read +
    one write of the [tokens, Vp] matrix); backward feeds that straight to the
    dgrad/wgrad GEMMs, which read the incoming loss gradient / N as a device
    scalar (``alpha_t``) -- no separate scaling pass over the 0.8 GB gradient.
    """

    @staticmethod
    def forward(ctx, x, wte, labels, pad_rows: int, ignore_index: int, label_smoothing: float = 0.0, z_loss: float = 0.0):
        C = ext()
        w16 = shadow(wte, pad_rows)
        xb = x.contiguous() if x.dtype == torch.bfloat16 else x.to(torch.bfloat16).contiguous()
        xb = xb.reshape(-1, xb.shape[-1])
        logits = C.linear_fwd(xb, w16, None, 0, False, None, None)
        lab = labels.reshape(-1).contiguous()
        out4, d = C.cross_entropy_mean(logits, lab, wte.shape[0], True, ignore_index, True,
                                       label_smoothing=label_smoothing, z_loss=z_loss)
        ctx.save_for_backward(xb, d, out4)
        ctx.wte, ctx.pad, ctx.xshape = wte, pad_rows, x.shape
        note_use(wte)
        return out4[2:3].reshape(())  # mean over the non-ignored tokens (kernel-side count)

    @staticmethod
    def backward(ctx, g):
        C = ext()
        xb, d, out4 = ctx.saved_tensors
        scale = g.float().reshape(1) * out4[3:4]  # dL/dlogits = (softmax - onehot) * g / n, applied by the GEMMs
        dx = C.linear_dgrad(d, shadow(ctx.wte, ctx.pad), None, scale)
        buf, direct = grad_sink(ctx.wte)
        C.linear_wgrad(d, xb, buf, 1.0, scale, None, 0, direct and grad_fresh(ctx.wte))
        grad_done(ctx.wte, direct)
        return dx.reshape(ctx.xshape), (None if direct else buf), None, None, None, None, None


def lm_head_ce(x, wte, labels, vocab_pad_to: int = 64, ignore_index: int = -100, label_smoothing: float = 0.0,
               z_loss: float = 0.0):
    """Mean CE of the tied LM head logits ``x @ wte^T`` against ``labels`` (fused), optionally label-smoothed
    and with ``z_loss * mean(logsumexp^2)``: both inside the CE kernel, the logits are not read again."""
    _check_ce_reg(label_smoothing, z_loss)
    if not x.is_cuda:
        logits = F.linear(x.float(), wte)
        return _ce_reference(logits.reshape(-1, logits.shape[-1]), labels.reshape(-1), ignore_index, label_smoothing, z_loss)
    V = wte.shape[0]
    Vp = (V + vocab_pad_to - 1) // vocab_pad_to * vocab_pad_to
    return _LMHeadCEFn.apply(x, wte, labels, Vp - V, ignore_index, float(label_smoothing), float(z_loss))


def lm_head(x, wte, vocab_pad_to: int = 64):
    V = wte.shape[0]
    Vp = (V + vocab_pad_to - 1) // vocab_pad_to * vocab_pad_to
    if not x.is_cuda:
        return F.linear(x.float(), wte)
    return _LMHeadFn.apply(x, wte, Vp - V)


# =============================================================== generation
# One decode step streams every weight and the KV cache once per token; its kernels (csrc/kernels/decode.hip) share
# nothing with the training tiles.  Each wrapper has a torch path for the CPU with the same semantics.
SKINNY_MAX_M = 16
# (N, K) -> the smallest M from which scripts/bench_decode.py measured Fx.linear faster than linear_skinny
# (docs/perf_notes.md, "GPT-2 decoding": GPT-2-small's five projection shapes at M = 1, 8, 16; only the LM head at
# M = 16 lost, by 4 %).  A shape that has not been measured runs on the skinny kernel: that default is an assumption
# from the byte count, not a measurement.
SKINNY_SLOWER: dict = {(50304, 768): 16}


def attn_decode(qkv_step, kc, vc, lens, n_head: int, scale: Optional[float] = None, splits: int = 0):
    """One query per (row, head) against the cache.  qkv_step [B, 3 * H * 64] (the new token's c_attn output),
    kc / vc [B, H, Tmax, 64], lens int32 [B] = tokens already cached per row (clamped into [0, Tmax - 1]).  Row b
    attends keys 0 .. lens[b]; key lens[b] is the step's own K/V, which is also stored into the cache at that
    index.  Returns [B, H * 64].  ``splits``: the number of key splits (0: a function of the launch shape)."""
    B = qkv_step.shape[0]
    D = qkv_step.numel() // (B * 3 * n_head)
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    if qkv_step.is_cuda:
        if D != 64:
            raise ValueError("attn_decode: the kernel takes head dim 64")
        return ext().attn_decode(qkv_step.reshape(B, 3, n_head, D), kc, vc, lens, float(scale), int(splits))
    Tmax = kc.shape[2]
    q, k, v = qkv_step.reshape(B, 3, n_head, D).to(kc.dtype).unbind(1)  # [B, H, D]
    L = lens.long().clamp(0, Tmax - 1)
    rows = torch.arange(B)
    kc[rows, :, L] = k
    vc[rows, :, L] = v
    seen = (torch.arange(Tmax)[None, :] <= L[:, None])[:, None, :]  # [B, 1, Tmax]
    s = torch.einsum("bhd,bhtd->bht", q.float(), kc.float()) * scale
    p = torch.softmax(torch.where(seen, s, torch.full_like(s, float("-inf"))), dim=-1)
    o = torch.einsum("bht,bhtd->bhd", p, torch.where(seen.unsqueeze(-1), vc.float(), torch.zeros((), dtype=torch.float32)))
    return o.reshape(B, n_head * D)


def linear_skinny(x, weight, bias=None, act: int = ACT_NONE, residual=None, out_f32: bool = False, pad_rows: int = 0,
                  ksplit: int = 0):
    """``linear`` / ``linear_residual`` for M <= 16 rows, no autograd: x [M, K] bf16 against the bf16 shadow of
    ``weight`` [N, K] (``pad_rows`` zero rows appended, the LM head's padding).  bf16 out with optional bias and
    GELU, or -- ``out_f32`` / ``residual`` -- fp32 out with optional bias and the fp32 residual, which is updated
    in place.  Shapes outside the kernel's envelope (M <= 16, K % 32 == 0, N % 16 == 0) or listed in SKINNY_SLOWER
    run on Fx.linear / Fx.linear_residual."""
    if act not in (ACT_NONE, ACT_GELU):
        raise ValueError("linear_skinny: act must be ACT_NONE or ACT_GELU")
    out_f32 = out_f32 or residual is not None
    if out_f32 and act != ACT_NONE:
        raise ValueError("linear_skinny: GELU goes with the bf16 output")
    with torch.no_grad():
        if not x.is_cuda:
            w = F.pad(weight, (0, 0, 0, pad_rows)) if pad_rows else weight
            if residual is not None:
                return residual.add_(F.linear(x.float(), w, bias))
            return linear(x, w, bias, act, out_f32)
        M, K = x.shape
        N = weight.shape[0] + pad_rows
        xb = x if x.dtype == torch.bfloat16 else x.to(torch.bfloat16)
        C = ext()
        if M >= SKINNY_SLOWER.get((N, K), SKINNY_MAX_M + 1) or not C.linear_skinny_ok(M, N, K, xb.stride(0) if M > 1 else K, K):
            if residual is not None:
                return linear_residual(xb, weight, bias, residual) if pad_rows == 0 else residual.add_(
                    _LinearFn.apply(xb, weight, bias, ACT_NONE, True))
            if pad_rows:
                assert bias is None and act == ACT_NONE, "a padded weight is the LM head"
                y = _LMHeadFn.apply(xb, weight, pad_rows)
                return y.float() if out_f32 else y
            return linear(xb, weight, bias, act, out_f32)
        return C.linear_skinny(xb, shadow(weight, pad_rows), bias.detach() if bias is not None else None, act == ACT_GELU,
                               out_f32, residual, residual, int(ksplit))


_sampler_states: dict = {}


def sampler_state(device) -> DropoutState:
    """The sampler's own device RNG state (seed, offset) of ``device``: a DropoutState apart from the dropout one,
    so generating between two training steps does not move the dropout masks."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    st = _sampler_states.get(device)
    if st is None:
        st = _sampler_states[device] = DropoutState(device)
    return st


def sample_keep(logits, temperature: float, top_k: int = 0, top_p: float = 1.0):
    """(s, keep) of the sampler's filters in torch ops: s = logits / temperature in fp32 and the bool mask of the
    columns that stay.  Defined on values: top-k keeps s >= the k-th largest value (ties stay); top-p then keeps j iff
    the softmax mass, over what top-k kept, of the strictly larger values is < top_p."""
    s = logits.float() / temperature
    V = s.shape[-1]
    keep = torch.ones_like(s, dtype=torch.bool)
    if 0 < top_k < V:
        keep = s >= torch.topk(s, top_k, dim=-1).values[..., -1:]
    if top_p < 1.0:
        sm = torch.where(keep, s, torch.full_like(s, float("-inf")))
        sv, order = torch.sort(sm, dim=-1, descending=True)
        pr = torch.softmax(sv, dim=-1)
        above = torch.cumsum(pr, dim=-1) - pr  # mass of the earlier entries; equal values share their group's first
        i = torch.arange(V, device=s.device).expand_as(sv)
        first = torch.cummax(torch.where(torch.cat([torch.ones_like(sv[..., :1], dtype=torch.bool),
                                                    sv[..., 1:] != sv[..., :-1]], dim=-1), i, torch.zeros_like(i)), dim=-1).values
        kept_sorted = torch.gather(above, -1, first) < top_p
        keep = keep & torch.zeros_like(keep).scatter(-1, order, kept_sorted)
    return s, keep


def sample_logits(logits, V: Optional[int] = None, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, state=None,
                  eos_id: Optional[int] = None, done=None, generator=None, stream: int = 0):
    """One token per row of ``logits`` [B, ld] (bf16 or fp32; only the first ``V`` columns are candidates) -> int64
    [B].  temperature 0: the argmax, lowest index on ties.  Otherwise s = z / temperature, the filters of
    ``sample_keep`` and the arg max over the kept columns of s + Gumbel noise, lowest index on ties.  On the GPU the
    noise is Philox from ``state`` (a DropoutState, default ``sampler_state``), which is advanced by B * ceil(V / 4);
    on the CPU it is drawn from torch's ``generator``.  ``done`` (int32 [B]) with ``eos_id``: a row whose flag is set
    emits eos_id, a row that draws eos_id sets its flag."""
    B, ld = logits.shape
    V = ld if V is None else int(V)
    if not 1 <= V <= ld:
        raise ValueError(f"sample_logits: V = {V} outside the {ld} columns")
    if not (temperature >= 0.0 and top_k >= 0 and 0.0 < top_p <= 1.0):
        raise ValueError("sample_logits: need temperature >= 0, top_k >= 0 and 0 < top_p <= 1")
    eos = -1 if eos_id is None else int(eos_id)
    if logits.is_cuda:
        if logits.dtype not in (torch.bfloat16, torch.float32):
            logits = logits.float()
        Vp = (V + 7) // 8 * 8
        if logits.stride(1) != 1 or (B > 1 and logits.stride(0) % 8) or ld < Vp or logits.data_ptr() % 16:
            logits = F.pad(logits[:, :V], (0, Vp - V))
        if state is None:
            state = sampler_state(logits.device)
        tok = ext().sample_logits(logits, V, float(temperature), int(top_k), float(top_p), state.tensor(), int(stream), eos, done)
        state.advance(B * ((V + 3) // 4))
        return tok
    z = logits[:, :V].float()
    col = torch.arange(V).expand(B, V)
    if temperature == 0.0:
        score = z
    else:
        s, keep = sample_keep(z, temperature, top_k, top_p)
        u = torch.rand(B, V, generator=generator).clamp_(min=2.0 ** -24, max=1.0 - 2.0 ** -24)
        score = torch.where(keep, s - torch.log(-torch.log(u)), torch.full_like(s, float("-inf")))
    tok = torch.where(score == score.max(dim=-1, keepdim=True).values, col, torch.full_like(col, V)).min(dim=-1).values
    if done is not None and eos >= 0:
        tok = torch.where(done != 0, torch.full_like(tok, eos), tok)
        done |= (tok == eos).to(done.dtype)
    return tok
