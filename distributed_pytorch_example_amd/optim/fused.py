"""Fused multi-tensor optimizers (Adam / AdamW / SGD-momentum, and the layer-wise LARS / LAMB).

Drop-in subclasses of the torch optimizers: identical constructor arguments,
identical ``state_dict()`` schema (so checkpoints interchange with the
reference's ``optim.Adam``), identical update math.  On GPU the
whole step is ONE HIP kernel launch over a device-resident (tensor, chunk)
table (csrc/kernels/optim.hip) that also refreshes each parameter's bf16
compute shadow; on CPU they defer to torch's implementation.

Replaces the reference's foreach-Adam (`train.py:249` ->
`$TORCH/optim/adam.py:554` `_multi_tensor_adam`: lerp/mul/addcmul/sqrt/div/
add/addcdiv launches per step).

Per-parameter ``step`` counters live in one device tensor (each state's
``step`` is a 0-d view of it), so a whole training step can be captured in a
hipGraph; ``lr`` and friends live in a device hyper-parameter block that the
host rewrites only when a group's values change.

Global-norm gradient clipping (``set_grad_clip``) is fused into the step: one
extra read of the gradients produces the norm on the device, a one-block
kernel turns it into the clip coefficient inside the hyper-parameter block,
and the update kernel multiplies every gradient by it.  The gradients are not
written back, the host is not involved, and the step still replays in a graph.

A learning-rate schedule (``set_lr_schedule``: warm-up, then constant / linear / cosine / polynomial decay)
is evaluated on the device too: a one-block kernel turns a device step counter into this step's lr inside the
hyper-parameter block, so no host copy happens per step and a captured step replays with an advancing lr.

An exponential moving average of the weights (``set_ema``) is one more operand of the update kernels: they
have the new weight in registers, so the average costs one load and one store per element, follows skipped
steps, graph replays and per-bucket steps, and ``ema_weights()`` swaps it in (with the bf16 shadows) for
validation.

``Muon`` (at the end of this file) shares the clip / schedule / state-dict machinery but has no GPU kernels yet:
it runs its formulas in torch ops on CPU parameters and raises on GPU parameters.
"""
from __future__ import annotations

import contextlib
import math
import struct

import torch

from ..ops._ext import ext
from ..ops import _state

_HP = 12
_CLIP_BUF = 5  # device clip block: total_norm, coef, ok, skipped steps | max_norm
_SCHED_KINDS = {"constant": 0, "linear": 1, "cosine": 2, "poly": 3}  # lr_schedule_kernel's kind


def _sched_header() -> int:
    return int(ext().optim_sched_header())


def lr_factor(s: int, kind: str, warmup_steps: int, total_steps: int, min_ratio: float = 0.0, power: float = 1.0) -> float:
    """The schedule's factor for the step taken after ``s`` scheduled steps (``set_lr_schedule``), in Python
    floats: what csrc/kernels/optim.hip's lr_schedule_kernel evaluates on the device."""
    W, T, r = warmup_steps, total_steps, min_ratio
    if s < W:
        return (s + 1.0) / W
    t = min(1.0, (s - W) / max(1.0, float(T - W)))
    if kind == "linear":
        return 1.0 - (1.0 - r) * t
    if kind == "cosine":
        return r + (1.0 - r) * (0.5 * (1.0 + math.cos(math.pi * t)))
    if kind == "poly":
        return r + (1.0 - r) * (1.0 - t) ** power
    return 1.0


def ema_decay_at(n: int, decay: float, warmup: bool = False) -> float:
    """``d_n`` of ``set_ema``: the decay of the update made after ``n`` earlier ones, in Python floats (what
    csrc/kernels/optim.hip's ema_decay_kernel evaluates on the device)."""
    if n < 1:
        return 0.0
    return min(decay, (1.0 + n) / (10.0 + n)) if warmup else decay


def _pack_desc(p, g, s1, s2, sh, n, group, ti):
    """One ``TensorDesc`` of csrc/kernels/optim.hip."""
    return struct.pack("<QQQQQqii", p, g, s1, s2, sh, n, group, ti)


class _FusedMixin:
    _kind = 0  # 0 adam, 1 sgd: the state schema and the plain update kernel
    _trust = None  # layer-wise trust ratio: None, 0 LARS, 1 LAMB (the kind of the ext().optim_trust_* calls)
    _trust_defaults = {}  # the per-group keys a trust optimizer adds to torch's

    def _fused_init(self):
        self._tab = None
        self._tab_key = None
        self._hp_key = None
        self._hp = None
        self._steps = None
        self.graph_safe = False  # when True: skip per-step host checks (caller guarantees static pointers)
        self._ov_stream = None  # DDP.overlap_optimizer: per-bucket steps during backward on this stream
        self._ov_open = False
        self._ov_done = set()
        self._ov_cache = {}
        self._clip_max = None  # set_grad_clip()
        self._clip_skip = False
        self._clip_buf = None  # allocated once per optimizer: the skipped-steps counter lives in it
        self._clip_part = None  # one partial sum of squares per (tensor, chunk), allocated with the table
        self._clip_ran = False
        self._trust_tab = None  # (first_chunk, part_w, part_x), allocated with the table
        self._trust_stats = None
        self._trust_ran = False
        self._sched_cfg = None  # set_lr_schedule(): (kind, warmup_steps, total_steps, min_ratio, power)
        self._sched = None  # device schedule block (fp64): counter, the arguments, one base lr per group
        self._sched_key = None
        self._sched_cur = None  # fp32 [n_groups]: the lr of the last scheduled step
        self._sched_ran = False
        self._sched_last = 0  # the counter while there is no device block (CPU path, a freshly loaded state)
        self._ema_cfg = None  # set_ema(): (decay, warmup)
        self._ema_blk = None  # device EMA block (fp64): updates done, decay, warm-up on / off
        self._ema_key = None
        self._ema_cur = None  # fp32 [1]: the d_n of the last step
        self._ema_ran = False
        self._ema_last = 0  # the counter while there is no device block
        self._ema_ptrs = None  # int64 [n_params] on the device: the averages' addresses, made with the table
        self._ema_swapped = False  # inside ema_weights(): the parameters hold the average
        self._swap_tab = None
        self._swap_key = None

    # ------------------------------------------------------ learning-rate schedule
    def set_lr_schedule(self, kind, *, warmup_steps: int = 0, total_steps=None, min_ratio: float = 0.0,
                        power: float = 1.0) -> None:
        """Scale every group's lr by ``f(s)`` in every following ``step()``; ``s`` counts the steps taken under
        the schedule (0 for the first).  ``kind`` is "constant", "linear", "cosine" or "poly"; ``None`` turns the
        schedule off and the base lr is used again.  With ``W = warmup_steps``, ``T = total_steps``,
        ``r = min_ratio``: ``f = (s + 1) / W`` while ``s < W``; afterwards, with
        ``t = min(1, (s - W) / max(1, T - W))``, constant ``1``, linear ``1 - (1 - r) t``, cosine
        ``r + (1 - r) (1 + cos(pi t)) / 2``, poly ``r + (1 - r) (1 - t)^power`` (past ``T`` it holds at ``r``).
        ``group["lr"]`` stays the base lr.  On GPU the factor is evaluated on the device from a device counter
        (no host copy per step; a captured step replays with an advancing lr); a step skipped by
        ``skip_nonfinite`` consumes no schedule step.  Setting a schedule again keeps the counter."""
        if kind is None:
            self._sched_cfg = None
            self._sched_ran = False
            self._hp_key = None  # the next step writes the base lr back into the hp rows
            return
        if kind not in _SCHED_KINDS:
            raise ValueError(f"set_lr_schedule: kind must be one of {sorted(_SCHED_KINDS)} or None, got {kind!r}")
        if total_steps is None:
            raise ValueError("set_lr_schedule: total_steps is required")
        W, T, r, pw = int(warmup_steps), int(total_steps), float(min_ratio), float(power)
        if W < 0:
            raise ValueError(f"set_lr_schedule: warmup_steps must be >= 0, got {warmup_steps}")
        if not T > W:
            raise ValueError(f"set_lr_schedule: total_steps ({total_steps}) must exceed warmup_steps ({warmup_steps})")
        if not 0.0 <= r <= 1.0:
            raise ValueError(f"set_lr_schedule: min_ratio must be in [0, 1], got {min_ratio}")
        if not pw > 0.0:
            raise ValueError(f"set_lr_schedule: power must be > 0, got {power}")
        self._sched_cfg = (kind, W, T, r, pw)
        if self._sched is not None:
            self._write_sched()  # device values, like max_norm: a captured step picks them up on replay

    def _sched_block(self):
        """The device schedule block, made on first use with the counter a loaded state left."""
        n = _sched_header() + len(self.param_groups)
        if self._sched is None or self._sched.numel() != n:
            dev = self._all_params()[0].device
            if self._sched is not None:
                self._sched_last = int(self._sched[0].item())
            self._sched = torch.zeros(n, dtype=torch.float64, device=dev)
            self._sched[0].fill_(float(self._sched_last))
            self._sched_cur = torch.zeros(len(self.param_groups), dtype=torch.float32, device=dev)
            self._sched_key = None
        return self._sched

    def _write_sched(self):
        """The schedule's arguments and the groups' base lrs into the device block, when they changed."""
        kind, W, T, r, pw = self._sched_cfg
        vals = [float(_SCHED_KINDS[kind]), float(W), float(T), r, pw] + [_lr(g) for g in self.param_groups]
        key = tuple(vals)
        sched = self._sched_block()
        if key != self._sched_key:
            sched[1:].copy_(torch.tensor(vals, dtype=torch.float64))
            self._sched_key = key

    def _sched_launch(self):
        """This step's lr into the hp rows (after the step's ok flag is final, before the first kernel that
        reads lr); the device counter advances by the ok flag."""
        if self._sched_cfg is not None:
            if self._sched_key is None:  # a schedule first set on a graph_safe optimizer: no block yet
                self._write_sched()
            ext().optim_lr_schedule(self._hp, self._sched, self._sched_cur)
            self._sched_ran = True

    @property
    def current_lr(self):
        """fp32 ``[n_groups]`` on the parameters' device: the lr the last scheduled step used.  ``None`` before
        the first scheduled step.  Reading it does not synchronise."""
        return self._sched_cur if self._sched_ran else None

    @property
    def schedule_step(self):
        """0-d fp64 counter on the parameters' device: the steps taken under the schedule."""
        if self._sched is not None:
            return self._sched[0]
        ps = self._all_params()
        if ps and ps[0].is_cuda:
            return self._sched_block()[0]
        return torch.tensor(float(self._sched_last), dtype=torch.float64)

    def _cpu_sched_begin(self):
        """CPU path: put ``base * f(s)`` into ``group["lr"]`` for the duration of the step."""
        if self._sched_cfg is None:
            return None
        f = lr_factor(self._sched_last, *self._sched_cfg)
        base = [g["lr"] for g in self.param_groups]
        for g in self.param_groups:
            g["lr"] = _lr(g) * f
        self._sched_cur = torch.tensor([g["lr"] for g in self.param_groups], dtype=torch.float32)
        return base

    def _cpu_sched_end(self, base):
        if base is not None:
            for g, b in zip(self.param_groups, base):
                g["lr"] = b
            self._sched_last += 1
            self._sched_ran = True

    # ------------------------------------------------------ weight EMA
    def set_ema(self, decay, *, warmup: bool = False) -> None:
        """Keep an exponential moving average of every parameter, updated inside every following ``step()``:
        with ``n`` the updates already done and ``w`` the weights the step just wrote,

            d_0 = 0 (the first update copies),  d_n = min(decay, (1 + n) / (10 + n)) if warmup else decay
            ema = ema + (1 - d_n) (w - ema)                                    (fp32, per element)

        -- ``torch.optim.swa_utils.AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(decay))`` called after
        every step, parameters only (buffers such as BatchNorm's running statistics stay the live ones).
        ``decay`` lies in [0, 1); ``None`` turns the average off and drops its state.  The average is the fp32
        state tensor ``state[p]["ema"]``.  On GPU it is one more operand of the fused update kernel, ``1 - d_n``
        comes from a device counter (``ema_num_updates``) that advances by the step's ok flag -- a step skipped
        by ``skip_nonfinite`` makes no update and consumes no warm-up step -- and a captured step replays with
        an advancing ``d_n``.  Setting it again keeps the average and the counter."""
        if self._ema_swapped:
            raise RuntimeError("set_ema: inside ema_weights() (the parameters hold the average)")
        if decay is None:
            if warmup:
                raise ValueError("set_ema: warmup needs a decay")
            if self._ema_cfg is not None:
                self._tab = self._tab_key = None  # the next step rebuilds the table without the averages
            self._ema_cfg = None
            self._ema_ran = False
            self._ema_ptrs = self._swap_tab = self._swap_key = None
            self._ema_reset()
            return
        decay = float(decay)
        if not 0.0 <= decay < 1.0:
            raise ValueError(f"set_ema: decay must be in [0, 1), got {decay}")
        if self._ema_cfg is None:
            self._tab = self._tab_key = None  # the next step rebuilds the table with the averages
        self._ema_cfg = (decay, bool(warmup))
        if self._ema_blk is not None:
            self._write_ema()  # device values: a captured step picks them up on replay

    def _ema_reset(self):
        """No average: drop the tensors, the counter restarts at 0 (whoever sets an EMA next starts afresh)."""
        for st in self.state.values():
            st.pop("ema", None)
        self._ema_last = 0
        if self._ema_blk is not None:
            self._ema_blk[0].fill_(0.0)

    @property
    def ema_config(self):
        """``{"decay", "warmup"}`` while an EMA is set, else ``None``."""
        return None if self._ema_cfg is None else {"decay": self._ema_cfg[0], "warmup": self._ema_cfg[1]}

    def _ema_block(self):
        if self._ema_blk is None:
            dev = self._all_params()[0].device
            self._ema_blk = torch.zeros(3, dtype=torch.float64, device=dev)
            self._ema_blk[0].fill_(float(self._ema_last))
            self._ema_cur = torch.zeros(1, dtype=torch.float32, device=dev)
            self._ema_key = None
        return self._ema_blk

    def _write_ema(self):
        """decay and warm-up into the device block, when they changed."""
        blk = self._ema_block()
        if self._ema_cfg != self._ema_key:
            blk[1:].copy_(torch.tensor([self._ema_cfg[0], 1.0 if self._ema_cfg[1] else 0.0], dtype=torch.float64))
            self._ema_key = self._ema_cfg

    def _ema_launch(self):
        """1 - d_n into the hp rows (after the step's ok flag is final, before the update kernel, like the lr
        schedule); the device counter advances by the ok flag."""
        if self._ema_cfg is not None:
            if self._ema_key is None:
                self._write_ema()
            ext().optim_ema_decay(self._hp, self._ema_blk, self._ema_cur)
            self._ema_ran = True

    @property
    def ema_num_updates(self):
        """0-d fp64 counter on the parameters' device: the EMA updates done."""
        if self._ema_blk is not None:
            return self._ema_blk[0]
        ps = self._all_params()
        if ps and ps[0].is_cuda:
            return self._ema_block()[0]
        return torch.tensor(float(self._ema_last), dtype=torch.float64)

    @property
    def ema_decay_now(self):
        """0-d fp32 tensor on the parameters' device: the ``d_n`` of the last step.  ``None`` before the first
        step with an EMA.  Reading it does not synchronise."""
        return self._ema_cur[0] if self._ema_ran else None

    def _ema_tensor(self, p):
        st = self.state[p]
        e = st.get("ema")
        if e is None:
            e = st["ema"] = torch.zeros_like(p, dtype=torch.float32, memory_format=torch.contiguous_format)
        return e

    def ema_parameters(self):
        """The averages, in ``param_groups`` order (zeros before the first update)."""
        if self._ema_cfg is None:
            raise RuntimeError("ema_parameters: no EMA is set (set_ema)")
        return [self._ema_tensor(p) for p in self._all_params()]

    def _ema_live(self):
        if self._ema_swapped:
            raise RuntimeError("optimizer.step() inside ema_weights(): the parameters hold the average")

    @torch.no_grad()
    def _cpu_ema(self):
        """CPU path, after an executed step: the same formula in torch ops (the first update copies, later
        ones are ``lerp_(ema, w, 1 - d_n)``, which is AveragedModel's EMA bit for bit)."""
        if self._ema_cfg is None:
            return
        d = ema_decay_at(self._ema_last, *self._ema_cfg)
        for p in self._all_params():
            e = self._ema_tensor(p)
            if self._ema_last == 0:
                e.copy_(p)
            else:
                e.lerp_(p, 1.0 - d)
        self._ema_last += 1
        self._ema_cur = torch.tensor([d], dtype=torch.float32)
        self._ema_ran = True

    @torch.no_grad()
    def swap_ema(self) -> None:
        """Exchange every parameter with its average, element for element (call it again to swap back: the
        round trip is bitwise).  On GPU one multi-tensor kernel that also writes the bf16 shadows of the new
        weights, followed by what a step does for derived shadows and cached filters.  ``step()`` refuses to
        run in between."""
        if self._ema_cfg is None:
            raise RuntimeError("swap_ema: no EMA is set (set_ema)")
        if int(self.ema_num_updates.item()) < 1:
            raise RuntimeError("swap_ema: the average has had no update yet")
        params = self._all_params()
        if self._use_fused():
            emas = [self._ema_tensor(p) for p in params]
            shs = []
            for p in params:
                sh = getattr(p, "_dpe_shadow", None)
                shs.append(sh if sh is not None and getattr(p, "_dpe_shadow_ver", -1) == p._version else None)
            key = tuple((p.data_ptr(), e.data_ptr(), sh.data_ptr() if sh is not None else 0)
                        for p, e, sh in zip(params, emas, shs))
            if key != self._swap_key:
                C = ext()
                chunk = C.optim_chunk_size()
                desc, chunks = bytearray(), []
                for ti, (p, e, sh) in enumerate(zip(params, emas, shs)):
                    if not (p.is_contiguous() and e.is_contiguous() and e.dtype == torch.float32 and e.numel() == p.numel()):
                        raise RuntimeError("swap_ema needs contiguous parameters and fp32 averages of their size")
                    desc += _pack_desc(p.data_ptr(), 0, 0, 0, sh.data_ptr() if sh is not None else 0, p.numel(), 0, ti)
                    chunks += [(ti, c) for c in range((p.numel() + chunk - 1) // chunk)]
                dev = params[0].device
                self._swap_tab = (torch.frombuffer(desc, dtype=torch.uint8).to(dev),
                                  torch.tensor(chunks, dtype=torch.int32).reshape(-1, 2).to(dev),
                                  torch.tensor([e.data_ptr() for e in emas], dtype=torch.int64).to(dev))
                self._swap_key = key
            ext().optim_ema_swap(*self._swap_tab)
            _state.after_optimizer_step()
        else:
            for p in params:
                e = self._ema_tensor(p)
                w = p.detach().clone()
                p.copy_(e)
                e.copy_(w)
        self._ema_swapped = not self._ema_swapped

    @contextlib.contextmanager
    def ema_weights(self):
        """``with optimizer.ema_weights():`` -- the model computes with the averaged weights inside (validation,
        exporting), and has its own back afterwards, bit for bit."""
        self.swap_ema()
        try:
            yield self
        finally:
            self.swap_ema()

    def state_dict(self):
        sd = super().state_dict()
        if self._ema_cfg is not None:
            n = int(self._ema_blk[0].item()) if self._ema_blk is not None else int(self._ema_last)
            sd["ema"] = {"decay": self._ema_cfg[0], "warmup": self._ema_cfg[1], "num_updates": n}
        if self._sched_cfg is not None:
            kind, W, T, r, pw = self._sched_cfg
            last = int(self._sched[0].item()) if self._sched is not None else int(self._sched_last)
            sd["lr_schedule"] = {"kind": kind, "warmup_steps": W, "total_steps": T, "min_ratio": r, "power": pw,
                                 "last_step": last}
        return sd

    # ------------------------------------------------------ gradient clipping
    def set_grad_clip(self, max_norm, *, skip_nonfinite: bool = False) -> None:
        """Clip the gradients of ALL param groups together to the global 2-norm ``max_norm`` inside every
        following ``step()`` (``torch.nn.utils.clip_grad_norm_(params, max_norm)`` followed by the step,
        except that on GPU the gradients themselves are left as they are).  ``None`` turns it off.  With
        ``skip_nonfinite`` a step whose gradient norm is inf/NaN changes nothing (parameters, states,
        shadows and ``step`` counters) and is counted in ``skipped_steps``.  Not part of ``state_dict()``."""
        if max_norm is None:
            if skip_nonfinite:
                raise ValueError("set_grad_clip: skip_nonfinite needs a max_norm")
        else:
            max_norm = float(max_norm)
            if not max_norm > 0.0:
                raise ValueError(f"set_grad_clip: max_norm must be > 0, got {max_norm}")
            if self._ov_stream is not None:
                raise RuntimeError("set_grad_clip: this optimizer steps per bucket during backward "
                                   "(DDP.overlap_optimizer), before the global gradient norm exists")
        if (max_norm is None) != (self._clip_max is None) or bool(skip_nonfinite) != self._clip_skip:
            # mode change: the next step rebuilds the table (scratch) and rewrites the hp rows (coef/ok = 1.0)
            self._tab = None
            self._tab_key = None
            self._hp_key = None
        self._clip_max, self._clip_skip = max_norm, bool(skip_nonfinite)
        if max_norm is not None and self._clip_buf is not None:
            self._clip_buf[4].fill_(max_norm)  # a device scalar, like lr: a captured step picks it up

    def _clip_scratch(self):
        if self._clip_buf is None:
            self._clip_buf = torch.zeros(_CLIP_BUF, dtype=torch.float32, device=self._all_params()[0].device)
            if self._clip_max is not None:
                self._clip_buf[4].fill_(self._clip_max)
        return self._clip_buf

    @property
    def grad_norm(self):
        """0-d fp32 tensor on the parameters' device: the gradient norm the last clipped step saw (before
        clipping).  ``None`` before the first clipped step.  Reading it does not synchronise."""
        return self._clip_buf[0] if self._clip_ran else None

    @property
    def skipped_steps(self):
        """0-d fp32 counter on the parameters' device: steps skipped for a non-finite gradient norm."""
        return self._clip_scratch()[3]

    @torch.no_grad()
    def _cpu_clip(self) -> bool:
        """torch's own clip on the optimizer's parameters; False when the step is to be skipped.  (Every CPU
        step starts here: the place that refuses to step inside ``ema_weights()``.)"""
        self._ema_live()
        if self._clip_max is None:
            return True
        params = self._all_params()
        buf = self._clip_scratch()
        norm = torch.nn.utils.get_total_norm([p.grad for p in params if p.grad is not None])
        buf[0].copy_(norm)
        self._clip_ran = True
        if self._clip_skip and not bool(torch.isfinite(norm)):
            buf[3].add_(1.0)
            return False
        torch.nn.utils.clip_grads_with_norm_(params, self._clip_max, norm)
        return True

    def _all_params(self):
        return [p for g in self.param_groups for p in g["params"]]

    def _use_fused(self) -> bool:
        ps = self._all_params()
        return len(ps) > 0 and all(p.is_cuda for p in ps)

    # -------------------------------------------------------- state setup
    def _ensure_state(self):
        params = self._all_params()
        dev = params[0].device
        if self._steps is None or self._steps.numel() != len(params):
            steps = torch.zeros(len(params), dtype=torch.float32, device=dev)
            for i, p in enumerate(params):
                st = self.state.get(p)
                if st and "step" in st:
                    steps[i] = float(st["step"])
                elif st and st.get("momentum_buffer") is not None:
                    # a stock torch.optim.SGD state has a momentum buffer but no step counter: the kernel's
                    # "first step" (b = g) must not discard the loaded buffer
                    steps[i] = 1.0
            self._steps = steps
        for i, p in enumerate(params):
            st = self.state[p]
            if self._kind == 0:
                if "exp_avg" not in st:
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            else:
                g = self._group_of(p)
                if g["momentum"] != 0 and st.get("momentum_buffer") is None:
                    st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            if st.get("step") is None or st["step"].data_ptr() != self._steps[i].data_ptr():
                st["step"] = self._steps[i]
            if self._ema_cfg is not None:
                self._ema_tensor(p)

    def _group_of(self, p):
        for g in self.param_groups:
            for q in g["params"]:
                if q is p:
                    return g
        raise KeyError

    def _build_table(self):
        C = ext()
        chunk = C.optim_chunk_size()
        params = self._all_params()
        desc = bytearray()
        chunks = []
        self._ti = {}
        gi_of = {}
        for gi, g in enumerate(self.param_groups):
            for p in g["params"]:
                gi_of[id(p)] = gi
        for ti, p in enumerate(params):
            st = self.state[p]
            if p.grad is None:
                raise RuntimeError("fused optimizer: parameter without .grad (use zero_grad(set_to_none=False) or DDP)")
            if not (p.is_contiguous() and p.grad.is_contiguous()):
                raise RuntimeError("fused optimizer needs contiguous params/grads")
            s1 = st["exp_avg"] if self._kind == 0 else st.get("momentum_buffer")
            s2 = st["exp_avg_sq"] if self._kind == 0 else None
            sh = getattr(p, "_dpe_shadow", None)
            if sh is not None and getattr(p, "_dpe_shadow_ver", -1) != p._version:
                sh = None  # stale shadow: let the layer re-cast it
            self._ti[id(p)] = ti
            if self._ema_cfg is not None:
                e = st["ema"]
                if not (e.is_contiguous() and e.dtype == torch.float32 and e.numel() == p.numel() and e.device == p.device):
                    raise RuntimeError("fused optimizer: state['ema'] must be a contiguous fp32 tensor of the parameter's size")
            desc += _pack_desc(p.data_ptr(), p.grad.data_ptr(), s1.data_ptr() if s1 is not None else 0,
                               s2.data_ptr() if s2 is not None else 0, sh.data_ptr() if sh is not None else 0,
                               p.numel(), gi_of[id(p)], ti)
            for c in range((p.numel() + chunk - 1) // chunk):
                chunks.append((ti, c))
        assert len(desc) == C.optim_desc_bytes() * len(params), "TensorDesc ABI mismatch"
        dev = params[0].device
        d = torch.frombuffer(desc, dtype=torch.uint8).to(dev)
        ck = torch.tensor(chunks, dtype=torch.int32).reshape(-1, 2).to(dev)
        self._tab = (d, ck)
        self._chunks_host = chunks
        self._ov_cache = {}
        self._ema_ptrs = None
        if self._ema_cfg is not None:
            self._ema_ptrs = torch.tensor([self.state[p]["ema"].data_ptr() for p in params], dtype=torch.int64).to(dev)
        if self._clip_max is not None:
            self._clip_part = torch.empty(max(len(chunks), 1), dtype=torch.float32, device=dev)
            self._clip_scratch()
        if self._trust is not None:
            # a tensor's chunks are contiguous in the table: tensor ti owns entries [first[ti], first[ti + 1])
            first, ti_next = [], 0
            for i, (ti, _) in enumerate(chunks):
                while ti_next <= ti:
                    first.append(i)
                    ti_next += 1
            first += [len(chunks)] * (len(params) + 1 - len(first))
            self._trust_tab = (torch.tensor(first, dtype=torch.int32).to(dev),
                               torch.zeros(max(len(chunks), 1), dtype=torch.float32, device=dev),
                               torch.zeros(max(len(chunks), 1), dtype=torch.float32, device=dev))
            if self._trust_stats is None or self._trust_stats.shape[0] != len(params) or self._trust_stats.device != dev:
                self._trust_stats = torch.zeros(len(params), 3, dtype=torch.float32, device=dev)

    def _key(self):
        ks = []
        for p in self._all_params():
            st = self.state[p]
            sh = getattr(p, "_dpe_shadow", None)
            s1 = st.get("exp_avg") if self._kind == 0 else st.get("momentum_buffer")
            s2 = st.get("exp_avg_sq") if self._kind == 0 else None
            e = st.get("ema") if self._ema_cfg is not None else None
            ks.append((p.data_ptr(), p.grad.data_ptr() if p.grad is not None else 0,
                       sh.data_ptr() if sh is not None and getattr(p, "_dpe_shadow_ver", -1) == p._version else 0,
                       s1.data_ptr() if s1 is not None else 0, s2.data_ptr() if s2 is not None else 0,
                       e.data_ptr() if e is not None else 0))
        return tuple(ks)

    def load_state_dict(self, state_dict):
        """torch's load puts fresh state tensors in ``self.state`` (the old ones go back to the caching
        allocator): drop the device table and the step counters so the next fused step rebuilds both
        from the loaded state instead of touching freed memory."""
        super().load_state_dict(state_dict)
        for g in self.param_groups:  # a stock torch.optim state has no trust keys: keep this optimizer's defaults
            for k, v in self._trust_defaults.items():
                g.setdefault(k, v)
        self._steps = None
        self._tab = None
        self._tab_key = None
        self._hp_key = None
        ls = state_dict.get("lr_schedule")
        if ls is not None:  # the checkpoint's schedule and counter; a state dict without one changes neither
            self.set_lr_schedule(ls["kind"], warmup_steps=ls["warmup_steps"], total_steps=ls["total_steps"],
                                 min_ratio=ls["min_ratio"], power=ls["power"])
            self._sched_last = int(ls["last_step"])
            if self._sched is not None:
                self._sched[0].fill_(float(self._sched_last))
            self._sched_ran = False
        es = state_dict.get("ema")
        self._ema_swapped = False
        self._swap_tab = self._swap_key = None
        if es is not None:  # the checkpoint's average, settings and counter
            self.set_ema(es["decay"], warmup=es["warmup"])
            self._ema_last = int(es["num_updates"])
            if self._ema_blk is not None:
                self._ema_blk[0].fill_(float(self._ema_last))
        else:  # a state without an average: an EMA set on this optimizer starts afresh
            self._ema_reset()
        self._ema_ran = False

    def _step_kernel(self, d, ck):
        """The plain update over chunk list ``ck``, with the EMA arm when one is set."""
        if self._ema_cfg is not None:
            ext().optim_step_ema(self._kind, d, ck, self._hp, self._steps, self._ema_ptrs)
        else:
            ext().optim_step(self._kind, d, ck, self._hp, self._steps)

    def _hp_row(self, g):
        raise NotImplementedError

    def _write_hp(self):
        rows = [self._hp_row(g) for g in self.param_groups]
        key = tuple(tuple(r) for r in rows)
        if key != self._hp_key:
            t = torch.tensor([v for r in rows for v in r], dtype=torch.float32)
            if self._hp is None or self._hp.numel() != t.numel():
                self._hp = t.to(self._all_params()[0].device)
            else:
                self._hp.copy_(t, non_blocking=False)
            self._hp_key = key

    # -------------------------------------------- optimizer in backward (DDP.overlap_optimizer)
    def _ov_attach(self, stream):
        if self._trust is not None:
            raise RuntimeError("overlap_optimizer: a layer-wise trust ratio needs every tensor's whole gradient and a "
                               "grid-wide step between backward and the update; it cannot step per bucket")
        self._ov_stream, self._ov_open, self._ov_done = stream, False, set()

    def _ov_detach(self):
        if self._ov_open:
            # buckets of this iteration were already stepped during backward: detaching now would leave
            # the rest for a normal step() that re-steps everything (a silent double update)
            raise RuntimeError("overlap_optimizer(enable=False) between backward and optimizer.step(): "
                               "call optimizer.step() first to finish the iteration's overlapped update")
        self._ov_stream, self._ov_open = None, False

    def _ov_launch(self, tis, stream):
        """The fused kernel over the chunks of tensors ``tis`` only (chunk lists cached per bucket)."""
        key = tuple(tis)
        ck = self._ov_cache.get(key)
        if ck is None:
            want = set(key)
            ck = torch.tensor([c for c in self._chunks_host if c[0] in want], dtype=torch.int32).reshape(-1, 2).to(
                self._tab[0].device)
            self._ov_cache[key] = ck
        with torch.cuda.stream(stream):
            self._step_kernel(self._tab[0], ck)
        self._ov_done.update(key)

    @torch.no_grad()
    def _ov_bucket_step(self, params, stream):
        """Step ``params`` (one DDP bucket whose gradients are final and whose readers have returned) on
        ``stream``, which the caller has already ordered after them.  The first bucket of an iteration
        refreshes the device table / hyper-parameters and advances every step counter once."""
        if not self._ov_open:
            self._ema_live()
            with torch.cuda.stream(stream):
                self._ensure_state()
                key = self._key()
                if key != self._tab_key:
                    self._build_table()
                    self._tab_key = key
                self._write_hp()
                if self._sched_cfg is not None:
                    self._write_sched()
                    self._sched_launch()  # nothing grid-wide precedes the update here: ok is the host's 1.0
                if self._ema_cfg is not None:
                    self._write_ema()
                    self._ema_launch()
                self._steps.add_(1.0)
            self._ov_open, self._ov_done = True, set()
        tis = sorted({self._ti[id(p)] for p in params if id(p) in self._ti} - self._ov_done)
        if tis:
            self._ov_launch(tis, stream)

    @torch.no_grad()
    def _fused_step(self):
        if self._ov_open:
            # the buckets were stepped during backward: step anything left, then join the stream
            rest = [ti for ti in range(len(self._all_params())) if ti not in self._ov_done]
            if rest:
                self._ov_launch(rest, self._ov_stream)
            torch.cuda.current_stream().wait_stream(self._ov_stream)
            self._ov_open = False
            _state.after_optimizer_step()
            return
        self._ema_live()
        if not self.graph_safe or self._tab is None:
            self._ensure_state()
            key = self._key()
            if key != self._tab_key:
                self._build_table()
                self._tab_key = key
            self._write_hp()
            if self._sched_cfg is not None:
                self._write_sched()
            if self._ema_cfg is not None:
                self._write_ema()
        d, ck = self._tab
        if self._trust is not None:
            self._trust_step(d, ck)
            _state.after_optimizer_step()
            return
        if self._clip_max is not None:
            # norm -> coef (and ok) into the hp rows, all on the device; a skipped step advances no counter
            buf = self._clip_buf
            ext().optim_grad_norm(d, ck, self._clip_part, buf, buf[4:], self._hp, self._clip_skip)
            self._clip_ran = True
            self._steps.add_(buf[2] if self._clip_skip else 1.0)
        else:
            self._steps.add_(1.0)
        self._sched_launch()
        self._ema_launch()
        self._step_kernel(d, ck)
        _state.after_optimizer_step()

    # ------------------------------------------------------ layer-wise trust ratios (LARS / LAMB)
    def _trust_step(self, d, ck):
        """partials -> per-tensor ratio -> update, all on the device (csrc/kernels/optim.hip).  LARS takes
        the gradient's partials together with the weight's, and the clip coefficient from those; LAMB's
        phase 1 needs the clipped gradient (and the advanced step counter), so the clip pair runs first."""
        C = ext()
        first, pw, px = self._trust_tab
        nck = ck.size(0)
        clip, buf = self._clip_max is not None, self._clip_buf
        if self._trust == 0:
            C.optim_trust_partials(0, d, ck, self._hp, self._steps, pw, px)
            if clip:
                C.optim_clip_coef(px, nck, buf, buf[4:], self._hp, self._clip_skip)
        elif clip:
            C.optim_grad_norm(d, ck, self._clip_part, buf, buf[4:], self._hp, self._clip_skip)
        if clip:
            self._clip_ran = True
        self._steps.add_(buf[2] if clip and self._clip_skip else 1.0)  # a skipped step advances no counter
        self._sched_launch()  # ok is final; LARS's update and LAMB's phase 2 (the readers of lr) come after
        self._ema_launch()
        if self._trust == 1:
            C.optim_trust_partials(1, d, ck, self._hp, self._steps, pw, px)
        C.optim_trust_ratio(self._trust, d, first, nck, pw, px, self._hp, self._trust_stats)
        if self._ema_cfg is not None:
            C.optim_trust_step_ema(self._trust, d, ck, self._hp, self._steps, self._trust_stats, self._ema_ptrs)
        else:
            C.optim_trust_step(self._trust, d, ck, self._hp, self._steps, self._trust_stats)
        self._trust_ran = True

    @property
    def trust_stats(self):
        """fp32 ``[n_params, 3]`` on the parameters' device, rows in ``param_groups`` order: weight norm,
        gradient norm (LARS, after clipping) or update norm (LAMB), trust ratio -- of the last step that
        was not skipped.  ``None`` before the first step and for optimizers without a trust ratio.
        Reading it does not synchronise."""
        return self._trust_stats if self._trust_ran else None

    def _group_trust_on(self, g) -> bool:
        return False

    def trust_on(self):
        """bool ``[n_params]`` (host): whether the tensor's group applies a trust ratio."""
        return torch.tensor([self._group_trust_on(g) for g in self.param_groups for _ in g["params"]], dtype=torch.bool)

    def _set_trust_defaults(self, **kw):
        self._trust_defaults = dict(kw)
        self.defaults.update(kw)
        for g in self.param_groups:
            for k, v in kw.items():
                g.setdefault(k, v)

    def _cpu_stats(self, rows):
        self._trust_stats = torch.tensor(rows, dtype=torch.float32).reshape(-1, 3)
        self._trust_ran = True


def _lr(g):
    lr = g["lr"]
    return float(lr.item() if torch.is_tensor(lr) else lr)


class Adam(_FusedMixin, torch.optim.Adam):
    """torch.optim.Adam with a one-launch fused HIP step on GPU."""

    _kind = 0
    _decoupled = False

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, *,
                 maximize=False, **kw):
        if amsgrad:
            raise NotImplementedError("amsgrad is not supported by the fused kernel")
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False,
                         maximize=maximize, **kw)
        self._fused_init()

    def _hp_row(self, g):
        flags = (2 if g.get("maximize", False) else 0) | (4 if (self._decoupled or g.get("decoupled_weight_decay", False)) else 0)
        b1, b2 = g["betas"]
        return [_lr(g), float(b1), float(b2), float(g["eps"]), float(g["weight_decay"]), float(flags), 1.0, 1.0, 1.0] + [0.0] * (_HP - 9)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self._use_fused():
            self._fused_step()
            return loss
        if not self._cpu_clip():
            return None
        base = self._cpu_sched_begin()
        # torch's Adam initialises a parameter's state only while it is empty: an average made before the first step
        # (ema_parameters()) steps aside for it
        early = [(st, st.pop("ema")) for st in self.state.values() if len(st) == 1 and "ema" in st]
        try:
            out = super().step()
        finally:
            for st, e in early:
                st["ema"] = e
            self._cpu_sched_end(base)
        self._cpu_ema()
        return out


class AdamW(Adam):
    _decoupled = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, **kw):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad,
                         decoupled_weight_decay=True, **kw)


class SGD(_FusedMixin, torch.optim.SGD):
    """torch.optim.SGD (momentum / nesterov / weight decay) with a fused HIP step on GPU."""

    _kind = 1

    def __init__(self, params, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, *,
                 maximize=False, **kw):
        super().__init__(params, lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                         nesterov=nesterov, maximize=maximize, **kw)
        self._fused_init()

    def _hp_row(self, g):
        flags = (1 if g["nesterov"] else 0) | (2 if g.get("maximize", False) else 0)
        return [_lr(g), float(g["momentum"]), float(g["dampening"]), 0.0, float(g["weight_decay"]), float(flags), 1.0, 1.0, 1.0] + [
            0.0] * (_HP - 9)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self._use_fused():
            self._fused_step()
            return loss
        if not self._cpu_clip():
            return None
        base = self._cpu_sched_begin()
        try:
            out = super().step()
        finally:
            self._cpu_sched_end(base)
        self._cpu_ema()
        return out


class LARS(SGD):
    """Layer-wise adaptive rate scaling (You, Gitman & Ginsburg 2017) on the fused SGD: per tensor

        ratio = trust_coefficient * |w| / (|g'| + weight_decay * |w| + trust_eps)   (1 if a norm is 0 / NaN)
        d     = ratio * (g' + weight_decay * w)

    and then torch SGD's momentum / dampening / nesterov rule on ``d`` with weight decay 0.  ``g'`` is the
    gradient after global-norm clipping (``set_grad_clip``) and ``maximize``.  ``trust_coefficient`` and
    ``trust_eps`` are per-group keys; a group with ``trust_coefficient == 0`` is plain SGD.  The state keeps
    SGD's schema, so a ``torch.optim.SGD`` state loads.  On GPU: one read of w and g for the partial sums,
    one wave per tensor for the ratios, one update launch; no host work, graph-replayable."""

    _trust = 0

    def __init__(self, params, lr=1e-3, momentum=0.9, dampening=0.0, weight_decay=0.0, nesterov=False,
                 trust_coefficient=1e-3, trust_eps=1e-8, *, maximize=False, **kw):
        if not trust_coefficient >= 0.0:
            raise ValueError(f"Invalid trust_coefficient: {trust_coefficient}")
        if not trust_eps >= 0.0:
            raise ValueError(f"Invalid trust_eps: {trust_eps}")
        super().__init__(params, lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                         nesterov=nesterov, maximize=maximize, **kw)
        self._set_trust_defaults(trust_coefficient=float(trust_coefficient), trust_eps=float(trust_eps))
        for g in self.param_groups:
            if not (g["trust_coefficient"] >= 0.0 and g["trust_eps"] >= 0.0):
                raise ValueError("Invalid trust_coefficient / trust_eps in a param group")

    def _group_trust_on(self, g):
        return g["trust_coefficient"] > 0

    def _hp_row(self, g):
        row = super()._hp_row(g)
        row[9], row[10] = float(g["trust_coefficient"]), float(g["trust_eps"])
        return row

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self._use_fused():
            self._fused_step()
            return loss
        if not self._cpu_clip():
            return None
        base = self._cpu_sched_begin()
        try:
            self._cpu_update()
        finally:
            self._cpu_sched_end(base)
        self._cpu_ema()
        return loss

    def _cpu_update(self):
        rows = []
        for group in self.param_groups:
            lr, mom, damp, wd = _lr(group), group["momentum"], group["dampening"], group["weight_decay"]
            tc, te = group["trust_coefficient"], group["trust_eps"]
            for p in group["params"]:
                if p.grad is None:
                    rows.append([float(p.norm()), 0.0, 1.0])
                    continue
                g = -p.grad if group.get("maximize", False) else p.grad
                wn, gn = p.norm(), g.norm()
                ratio = tc * wn / (gn + wd * wn + te) if (tc > 0 and wn > 0 and gn > 0) else torch.ones(())
                rows.append([float(wn), float(gn), float(ratio)])
                d = (g + wd * p) * ratio
                st = self.state[p]
                st["step"] = st.get("step", torch.zeros((), dtype=torch.float32)) + 1.0
                if mom != 0:
                    buf = st.get("momentum_buffer")
                    if buf is None:
                        buf = st["momentum_buffer"] = d.clone()
                    else:
                        buf.mul_(mom).add_(d, alpha=1.0 - damp)
                    d = d.add(buf, alpha=mom) if group["nesterov"] else buf
                p.add_(d, alpha=-lr)
        self._cpu_stats(rows)


class LAMB(Adam):
    """LAMB (You et al. 2020) on the fused Adam machinery: with ``t`` the step counter after its increment,

        m = lerp(m, g', 1 - b1),  v = b2 * v + (1 - b2) * g'^2
        u = (m / (1 - b1^t)) / (sqrt(v / (1 - b2^t)) + eps) + weight_decay * w
        w -= lr * (|w| / |u|) * u                                  (ratio 1 if a norm is 0 / NaN)

    The weight decay sits inside ``u``, before the ratio (not AdamW's decoupled multiply).  ``trust_ratio`` is
    a per-group key; a group with it off takes ``w -= lr * u``.  The state keeps Adam's schema, so a
    ``torch.optim.AdamW`` state loads.  On GPU the step is two passes around the per-tensor ratio kernel:
    phase 1 writes m, v and the partial sums of w^2 and u^2, phase 2 recomputes the same u and writes w."""

    _trust = 1

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, trust_ratio=True, *,
                 maximize=False, **kw):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, maximize=maximize, **kw)
        self._set_trust_defaults(trust_ratio=bool(trust_ratio))

    def _group_trust_on(self, g):
        return bool(g["trust_ratio"])

    def _hp_row(self, g):
        b1, b2 = g["betas"]
        return [_lr(g), float(b1), float(b2), float(g["eps"]), float(g["weight_decay"]), 2.0 if g.get("maximize", False) else 0.0,
                1.0, 1.0, 1.0, 1.0 if g["trust_ratio"] else 0.0, 0.0, 0.0]

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self._use_fused():
            self._fused_step()
            return loss
        if not self._cpu_clip():
            return None
        base = self._cpu_sched_begin()
        try:
            self._cpu_update()
        finally:
            self._cpu_sched_end(base)
        self._cpu_ema()
        return loss

    def _cpu_update(self):
        rows = []
        for group in self.param_groups:
            lr, (b1, b2), eps, wd = _lr(group), group["betas"], group["eps"], group["weight_decay"]
            for p in group["params"]:
                if p.grad is None:
                    rows.append([float(p.norm()), 0.0, 1.0])
                    continue
                g = -p.grad if group.get("maximize", False) else p.grad
                st = self.state[p]
                if "exp_avg" not in st:
                    st["step"] = torch.zeros((), dtype=torch.float32)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["step"] = st["step"] + 1.0
                t = float(st["step"])
                m, v = st["exp_avg"], st["exp_avg_sq"]
                m.lerp_(g, 1.0 - b1)
                v.mul_(b2).addcmul_(g, g, value=1.0 - b2)
                u = (m / (1.0 - b1 ** t)) / ((v / (1.0 - b2 ** t)).sqrt() + eps) + wd * p
                wn, un = p.norm(), u.norm()
                ratio = wn / un if (group["trust_ratio"] and wn > 0 and un > 0) else torch.ones(())
                rows.append([float(wn), float(un), float(ratio)])
                p.add_(u * ratio, alpha=-lr)
        self._cpu_stats(rows)


# ------------------------------------------------------------------ Muon
NS_COEFFICIENTS = (3.4445, -4.7750, 2.0315)
_MUON_SCALES = ("match_rms", "spectral")


def muon_gamma(scale: str, rows: int, cols: int) -> float:
    """The update's scale for one orthogonalised ``[rows, cols]`` block."""
    if scale == "match_rms":
        return 0.2 * math.sqrt(max(rows, cols))
    if scale == "spectral":
        return math.sqrt(max(1.0, rows / cols))
    raise ValueError(f"Muon: scale must be one of {_MUON_SCALES}, got {scale!r}")


def newton_schulz(u, ns_steps: int = 5, coefficients=NS_COEFFICIENTS):
    """``NS_k(u)`` of one fp32 ``[rows, cols]`` block in torch ops: ``X = u / (|u|_F + 1e-7)`` rounded to bf16,
    then ``ns_steps`` times ``A = X X^T, B = b A + c A A, X = a X + B X`` (a tall block takes the Gram matrix of
    its short side: ``A = X^T X, X = a X + X B``; no transposed copy).  ``X``, ``A`` and ``B`` are bf16 tensors
    between the products; every product takes bf16 operands and accumulates in fp32, and its epilogue
    (``b A + c acc``, ``a X + acc``) is rounded to bf16 once.  Returns bf16."""
    a, b, c = (float(v) for v in coefficients)
    X = (u.float() / (u.float().norm() + 1e-7)).bfloat16()
    tall = X.shape[0] > X.shape[1]
    for _ in range(int(ns_steps)):
        Xf = X.float()
        A = (Xf.T @ Xf if tall else Xf @ Xf.T).bfloat16()
        Af = A.float()
        B = (b * Af + c * (Af @ Af)).bfloat16()
        X = (a * Xf + (Xf @ B.float() if tall else B.float() @ Xf)).bfloat16()
    return X


def _muon_split(p) -> int:
    return int(getattr(p, "_dpe_muon_split", 1) or 1)


class Muon(_FusedMixin, torch.optim.Optimizer):
    """Muon (momentum SGD with a Newton-Schulz-orthogonalised update) for the hidden weight matrices and the
    AdamW rule for everything else, in one optimizer.  The per-group key ``use_muon`` selects the rule.  For a
    ``[rows, cols]`` parameter of a Muon group, with ``g'`` the gradient after clipping and ``maximize``:

        buf = buf + (1 - momentum) (g' - buf)
        u   = g' + momentum (buf - g')   if nesterov else   buf
        O   = NS_k(u)                    per block when ``p._dpe_muon_split = s`` splits the rows in s blocks
        W   = W (1 - lr weight_decay) - lr gamma O

    ``NS_k``: ``newton_schulz`` above.  ``gamma`` is ``0.2 sqrt(max(rows, cols))`` of the block for
    ``scale="match_rms"`` (the update's RMS is about AdamW's, so one lr and one weight decay serve both kinds of
    group) and ``sqrt(max(1, rows / cols))`` for ``"spectral"``.  Muon groups keep SGD's state schema
    (``momentum_buffer``); the other groups take torch.optim.AdamW's own update and state keys, so on them the
    result is ``optim.AdamW``'s bit for bit.  ``set_grad_clip`` (one global norm over all groups),
    ``set_lr_schedule``, ``grad_norm``, ``current_lr`` and the state dict work as for the other optimizers.

    The formulas run in torch ops on CPU parameters.  There are no GPU kernels for it yet: a step on GPU
    parameters raises instead of falling back to eager torch (docs/perf_notes.md, "Muon")."""

    _kind = 0
    _whole_matrix = True  # DDP.overlap_optimizer refuses it: whole matrices, after the whole backward

    def __init__(self, params, lr=1e-3, momentum=0.95, nesterov=True, ns_steps=5, ns_coefficients=NS_COEFFICIENTS,
                 scale="match_rms", weight_decay=0.0, betas=(0.9, 0.999), eps=1e-8, use_muon=True, *, maximize=False):
        defaults = dict(lr=lr, use_muon=bool(use_muon), momentum=momentum, nesterov=bool(nesterov), ns_steps=ns_steps,
                        ns_coefficients=tuple(ns_coefficients), scale=scale, weight_decay=weight_decay, betas=tuple(betas),
                        eps=eps, maximize=bool(maximize))
        super().__init__(params, defaults)
        for g in self.param_groups:
            self._check_group(g)
        self._fused_init()

    @staticmethod
    def _check_group(g):
        if not _lr(g) >= 0.0:
            raise ValueError(f"Invalid learning rate: {g['lr']}")
        if not g["weight_decay"] >= 0.0:
            raise ValueError(f"Invalid weight_decay value: {g['weight_decay']}")
        if g["use_muon"]:
            if not 0.0 <= g["momentum"] < 1.0:
                raise ValueError(f"Muon: momentum must be in [0, 1), got {g['momentum']}")
            if int(g["ns_steps"]) != g["ns_steps"] or g["ns_steps"] < 1:
                raise ValueError(f"Muon: ns_steps must be a positive integer, got {g['ns_steps']}")
            if len(tuple(g["ns_coefficients"])) != 3:
                raise ValueError("Muon: ns_coefficients is (a, b, c)")
            if g["scale"] not in _MUON_SCALES:
                raise ValueError(f"Muon: scale must be one of {_MUON_SCALES}, got {g['scale']!r}")
            for p in g["params"]:
                if p.ndim != 2:
                    raise ValueError(f"Muon: a use_muon group takes 2-D parameters, got shape {tuple(p.shape)}")
                if p.shape[0] % _muon_split(p) != 0:
                    raise ValueError(f"Muon: _dpe_muon_split = {_muon_split(p)} does not divide {p.shape[0]} rows")
        else:
            b1, b2 = g["betas"]
            if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0 and g["eps"] >= 0.0):
                raise ValueError("Muon: invalid betas / eps in an AdamW group")

    def _ov_attach(self, stream):
        raise RuntimeError("overlap_optimizer: Muon orthogonalises whole matrices after the whole backward; it cannot "
                           "step per bucket")

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if any(p.is_cuda for p in self._all_params()):
            raise NotImplementedError("optim.Muon has no GPU kernels yet (batched Newton-Schulz GEMMs); it steps CPU "
                                      "parameters only and does not fall back to eager torch ops on the GPU")
        if not self._cpu_clip():
            return None
        base = self._cpu_sched_begin()
        try:
            self._cpu_update()
        finally:
            self._cpu_sched_end(base)
        self._cpu_ema()
        return loss

    def _cpu_update(self):
        from torch.optim.adam import adam

        for group in self.param_groups:
            lr, wd, mx = _lr(group), group["weight_decay"], group.get("maximize", False)
            ps = [p for p in group["params"] if p.grad is not None]
            for p in ps:
                st = self.state[p]
                if "step" not in st:
                    st["step"] = torch.zeros((), dtype=torch.float32)
                    for k in (("momentum_buffer",) if group["use_muon"] else ("exp_avg", "exp_avg_sq")):
                        st[k] = torch.zeros_like(p, memory_format=torch.preserve_format)
            if not group["use_muon"]:
                b1, b2 = group["betas"]
                if ps:  # torch.optim.AdamW's own call, so the result is optim.AdamW's bit for bit
                    adam(ps, [p.grad for p in ps], [self.state[p]["exp_avg"] for p in ps],
                         [self.state[p]["exp_avg_sq"] for p in ps], [], [self.state[p]["step"] for p in ps], amsgrad=False,
                         beta1=b1, beta2=b2, lr=lr, weight_decay=wd, eps=group["eps"], maximize=mx,
                         decoupled_weight_decay=True)
                continue
            mom = group["momentum"]
            for p in ps:
                st = self.state[p]
                st["step"] += 1.0
                g = -p.grad if mx else p.grad
                buf = st["momentum_buffer"]
                buf.add_((g - buf) * (1.0 - mom))
                u = g + mom * (buf - g) if group["nesterov"] else buf
                s = _muon_split(p)
                rows = p.shape[0] // s
                gamma = muon_gamma(group["scale"], rows, p.shape[1])
                p.mul_(1.0 - lr * wd)
                for b in range(s):
                    O = newton_schulz(u[b * rows:(b + 1) * rows], group["ns_steps"], group["ns_coefficients"])
                    p[b * rows:(b + 1) * rows].add_(O.float(), alpha=-lr * gamma)
