import torch

from .fused import LAMB, LARS, SGD, Adam, AdamW, Muon, _CLIP_BUF, _pack_desc, ema_decay_at, lr_factor, newton_schulz

__all__ = ["SGD", "Adam", "AdamW", "LARS", "LAMB", "Muon", "build_optimizer", "clip_grad_norm_", "ema_decay_at", "lr_factor",
           "newton_schulz"]


def _trust_groups(params, weight_decay, off):
    """A flat parameter list becomes two groups: matrices / filters keep the weight decay and the trust
    ratio, tensors with ndim <= 1 (biases, BatchNorm / LayerNorm gains) get neither (``off``).  Param groups
    the caller made are kept as they are."""
    params = list(params)
    if not params or isinstance(params[0], dict):
        return params
    big = [p for p in params if p.ndim > 1]
    small = [p for p in params if p.ndim <= 1]
    groups = [{"params": big}] if big else []
    if small:
        groups.append({"params": small, "weight_decay": 0.0, **off})
    return groups


def _muon_groups(params, weight_decay):
    """A flat parameter list becomes three groups: Muon for the matrices (2-D, not marked ``_dpe_muon = False``,
    every dimension of every row block a multiple of 8, the envelope of bf16 MFMA kernels), AdamW with the
    weight decay for the other tensors with ndim > 1 (embeddings, output layers, conv filters), AdamW without it
    for ndim <= 1.  Param groups the caller made are kept as they are."""
    params = list(params)
    if not params or isinstance(params[0], dict):
        return params

    def takes(p):
        s = int(getattr(p, "_dpe_muon_split", 1) or 1)
        return (p.ndim == 2 and getattr(p, "_dpe_muon", True) and p.shape[0] % s == 0 and (p.shape[0] // s) % 8 == 0
                and p.shape[1] % 8 == 0)

    groups = [{"params": [p for p in params if takes(p)], "use_muon": True},
              {"params": [p for p in params if p.ndim > 1 and not takes(p)], "use_muon": False},
              {"params": [p for p in params if p.ndim <= 1], "use_muon": False, "weight_decay": 0.0}]
    return [g for g in groups if g["params"]]


def build_optimizer(name: str, params, lr: float, weight_decay: float = 0.0, momentum=None, *,
                    clip_grad_norm=None, skip_nonfinite: bool = False, trust_coefficient=None, lr_schedule=None,
                    ns_steps=None, ema=None):
    """``ema``: a dict of ``set_ema``'s arguments (``decay`` and optionally ``warmup``).  ``lr_schedule``: a dict of ``set_lr_schedule``'s arguments (``kind``, ``total_steps`` and optionally
    ``warmup_steps``, ``min_ratio``, ``power``).  ``momentum`` defaults to 0.9, for ``"muon"`` to 0.95;
    ``ns_steps`` is Muon's."""
    if ns_steps is not None and name.lower() != "muon":
        raise ValueError(f"ns_steps is for muon, not {name!r}")
    if momentum is None:
        momentum = 0.95 if name.lower() == "muon" else 0.9
    name = name.lower()
    if lr_schedule is not None:
        lr_schedule = dict(lr_schedule)
        unknown = set(lr_schedule) - {"kind", "warmup_steps", "total_steps", "min_ratio", "power"}
        if unknown or "kind" not in lr_schedule:
            raise ValueError(f"lr_schedule: a dict with 'kind', 'total_steps' and optionally 'warmup_steps', "
                             f"'min_ratio', 'power'; got keys {sorted(lr_schedule)}")
    if ema is not None:
        ema = dict(ema)
        if set(ema) - {"decay", "warmup"} or "decay" not in ema:
            raise ValueError(f"ema: a dict with 'decay' and optionally 'warmup'; got keys {sorted(ema)}")
    if trust_coefficient is not None and name not in ("lars", "lamb"):
        raise ValueError(f"trust_coefficient is for lars / lamb, not {name!r}")
    if name == "adam":
        opt = Adam(params, lr=lr, weight_decay=weight_decay)
    elif name == "adamw":
        opt = AdamW(params, lr=lr, weight_decay=weight_decay)
    elif name == "sgd":
        opt = SGD(params, lr=lr, momentum=momentum, weight_decay=weight_decay)
    elif name == "lars":
        opt = LARS(_trust_groups(params, weight_decay, {"trust_coefficient": 0.0}), lr=lr, momentum=momentum,
                   weight_decay=weight_decay, trust_coefficient=1e-3 if trust_coefficient is None else trust_coefficient)
    elif name == "lamb":
        # LAMB's ratio has no coefficient: trust_coefficient=0 turns it off, anything else leaves it on
        if trust_coefficient is not None and not trust_coefficient >= 0.0:
            raise ValueError(f"Invalid trust_coefficient: {trust_coefficient}")
        opt = LAMB(_trust_groups(params, weight_decay, {"trust_ratio": False}), lr=lr, weight_decay=weight_decay,
                   trust_ratio=trust_coefficient is None or trust_coefficient > 0)
    elif name == "muon":
        opt = Muon(_muon_groups(params, weight_decay), lr=lr, momentum=momentum, weight_decay=weight_decay,
                   ns_steps=5 if ns_steps is None else ns_steps, scale="match_rms")
    else:
        raise ValueError(f"unknown optimizer {name!r}")
    if clip_grad_norm is not None or skip_nonfinite:
        opt.set_grad_clip(clip_grad_norm, skip_nonfinite=skip_nonfinite)
    if lr_schedule is not None:
        opt.set_lr_schedule(lr_schedule.pop("kind"), **lr_schedule)
    if ema is not None:
        opt.set_ema(ema["decay"], warmup=bool(ema.get("warmup", False)))
    return opt


# clip_grad_norm_: the device table of the last gradient set (a training loop passes the same one every step)
_clip_cache = {"key": None, "tab": None}


def _clip_table(grads):
    from ..ops._ext import ext

    key = tuple((g.data_ptr(), g.numel()) for g in grads)
    if _clip_cache["key"] != key:
        chunk = ext().optim_chunk_size()
        desc = bytearray()
        chunks = []
        for ti, g in enumerate(grads):
            desc += _pack_desc(0, g.data_ptr(), 0, 0, 0, g.numel(), 0, ti)
            chunks += [(ti, c) for c in range((g.numel() + chunk - 1) // chunk)]
        dev = grads[0].device
        _clip_cache["tab"] = (torch.frombuffer(desc, dtype=torch.uint8).to(dev),
                              torch.tensor(chunks, dtype=torch.int32).reshape(-1, 2).to(dev),
                              torch.empty(max(len(chunks), 1), dtype=torch.float32, device=dev),
                              torch.zeros(_CLIP_BUF, dtype=torch.float32, device=dev))
        _clip_cache["key"] = key
    return _clip_cache["tab"]


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """Drop-in for ``torch.nn.utils.clip_grad_norm_``.  For the 2-norm of contiguous fp32 GPU gradients it
    runs the fused optimizers' norm kernels and one in-place scale (three launches, no host
    synchronisation unless ``error_if_nonfinite``); anything else goes to torch."""
    from ..ops._ext import ext

    parameters = [parameters] if isinstance(parameters, torch.Tensor) else list(parameters)
    grads = [p.grad for p in parameters if p.grad is not None]
    fused = len(grads) > 0 and float(norm_type) == 2.0 and all(
        g.is_cuda and g.device == grads[0].device and g.dtype == torch.float32 and g.is_contiguous() and g.numel() > 0
        for g in grads)
    if not fused:
        return torch.nn.utils.clip_grad_norm_(parameters, max_norm, norm_type, error_if_nonfinite, foreach)
    with torch.cuda.device(grads[0].device):
        desc, chunks, partials, buf = _clip_table(grads)
        buf[4].fill_(float(max_norm))
        ext().optim_grad_norm(desc, chunks, partials, buf, buf[4:])
        if error_if_nonfinite and not bool(buf[2]):
            raise RuntimeError(f"The total norm of order {norm_type} for gradients from `parameters` is non-finite, "
                               "so it cannot be clipped. To disable this error and scale the gradients by the "
                               "non-finite norm anyway, set `error_if_nonfinite=False`")
        ext().optim_grad_scale(desc, chunks, buf)
        return buf[0].clone()
