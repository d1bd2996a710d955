import torch

from .fused import SGD, Adam, AdamW, _CLIP_BUF, _pack_desc

__all__ = ["SGD", "Adam", "AdamW", "build_optimizer", "clip_grad_norm_"]


def build_optimizer(name: str, params, lr: float, weight_decay: float = 0.0, momentum: float = 0.9, *,
                    clip_grad_norm=None, skip_nonfinite: bool = False):
    name = name.lower()
    if name == "adam":
        opt = Adam(params, lr=lr, weight_decay=weight_decay)
    elif name == "adamw":
        opt = AdamW(params, lr=lr, weight_decay=weight_decay)
    elif name == "sgd":
        opt = SGD(params, lr=lr, momentum=momentum, weight_decay=weight_decay)
    else:
        raise ValueError(f"unknown optimizer {name!r}")
    if clip_grad_norm is not None or skip_nonfinite:
        opt.set_grad_clip(clip_grad_norm, skip_nonfinite=skip_nonfinite)
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
