"""Training application -- CLI-, log- and checkpoint-compatible with the
reference `train.py` (`train.py:212-318`), executed on the MI355X stack.

Same 6 flags with the same defaults (`train.py:213-221`), the same log lines
(`train.py:77-80,226-247,285-316`), the same per-epoch flow (set_epoch ->
train -> validate -> metric all-reduce / world -> rank-0 checkpoints ->
barrier) and the same checkpoint files/keys.  Additive flags select the
BASELINE-scope models, backend, bucket size, grad accumulation, etc.

Deliberate fixes: resume is read by rank 0 and broadcast; the
training loss is accumulated on the device (the reference forces a device
sync with ``loss.item()`` every step, `train.py:141`); synthetic data lives in
HBM (no DataLoader worker processes, no per-batch H2D) unless ``--loader torch``.
"""
from __future__ import annotations

import argparse
import os
import time

import torch
from torch.distributed.elastic.multiprocessing.errors import record

from .data import BatchMixer, SyntheticDataset, SyntheticTokens, create_data_loader
from .models import get_model
from .ops import functional as Fx
from .optim import build_optimizer
from .parallel import DDP
from .parallel import dist as pdist
from .utils.checkpoint import load_checkpoint, resume_exists, save_checkpoint, wait_pending
from .utils.env import ensure_single_process_env
from .utils.logging import get_logger
from .utils import fault, tracing

logger = get_logger("__main__")


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser()
    # ---- reference flags (train.py:213-221), identical names and defaults
    p.add_argument("--epochs", type=int, default=10)
    p.add_argument("--batch-size", type=int, default=64)
    p.add_argument("--lr", type=float, default=0.001)
    p.add_argument("--num-samples", type=int, default=10000)
    p.add_argument("--checkpoint-dir", type=str, default="./checkpoints")
    p.add_argument("--resume", type=str, default=None)
    # ---- additive
    p.add_argument("--model", default="simplenet", choices=["simplenet", "resnet50", "resnet_tiny", "gpt2", "gpt2-tiny",
                                                                   "vit-tiny", "vit-s16", "vit-b16"])
    p.add_argument("--backend", default="auto", choices=["auto", "rccl", "nccl", "gloo"])
    p.add_argument("--dtype", default=None, choices=[None, "fp32", "bf16"],
                   help="compute dtype on the GPU (default: fp32 for simplenet as the reference, bf16 otherwise; "
                        "fp32 masters and gradients always)")
    p.add_argument("--optimizer", default=None, choices=[None, "adam", "adamw", "sgd", "lars", "lamb", "muon"])
    p.add_argument("--muon-momentum", type=float, default=None, help="--optimizer muon: the momentum (default 0.95)")
    p.add_argument("--muon-ns-steps", type=int, default=None,
                   help="--optimizer muon: Newton-Schulz iterations per step (default 5)")
    p.add_argument("--trust-coefficient", type=float, default=None,
                   help="--optimizer lars: the trust coefficient (default 1e-3); lamb: 0 turns the trust ratio off")
    p.add_argument("--weight-decay", type=float, default=0.0)
    p.add_argument("--clip-grad-norm", type=float, default=None,
                   help="clip gradients to this global 2-norm inside the optimizer step (default: off)")
    p.add_argument("--skip-nonfinite-steps", action="store_true",
                   help="with --clip-grad-norm: a step whose gradient norm is inf/NaN changes nothing")
    p.add_argument("--lr-schedule", default=None, choices=["constant", "linear", "cosine", "poly"],
                   help="scale --lr per optimizer step, on the device: linear warm-up over --warmup-steps, then this decay "
                        "down to --lr-min-ratio at the run's last step (epochs x optimizer steps per epoch); default: off")
    p.add_argument("--warmup-steps", type=int, default=None, help="with --lr-schedule: warm-up steps (default 0)")
    p.add_argument("--lr-min-ratio", type=float, default=None,
                   help="with --lr-schedule: the factor the decay ends at, in [0, 1] (default 0)")
    p.add_argument("--lr-power", type=float, default=None, help="with --lr-schedule poly: the exponent (default 1)")
    p.add_argument("--label-smoothing", type=float, default=0.0,
                   help="label smoothing of the training loss, in [0, 1), inside the fused cross-entropy kernel; the "
                        "validation loss stays the plain cross-entropy, the logged train loss includes the regularisers")
    p.add_argument("--z-loss", type=float, default=0.0,
                   help="weight of the z-loss (mean logsumexp^2) added to the training loss; validation stays plain")
    p.add_argument("--mixup-alpha", type=float, default=0.0,
                   help="mixup: blend every training batch with itself rolled by one, lam ~ Beta(alpha, alpha) drawn on the "
                        "device per step (0: off); on the GPU the blend happens inside the pass that packs the images and "
                        "the fused cross-entropy takes both labels; validation stays plain; not for gpt2 models")
    p.add_argument("--cutmix-alpha", type=float, default=0.0,
                   help="cutmix: paste torchvision's random box from the rolled batch, area 1 - lam, lam ~ Beta(alpha, alpha) "
                        "(0: off; image models only)")
    p.add_argument("--mix-prob", type=float, default=None,
                   help="with --mixup-alpha / --cutmix-alpha: the probability of mixing a batch at all (default 1)")
    p.add_argument("--mix-switch-prob", type=float, default=None,
                   help="with both alphas: the probability of cutmix over mixup (default 0.5)")
    p.add_argument("--dropout", type=float, default=0.0,
                   help="gpt2 models: dropout rate in [0, 1) on the embedding sum, the attention probabilities (inside "
                        "the flash kernels, at the 8-bit rate round(256 p) / 256) and both residual branches; training "
                        "only (validation runs in eval mode); the mask state lives on the device and is not checkpointed")
    p.add_argument("--ema-decay", type=float, default=None,
                   help="keep an exponential moving average of the weights with this decay, in [0, 1), inside the optimizer "
                        "step; every epoch validates a second time with the averaged weights and the checkpoints carry them "
                        "in the optimizer state (default: off)")
    p.add_argument("--ema-warmup", action="store_true",
                   help="with --ema-decay: the decay of update n is min(decay, (1 + n) / (10 + n))")
    p.add_argument("--bucket-mb", type=float, default=None,
                   help="gradient bucket cap (default: the 7-link xGMI policy, parallel/buckets.py)")
    p.add_argument("--last-bucket-mb", type=float, default=None,
                   help="re-split the last-ready gradient bucket into pieces of at most this size (0: off; "
                        "default: policy, 2 MiB)")
    p.add_argument("--comm-max-channels", type=int, default=None,
                   help="cap RCCL's channels (= CUs a collective occupies while it overlaps backward)")
    p.add_argument("--grad-accum", type=int, default=1)
    p.add_argument("--seed", type=int, default=None, help="seed the synthetic data (reference: unseeded)")
    p.add_argument("--loader", default="auto", choices=["auto", "device", "torch"])
    p.add_argument("--image-size", type=int, default=None,
                   help="resnet and vit models: the square input size (default 224; vit-tiny 32)")
    p.add_argument("--seq-len", type=int, default=1024)
    p.add_argument("--doc-len-mean", type=float, default=None,
                   help="gpt2 models: pack documents of this mean length (geometric) into every row; attention stays "
                        "inside a document, positions restart, targets across a boundary are ignored")
    p.add_argument("--max-steps", type=int, default=None, help="stop each epoch after this many steps")
    p.add_argument("--async-checkpoint", action="store_true")
    p.add_argument("--auto-resume", action="store_true", help="resume from <checkpoint-dir>/latest_model.pt if present")
    p.add_argument("--profile", type=str, default=None, help="write a torch.profiler chrome trace to this path")
    p.add_argument("--roctx", action="store_true", help="roctx ranges (forward/backward/optimizer) for rocprofv3")
    p.add_argument("--gradient-compression", default="none", choices=["none", "bf16"],
                   help="all-reduce bf16 copies of the fp32 gradient buckets")
    p.add_argument("--ddp-debug", action="store_true", help="cross-rank bucket-layout check + per-bucket stream sync")
    p.add_argument("--watchdog-timeout", type=float, default=None,
                   help="abort the job when no training step completes for this many seconds or RCCL reports an "
                        "async error (0 = off; default: 1800 s -- the reference's gloo collective timeout -- on the "
                        "rccl backend at world > 1, off otherwise)")
    p.add_argument("--watchdog-checkpoint-grace", type=float, default=600.0,
                   help="extra seconds the watchdog allows in the end-of-epoch barrier (rank 0 writes checkpoints)")
    return p


def _datasets(args, device):
    if args.model == "simplenet":
        tr = SyntheticDataset(args.num_samples, 784, 10, seed=args.seed)
        va = SyntheticDataset(args.num_samples // 10, 784, 10, seed=None if args.seed is None else args.seed + 1)
        return tr, va, 10
    if args.model.startswith(("resnet", "vit")):
        shp = (3, args.image_size, args.image_size)
        ncls = 1000 if args.model in ("resnet50", "vit-s16", "vit-b16") else 10
        tr = SyntheticDataset(args.num_samples, shp, ncls, seed=args.seed)
        va = SyntheticDataset(max(1, args.num_samples // 10), shp, ncls, seed=None if args.seed is None else args.seed + 1)
        return tr, va, ncls
    vocab = 50257 if args.model == "gpt2" else 512
    tr = SyntheticTokens(args.num_samples, args.seq_len, vocab, seed=args.seed, doc_len_mean=args.doc_len_mean)
    va = SyntheticTokens(max(1, args.num_samples // 10), args.seq_len, vocab, seed=None if args.seed is None else args.seed + 1,
                         doc_len_mean=args.doc_len_mean)
    return tr, va, vocab


def train_epoch(model, loader, optimizer, criterion, device, epoch, rank, grad_accum=1, max_steps=None, watchdog=None,
                fused_loss=False, mixer=None):
    """Reference `train_epoch` (`train.py:119-151`); loss accumulated on device.  ``fused_loss``: the
    model takes the targets and returns the loss itself (GPT-2's fused LM head + CE, reference
    `train.py:136-137` as one op: the [B, T, V] logits never materialise).  ``mixer`` (a ``BatchMixer``): every batch
    is mixed once it is on the device and ``criterion`` gets the target triple ``(y, y2, w)``."""
    model.train()
    total_loss = torch.zeros((), dtype=torch.float64, device=device)
    num_batches = 0
    nb = len(loader)
    # the epoch's last micro-batch always syncs and steps, also when --max-steps cuts the epoch
    # short: leftover no_sync gradients must not leak into the next epoch's first update
    n_eff = min(nb, max_steps) if max_steps is not None else nb
    for batch_idx, (data, target, *doc) in enumerate(loader):  # doc: [doc_start] of a packed-document dataset
        if max_steps is not None and batch_idx >= max_steps:
            break
        fault.maybe_inject(epoch, batch_idx)
        data, target = data.to(device, non_blocking=True), target.to(device, non_blocking=True)
        doc = [d.to(device, non_blocking=True) for d in doc]
        if mixer is not None:
            data, target = mixer(data, target, **_mix_layout(model))
        sync = (batch_idx + 1) % grad_accum == 0 or batch_idx + 1 == n_eff
        ctx = model.no_sync() if (not sync and hasattr(model, "no_sync")) else _null()
        with ctx:
            with tracing.range("forward"):
                if fused_loss:
                    loss = model(data, target, *doc)
                else:
                    output = model(data)
                    loss = criterion(output, target)
            with tracing.range("backward"):
                (loss / grad_accum if grad_accum > 1 else loss).backward()
        if sync:
            with tracing.range("optimizer"):
                optimizer.step()
                optimizer.zero_grad()
        if watchdog is not None:
            watchdog.beat()
        total_loss += loss.detach()
        num_batches += 1
        if batch_idx % 10 == 0 and rank == 0:
            logger.info(f"Epoch {epoch}, Batch {batch_idx}/{nb}, Loss: {loss.item():.4f}")
    return (total_loss / max(1, num_batches)).item()


def _mix_layout(model) -> dict:
    """The packed form the model's stem takes (``BatchMixer.__call__``): ResNet's space-to-depth stem or its NHWC one."""
    m = getattr(model, "module", model)
    if getattr(m, "s2d_stem", True):
        return {"layout": "s2d"}
    return {"layout": "nhwc", "cpad": getattr(m, "in_pad", 8)}


@torch.no_grad()
def validate(model, loader, criterion, device, num_classes, max_steps=None, watchdog=None):
    """Reference `validate` (`train.py:154-175`): mean of per-batch losses, accuracy in %."""
    model.eval()
    total_loss = torch.zeros((), dtype=torch.float64, device=device)
    correct = torch.zeros((), dtype=torch.float64, device=device)
    total = 0
    nbatches = 0
    for i, (data, target, *doc) in enumerate(loader):
        if max_steps is not None and i >= max_steps:
            break
        data, target = data.to(device), target.to(device)
        output = model(data, None, doc[0].to(device)) if doc else model(data)
        s, c = Fx.cross_entropy_eval(output, target, num_classes)
        total_loss += s / target.numel()
        correct += c
        total += target.numel()
        nbatches += 1
        if watchdog is not None:
            watchdog.beat()
    return (total_loss / max(1, nbatches)).item(), (100.0 * correct / max(1, total)).item()


def schedule_total_steps(epochs: int, batches_per_epoch: int, max_steps=None, grad_accum: int = 1) -> int:
    """Optimizer steps of the whole run: per epoch ``ceil(min(batches, max_steps) / grad_accum)`` -- the epoch's
    last micro-batch always steps (``train_epoch``'s ``sync``)."""
    n_eff = min(batches_per_epoch, max_steps) if max_steps is not None else batches_per_epoch
    return epochs * -(-n_eff // max(1, grad_accum))


def _lr_schedule_kw(parser, args, batches_per_epoch: int):
    """--lr-schedule and friends -> ``build_optimizer``'s ``lr_schedule`` dict (None: no schedule)."""
    if args.lr_schedule is None:
        return None
    total = schedule_total_steps(args.epochs, batches_per_epoch, args.max_steps, args.grad_accum)
    warmup = args.warmup_steps or 0
    if warmup >= total:
        parser.error(f"--warmup-steps {warmup} is not shorter than the run's {total} optimizer steps")
    return {"kind": args.lr_schedule, "warmup_steps": warmup, "total_steps": total,
            "min_ratio": 0.0 if args.lr_min_ratio is None else args.lr_min_ratio,
            "power": 1.0 if args.lr_power is None else args.lr_power}


def _dtype_kw(args) -> dict:
    """--dtype -> model kwargs: SimpleNet runs fp32 (reference) or bf16; the BASELINE-scope models are bf16."""
    if args.model == "simplenet":
        return {"compute_dtype": args.dtype or "fp32"}
    if args.dtype == "fp32":
        raise SystemExit(f"--dtype fp32 is implemented for simplenet only ({args.model} runs bf16 with fp32 masters)")
    return {}


@record
def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    vit = args.model.startswith("vit")
    if args.image_size is None:
        args.image_size = 32 if args.model == "vit-tiny" else 224
    if vit:
        # the mixed input pack emits ResNet's layouts, and the bidirectional blocks take no dropout or packed documents
        for flag, on in (("--mixup-alpha", args.mixup_alpha != 0.0), ("--cutmix-alpha", args.cutmix_alpha != 0.0),
                         ("--dropout", args.dropout != 0.0), ("--doc-len-mean", args.doc_len_mean is not None)):
            if on:
                parser.error(f"{flag} is not available for the vit models")
        patch = 8 if args.model == "vit-tiny" else 16
        if args.image_size < patch or args.image_size % patch:
            parser.error(f"--image-size must be a positive multiple of the patch size {patch} for {args.model}")
    if args.skip_nonfinite_steps and args.clip_grad_norm is None:
        parser.error("--skip-nonfinite-steps needs --clip-grad-norm")
    if args.clip_grad_norm is not None and not args.clip_grad_norm > 0:
        parser.error("--clip-grad-norm must be > 0")
    if args.doc_len_mean is not None and not args.model.startswith("gpt2"):
        parser.error("--doc-len-mean needs a gpt2 model")
    if args.doc_len_mean is not None and not args.doc_len_mean >= 1:
        parser.error("--doc-len-mean must be >= 1")
    if args.trust_coefficient is not None and args.optimizer not in ("lars", "lamb"):
        parser.error("--trust-coefficient needs --optimizer lars or lamb")
    for flag, v in (("--muon-momentum", args.muon_momentum), ("--muon-ns-steps", args.muon_ns_steps)):
        if v is not None and args.optimizer != "muon":
            parser.error(f"{flag} needs --optimizer muon")
    if args.muon_momentum is not None and not 0.0 <= args.muon_momentum < 1.0:
        parser.error("--muon-momentum must be in [0, 1)")
    if args.muon_ns_steps is not None and args.muon_ns_steps < 1:
        parser.error("--muon-ns-steps must be >= 1")
    if args.lr_schedule is None:
        for flag, v in (("--warmup-steps", args.warmup_steps), ("--lr-min-ratio", args.lr_min_ratio), ("--lr-power", args.lr_power)):
            if v is not None:
                parser.error(f"{flag} needs --lr-schedule")
    if args.warmup_steps is not None and args.warmup_steps < 0:
        parser.error("--warmup-steps must be >= 0")
    if args.lr_min_ratio is not None and not 0.0 <= args.lr_min_ratio <= 1.0:
        parser.error("--lr-min-ratio must be in [0, 1]")
    if args.lr_power is not None and not args.lr_power > 0:
        parser.error("--lr-power must be > 0")
    if not 0.0 <= args.label_smoothing < 1.0:
        parser.error("--label-smoothing must be in [0, 1)")
    if not args.z_loss >= 0.0:
        parser.error("--z-loss must be >= 0")
    if not 0.0 <= args.dropout < 1.0:
        parser.error("--dropout must be in [0, 1)")
    if args.ema_warmup and args.ema_decay is None:
        parser.error("--ema-warmup needs --ema-decay")
    if args.ema_decay is not None and not 0.0 <= args.ema_decay < 1.0:
        parser.error("--ema-decay must be in [0, 1)")
    if args.dropout > 0.0 and not args.model.startswith("gpt2"):
        parser.error("--dropout needs a gpt2 model")
    if not args.mixup_alpha >= 0.0:
        parser.error("--mixup-alpha must be >= 0")
    if not args.cutmix_alpha >= 0.0:
        parser.error("--cutmix-alpha must be >= 0")
    mixing = args.mixup_alpha > 0.0 or args.cutmix_alpha > 0.0
    for flag, v in (("--mix-prob", args.mix_prob), ("--mix-switch-prob", args.mix_switch_prob)):
        if v is not None and not mixing:
            parser.error(f"{flag} needs --mixup-alpha or --cutmix-alpha")
        if v is not None and not 0.0 <= v <= 1.0:
            parser.error(f"{flag} must be in [0, 1]")
    if args.model.startswith("gpt2") and (mixing or args.mix_prob is not None or args.mix_switch_prob is not None):
        parser.error("--mixup-alpha / --cutmix-alpha / --mix-prob / --mix-switch-prob are for the image and feature "
                     "models, not gpt2")
    if args.cutmix_alpha > 0.0 and not args.model.startswith("resnet"):
        parser.error("--cutmix-alpha needs an image model (resnet50, resnet_tiny)")
    ensure_single_process_env()
    rank, world_size, local_rank = pdist.init_process_group(args.backend, comm_max_channels=args.comm_max_channels)
    logger.info(f"Initialized process group: rank={rank}, world_size={world_size}, local_rank={local_rank}")
    device = pdist.get_device(local_rank)

    logger.info(f"Starting distributed training with {world_size} processes")
    logger.info(f"Configuration: epochs={args.epochs}, batch_size={args.batch_size}, lr={args.lr}")

    reg_kw = {"label_smoothing": args.label_smoothing, "z_loss": args.z_loss, "dropout": args.dropout}
    model_kw = reg_kw if args.model.startswith("gpt2") else ({"image_size": args.image_size} if vit else {})
    model = get_model(args.model, **_dtype_kw(args), **model_kw).to(device)
    model = DDP(model, bucket_cap_mb=args.bucket_mb,
                last_bucket_mb="auto" if args.last_bucket_mb is None else (args.last_bucket_mb or None),
                gradient_compression=None if args.gradient_compression == "none" else args.gradient_compression,
                debug=args.ddp_debug or None)
    if args.roctx:
        tracing.enable(True)
    wd_timeout = pdist.default_watchdog_timeout(args.watchdog_timeout, pdist.backend(), world_size)
    watchdog = pdist.start_watchdog(wd_timeout) if wd_timeout > 0 else None
    logger.info(f"Model parameters: {sum(p.numel() for p in model.parameters()):,}")

    train_dataset, val_dataset, num_classes = _datasets(args, device)
    mode = args.loader if args.loader != "auto" else ("device" if device.type == "cuda" else "torch")
    train_loader, train_sampler = create_data_loader(train_dataset, args.batch_size, rank, world_size, mode=mode,
                                                     device=device)
    val_loader, _ = create_data_loader(val_dataset, args.batch_size, rank, world_size, mode=mode, device=device)
    logger.info(f"Dataset size: {len(train_dataset)}, batches per epoch: {len(train_loader)}")

    opt_name = args.optimizer or ("adam" if args.model == "simplenet" else ("sgd" if args.model.startswith("resnet") else "adamw"))
    optimizer = build_optimizer(opt_name, model.parameters(), lr=args.lr, weight_decay=args.weight_decay,
                                clip_grad_norm=args.clip_grad_norm, skip_nonfinite=args.skip_nonfinite_steps,
                                lr_schedule=_lr_schedule_kw(parser, args, len(train_loader)),
                                ema=None if args.ema_decay is None else {"decay": args.ema_decay, "warmup": args.ema_warmup},
                                **({"trust_coefficient": args.trust_coefficient} if opt_name in ("lars", "lamb") else {}),
                                **({"momentum": 0.95 if args.muon_momentum is None else args.muon_momentum,
                                    "ns_steps": 5 if args.muon_ns_steps is None else args.muon_ns_steps}
                                   if opt_name == "muon" else {}))

    def criterion(out, tgt):  # training only: validate() takes Fx.cross_entropy_eval, the plain cross-entropy
        if isinstance(tgt, tuple):  # a BatchMixer's (y, y2, w)
            return Fx.cross_entropy(out, tgt[0], num_classes, label_smoothing=args.label_smoothing, z_loss=args.z_loss,
                                    labels2=tgt[1], mix_w=tgt[2])
        return Fx.cross_entropy(out, tgt, num_classes, label_smoothing=args.label_smoothing, z_loss=args.z_loss)

    mixer = None
    if mixing:
        mixer = BatchMixer(args.mixup_alpha, args.cutmix_alpha, 1.0 if args.mix_prob is None else args.mix_prob,
                           0.5 if args.mix_switch_prob is None else args.mix_switch_prob, device=device)

    start_epoch = 0
    if rank == 0:
        os.makedirs(args.checkpoint_dir, exist_ok=True)
    resume = args.resume
    if resume is None and args.auto_resume:
        resume = os.path.join(args.checkpoint_dir, "latest_model.pt")
    if resume_exists(resume):
        start_epoch = load_checkpoint(model, optimizer, resume, device)

    pdist.barrier()

    best_accuracy = 0.0
    start_time = time.time()
    prof = _profiler(args.profile, rank)

    for epoch in range(start_epoch, args.epochs):
        epoch_start = time.time()
        train_sampler.set_epoch(epoch)
        train_loss = train_epoch(model, train_loader, optimizer, criterion, device, epoch, rank, args.grad_accum,
                                 args.max_steps, watchdog, fused_loss=args.model.startswith("gpt2"), mixer=mixer)
        val_loss, val_accuracy = validate(model, val_loader, criterion, device, num_classes, args.max_steps, watchdog)

        metrics = torch.tensor([train_loss, val_loss, val_accuracy], device=device)
        pdist.all_reduce(metrics, "sum")
        metrics /= world_size
        avg_train_loss, avg_val_loss, avg_val_accuracy = (v.item() for v in metrics)

        # the averaged weights (set by --ema-decay or by the resumed checkpoint): a second validation with them
        ema_on = optimizer.ema_config is not None and int(optimizer.ema_num_updates.item()) > 0
        if ema_on:
            with optimizer.ema_weights():
                ema_metrics = torch.tensor(validate(model, val_loader, criterion, device, num_classes, args.max_steps, watchdog),
                                           device=device)
            pdist.all_reduce(ema_metrics, "sum")
            ema_metrics /= world_size
            ema_val_loss, ema_val_accuracy = (v.item() for v in ema_metrics)

        epoch_time = time.time() - epoch_start
        if rank == 0:
            logger.info(f"Epoch {epoch} completed in {epoch_time:.2f}s")
            logger.info(f"  Train Loss: {avg_train_loss:.4f}")
            logger.info(f"  Val Loss: {avg_val_loss:.4f}, Val Accuracy: {avg_val_accuracy:.2f}%")
            nb = min(len(train_loader), args.max_steps or len(train_loader))
            logger.info(f"  Throughput: {nb * args.batch_size * world_size / epoch_time:.1f} samples/s (incl. validation)")
            if args.clip_grad_norm is not None and optimizer.grad_norm is not None:
                gn, skipped = torch.stack([optimizer.grad_norm, optimizer.skipped_steps]).tolist()
                logger.info(f"  Grad norm (last step): {gn:.4f}, skipped steps: {int(skipped)}")
            if getattr(optimizer, "trust_stats", None) is not None:
                on = optimizer.trust_on()
                if on.any():
                    r = optimizer.trust_stats[:, 2].cpu()[on]
                    logger.info(f"  Trust ratio (last step): min {r.min().item():.4g}, median {r.median().item():.4g}, "
                                f"max {r.max().item():.4g}")
            if getattr(optimizer, "current_lr", None) is not None:
                logger.info("  LR (last step): " + ", ".join(f"{v:.6g}" for v in optimizer.current_lr.tolist())
                            + f", schedule step: {int(optimizer.schedule_step.item())}")
            if ema_on:
                logger.info(f"  EMA Val Loss: {ema_val_loss:.4f}, EMA Val Accuracy: {ema_val_accuracy:.2f}% "
                            f"(decay {float(optimizer.ema_decay_now):.6g})")
            # no step heartbeat while rank 0 writes (RCCL async errors are still polled)
            with (watchdog.suspended() if watchdog is not None else _null()):
                if avg_val_accuracy > best_accuracy:
                    best_accuracy = avg_val_accuracy
                    save_checkpoint(model, optimizer, epoch, avg_train_loss,
                                    os.path.join(args.checkpoint_dir, "best_model.pt"), args.async_checkpoint)
                save_checkpoint(model, optimizer, epoch, avg_train_loss,
                                os.path.join(args.checkpoint_dir, "latest_model.pt"), args.async_checkpoint)
        if prof is not None:
            prof.step()
        # the other ranks wait here for rank 0's write: stall detection stays on, with a bounded
        # extra allowance for the checkpoint (a peer dying in this barrier still aborts the job)
        with (watchdog.grace(args.watchdog_checkpoint_grace) if watchdog is not None else _null()):
            pdist.barrier()

    wait_pending()
    if watchdog is not None:
        watchdog.stop()
    total_time = time.time() - start_time
    if prof is not None:
        prof.__exit__(None, None, None)
    if rank == 0:
        logger.info(f"Training completed in {total_time:.2f}s")
        logger.info(f"Best validation accuracy: {best_accuracy:.2f}%")
    pdist.destroy_process_group()


def _profiler(path, rank):
    if not path:
        return None
    from torch.profiler import ProfilerActivity, profile

    acts = [ProfilerActivity.CPU] + ([ProfilerActivity.CUDA] if torch.cuda.is_available() else [])

    def handler(p):
        p.export_chrome_trace(path.replace(".json", f".rank{rank}.json"))

    prof = profile(activities=acts, on_trace_ready=handler)
    prof.__enter__()
    return prof


class _null:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


if __name__ == "__main__":
    main()
