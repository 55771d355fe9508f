"""Optimizer selection (reference: train_utils/optimizer.py:3-35): same config keys, AdamW runs as the fused
arena kernel; `name: LAMB` (not in the reference) is the layer-wise adaptive form on the same state."""
import os
import sys

_ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..", ".."))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

import logging  # noqa: E402
import math  # noqa: E402

from focal_amd.optim import FocalAdamW, FocalLAMB  # noqa: E402


def _max_grad_norm(args, cfg, section):
    """-clip_grad: the section's `clip_grad` becomes the bound of the global gradient norm.  Without the switch the key is not read (the
    reference never reads it, and the pinned trajectories follow the reference)."""
    if not getattr(args, "clip_grad", False):
        return None
    value = cfg.get("clip_grad")
    ok = isinstance(value, (int, float)) and not isinstance(value, bool) and not math.isnan(value) and value > 0
    if not ok:
        raise ValueError(f"-clip_grad: `{section}: clip_grad` of the dataset YAML is {value!r}; it must be a positive number "
                         "(.inf records the gradient norms and clips nothing)")
    return float(value)


def _lamb_options(cfg, section):
    """`name: LAMB`: the optional keys `lamb_exclude_1d` (default true: tensors with ndim <= 1 are neither adapted nor decayed) and
    `lamb_max_trust` (default .inf: a finite value clamps the trust ratio)."""
    exclude_1d = cfg.get("lamb_exclude_1d", True)
    if not isinstance(exclude_1d, bool):
        raise ValueError(f"`{section}: lamb_exclude_1d` of the dataset YAML is {exclude_1d!r}; it must be true or false")
    max_trust = cfg.get("lamb_max_trust", math.inf)
    ok = isinstance(max_trust, (int, float)) and not isinstance(max_trust, bool) and not math.isnan(max_trust) and max_trust > 0
    if not ok:
        raise ValueError(f"`{section}: lamb_max_trust` of the dataset YAML is {max_trust!r}; it must be a positive number (.inf: no clamp)")
    return exclude_1d, float(max_trust)


def define_optimizer(args, parameters):
    if args.train_mode in {"supervised"}:
        section = f"{args.model}: optimizer"
        cfg = args.dataset_config[args.model]["optimizer"]
    elif args.stage == "pretrain":
        section = f"{args.learn_framework}: pretrain_optimizer"
        cfg = args.dataset_config[args.learn_framework]["pretrain_optimizer"]
    elif args.stage == "finetune":
        section = f"{args.learn_framework}: finetune_optimizer"
        cfg = args.dataset_config[args.learn_framework]["finetune_optimizer"]
    else:
        raise Exception("Optimizer not defined.")
    wd = cfg["weight_decay"][args.model] if isinstance(cfg["weight_decay"], dict) else cfg["weight_decay"]
    clip = _max_grad_norm(args, cfg, section)
    if cfg["name"] == "AdamW":
        return FocalAdamW(parameters, lr=cfg["start_lr"], weight_decay=wd, max_grad_norm=clip)
    if cfg["name"] == "Adam":  # torch.optim.Adam: L2 weight decay folded into the gradient (the finetune optimizer)
        return FocalAdamW(parameters, lr=cfg["start_lr"], weight_decay=wd, l2_decay=True, max_grad_norm=clip)
    if cfg["name"] == "LAMB":  # layer-wise trust ratios on AdamW's moments (large global batches); opt-in, no shipped config names it
        exclude_1d, max_trust = _lamb_options(cfg, section)
        return FocalLAMB(parameters, lr=cfg["start_lr"], weight_decay=wd, max_grad_norm=clip, exclude_1d=exclude_1d, max_trust=max_trust)
    raise NotImplementedError(f"Optimizer {cfg['name']} not implemented.")


def log_trust_stats(optimizer, epoch):
    """LAMB: one line per epoch with the trust ratios of the epoch's last step (one read of the per-tensor record)."""
    stats = optimizer.trust_stats() if hasattr(optimizer, "trust_stats") else None
    if not stats:
        return
    logging.info(f"epoch {epoch}: trust ratio min {stats['min']:.2g} ({stats['min_name']}), median {stats['median']:.2g}, "
                 f"max {stats['max']:.2g} ({stats['max_name']})")


def log_clip_stats(optimizer, epoch):
    """With clipping on: one line per epoch from the device-side record (one read, where the epoch's last loss has just been read).
    With LAMB the trust-ratio line follows from the same place."""
    log_trust_stats(optimizer, epoch)
    stats = optimizer.clip_stats() if getattr(optimizer, "max_grad_norm", None) is not None else None
    if not stats or stats["steps"] == 0:
        return
    logging.info(f"epoch {epoch}: gradient norm mean {stats['norm_mean']:.4g}, max {stats['norm_max']:.4g}; {stats['clipped']} of "
                 f"{stats['steps']} steps clipped, {stats['skipped']} skipped (max_norm {optimizer.max_grad_norm:g})")
