#!/usr/bin/env python3
"""What gradient clipping (`train.py -clip_grad`) costs, on one box in one process.

  python tools/mb_clip_grad.py [--out profiles/clip_grad.txt] [--batch 256] [--rounds 5] [--steps 40] [--only MODEL]

Workloads: FOCAL pretraining on MOD, bf16 operands, SW_Transformer and DeepSense.  Per workload two measurements, each alternating the
unclipped and the clipped form `rounds` times:
  optimizer : FocalAdamW.step() alone on the arena holding the gradients of one backward pass -- the plain update (adamw_kernel) against the
              norm pass + the clipped update (grad_norm_kernel, adamw_clip_kernel); microseconds per step between two events, enqueue included
  step      : the whole captured training step (focal_amd/graph_step.py: CapturedTrainStep) replayed on fixed views, two models side by side
              that differ in max_grad_norm only; steps per second
Written per form: the median and the spread (max - min) over the windows, the ratio clipped / unclipped of the medians, and whether the
clipped median lies inside the unclipped form's own spread."""
import argparse
import copy
import os
import statistics
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
for p in (ROOT, os.path.join(ROOT, "focal_amd", "src")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def build(cfg, model, batch, clip):
    from focal_amd.graph_step import CapturedTrainStep
    from models.FOCALModules import FOCAL
    from models.loss import FOCALLoss
    from oracle.weights import fill_state_dict_, synthetic_freq_input
    from train_utils.optimizer import define_optimizer
    args = argparse.Namespace(model=model, dataset="MOD", device=torch.device("cuda:0"), train_mode="contrastive", learn_framework="FOCAL",
                              stage="pretrain", task="vehicle_classification", tag=None, dataset_config=copy.deepcopy(cfg), compute_dtype="bf16",
                              clip_grad=clip)
    if model == "SW_Transformer":
        from models.SW_Transformer import SW_Transformer as Net
    else:
        from models.DeepSense import DeepSense as Net
    net = Net(args)
    fill_state_dict_(net.state_dict())
    net = net.to(args.device).train()
    focal, loss_fn = FOCAL(args, net), FOCALLoss(args)
    opt = define_optimizer(args, focal.parameters())
    to = lambda d: {l: {m: v.cuda() for m, v in mm.items()} for l, mm in d.items()}
    views = to(synthetic_freq_input(cfg, batch, seed=101)), to(synthetic_freq_input(cfg, batch, seed=202))
    return dict(net=net, opt=opt, views=views, step=CapturedTrainStep(focal, loss_fn, opt))


def report(say, what, unit, vals, higher_is_better):
    med = {k: statistics.median(v) for k, v in vals.items()}
    spread = {k: max(v) - min(v) for k, v in vals.items()}
    for k in ("unclipped", "clipped"):
        say(f"  {what} {k:9s}: {med[k]:10.2f} {unit} median, spread {spread[k]:8.2f}  [{', '.join(f'{v:.2f}' for v in vals[k])}]")
    slow = med["unclipped"] / med["clipped"] if higher_is_better else med["clipped"] / med["unclipped"]
    inside = abs(med["clipped"] - med["unclipped"]) <= spread["unclipped"]
    say(f"  {what} slowdown with clipping on: x{slow:.4f} ({'inside' if inside else 'OUTSIDE'} the unclipped form's own spread)")


def measure(cfg, model, a, say):
    from focal_amd.optim import FocalAdamW
    w = {"unclipped": build(cfg, model, a.batch, False), "clipped": build(cfg, model, a.batch, True)}
    for k, b in w.items():   # warm-up: two eager steps, the capture, two replays
        for _ in range(5):
            b["step"](*b["views"])
        torch.cuda.synchronize()
        assert b["step"].replays > 0, f"the {k} step was not captured"
    max_norm = w["clipped"]["opt"].max_grad_norm
    ar = w["clipped"]["net"].arena()
    say(f"{model} (MOD, FOCAL pretraining, bf16, B = {a.batch}; arena of {ar.size} fp32 words = {ar.size * 4 / 1e6:.1f} MB of gradients; "
        f"max_norm {max_norm:g}; {a.rounds} alternating windows)")
    rate = {k: [] for k in w}
    for _ in range(a.rounds):
        for k, b in w.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                b["step"](*b["views"])
            torch.cuda.synchronize()
            rate[k].append(a.steps / (time.perf_counter() - t0))
    report(say, "step     ", "steps/s", rate, True)
    s = w["clipped"]["opt"].clip_stats()
    say(f"  (the clipped run: norm mean {s['norm_mean']:.4g}, max {s['norm_max']:.4g}, {s['clipped']} of {s['steps']} steps clipped, {s['skipped']} skipped)")

    # the optimizer alone: both forms on ONE arena (the clipped model's, gradients of its last backward pass in place)
    params = list(w["clipped"]["net"].parameters())
    g0 = w["clipped"]["opt"].param_groups[0]
    opts = {"unclipped": FocalAdamW(params, lr=g0["lr"], weight_decay=g0["weight_decay"]),
            "clipped": FocalAdamW(params, lr=g0["lr"], weight_decay=g0["weight_decay"], max_grad_norm=max_norm)}
    us = {k: [] for k in opts}
    for o in opts.values():
        for _ in range(10):
            o.step()
    for _ in range(a.rounds):
        for k, o in opts.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(100):
                o.step()
            e1.record()
            torch.cuda.synchronize()
            us[k].append(e0.elapsed_time(e1) * 1e3 / 100)
    report(say, "optimizer", "us/step", us, False)
    s = opts["clipped"].clip_stats()
    say(f"  (those clipped optimizer steps: norm mean {s['norm_mean']:.4g}, {s['clipped']} of {s['steps']} clipped, {s['skipped']} skipped)")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_grad.txt"))
    p.add_argument("--batch", type=int, default=256)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--steps", type=int, default=40)
    p.add_argument("--only", default=None, help="one model")
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mb_clip_grad.py measures on the GPU: none found")
    from oracle.config import load_config
    cfg = load_config()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")
    say(f"gradient clipping, off against on ({torch.cuda.get_device_name(0)}; tools/mb_clip_grad.py)")
    for model in ("SW_Transformer", "DeepSense"):
        if a.only in (None, model):
            measure(cfg, model, a, say)
            torch.cuda.synchronize()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
