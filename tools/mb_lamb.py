#!/usr/bin/env python3
"""What LAMB (`name: LAMB` in the optimizer section) costs against AdamW, on one box in one process.

  python tools/mb_lamb.py [--out profiles/lamb.txt] [--batch 256] [--rounds 5] [--steps 40] [--only MODEL]

Workloads: FOCAL pretraining on MOD, bf16 operands, SW_Transformer and DeepSense.  Per workload three measurements, each alternating AdamW
and LAMB `rounds` times:
  step      : the whole captured training step (focal_amd/graph_step.py: CapturedTrainStep) replayed on fixed views, two models side by side
              that differ in the optimizer's name only; steps per second
  optimizer : step() alone, launched eagerly, on ONE arena holding the gradients of one backward pass -- adamw_kernel against
              lamb_moments_kernel + lamb_apply_kernel; microseconds per step between two events, enqueue included (the host's launch cost
              is part of this number and bounds it from below)
  replayed  : the same step() captured once and replayed: microseconds per step on the device, and the bytes the update has to move over
              that time.  The buffers (w, g, m, v and the bf16 shadow: 18 B per element) are the same ones every replay, so whatever of them
              fits the 256 MiB Infinity Cache is served from it: this is a cache-resident rate, NOT an HBM rate, and it says so in the output.
Written per form: the median and the spread (max - min) over the windows, the ratio LAMB / AdamW of the medians, and whether LAMB's median
lies inside AdamW's own spread.  No threshold: LAMB is opt-in."""
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

FORMS = ("AdamW", "LAMB")
BYTES = {"AdamW": 16 + 12 + 2, "LAMB": (16 + 8) + (12 + 4 + 2)}  # per element, bf16 shadow included: read + written (LAMB: per launch)


def build(cfg, model, batch, name):
    from focal_amd.graph_step import CapturedTrainStep
    from models.FOCALModules import FOCAL
    from models.loss import FOCALLoss
    from oracle.weights import fill_state_dict_, synthetic_freq_input
    from train_utils.optimizer import define_optimizer
    c = copy.deepcopy(cfg)
    c["FOCAL"]["pretrain_optimizer"]["name"] = name
    args = argparse.Namespace(model=model, dataset="MOD", device=torch.device("cuda:0"), train_mode="contrastive", learn_framework="FOCAL",
                              stage="pretrain", task="vehicle_classification", tag=None, dataset_config=c, compute_dtype="bf16")
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
    for k in FORMS:
        say(f"  {what} {k:5s}: {med[k]:10.2f} {unit} median, spread {spread[k]:8.2f}  [{', '.join(f'{v:.2f}' for v in vals[k])}]")
    slow = med["AdamW"] / med["LAMB"] if higher_is_better else med["LAMB"] / med["AdamW"]
    inside = abs(med["LAMB"] - med["AdamW"]) <= spread["AdamW"]
    say(f"  {what} LAMB against AdamW: x{slow:.4f} ({'inside' if inside else 'OUTSIDE'} AdamW's own spread)")
    return med


def measure(cfg, model, a, say):
    from focal_amd import runtime
    from focal_amd.optim import FocalAdamW, FocalLAMB
    w = {k: build(cfg, model, a.batch, k) for k in FORMS}
    assert type(w["AdamW"]["opt"]) is FocalAdamW and type(w["LAMB"]["opt"]) is FocalLAMB
    for k, b in w.items():   # warm-up: two eager steps, the capture, two replays
        for _ in range(5):
            b["step"](*b["views"])
        torch.cuda.synchronize()
        assert b["step"].replays > 0, f"the {k} step was not captured"
    ar = w["LAMB"]["net"].arena()
    table = next(iter(w["LAMB"]["opt"]._tables.values()))[1]
    say(f"{model} (MOD, FOCAL pretraining, bf16, B = {a.batch}; arena of {ar.size} fp32 words = {ar.size * 4 / 1e6:.1f} MB per buffer, "
        f"{len(table['tensors'])} tensors in {len(table['pieces'])} pieces; {a.rounds} alternating windows)")
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
    s = w["LAMB"]["opt"].trust_stats()
    say(f"  (the LAMB run's last step: trust ratio min {s['min']:.3g} ({s['min_name']}), median {s['median']:.3g}, max {s['max']:.3g} "
        f"({s['max_name']}) over {s['tensors']} adapted tensors)")

    # the optimizer alone: both forms on ONE arena (the LAMB model's, gradients of its last backward pass in place), learning rate 0 so
    # that hundreds of steps on one gradient leave the weights where they are
    params = list(w["LAMB"]["net"].parameters())
    g0 = w["LAMB"]["opt"].param_groups[0]
    opts = {"AdamW": FocalAdamW(params, lr=0.0, weight_decay=g0["weight_decay"]),
            "LAMB": FocalLAMB(params, lr=0.0, weight_decay=g0["weight_decay"])}
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

    graphs = {}
    for k, o in opts.items():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        torch.cuda.synchronize()
        graphs[k] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[k], stream=side):
            for st in runtime._SIDE.values():  # (step() joins the backbones' side streams: fork them, so the join stays inside the capture)
                st.wait_stream(side)
            for _ in range(10):
                o.step(reduce=False)
        graphs[k].replay()
    torch.cuda.synchronize()
    us = {k: [] for k in opts}
    for _ in range(a.rounds):
        for k in opts:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(10):
                graphs[k].replay()
            e1.record()
            torch.cuda.synchronize()
            us[k].append(e0.elapsed_time(e1) * 1e3 / 100)
    med = report(say, "replayed ", "us/step", us, False)
    resident = ar.size * 18 / 2 ** 20
    for k in FORMS:
        say(f"  replayed  {k:5s}: {BYTES[k]} B per element = {ar.size * BYTES[k] / 1e6:.1f} MB per step -> {ar.size * BYTES[k] / med[k] / 1e6:.2f} TB/s "
            f"(cache-resident rate: the {resident:.0f} MiB of w, g, m, v and shadow are re-used by every replay and "
            f"{'fit' if resident < 256 else 'exceed'} the 256 MiB Infinity Cache; not an HBM rate)")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "lamb.txt"))
    p.add_argument("--batch", type=int, default=256)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--steps", type=int, default=40)
    p.add_argument("--only", default=None, help="one model")
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mb_lamb.py measures on the GPU: none found")
    from oracle.config import load_config
    cfg = load_config()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")
    say(f"LAMB against AdamW ({torch.cuda.get_device_name(0)}; tools/mb_lamb.py)")
    for model in ("SW_Transformer", "DeepSense"):
        if a.only in (None, model):
            measure(cfg, model, a, say)
            torch.cuda.synchronize()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
