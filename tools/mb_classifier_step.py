#!/usr/bin/env python3
"""The classifier stages of train.py, eager against captured, on one box in one process.

  python tools/mb_classifier_step.py [--out profiles/classifier_step.txt] [--batch 256] [--rounds 5] [--steps 48]

Workloads: MOD, bf16 operands, supervised (`-learn_framework=no`) and finetune (`-stage=finetune`), SW_Transformer and DeepSense.
Per workload two forms of the SAME loop body (train_utils/supervised_train.py: run_classifier_epoch) alternate `rounds` times:
  eager    : `-no_graph -host_draws` -- every kernel launched through ctypes, Mixup drawn on the host, loss.item() behind every step
  captured : the default -- one hipGraph replay per step, the fixed pipeline drawn on the device inside it, the loss read one step late
Written per workload and form: windows/s as median and spread (max - min) over the rounds, the library launches of one eager step of
that form's body (the library's launch trace; torch's own few kernels -- copies, argmax -- are not in it), and the default rule's verdict:
captured is the default where its median is not below the eager median by more than the eager form's own spread.
Last, the mix pass alone: focal_mixup_multi (one launch, device record) against the two focal_mixup_fwd launches it replaces."""
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


def build(cfg, model, stage, batch):
    from data_augmenter.Augmenter import Augmenter
    from focal_amd.graph_step import CapturedClassifierStep
    from general_utils.weight_utils import set_learnable_params_finetune
    from input_utils.multi_modal_dataloader import SyntheticSequenceLoader
    from models.loss import CrossEntropyLoss
    from oracle.weights import fill_state_dict_
    from train_utils.optimizer import define_optimizer
    args = argparse.Namespace(model=model, dataset="MOD", device=torch.device("cuda:0"), train_mode="contrastive", learn_framework="FOCAL",
                              stage="pretrain", task="vehicle_classification", tag=None, dataset_config=copy.deepcopy(cfg), compute_dtype="bf16")
    if stage == "supervised":
        args.train_mode, args.learn_framework = "supervised", "no"
    else:
        args.stage = "finetune"
    if model == "SW_Transformer":
        from models.SW_Transformer import SW_Transformer as Net
    else:
        from models.DeepSense import DeepSense as Net
    net = Net(args)
    fill_state_dict_(net.state_dict())
    net = net.to(args.device).train()
    params = set_learnable_params_finetune(args, net) if stage == "finetune" else net.parameters()
    opt, loss_fn, aug = define_optimizer(args, params), CrossEntropyLoss(), Augmenter(args)
    loader = SyntheticSequenceLoader(args, batch, num_batches=8)
    option = "fixed" if stage == "supervised" else "no"

    def parent_step(time_loc_inputs, labels):   # the loop body of `-no_graph -host_draws`
        x, labels = aug.forward(option, time_loc_inputs, labels)
        opt.zero_grad()
        loss = loss_fn(net(x), labels)
        loss.backward()
        opt.step()
        return loss.item()
    return dict(args=args, net=net, opt=opt, loss_fn=loss_fn, aug=aug, loader=loader, option=option, parent_step=parent_step,
                eager=CapturedClassifierStep(net, loss_fn, opt, enabled=False), captured=CapturedClassifierStep(net, loss_fn, opt))


def epoch(w, form):
    from train_utils.supervised_train import run_classifier_epoch
    if form == "eager":
        return run_classifier_epoch(w["eager"], w["aug"], w["loader"], w["option"], False, True, w["parent_step"])
    return run_classifier_epoch(w["captured"], w["aug"], w["loader"], w["option"], True, False, w["parent_step"])


def traced_launches(fn):
    from focal_amd import _lib
    lib = _lib.load()
    torch.cuda.synchronize()
    lib.focal_trace_begin(8192, _lib.TRACE_DISPATCH)
    fn()
    torch.cuda.synchronize()
    lib.focal_trace_end()
    return lib.focal_trace_count()


def measure(cfg, model, stage, a, say):
    w = build(cfg, model, stage, a.batch)
    epochs = max(1, a.steps // len(w["loader"]))
    steps = epochs * len(w["loader"])
    for form in ("eager", "captured"):   # warm-up of every shape both forms use; the second captured epoch replays
        epoch(w, form)
        epoch(w, form)
    torch.cuda.synchronize()
    assert w["captured"].replays > 0, "the step was not captured"
    rates = {"eager": [], "captured": []}
    for _ in range(a.rounds):
        for form in ("eager", "captured"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(epochs):
                epoch(w, form)
            torch.cuda.synchronize()
            rates[form].append(steps * a.batch / (time.perf_counter() - t0))
    batch, labels = next(iter(w["loader"]))
    labels = labels.to(w["args"].device)
    n_eager = traced_launches(lambda: w["parent_step"](batch, labels))
    body = type(w["eager"])(w["net"], w["loss_fn"], w["opt"], enabled=False)
    n_body = traced_launches(lambda: body.step_from_inputs(w["aug"], batch, labels, w["option"]))
    med = {f: statistics.median(v) for f, v in rates.items()}
    spread = {f: max(v) - min(v) for f, v in rates.items()}
    keep = med["captured"] >= med["eager"] - spread["eager"]
    say(f"{model} {stage} (MOD, bf16, B = {a.batch}; {a.rounds} alternating windows of {steps} steps per form)")
    say(f"  eager    (-no_graph -host_draws): {med['eager']:9.1f} windows/s median, spread {spread['eager']:7.1f}  "
        f"[{', '.join(f'{v:.0f}' for v in rates['eager'])}]; {n_eager} library launches per step, each through ctypes")
    say(f"  captured (device draws)         : {med['captured']:9.1f} windows/s median, spread {spread['captured']:7.1f}  "
        f"[{', '.join(f'{v:.0f}' for v in rates['captured'])}]; {n_body} library launches in the captured body, replayed by one graph launch")
    say(f"  captured / eager = {med['captured'] / med['eager']:.3f} -> default: {'captured' if keep else 'EAGER (captured is below eager by more than its spread)'}")
    return keep


def mix_pass(a, say):
    from focal_amd import ops
    B = a.batch
    g = torch.Generator().manual_seed(1)
    xs = [torch.randn(B, 1, 10, 20, generator=g).cuda(), torch.randn(B, 1, 10, 1600, generator=g).cuda()]
    ys = [torch.empty_like(x) for x in xs]
    rec, perm = ops.new_mix_record("cuda"), torch.randperm(B, generator=g).to(torch.int32).cuda()
    moved = sum(3 * x.numel() * 4 for x in xs)   # both operands read, the result written
    out = {}
    for tag, kw in (("blend", dict(apply=1, cut=0, lam=0.37, boxes=[(0, 0, 0, 0)] * 2)), ("cutmix", dict(apply=1, cut=1, lam=0.37, boxes=[(2, 9, 3, 18), (2, 9, 200, 1400)]))):
        ops.write_mix_record(rec, **kw)
        forms = {"focal_mixup_multi, 1 launch": lambda: ops.mixup_multi([dict(x=x, y=y, slot=i) for i, (x, y) in enumerate(zip(xs, ys))], rec, perm),
                 "focal_mixup_fwd x 2 launches": lambda: [ops.mixup(x, perm, kw["lam"], kw["boxes"][i] if kw["cut"] else None) for i, x in enumerate(xs)]}
        times = {k: [] for k in forms}
        for fn in forms.values():
            for _ in range(20):
                fn()
        for _ in range(a.rounds):
            for k, fn in forms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(200):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / 200)
        say(f"mix pass, {tag}, B = {B}, audio + seismic windows: {moved / 1e6:.1f} MB moved per call (two operands read, one result written;"
            " a CutMix paste reads less of the second operand)")
        for k, v in times.items():
            m = statistics.median(v)
            out[(tag, k)] = (m, max(v) - min(v))
            say(f"  {k:30s}: {m:7.2f} us median per call (back to back, enqueue included), spread {max(v) - min(v):5.2f} us, {moved / m / 1e3:7.1f} GB/s")
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "classifier_step.txt"))
    p.add_argument("--batch", type=int, default=256)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--steps", type=int, default=48)
    p.add_argument("--only", default=None, help="MODEL:STAGE, one workload")
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mb_classifier_step.py measures on the GPU: none found")
    from oracle.config import load_config
    cfg = load_config()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")
    say(f"classifier step, eager against captured ({torch.cuda.get_device_name(0)}; tools/mb_classifier_step.py)")
    for model in ("SW_Transformer", "DeepSense"):
        for stage in ("supervised", "finetune"):
            if a.only in (None, f"{model}:{stage}"):
                measure(cfg, model, stage, a, say)
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
    mix_pass(a, say)


if __name__ == "__main__":
    main()
