"""Child process of tests/test_deepsense_multiloc_gpu.py::test_captured_step_matches_eager: the multi-location DeepSense FOCAL step on
HAR3LOC (fp32, B = 8, learning rate 0) three times eagerly and three times through graph_step.CapturedTrainStep with dropout off, then
three captured steps with dropout on; prints one JSON line
{"replays": n, "steps": [[eager loss, replayed loss, max |gradient difference| / max |eager gradient|], ...],
 "dropout": {"replays": n, "losses": [...], "finite": bool, "grads_differ": bool}}."""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "focal_amd", "src"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from conftest import no_dropout  # noqa: E402


def step_state(cfg, replay):
    from focal_amd import graph_step, runtime
    from models.DeepSense import DeepSense
    from models.FOCALModules import FOCAL
    from models.loss import FOCALLoss
    from oracle.weights import fill_state_dict_, synthetic_freq_input
    from train_utils.optimizer import define_optimizer
    args = argparse.Namespace(model="DeepSense", dataset="HAR3LOC", device=torch.device("cuda"), train_mode="contrastive",
                              learn_framework="FOCAL", stage="pretrain", task="activity_classification", tag=None, dataset_config=cfg,
                              compute_dtype="fp32")
    net = DeepSense(args)
    fill_state_dict_(net.state_dict())
    net = net.to("cuda").train()
    focal, loss_fn = FOCAL(args, net), FOCALLoss(args)
    to = lambda d: {l: {m: v.cuda() for m, v in mm.items()} for l, mm in d.items()}
    x1, x2 = to(synthetic_freq_input(cfg, 8, seed=311)), to(synthetic_freq_input(cfg, 8, seed=312))
    opt = define_optimizer(args, focal.parameters())
    step = graph_step.CapturedTrainStep(focal, loss_fn, opt, warm_steps=1, enabled=replay)
    out = []
    runtime.rng_state("cuda", seed=1234)
    for _ in range(3):
        loss = step(x1, x2)
        torch.cuda.synchronize()
        out.append((float(loss), net.arena().grad.clone()))
    return out, step


def main():
    from oracle.config import load_config
    cfg = copy.deepcopy(load_config(os.path.join(ROOT, "focal_amd", "src", "data", "HAR3LOC.yaml")))
    cfg["FOCAL"]["pretrain_optimizer"]["start_lr"] = 0.0  # the weights stay put: every step sees the same model
    eager, _ = step_state(no_dropout(cfg), False)
    replayed, st = step_state(no_dropout(cfg), True)
    steps = [[le, lr, ((ge - gr).abs().max() / ge.abs().max()).item()] for (le, ge), (lr, gr) in zip(eager, replayed)]
    on, st_on = step_state(cfg, True)  # dropout as shipped (0.2)
    import math
    drop = {"replays": st_on.replays, "losses": [l for l, _ in on],
            "finite": all(math.isfinite(l) and bool(torch.isfinite(g).all()) for l, g in on),
            "grads_differ": not torch.equal(on[1][1], on[2][1])}
    print(json.dumps({"replays": st.replays, "steps": steps, "dropout": drop}))


if __name__ == "__main__":
    main()
