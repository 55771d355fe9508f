"""Child process of tests/test_lamb_gpu.py::test_captured_training_step_matches_eager: the DeepSense FOCAL step on MOD (fp32, B = 8, dropout
off, `pretrain_optimizer.name: LAMB`, learning rate 0) three times eagerly and three times through graph_step.CapturedTrainStep; prints one
JSON line {"optimizer", "replays", "steps": [[eager loss, replayed loss, max |gradient difference| / max |eager gradient|], ...],
"step_count": [eager, replayed], "trust": the replayed run's trust_stats() without the per-tensor list, "weights_moved"}."""
import copy
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "focal_amd", "src"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from conftest import make_args, no_dropout  # noqa: E402


def run(cfg, replay):
    from focal_amd import graph_step, runtime
    from models.DeepSense import DeepSense
    from models.FOCALModules import FOCAL
    from models.loss import FOCALLoss
    from oracle.weights import fill_state_dict_, synthetic_freq_input
    from train_utils.optimizer import define_optimizer
    args = make_args(no_dropout(cfg), "DeepSense", torch.device("cuda"), "fp32")
    net = DeepSense(args)
    fill_state_dict_(net.state_dict())
    net = net.to("cuda").train()
    focal, loss_fn = FOCAL(args, net), FOCALLoss(args)
    to = lambda d: {l: {m: v.cuda() for m, v in mm.items()} for l, mm in d.items()}
    x1, x2 = to(synthetic_freq_input(cfg, 8, seed=101)), to(synthetic_freq_input(cfg, 8, seed=202))
    opt = define_optimizer(args, focal.parameters())
    step = graph_step.CapturedTrainStep(focal, loss_fn, opt, warm_steps=1, enabled=replay)
    out, start = [], None
    runtime.rng_state("cuda", seed=1234)
    for _ in range(3):
        loss = step(x1, x2)
        torch.cuda.synchronize()
        if start is None:
            start = net.arena().flat.clone()
        out.append((float(loss), net.arena().grad.clone()))
    moved = not torch.equal(start, net.arena().flat)
    return out, step, opt, moved


def main():
    from oracle.config import load_config
    cfg = copy.deepcopy(load_config())
    cfg["FOCAL"]["pretrain_optimizer"]["name"] = "LAMB"
    cfg["FOCAL"]["pretrain_optimizer"]["start_lr"] = 0.0  # the weights stay put: every step sees the same model
    eager, _, opt_e, _ = run(cfg, False)
    replayed, st, opt_r, moved = run(cfg, True)
    steps = [[le, lr, ((ge - gr).abs().max() / ge.abs().max()).item()] for (le, ge), (lr, gr) in zip(eager, replayed)]
    trust = {k: v for k, v in opt_r.trust_stats().items() if k != "phi"}
    print(json.dumps({"optimizer": type(opt_r).__name__, "replays": st.replays, "steps": steps,
                      "step_count": [int(opt_e._step_state[1]), int(opt_r._step_state[1])], "trust": trust, "weights_moved": moved}))


if __name__ == "__main__":
    main()
