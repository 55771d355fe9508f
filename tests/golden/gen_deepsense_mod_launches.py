#!/usr/bin/env python3
"""Kernel names of ONE eager DeepSense / MOD B = 8 bf16 training step (forward of both views, loss, backward), as the library's launch
trace (focal_trace_*) sees them, as a multiset: tests/golden/DeepSense_MOD_b8_launches.json.

Run on a GPU box AT THE COMMIT WHOSE LAUNCHES ARE THE YARDSTICK (the parent of the multi-location stage: the refactor of
focal_amd/deepsense_engine.py into a conv stack and a GRU part must not add, drop or swap a launch on the single-location path;
tests/test_deepsense_multiloc_gpu.py::test_single_location_launches_unchanged compares against it):

    python tests/golden/gen_deepsense_mod_launches.py [out.json]

The file names the commit it was recorded at ("commit": `git rev-parse HEAD` of the checkout the script ran in, or the COMMIT environment
variable where the tree is a copy without its history), so the yardstick can be re-derived: check that commit out, build, run this.

The first step of a process builds the arena and the BatchNorm counter blocks; the SECOND step is recorded.  Template arguments stay in the
(mangled) names: a kernel swapped for another instantiation shows."""
import argparse
import collections
import copy
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
for p in (ROOT, os.path.join(ROOT, "focal_amd", "src")):
    if p not in sys.path:
        sys.path.insert(0, p)


def step_launches(B=8, ct="bf16"):
    from focal_amd import _lib
    from models.DeepSense import DeepSense
    from models.FOCALModules import FOCAL
    from models.loss import FOCALLoss
    from oracle.config import load_config
    from oracle.weights import fill_state_dict_, synthetic_freq_input
    cfg = copy.deepcopy(load_config())
    cfg["DeepSense"]["dropout_ratio"] = 0.0
    args = argparse.Namespace(model="DeepSense", dataset="MOD", device=torch.device("cuda"), train_mode="contrastive", learn_framework="FOCAL",
                              stage="pretrain", task="vehicle_classification", tag=None, dataset_config=cfg, compute_dtype=ct)
    net = DeepSense(args)
    fill_state_dict_(net.state_dict())
    net = net.to("cuda").train()
    focal, loss_fn = FOCAL(args, net), FOCALLoss(args)
    to = lambda d: {l: {m: v.cuda() for m, v in mm.items()} for l, mm in d.items()}
    x1, x2 = to(synthetic_freq_input(cfg, B, seed=311)), to(synthetic_freq_input(cfg, B, seed=312))
    lib = _lib.load()
    names = []
    for it in range(2):
        net.arena().zero_grad()
        torch.cuda.synchronize()
        _lib.check(lib.focal_trace_begin(8192, _lib.TRACE_DISPATCH))
        try:
            f1, f2 = focal(x1, x2, proj_head=True)
            loss_fn(f1, f2).backward()
            torch.cuda.synchronize()
        finally:
            lib.focal_trace_end()
        n = lib.focal_trace_count()
        recs = (_lib.TraceRecord * max(n, 1))()
        _lib.check(lib.focal_trace_read(0, n, recs))
        names = [recs[i].kernel.decode() for i in range(n)]
    return dict(sorted(collections.Counter(names).items()))


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "DeepSense_MOD_b8_launches.json")
    import subprocess
    try:
        commit = os.environ.get("COMMIT") or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        commit = "unknown"
    got = step_launches()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump({"commit": commit, "workload": "one eager DeepSense / MOD B = 8 bf16 FOCAL training step (forward of both views, loss, "
                   "backward), second step of the process", "launches": got}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{sum(got.values())} launches of {len(got)} kernels -> {out}")
