#!/usr/bin/env python3
"""What one eager training step enqueued, stream by stream, BEFORE the backbone plumbing was folded (three stage nodes -> one, the pass
preamble and forward_classifier of the two models -> HipBackbone, pass_order / views_in_batch from engine attributes -> run_stage
arguments): tests/golden/plumbing_launches_parent.json.  tests/test_backbone_plumbing_gpu.py records the same steps on the folded code and
requires equality.

Recorded on an MI355X in a checkout of the parent of the fold,

    d3ad035 "Honour clip_grad: global-norm gradient clipping inside the step"

with this file and tests/test_backbone_plumbing_gpu.py (whose step_launches() goes through the models' constructors, `FOCAL(x1, x2,
proj_head=True)` and `net(freq_x)`, which the fold leaves alone) copied in:

    python tests/golden/gen_plumbing_launches_parent.py [out.json] [--multiset WORKLOAD ...]

Per workload (test_backbone_plumbing_gpu.WORKLOADS: B = 8, bf16, dropout off, synthetic inputs, the SECOND step of the process) under
`focal_trace_begin(8192, TRACE_DISPATCH)`: the launch count; per stream, numbered by first appearance, the SHA-256 of the ordered list of
(mangled kernel name, grid, block); the number of streams; the SHA-256 of the launches as a multiset.  "form" says what the test holds the
folded code to: "streams" (count, multiset, number of streams and the per-stream sequences) where two runs of this script at the parent
gave the same per-stream digests, "multiset" (count, multiset, number of streams) for a workload named after --multiset because they did
not.  The parent alone decides the form.  At d3ad035 the two runs agreed on every workload: all are "streams".

The file names the commit it was recorded at (`git rev-parse HEAD`, or the COMMIT environment variable where the tree is a copy without
its history) and the device."""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
for p in (ROOT, os.path.join(ROOT, "focal_amd", "src"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

if __name__ == "__main__":
    argv = sys.argv[1:]
    loose = argv[argv.index("--multiset") + 1:] if "--multiset" in argv else []
    argv = argv[:argv.index("--multiset")] if "--multiset" in argv else argv
    out = argv[0] if argv else os.path.join(HERE, "plumbing_launches_parent.json")
    try:
        commit = os.environ.get("COMMIT") or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        commit = "unknown"
    import datetime

    import torch

    from test_backbone_plumbing_gpu import WORKLOADS, step_launches
    got = {}
    for name in WORKLOADS:
        got[name] = dict(step_launches(name), form="multiset" if name in loose else "streams")
        print(f"{name}: {got[name]['count']} launches on {got[name]['n_streams']} streams", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump({"commit": commit, "device": torch.cuda.get_device_name(0), "recorded": datetime.date.today().isoformat(),
                   "workloads": got}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(got)} workloads at {commit} -> {out}")
