#!/usr/bin/env python3
"""The parameter arena's layout BEFORE the backbone plumbing was folded (seven `is_hot*` predicates, an if-ladder and an identity patch ->
one rule object built from one table): tests/golden/arena_layouts_parent.json.  tests/test_backbone_plumbing_cpu.py rebuilds every case on
the folded code and requires equality.

Recorded on the CPU in a checkout of the parent of the fold,

    d3ad035 "Honour clip_grad: global-norm gradient clipping inside the step"

with this file and tests/test_backbone_plumbing_cpu.py (whose build() / record() go through constructor arguments and
`arena.layout(net, net._hot)`, which the fold leaves alone) copied in:

    python tests/golden/gen_arena_layouts_parent.py [out.json]

Cases: every yaml under focal_amd/src/data x {DeepSense, SW_Transformer with APE off / on} x {pretrain, finetune, supervised}.  Per case
either {"raises": "NotImplementedError"} or the number of hot parameters, the arena's total elements and the SHA-256 of the JSON of the
ordered [name, offset, numel, shape] list.  The file names the commit it was recorded at (`git rev-parse HEAD`, or the COMMIT environment
variable where the tree is a copy without its history)."""
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
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "arena_layouts_parent.json")
    try:
        commit = os.environ.get("COMMIT") or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        commit = "unknown"
    from test_backbone_plumbing_cpu import case_ids, record
    got = {case: record(case) for case in case_ids()}
    with open(out, "w") as f:
        json.dump({"commit": commit, "cases": got}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(got)} cases ({sum('raises' in v for v in got.values())} raise) at {commit} -> {out}")
