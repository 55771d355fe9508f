#!/usr/bin/env python3
"""What the seven tile kernels of the evaluation tools wrote BEFORE their tile loop was folded into knn_dist.hpp's PairTile, as SHA-256
digests of raw output bytes: tests/golden/pair_tile_parent.json.  tests/test_pair_tile_parent_gpu.py recomputes the same digests on the
folded library and requires equality.

Recorded on an MI355X with the library of the parent of the fold,

    454b31a "Add LAMB: per-tensor trust ratios over the arena, two fused launches"   (ABI unchanged by the fold)

built into a folder of its own and selected with FOCAL_HIP_LIB (focal_amd/_lib.py); the fold leaves focal_amd/ops.py and _lib.py alone,
so this tree's Python drives either library:

    COMMIT=<the parent's full hash> FOCAL_HIP_LIB=<parent build>/libfocal_hip.so python tests/golden/gen_pair_tile_parent.py [out.json]

Digests (pair_tile_digests() of the test names the shapes): knn_search_vote predictions, neighbours and confusion matrix; rank_positive
before, tied and pos_d2; pair_sums with one group, 7 groups leaving out the row itself, and 40 groups; seq_rank's six outputs for every L,
both functions; kmeans_assign labels and min_d2; probe_forward ce, g and preds; tsne_dist d2 and norms.  The file names the commit it was
recorded at (the COMMIT environment variable, else `git rev-parse HEAD`)."""
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
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "pair_tile_parent.json")
    try:
        commit = os.environ.get("COMMIT") or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        commit = "unknown"
    from focal_amd import _lib, ops
    from test_pair_tile_parent_gpu import pair_tile_digests
    got = pair_tile_digests(ops)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump({"commit": commit, "abi": _lib.load().focal_abi_version(), "sha256": got}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(got)} digests at {commit} (ABI {_lib.load().focal_abi_version()}) -> {out}")
