#!/usr/bin/env python3
"""What the view path wrote BEFORE the fold to one pool struct, one draw export and one transform entry point, as SHA-256 digests of raw
output bytes: tests/golden/view_fold_parent.json.  tests/test_view_fold_gpu.py recomputes the same digests on the folded library and
requires equality.

Recorded on an MI355X in a checkout of the parent of the fold,

    b4f5b43 "Add test.py; keep evaluation loss and confusion matrix on the device"   (ABI 13)

with this file and tests/test_view_fold_gpu.py (whose fold_digests() goes through Python signatures the fold leaves alone) copied in:

    python tests/golden/gen_view_fold_parent.py [out.json]

Digests: view_draw and view_draw_shared plans (and the final state words) of the shipped 7-entry pool, 2 views x 2 slots, 20 seed words each;
view_draw plans and extras of the full 11-entry pool, 2 x 2, 20 seed words; fft_realpack_multi at (2,3,10,20), (2,2,10,256) and
(2,1,10,1600) -- the small-row kernel, the MFMA kernel, the MFMA kernel at 40 x 40 with the raised LDS grant -- each plain, with a forced
plan (scale, flip, perm, phase) and with the composed forced extra.  The file names the commit it was recorded at (`git rev-parse HEAD`, or
the COMMIT environment variable where the tree is a copy without its history)."""
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
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "view_fold_parent.json")
    try:
        commit = os.environ.get("COMMIT") or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        commit = "unknown"
    from focal_amd import _lib, ops
    from test_view_fold_gpu import fold_digests
    got = fold_digests(ops)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump({"commit": commit, "abi": _lib.load().focal_abi_version(), "sha256": got}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(got)} digests at {commit} (ABI {_lib.load().focal_abi_version()}) -> {out}")
