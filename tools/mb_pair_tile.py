#!/usr/bin/env python3
"""The seven exports built on knn_dist.hpp's PairTile, timed alone, for whichever library FOCAL_HIP_LIB names (else the tree's own).

  [FOCAL_HIP_LIB=other/libfocal_hip.so] python tools/mb_pair_tile.py [--rounds 5] [--json out.jsonl]

Each export runs at the larger shape its tool's profile names (profiles/knn_fused.txt, kmeans_fused.txt, linear_probe_fused.txt,
tsne_fused.txt, retrieval_fused.txt, geometry_fused.txt with G = 1 and G = 7, temporal_fused.txt), with the slices that profile ran, on
random fp32 rows.  After a warm-up call, `rounds` windows of `calls` calls each between two device events; written per export: the time
per call as median and spread (max - min) over the windows.  Two builds are compared by running this once per build, alternately, in one
session: the rule is the project's, the new median no slower than the old one by more than the old one's spread.  --json appends one
line {"lib": ..., "ms": {export: [windows]}} for the comparison."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
for p in (ROOT, os.path.join(ROOT, "focal_amd", "src")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def cases(ops):
    """(name, calls per window, the call) for each export; the operands of a case are freed before the next is built."""
    g = torch.Generator(device="cuda").manual_seed(7)

    def rnd(n, D):
        return torch.randn(n, D, generator=g, device="cuda")

    def sq(t):
        return (t * t).sum(1)

    def knn():
        q, t = rnd(8192, 1024), rnd(65536, 1024)
        t_sq, lab = sq(t), torch.randint(0, 7, (65536,), generator=g, device="cuda")
        return lambda: ops.knn_search_vote(q, t, t_sq, lab, 5, 7, slices=8)

    def kmeans():
        x, c = rnd(65536, 1024), rnd(70, 1024)
        c_sq, labels = sq(c), torch.zeros(10, 65536, dtype=torch.int32, device="cuda")
        return lambda: ops.kmeans_assign(x, c, c_sq, 7, labels=labels)

    def probe():
        x, w, b = rnd(65536, 1024), 0.03 * rnd(28, 1024), rnd(1, 28)[0]
        y = torch.randint(0, 7, (65536,), generator=g, device="cuda").int()
        ce, gr = torch.empty(4, 65536, device="cuda"), torch.empty(65536, 28, device="cuda")
        return lambda: ops.probe_forward(x, w, b, 7, y=y, ce=ce, g=gr, check_labels=False)

    def tsne():
        x = rnd(16384, 512)
        return lambda: ops.tsne_dist(x)

    def rank():
        q, t = rnd(65536, 128), rnd(65536, 128)
        t_sq, pos = sq(t), torch.randint(0, 65536, (65536,), generator=g, device="cuda").int()
        return lambda: ops.rank_positive(q, t, t_sq, pos, slices=1)

    def pairsum(G):
        def build():
            t = rnd(65536, 1024)
            t_sq = sq(t)
            grp = torch.randint(0, 7, (65536,), generator=g, device="cuda").int()
            if G == 1:
                return lambda: ops.pair_sums(t, t, t_sq, fn="gauss", scale=0.001, self_offset=0, slices=1)
            return lambda: ops.pair_sums(t, t, t_sq, group=grp, G=7, fn="dist", self_offset=0, slices=1)
        return build

    def seqrank():
        z = rnd(65536, 256)
        z_sq = sq(z)
        return lambda: ops.seq_rank(z, z_sq, 4, 1.0, fn="dist", slices=1)

    return [("knn_search_vote 8192x65536x1024 k=5 slices=8", 10, knn), ("kmeans_assign 65536x1024 K=7 R=10", 100, kmeans),
            ("probe_forward 65536x1024 C=7 R=4", 200, probe), ("tsne_dist 16384x512", 10, tsne),
            ("rank_positive 65536x65536x128 slices=1", 10, rank), ("pair_sums 65536x1024 G=1 gauss slices=1", 3, pairsum(1)),
            ("pair_sums 65536x1024 G=7 dist slices=1", 3, pairsum(7)), ("seq_rank 65536x256 L=4 slices=1", 5, seqrank)]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--json", default=None)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mb_pair_tile.py measures on the GPU: none found")
    from focal_amd import _lib, ops
    print(f"PairTile exports, {_lib.LIB_PATH} ({torch.cuda.get_device_name(0)}; tools/mb_pair_tile.py, {a.rounds} windows)", flush=True)
    ms = {}
    for name, calls, build in cases(ops):
        fn = build()
        fn()
        torch.cuda.synchronize()
        wins = []
        for _ in range(a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            e1.synchronize()
            wins.append(e0.elapsed_time(e1) / calls)
        ms[name] = wins
        print(f"  {name:46s}: {statistics.median(wins):9.4f} ms median per call, spread {max(wins) - min(wins):7.4f} ms  "
              f"[{', '.join(f'{v:.4f}' for v in wins)}] ({calls} calls per window)", flush=True)
        del fn
        torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "a") as f:
            f.write(json.dumps({"lib": _lib.LIB_PATH, "ms": ms}) + "\n")


if __name__ == "__main__":
    main()
