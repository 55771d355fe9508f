#!/usr/bin/env python3
"""silhouette / uniformity (fused=False) against the fused forms (train_utils/geometry.py), on one box in one process.

  python tools/mb_geometry.py [--out profiles/geometry_fused.txt] [--rounds 5] [--calls 3]

Random fp32 features (class means 0.3 N(0, 1) plus N(0, 1) noise, labels uniform) at n = 65 536, D = 1024 -- G = 7 classes for the
silhouette, one group for the uniformity -- and at n = 16 384, D = 512.  Per shape and score the two forms alternate `rounds` times, each
window `calls` calls between two device synchronisations (host clock; the uniformity's one float read ends each of its calls).  Written
per shape, score and form: the wall time per call as median and spread (max - min) over the windows, the peak device memory of one call
above what is resident before it (torch.cuda.max_memory_allocated), and the achieved fp32 rate over 2 n n D -- a whole-call rate: the
torch form's call holds torch.cdist, the element-wise passes and the per-class sums per chunk of 8192 queries; the fused form's the
norms (and for the uniformity the normalisation) and focal_pair_sums' one or two launches.  Then how far the two forms' scores lie
apart, and the rule's verdict, taken per score: eval_geometry.py calls the fused form unless its median is slower than the torch form's by
more than the torch form's own spread at one of the shapes.

What sits where (256 MiB of Infinity Cache): at n = 65 536, D = 1024 the features are 256 MiB -- as large as the cache, so the gallery
the fused form re-reads once per 128 queries streams from HBM in part -- and the torch form's [8192, 65 536] fp32 chunk matrix is 2 GiB
(HBM); at n = 16 384, D = 512 the features are 32 MiB (cached) and the torch form's [8192, 16 384] chunk matrix is 512 MiB (HBM)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
for p in (ROOT, os.path.join(ROOT, "focal_amd", "src")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

SHAPES = [(65536, 1024, 7), (16384, 512, 7)]
CACHE_MIB = 256


def measure(shape, a, say):
    from focal_amd import ops
    from train_utils.geometry import silhouette, uniformity
    n, D, G = shape
    g = torch.Generator().manual_seed(n + D)
    labels = torch.randint(0, G, (n,), generator=g)
    x = (0.3 * torch.randn(G, D, generator=g)[labels] + torch.randn(n, D, generator=g)).cuda()
    labels = labels.cuda()
    scores = {"silhouette": {"torch": lambda: silhouette(x, labels, G, fused=False)[1], "fused": lambda: silhouette(x, labels, G, fused=True)[1]},
              "uniformity": {"torch": lambda: uniformity(x, fused=False), "fused": lambda: uniformity(x, fused=True)}}
    flop = 2.0 * n * n * D
    slices = ops.knn_default_slices(n, n, x.device)
    mib = n * D * 4 / 2 ** 20
    say(f"n = {n}, D = {D} ({a.rounds} alternating windows of {a.calls} calls per form; {flop / 1e12:.3f} TFLOP in the product; features "
        f"{mib:.0f} MiB: {'within' if mib < CACHE_MIB else 'as large as or beyond'} the {CACHE_MIB} MiB Infinity Cache; "
        f"{slices} slices, {-(-n // 128) * slices} workgroups)")
    keeps = {}
    for score, forms in scores.items():
        out, peak = {}, {}
        for name, fn in forms.items():   # warm-up of both forms, then one call alone for its peak memory
            out[name] = fn()
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            fn()
            torch.cuda.synchronize()
            peak[name] = torch.cuda.max_memory_allocated() - base
        times = {k: [] for k in forms}
        for _ in range(a.rounds):
            for name, fn in forms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    fn()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) / a.calls)
        med = {k: statistics.median(v) for k, v in times.items()}
        spread = {k: max(v) - min(v) for k, v in times.items()}
        groups = G if score == "silhouette" else 1
        say(f" {score} (G = {groups}): torch {out['torch']:.7f}, fused {out['fused']:.7f}")
        for name in forms:
            extra = (f"; S [{n}, {groups}] and the slices' partials" if name == "fused"
                     else f"; chunks of 8192 queries: a [{min(n, 8192)}, {n}] fp32 matrix of {min(n, 8192) * n * 4 / 2 ** 20:.0f} MiB")
            say(f"  {name:6s}: {med[name] * 1e3:9.3f} ms median per call, spread {spread[name] * 1e3:7.3f} ms  "
                f"[{', '.join(f'{v * 1e3:.2f}' for v in times[name])}]; {flop / med[name] / 1e12:6.1f} TFLOP/s fp32 over the call; "
                f"peak device memory {peak[name] / 2 ** 20:8.1f} MiB{extra}")
        keep = med["fused"] <= med["torch"] + spread["torch"]
        keeps[score] = keep
        say(f"  the two scores differ by {abs(out['torch'] - out['fused']):.2e}; fused / torch = {med['fused'] / med['torch']:.3f} in time, "
            f"{peak['fused'] / max(peak['torch'], 1):.4f} in peak memory -> "
            f"{'fused' if keep else 'TORCH (fused is slower than the torch form by more than its spread)'}")
    return keeps


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "geometry_fused.txt"))
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--calls", type=int, default=3)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mb_geometry.py measures on the GPU: none found")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")
    say(f"Embedding geometry, silhouette / uniformity (fused=False) against the fused forms ({torch.cuda.get_device_name(0)}; tools/mb_geometry.py)")
    keeps = []
    for shape in SHAPES:
        keeps.append(measure(shape, a, say))
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    verdict = ", ".join(f"{score} fused={all(k[score] for k in keeps)}" for score in keeps[0])
    say(f"eval_geometry.py calls: {verdict} (the rule, per score: fused unless its median is slower than the torch form's by more than the torch form's spread, at every shape)")


if __name__ == "__main__":
    main()
