#!/usr/bin/env python3
"""cross_modal_ranks(fused=False) against cross_modal_ranks(fused=True), on one box in one process.

  python tools/mb_retrieval.py [--out profiles/retrieval_fused.txt] [--rounds 5] [--calls 10]

Random unit rows at n = 8192, D = 128 and at n = 65 536, D = 128 (a shared or private half of the shipped 256-wide embedding): b random,
a = b + noise, so the positives spread over many ranks.  Per shape the two forms alternate `rounds` times, each window `calls` calls
between two device synchronisations (host clock; both forms end in device work only).  Written per shape and form: the wall time per call
as median and spread (max - min) over the windows, the peak device memory of one call above what is resident before it
(torch.cuda.max_memory_allocated), and the achieved fp32 rate over 2 n n D -- a whole-call rate: the torch form's call holds the
normalisation, the product, the element-wise passes and the counting per chunk of 8192 queries; the fused form's the normalisation and
focal_rank_positive's two launches.  Then the share of queries on which the two ranks agree, and the rule's verdict: eval_retrieval.py
calls the fused form unless its median is slower than the torch form's by more than the torch form's own spread.

What sits where (256 MiB of Infinity Cache): at n = 8192 the two operands are 4 MiB each and the torch form's [8192, 8192] fp32 matrix is
256 MiB -- as large as the cache, and three more of its size are written around it; at n = 65 536 the operands are 32 MiB each (cached;
the fused form re-reads the gallery once per 128 queries from there) and the torch form's [8192, 65 536] chunk matrix is 2 GiB (HBM)."""
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

SHAPES = [(8192, 128), (65536, 128)]


def measure(shape, a, say):
    from focal_amd import ops
    from train_utils.retrieval import cross_modal_ranks
    n, D = shape
    g = torch.Generator().manual_seed(n + D)
    b = torch.nn.functional.normalize(torch.randn(n, D, generator=g), dim=1).cuda()
    x = torch.nn.functional.normalize(b.cpu() + 0.25 * torch.randn(n, D, generator=g), dim=1).cuda()
    forms = {"torch": lambda: cross_modal_ranks(x, b, fused=False), "fused": lambda: cross_modal_ranks(x, b, fused=True)}
    out, peak = {}, {}
    for name, fn in forms.items():   # warm-up of every shape both forms use, then one call alone for its peak memory
        out[name] = fn()[0]
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
    flop = 2.0 * n * n * D
    slices = ops.knn_default_slices(n, n, x.device)
    ranks = out["fused"]
    say(f"n = {n}, D = {D} ({a.rounds} alternating windows of {a.calls} calls per form; {flop / 1e12:.3f} TFLOP in the product; operands "
        f"{n * D * 4 / 2 ** 20:.0f} MiB each; ranks {int(ranks.min())} .. {int(ranks.max())}, median {float(ranks.float().median()):.0f})")
    for name in forms:
        extra = (f"; {slices} slices, {-(-n // 128) * slices} + {-(-n // 128)} workgroups" if name == "fused"
                 else f"; chunks of 8192 queries: a [{min(n, 8192)}, {n}] fp32 matrix of {min(n, 8192) * n * 4 / 2 ** 20:.0f} MiB")
        say(f"  {name:6s}: {med[name] * 1e3:9.3f} ms median per call, spread {spread[name] * 1e3:7.3f} ms  [{', '.join(f'{v * 1e3:.2f}' for v in times[name])}]; "
            f"{flop / med[name] / 1e12:6.1f} TFLOP/s fp32 over the call; peak device memory {peak[name] / 2 ** 20:8.1f} MiB{extra}")
    agree = (out["torch"] == out["fused"]).float().mean().item()
    keep = med["fused"] <= med["torch"] + spread["torch"]
    say(f"  the two ranks agree on {agree:.4f} of the queries; fused / torch = {med['fused'] / med['torch']:.3f} in time, "
        f"{peak['fused'] / max(peak['torch'], 1):.4f} in peak memory -> "
        f"{'fused' if keep else 'TORCH (fused is slower than the torch form by more than its spread)'}")
    return keep


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "retrieval_fused.txt"))
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--calls", type=int, default=10)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mb_retrieval.py measures on the GPU: none found")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")
    say(f"Cross-modal retrieval, cross_modal_ranks(fused=False) against cross_modal_ranks(fused=True) ({torch.cuda.get_device_name(0)}; tools/mb_retrieval.py)")
    keeps = []
    for shape in SHAPES:
        keeps.append(measure(shape, a, say))
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    say(f"eval_retrieval.py calls: {'fused=True' if all(keeps) else 'fused=False'} (the rule: fused unless its median is slower than the torch form's by more than the torch form's spread, at every shape)")


if __name__ == "__main__":
    main()
