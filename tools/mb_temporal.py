#!/usr/bin/env python3
"""sequence_ranking (fused=False) against the fused form (train_utils/temporal.py), on one box in one process.

  python tools/mb_temporal.py [--out profiles/temporal_fused.txt] [--rounds 5] [--calls 3]

Random fp32 rows (per sequence of L = 4 rows a centre N(0, 1) plus sigma N(0, 1) noise, sigma uniform in [0.2, 1.5]) at n = 65 536,
D = 256 and at n = 16 384, D = 256, margin 1, f = the distance.  Per shape the two forms alternate `rounds` times, each window `calls`
calls between two device synchronisations (host clock).  Written per shape and form: the wall time per call as median and spread (max -
min) over the windows, the peak device memory of one call above what is resident before it (torch.cuda.max_memory_allocated), and the
achieved fp32 rate over 2 n n D -- a whole-call rate: the torch form's call holds torch.cdist, the block pooling and the comparisons per
chunk of 8192 queries; the fused form's the norms and focal_seq_rank's three launches.  Then whether the two forms' integer counts
agree and how far their float sums lie apart, and the rule's verdict: eval_temporal.py calls the fused form unless its median is slower
than the torch form's by more than the torch form's own spread at one of the shapes.

What sits where (256 MiB of Infinity Cache): at n = 65 536, D = 256 the rows are 64 MiB and at n = 16 384 they are 16 MiB -- both within
the cache, so the gallery the fused form re-reads once per 128 queries is served from it and its rate is a cache rate, not an HBM
rate; the torch form's [8192, n] fp32 chunk matrix is 2 GiB and 512 MiB (HBM)."""
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

SHAPES = [(65536, 256, 4), (16384, 256, 4)]
CACHE_MIB = 256
MARGIN = 1.0
COUNTS = ("before", "viol")
SUMS = ("intra_sum", "inter_sum", "hinge_sum")


def measure(shape, a, say):
    from focal_amd import ops
    from train_utils.temporal import sequence_ranking, temporal_metrics
    n, D, L = shape
    g = torch.Generator().manual_seed(n + D)
    S = n // L
    x = (torch.randn(S, 1, D, generator=g) + (0.2 + 1.3 * torch.rand(S, 1, 1, generator=g)) * torch.randn(S, L, D, generator=g))
    x = x.reshape(n, D).cuda()
    forms = {"torch": lambda: sequence_ranking(x, L, MARGIN, fused=False), "fused": lambda: sequence_ranking(x, L, MARGIN, fused=True)}
    flop = 2.0 * n * n * D
    slices = ops.knn_default_slices(n, n, x.device)
    mib = n * D * 4 / 2 ** 20
    say(f"n = {n}, D = {D}, L = {L}, S = {S} ({a.rounds} alternating windows of {a.calls} calls per form; {flop / 1e12:.3f} TFLOP in the "
        f"product; rows {mib:.0f} MiB: {'within' if mib < CACHE_MIB else 'as large as or beyond'} the {CACHE_MIB} MiB Infinity Cache; "
        f"{slices} slices, {-(-n // 128) * slices} workgroups)")
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
    for name in forms:
        m = temporal_metrics(out[name], L)
        extra = ("; the per-sequence outputs, intra_d2 and the slices' partials" if name == "fused"
                 else f"; chunks of 8192 queries: a [{min(n, 8192)}, {n}] fp32 matrix of {min(n, 8192) * n * 4 / 2 ** 20:.0f} MiB")
        say(f"  {name:6s}: {med[name] * 1e3:9.3f} ms median per call, spread {spread[name] * 1e3:7.3f} ms  "
            f"[{', '.join(f'{v * 1e3:.2f}' for v in times[name])}]; {flop / med[name] / 1e12:6.1f} TFLOP/s fp32 over the call; "
            f"peak device memory {peak[name] / 2 ** 20:8.1f} MiB{extra}")
        say(f"          ranking loss {m['ranking_loss']:.7f}, margin satisfied {m['margin_satisfied']:.7f}, ordered {m['ordered']:.7f}, "
            f"ratio {m['ratio']:.7f}")
    differ = {k: int((out["torch"][k] != out["fused"][k]).sum()) for k in COUNTS}
    apart = {k: float(((out["torch"][k] - out["fused"][k]).abs() / out["torch"][k].abs().clamp_min(1e-30)).max()) for k in SUMS}
    keep = med["fused"] <= med["torch"] + spread["torch"]
    say(f"  integer counts: {', '.join(f'{k} differs at {v} of {S} sequences' for k, v in differ.items())} (a pair whose two sides lie "
        f"within rounding of each other may fall either way: the forms take d2 from different products); float sums apart by at most "
        f"{', '.join(f'{k} {v:.2e}' for k, v in apart.items())} (relative)")
    say(f"  fused / torch = {med['fused'] / med['torch']:.3f} in time, {peak['fused'] / max(peak['torch'], 1):.4f} in peak memory -> "
        f"{'fused' if keep else 'TORCH (fused is slower than the torch form by more than its spread)'}")
    return keep


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_fused.txt"))
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--calls", type=int, default=3)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mb_temporal.py measures on the GPU: none found")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")
    say(f"Temporal ranking, sequence_ranking (fused=False) against the fused form ({torch.cuda.get_device_name(0)}; tools/mb_temporal.py)")
    keeps = []
    for shape in SHAPES:
        keeps.append(measure(shape, a, say))
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    say(f"eval_temporal.py calls: fused={all(keeps)} (the rule: fused unless its median is slower than the torch form's by more than the "
        "torch form's spread, at every shape)")


if __name__ == "__main__":
    main()
