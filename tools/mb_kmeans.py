#!/usr/bin/env python3
"""GpuKMeans.fit(fused=True) against fit(fused=False), on one box in one process.

  python tools/mb_kmeans.py [--out profiles/kmeans_fused.txt] [--rounds 5] [--iters 10]

Random fp32 features at n = 65 536, D = 1024 and at n = 16 384, D = 512; K = 7, n_init = 10, init = "random" (the seeding is a row gather in
both forms: the windows time Lloyd's iterations).  max_iter is fixed at `iters` and the convergence checks are off, so both forms do the
same work: `iters` iterations of all 10 restarts and the final assignment.  Per shape the two forms alternate `rounds` times, each window
one fit between two device synchronisations (host clock).  Written per shape and form: the wall time per fit as median and spread (max -
min) over the windows, the time per Lloyd iteration (median / iters: all restarts), the peak device memory of one fit above what is
resident before it, whether two fits of that form are bit-identical (centroids, labels, inertia), and the three launches of one fused
iteration timed on their dispatches.  The features of both shapes
(256 MiB, 32 MiB) fit or nearly fit the 256 MiB Infinity Cache and every pass re-reads them, so the effective rate over x (two reads per
iteration for the fused form) is a cache rate, not an HBM rate.  Then the rule's verdict: eval_cluster.py calls the fused form unless
its median is slower than the torch form's by more than the torch form's own spread."""
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

SHAPES = [(65536, 1024, 7, 10), (16384, 512, 7, 10)]


def same_bits(a, b):
    return (torch.equal(a.all_centers_.view(torch.int32), b.all_centers_.view(torch.int32)) and torch.equal(a.labels_, b.labels_)
            and a.inertia_ == b.inertia_)


def one_iteration(x, K, R, slices):
    """The three launches of one Lloyd iteration of all restarts, timed on the dispatches themselves (focal_trace_*)."""
    from focal_amd import _lib, ops
    n, D = x.shape
    c = x[torch.randperm(n, device=x.device)[:R * K]].contiguous()
    c_sq = (c * c).sum(1)
    labels, min_d2 = ops.kmeans_assign(x, c, c_sq, K, want_min_d2=True)
    ws = ops.kmeans_workspace(n, D, K, R, slices, x.device)
    ops.kmeans_update(x, labels, c, c_sq, K, min_d2=min_d2, slices=slices, workspace=ws)
    torch.cuda.synchronize()
    lib = _lib.load()
    _lib.check(lib.focal_trace_begin(16, _lib.TRACE_DISPATCH))
    try:
        ops.kmeans_assign(x, c, c_sq, K, labels=labels, min_d2=min_d2)
        ops.kmeans_update(x, labels, c, c_sq, K, min_d2=min_d2, slices=slices, workspace=ws)
        torch.cuda.synchronize()
    finally:
        lib.focal_trace_end()
    cnt = lib.focal_trace_count()
    recs = (_lib.TraceRecord * cnt)()
    _lib.check(lib.focal_trace_read(0, cnt, recs))
    return [f"{r.kernel.decode().split('(')[0][:40]:40s} grid {tuple(r.grid)} {r.us:9.1f} us" for r in recs]


def measure(shape, a, say):
    from focal_amd import ops
    from train_utils.kmeans import GpuKMeans
    n, D, K, R = shape
    g = torch.Generator().manual_seed(n + D)
    x = torch.randn(n, D, generator=g).cuda()
    forms = {"torch": lambda: GpuKMeans(K, n_init=R, max_iter=a.iters, init="random", seed=1).fit(x, fused=False, check_convergence=False),
             "fused": lambda: GpuKMeans(K, n_init=R, max_iter=a.iters, init="random", seed=1).fit(x, fused=True, check_convergence=False)}
    peak, repeat = {}, {}
    for name, fn in forms.items():   # warm-up, then one fit alone for its peak memory; the two are compared bit for bit
        first = fn()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        second = fn()
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated() - base
        repeat[name] = same_bits(first, second)
        del first, second
    times = {k: [] for k in forms}
    for _ in range(a.rounds):
        for name, fn in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = {k: max(v) - min(v) for k, v in times.items()}
    slices = ops.kmeans_default_slices(n, D, x.device)
    say(f"n = {n}, D = {D}, K = {K}, n_init = {R}, {a.iters} iterations per fit, checks off ({a.rounds} alternating windows of one fit per form; "
        f"x is {n * D * 4 / 2 ** 20:.0f} MiB)")
    for name in forms:
        extra = (f"; assign {-(-n // 128)} workgroups, update {slices} slices x {-(-D // 64)} column chunks; x read twice per iteration: "
                 f"{2 * n * D * 4 * a.iters / med[name] / 1e9:7.1f} GB/s over x (a cache rate)") if name == "fused" else \
            f"; per restart and iteration cdist + argmin + index_add_ + bincount: a [{n}, {K}] fp32 matrix"
        say(f"  {name:5s}: {med[name] * 1e3:10.3f} ms median per fit, spread {spread[name] * 1e3:8.3f} ms  [{', '.join(f'{v * 1e3:.2f}' for v in times[name])}]; "
            f"{med[name] / a.iters * 1e3:8.3f} ms per iteration of all restarts; peak device memory {peak[name] / 2 ** 20:8.1f} MiB; "
            f"two fits bit-identical: {'yes' if repeat[name] else 'NO'}{extra}")
    for rec in one_iteration(x, K, R, slices):
        say(f"    one iteration, per kernel (the library's dispatch trace): {rec}")
    keep = med["fused"] <= med["torch"] + spread["torch"]
    say(f"  fused / torch = {med['fused'] / med['torch']:.3f} in time, {peak['fused'] / max(peak['torch'], 1):.3f} in peak memory -> "
        f"{'fused' if keep else 'TORCH (fused is slower than the torch form by more than its spread)'}")
    return keep


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeans_fused.txt"))
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--iters", type=int, default=10)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mb_kmeans.py measures on the GPU: none found")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")
    say(f"K-means, fit(fused=False) against fit(fused=True) ({torch.cuda.get_device_name(0)}; "
        f"python tools/mb_kmeans.py --rounds {a.rounds} --iters {a.iters})")
    keeps = []
    for shape in SHAPES:
        keeps.append(measure(shape, a, say))
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    say(f"eval_cluster.py calls: {'fit(fused=True)' if all(keeps) else 'fit(fused=False)'} (the rule: fused unless its median is slower than "
        "the torch form's by more than the torch form's spread, at every shape)")


if __name__ == "__main__":
    main()
