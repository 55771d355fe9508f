#!/usr/bin/env python3
"""GpuTSNE's fused iteration against its plain torch form, on one box in one process.

  python tools/mb_tsne.py [--out profiles/tsne_fused.txt] [--rounds 5] [--iters 50]

Random fp32 features at n = 16 384, D = 512 and at n = 4096, D = 512, perplexity 30.  Per shape: the setup (distances, 64 bisection steps
per row, symmetrisation) of both forms, timed once each after a warm-up and reported apart; then, on the fused form's P, the two forms of
the descent alternate `rounds` times, each window `iters` iterations (early exaggeration, one KL evaluation at the end) between two device
synchronisations (host clock), both from the same start.  Written per shape and form: the wall time per window as median and spread (max -
min), the time per iteration, the peak device memory of a window above what is resident before it (P is resident: not counted; the
setup's peak does count the P it returns), whether two
windows of that form are bit-identical, and the two launches of one fused iteration timed on their dispatches.  P at n = 16 384 is 1 GiB
and does not fit the 256 MiB Infinity Cache: the gradient launch's rate over P is an HBM rate and is written as a fraction of the 6.3 TB/s
a streaming read achieves on this part (8 TB/s peak); P at n = 4096 is 64 MiB and stays in the cache, so there the rate is a cache rate.
Then the rule's verdict: eval_tsne.py calls the fused form unless its median is slower than the torch form's by more than the torch
form's own spread."""
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

SHAPES = [(16384, 512), (4096, 512)]
HBM_ACHIEVABLE = 6.3e12  # bytes / s of a streaming read (8e12 peak)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def one_iteration(P, plogp, y0, slices):
    """The two launches of one fused iteration, timed on the dispatches themselves (focal_trace_*)."""
    from focal_amd import _lib, ops
    n = y0.shape[0]
    y, upd, gains = y0.clone(), torch.zeros_like(y0), torch.ones_like(y0)
    ws = ops.tsne_workspace(n, slices, y.device)
    ops.tsne_grad_step(y, P, plogp, upd, gains, 50.0, 0.5, 12.0, slices=slices, workspace=ws)
    torch.cuda.synchronize()
    lib = _lib.load()
    _lib.check(lib.focal_trace_begin(16, _lib.TRACE_DISPATCH))
    try:
        ops.tsne_grad_step(y, P, plogp, upd, gains, 50.0, 0.5, 12.0, slices=slices, workspace=ws)
        torch.cuda.synchronize()
    finally:
        lib.focal_trace_end()
    cnt = lib.focal_trace_count()
    recs = (_lib.TraceRecord * cnt)()
    _lib.check(lib.focal_trace_read(0, cnt, recs))
    return [(r.kernel.decode().split("(")[0][:40], tuple(r.grid), r.us) for r in recs]


def measure(shape, a, say):
    from focal_amd import ops
    from train_utils.tsne import GpuTSNE, affinities_torch
    n, D = shape
    g = torch.Generator().manual_seed(n + D)
    x = torch.randn(n, D, generator=g).cuda()
    y0 = (torch.randn(n, 2, generator=g) * 1e-4).cuda()
    say(f"n = {n}, D = {D}, perplexity 30 (P is {n * n * 4 / 2 ** 20:.0f} MiB)")
    setup = {}
    for name, fn in (("fused", lambda: ops.tsne_affinities(x, 30.0)), ("torch", lambda: affinities_torch(x, 30.0))):
        fn()  # warm-up
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        t, out = timed(fn)
        setup[name] = (t, torch.cuda.max_memory_allocated() - base)
        if name == "fused":
            P, _, plogp = out
        else:
            gap = float((out[0] - P).abs().max() / P.max())
        del out
    say(f"  setup: fused {setup['fused'][0] * 1e3:9.2f} ms, peak {setup['fused'][1] / 2 ** 20:8.1f} MiB; torch {setup['torch'][0] * 1e3:9.2f} ms, "
        f"peak {setup['torch'][1] / 2 ** 20:8.1f} MiB; max |P_torch - P_fused| / max P = {gap:.2e}")
    est = GpuTSNE(n_iter=a.iters)
    forms = {"torch": lambda: est.descend(P, plogp, y0.clone(), fused=False)[0], "fused": lambda: est.descend(P, plogp, y0.clone(), fused=True)[0]}
    peak, repeat, last = {}, {}, {}
    for name, fn in forms.items():  # warm-up, then one window alone for its peak memory; the two are compared bit for bit
        first = fn()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        second = fn()
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated() - base
        repeat[name] = torch.equal(first.view(torch.int32), second.view(torch.int32))
        last[name] = second
    agree = float((last["fused"] - last["torch"]).abs().max() / last["torch"].abs().max())
    times = {k: [] for k in forms}
    for fn in forms.values():  # (the allocator's cache was emptied for the peak figures: fill it again outside the windows)
        fn()
    for _ in range(a.rounds):
        for name, fn in forms.items():
            times[name].append(timed(fn)[0])
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = {k: max(v) - min(v) for k, v in times.items()}
    slices = ops.tsne_default_slices(n, x.device)
    for name in forms:
        extra = f"; gradient grid {slices} slices x {-(-n // 32)} row tiles" if name == "fused" else "; per iteration cdist, q, P q, q^2 and two [n, n] x [n, 2] products"
        say(f"  {name:5s}: {med[name] * 1e3:10.3f} ms median per window of {a.iters} iterations, spread {spread[name] * 1e3:8.3f} ms  "
            f"[{', '.join(f'{v * 1e3:.2f}' for v in times[name])}]; {med[name] / a.iters * 1e6:9.1f} us per iteration; peak device memory "
            f"{peak[name] / 2 ** 20:8.1f} MiB; two windows bit-identical: {'yes' if repeat[name] else 'NO'}{extra}")
    say(f"  the two forms after {a.iters} iterations: max |y_fused - y_torch| / max |y| = {agree:.2e} (the descent is chaotic from a 1e-4 start: "
        "two fp32 orders of summation part company well before 50 iterations; tests/test_tsne_gpu.py compares ten)")
    trace = one_iteration(P, plogp, y0, slices)
    for kernel, grid, us in trace:
        rate = ""
        if "grad" in kernel:
            bps = n * n * 4 / (us * 1e-6)
            where = "HBM" if n * n * 4 > 256 * 2 ** 20 else "the Infinity Cache"
            rate = f"; P once: {bps / 1e12:.2f} TB/s from {where} = {bps / HBM_ACHIEVABLE:.2f} of the achievable HBM rate ({bps / 8e12:.2f} of peak)"
        say(f"    one iteration, per kernel (the library's dispatch trace): {kernel:40s} grid {grid} {us:9.1f} us{rate}")
    if sum(us for _, _, us in trace) > med["fused"] / a.iters * 1e6:
        say("    (the traced launches add up to more than the wall time per iteration: the dispatch trace of a one-workgroup launch this short "
            "is not relied on; the wall time is)")
    keep = med["fused"] <= med["torch"] + spread["torch"]
    say(f"  fused / torch = {med['fused'] / med['torch']:.3f} in time, {peak['fused'] / max(peak['torch'], 1):.4f} in peak memory -> "
        f"{'fused' if keep else 'TORCH (fused is slower than the torch form by more than its spread)'}")
    return keep


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsne_fused.txt"))
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--iters", type=int, default=50)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mb_tsne.py measures on the GPU: none found")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")
    say(f"Exact t-SNE, descend(fused=False) against descend(fused=True) ({torch.cuda.get_device_name(0)}; "
        f"python tools/mb_tsne.py --rounds {a.rounds} --iters {a.iters})")
    keeps = []
    for shape in SHAPES:
        keeps.append(measure(shape, a, say))
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    say(f"eval_tsne.py calls: {'fit(fused=True)' if all(keeps) else 'fit(fused=False)'} (the rule: fused unless its median is slower than "
        "the torch form's by more than the torch form's spread, at every shape)")


if __name__ == "__main__":
    main()
