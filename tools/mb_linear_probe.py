#!/usr/bin/env python3
"""GpuLinearProbe.fit(fused=True) against fit(fused=False), on one box in one process.

  python tools/mb_linear_probe.py [--out profiles/linear_probe_fused.txt] [--rounds 5] [--evals 50]

Random fp32 features at n = 65 536, D = 1024 and at n = 16 384, D = 512; C = 7 classes, four L2 strengths (1e-4 .. 1e-1).  Every fit runs
exactly `evals` evaluations with the stopping tests off, so both forms do the same work under the same host driver (lbfgs_minimize: one
copy up, one evaluation of all four problems, one copy down per evaluation).  Per shape the two forms alternate `rounds` times, each window
one fit between two device synchronisations (host clock; the standardisation of the features is inside the window for both).  Written
per shape and form: the wall time per fit as median and spread (max - min) over the windows, the time per evaluation (median / evals: all
strengths, host driver included), the peak device memory of one fit above what is resident before it, whether two fits of that form are
bit-identical (the float64 iterates and the fp32 weights), and the three launches of one fused evaluation timed on their dispatches.  The
features of both shapes (256 MiB, 32 MiB) fit or nearly fit the 256 MiB Infinity Cache and every pass re-reads them, so the effective
rate over x (two reads per evaluation for the fused form) is a cache rate, not an HBM rate.  Then the rule's verdict: eval_linear.py
calls the fused form unless its median is slower than the torch form's by more than the torch form's own spread."""
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
L2 = (1e-4, 1e-3, 1e-2, 1e-1)


def same_bits(a, b):
    return a.theta_.tobytes() == b.theta_.tobytes() and torch.equal(a.coef_.view(torch.int32), b.coef_.view(torch.int32))


def one_evaluation(x, y, C, R, slices):
    """The three launches of one evaluation of all problems, timed on the dispatches themselves (focal_trace_*)."""
    from focal_amd import _lib, ops
    n, D = x.shape
    w = (0.01 * torch.randn(R * C, D, device=x.device)).contiguous()
    b = torch.zeros(R * C, device=x.device)
    lam = torch.tensor(L2, dtype=torch.float32, device=x.device)
    ce, g, _ = ops.probe_forward(x, w, b, C, y=y, want_ce=True, want_g=True)
    ws = ops.probe_workspace(n, D, C, R, slices, x.device)
    f, gw, gb = ops.probe_grad(x, g, ce, w, lam, C, slices=slices, workspace=ws)
    torch.cuda.synchronize()
    lib = _lib.load()
    _lib.check(lib.focal_trace_begin(16, _lib.TRACE_DISPATCH))
    try:
        ops.probe_forward(x, w, b, C, y=y, ce=ce, g=g, check_labels=False)
        ops.probe_grad(x, g, ce, w, lam, C, gw=gw, gb=gb, f=f, slices=slices, workspace=ws)
        torch.cuda.synchronize()
    finally:
        lib.focal_trace_end()
    cnt = lib.focal_trace_count()
    recs = (_lib.TraceRecord * cnt)()
    _lib.check(lib.focal_trace_read(0, cnt, recs))
    return [f"{r.kernel.decode().split('(')[0][:40]:40s} grid {tuple(r.grid)} {r.us:9.1f} us" for r in recs]


def measure(shape, a, say):
    from focal_amd import ops
    from train_utils.linear_probe import GpuLinearProbe
    n, D, C = shape
    R = len(L2)
    g = torch.Generator().manual_seed(n + D)
    x = torch.randn(n, D, generator=g).cuda()
    y = torch.randint(0, C, (n,), generator=g).cuda()
    forms = {"torch": lambda: GpuLinearProbe(l2=L2).fit(x, y, C, fused=False, stop=False, max_eval=a.evals),
             "fused": lambda: GpuLinearProbe(l2=L2).fit(x, y, C, fused=True, stop=False, max_eval=a.evals)}
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
    slices = ops.probe_default_slices(n, D, x.device)
    say(f"n = {n}, D = {D}, C = {C}, {R} strengths, {a.evals} evaluations per fit, stopping tests off ({a.rounds} alternating windows of one fit "
        f"per form; x is {n * D * 4 / 2 ** 20:.0f} MiB, g [n, R C] {n * R * C * 4 / 2 ** 20:.1f} MiB)")
    for name in forms:
        extra = (f"; forward {-(-n // 128)} workgroups, gradient {slices} slices x {-(-D // 64)} column chunks; x read twice per evaluation: "
                 f"{2 * n * D * 4 * a.evals / med[name] / 1e9:7.1f} GB/s over x (a cache rate, host driver included)") if name == "fused" else \
            f"; per evaluation einsum + logsumexp + softmax + einsum: [{n}, {R}, {C}] fp32 logits, probabilities and their copies"
        say(f"  {name:5s}: {med[name] * 1e3:10.3f} ms median per fit, spread {spread[name] * 1e3:8.3f} ms  [{', '.join(f'{v * 1e3:.2f}' for v in times[name])}]; "
            f"{med[name] / a.evals * 1e3:8.3f} ms per evaluation of all strengths; peak device memory {peak[name] / 2 ** 20:8.1f} MiB; "
            f"two fits bit-identical: {'yes' if repeat[name] else 'NO'}{extra}")
    for rec in one_evaluation(x, y.to(torch.int32), C, R, slices):
        say(f"    one evaluation, per kernel (the library's dispatch trace): {rec}")
    keep = med["fused"] <= med["torch"] + spread["torch"]
    say(f"  fused / torch = {med['fused'] / med['torch']:.3f} in time, {peak['fused'] / max(peak['torch'], 1):.3f} in peak memory -> "
        f"{'fused' if keep else 'TORCH (fused is slower than the torch form by more than its spread)'}")
    return keep


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "linear_probe_fused.txt"))
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--evals", type=int, default=50)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mb_linear_probe.py measures on the GPU: none found")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")
    say(f"Linear probe, fit(fused=False) against fit(fused=True) ({torch.cuda.get_device_name(0)}; "
        f"python tools/mb_linear_probe.py --rounds {a.rounds} --evals {a.evals})")
    keeps = []
    for shape in SHAPES:
        keeps.append(measure(shape, a, say))
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    say(f"eval_linear.py calls: {'fit(fused=True)' if all(keeps) else 'fit(fused=False)'} (the rule: fused unless its median is slower than "
        "the torch form's by more than the torch form's spread, at every shape)")


if __name__ == "__main__":
    main()
