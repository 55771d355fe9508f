#!/usr/bin/env python3
"""GpuKNNClassifier.predict against predict_fused, on one box in one process.

  python tools/mb_knn.py [--out profiles/knn_fused.txt] [--rounds 5] [--calls 10]

Random fp32 features at nq = 8192, nt = 65 536, D = 1024, C = 7 and at nq = 2048, nt = 16 384, D = 512.  Per shape the two forms alternate
`rounds` times, each window `calls` calls between two device synchronisations (host clock; both forms end in device work only).  Written
per shape and form: the wall time per call as median and spread (max - min) over the windows, the peak device memory of one call above
what is resident before it (torch.cuda.max_memory_allocated), and the achieved fp32 rate over 2 nq nt D -- a whole-call rate: predict()'s
call holds the product, the element-wise pass, top-k and the vote; predict_fused's the search and the vote launch.  Then the share of
queries on which the two agree, and the rule's verdict: eval_knn.py calls the fused form unless its median is slower than predict()'s by
more than predict()'s own spread."""
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

SHAPES = [(8192, 65536, 1024, 7), (2048, 16384, 512, 7)]


def measure(shape, a, say):
    from focal_amd import ops
    from train_utils.knn import GpuKNNClassifier
    nq, nt, D, C = shape
    g = torch.Generator().manual_seed(nq + nt + D)
    est = GpuKNNClassifier().fit(torch.randn(nt, D, generator=g).cuda(), torch.randint(0, C, (nt,), generator=g).cuda())
    q = torch.randn(nq, D, generator=g).cuda()
    forms = {"predict": lambda: est.predict(q), "predict_fused": lambda: est.predict_fused(q)}
    out, peak = {}, {}
    for name, fn in forms.items():   # warm-up of every shape both forms use, then one call alone for its peak memory
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
    flop = 2.0 * nq * nt * D
    slices = ops.knn_default_slices(nq, nt, q.device)
    say(f"nq = {nq}, nt = {nt}, D = {D}, C = {C}, k = 5 ({a.rounds} alternating windows of {a.calls} calls per form; {flop / 1e12:.3f} TFLOP in the product)")
    for name in forms:
        extra = f"; {slices} slices, {-(-nq // 128) * slices} workgroups" if name == "predict_fused" else f"; chunks of 8192 queries: a [{min(nq, 8192)}, {nt}] fp32 matrix"
        say(f"  {name:14s}: {med[name] * 1e3:9.3f} ms median per call, spread {spread[name] * 1e3:7.3f} ms  [{', '.join(f'{v * 1e3:.2f}' for v in times[name])}]; "
            f"{flop / med[name] / 1e12:6.1f} TFLOP/s fp32 over the call; peak device memory {peak[name] / 2 ** 20:8.1f} MiB{extra}")
    agree = (out["predict"] == out["predict_fused"]).float().mean().item()
    keep = med["predict_fused"] <= med["predict"] + spread["predict"]
    say(f"  the two agree on {agree:.4f} of the queries; predict_fused / predict = {med['predict_fused'] / med['predict']:.3f} in time, "
        f"{peak['predict_fused'] / max(peak['predict'], 1):.4f} in peak memory -> "
        f"{'fused' if keep else 'PREDICT (fused is slower than predict by more than its spread)'}")
    return keep


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_fused.txt"))
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--calls", type=int, default=10)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mb_knn.py measures on the GPU: none found")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")
    say(f"KNN scoring, predict() against predict_fused() ({torch.cuda.get_device_name(0)}; tools/mb_knn.py)")
    keeps = []
    for shape in SHAPES:
        keeps.append(measure(shape, a, say))
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    say(f"eval_knn.py calls: {'predict_fused' if all(keeps) else 'predict'} (the rule: fused unless its median is slower than predict's by more than predict's spread, at every shape)")


if __name__ == "__main__":
    main()
