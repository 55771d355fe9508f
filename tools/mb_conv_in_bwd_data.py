"""Microbenchmark of focal_conv_in_bwd_data (the data gradient of the second ConvBlock's in-conv of a multi-location DeepSense) at the
bench shape: dz [2 * batch * 10 * 128, 64] rows (both views of `batch` windows, 10 intervals, spectrum 128), k = 4, scale 1 / 3.
Next to it, in the same run and on the same rows, the existing focal_conv_bwd_data launch (the [1,4] 64 -> 64 residual layer's data
gradient: the row-ring kernel in bf16).  Each is captured as a hipGraph of `per_graph` launches and replayed; time per launch from device
events.  Bytes are what the kernel must move, from the shapes: conv_in_bwd_data reads dz once and writes dx once; conv_bwd_data reads
dz and g_in once and writes g_out once (weights: a few KB, not counted).  Prints one JSON line per kernel.

Two forms per kernel: "replay" launches on ONE set of buffers again and again -- 87 ... 503 MB, much of which stays in the 256 MiB
Infinity Cache, so its rate says how the kernels compare, not what HBM delivers --, and "cold" rotates the launches of a graph over enough
buffer sets (>= 1 GiB in all) that every launch finds its operands evicted: the rate a step sees."""
import argparse
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "focal_amd", "src")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def timed(body, per_graph, replays):
    """us per launch of body(i), i = 0 .. per_graph - 1 captured as one graph (i selects the buffer set)."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for i in range(per_graph):
            body(i)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for i in range(per_graph):
            body(i)
    for _ in range(5):
        graph.replay()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(replays):
        graph.replay()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / (replays * per_graph)  # us per launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--per-graph", type=int, default=20)
    ap.add_argument("--replays", type=int, default=50)
    a = ap.parse_args()
    from focal_amd import ops
    B, I, S, C, k = 2 * a.batch, 10, 128, 64, 4
    rows = B * I * S
    g = torch.Generator().manual_seed(0)
    w_in = (torch.randn(C, 1, 1, k, generator=g) * 0.5).cuda()
    w = (torch.randn(C, C, 1, k, generator=g) * (C * k) ** -0.5).cuda()
    d_in = ops.conv_in_desc(B, 1, I, S, S, k, 1, (k - 1) // 2, C)
    for ct in (torch.bfloat16, torch.float32):
        es = 2 if ct == torch.bfloat16 else 4
        d_cv = ops.conv_desc(ops.code(ct), rows, S, C, C, k)
        w_bwd = ops.conv_pack_bwd(d_cv, w, ct)
        for form in ("replay", "cold"):
            in_bytes, cv_bytes = rows * C * es + rows * 4, rows * C * es + 2 * rows * C * 4
            n_in = 1 if form == "replay" else -(-(1 << 30) // in_bytes)
            n_cv = 1 if form == "replay" else -(-(1 << 30) // cv_bytes)
            dzs = [torch.randn(rows, C, generator=g).cuda().to(ct) for _ in range(max(n_in, n_cv))]
            dxs = [torch.empty(B * I, S, device="cuda") for _ in range(n_in)]
            us = timed(lambda i: ops.conv_in_bwd_data(d_in, dzs[i % n_in], w_in, 1.0 / 3.0, out=dxs[i % n_in]), a.per_graph, a.replays)
            print(json.dumps({"kernel": "focal_conv_in_bwd_data", "form": form, "buffer_sets": n_in, "dz": str(ct)[6:], "tokens": B * I, "S": S,
                              "k": k, "us_per_launch": round(us, 2), "bytes": in_bytes, "GBps": round(in_bytes / us * 1e-3, 1)}))
            del dxs
            gin = [torch.randn(rows, C, generator=g).cuda() for _ in range(n_cv)]
            gout = [torch.empty(rows, C, device="cuda") for _ in range(n_cv)]
            us = timed(lambda i: ops.conv_bwd_data(d_cv, dzs[i % n_cv], w_bwd, gin[i % n_cv], gout[i % n_cv]), a.per_graph, a.replays)
            print(json.dumps({"kernel": "focal_conv_bwd_data", "form": form, "buffer_sets": n_cv, "dz": str(ct)[6:], "rows": rows, "S": S, "k": k,
                              "us_per_launch": round(us, 2), "bytes": cv_bytes, "GBps": round(cv_bytes / us * 1e-3, 1)}))
            del dzs, gin, gout


if __name__ == "__main__":
    main()
