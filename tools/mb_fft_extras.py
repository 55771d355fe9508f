"""Microbenchmark of the view augmenters that travel in a focal_view_extra (jitter, channel shuffle, time mask, freq mask) at the MOD audio
shape of a step, [B, 1, 10, 1600]: the plain transform, each extra folded into it, and -- for jitter -- the two-pass form the fold
replaces, `torch.randn_like(x) * s + x` followed by the plain transform, all timed in the same run by device events over replays of captured graphs (10 calls each),
the variants interleaved.  Prints one JSON line per variant (us per call, median of `--reps` windows of `--iters` calls) and, with `--launches`, the
library launches of one `Augmenter.forward_random_pair` for the shipped pool and for the reference's full eleven-augmenter pool."""
import argparse
import copy
import json
import os
import statistics
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "focal_amd", "src")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def launches_of_a_pair(batch):
    from data_augmenter.Augmenter import Augmenter
    from focal_amd import _lib
    from oracle.config import load_config
    lib = _lib.load()
    base = load_config()
    full = copy.deepcopy(base)
    full["FOCAL"]["random_augmenters"] = {"time_augmenters": ["permutation", "negation", "time_warp", "horizontal_flip", "mag_warp", "scaling", "jitter",
                                                              "channel_shuffle", "time_mask"], "freq_augmenters": ["phase_shift", "freq_mask"]}
    full["jitter"]["value_range"] = {m: 1.0 for m in full["modality_names"]}
    x = {"shake": {"audio": torch.randn(batch, 1, 10, 1600, device="cuda"), "seismic": torch.randn(batch, 1, 10, 20, device="cuda")}}
    for name, cfg in (("shipped pool (7)", base), ("full pool (11)", full)):
        args = argparse.Namespace(model="SW_Transformer", dataset="MOD", device=torch.device("cuda"), train_mode="contrastive", learn_framework="FOCAL",
                                  stage="pretrain", task="vehicle_classification", tag=None, dataset_config=cfg, compute_dtype="bf16")
        aug = Augmenter(args)
        aug.forward_random_pair(x)
        torch.cuda.synchronize()
        _lib.check(lib.focal_trace_begin(64, _lib.TRACE_EVENTS))
        aug.forward_random_pair(x)
        _lib.check(lib.focal_trace_end())
        n = lib.focal_trace_count()
        recs = (_lib.TraceRecord * n)()
        _lib.check(lib.focal_trace_read(0, n, recs))
        print(json.dumps({"metric": "launches of forward_random_pair", "pool": name, "launches": n,
                          "kernels": [r.kernel.decode().split("(")[0][:48] for r in recs]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--launches", action="store_true")
    a = ap.parse_args()
    from focal_amd import ops
    x = torch.randn(a.batch, 1, 10, 1600, device="cuda")
    out = torch.empty(a.batch, 2, 10, 1600, device="cuda")
    std = 0.5

    def two_pass():
        ops.fft_realpack(torch.randn_like(x) * std + x, out=out)

    variants = {"plain": lambda: ops.fft_realpack(x, out=out),
                "plain through the multi export (noise_salt only: the plain kernels)": lambda: ops.fft_realpack(x, out=out, noise_salt=0),
                "identity extra (the extended kernels' plain branch)": lambda: ops.fft_realpack(x, out=out, time_mask=(0, 0)),
                "jitter folded": lambda: ops.fft_realpack(x, out=out, jitter=(std, 12345)),
                "jitter two-pass (randn_like * s + x, then plain)": two_pass,
                "channel_shuffle": lambda: ops.fft_realpack(x, out=out, chan=[0]),
                "time_mask": lambda: ops.fft_realpack(x, out=out, time_mask=(400, 300)),
                "freq_mask": lambda: ops.fft_realpack(x, out=out, freq_mask=(500, 300))}
    # each variant as a captured graph of `per` calls, so that the host's launch cost is not what is timed
    per, graphs = 10, {}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for fn in variants.values():
            for _ in range(5):
                fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for k, fn in variants.items():
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(per):
                fn()
        g.replay()
        graphs[k] = g
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(a.reps):
        for k, g in graphs.items():   # interleaved: one window of each per repetition
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.iters // per):
                g.replay()
            t1.record()
            torch.cuda.synchronize()
            times[k].append(t0.elapsed_time(t1) * 1000.0 / (a.iters // per * per))
    for k, v in times.items():
        print(json.dumps({"metric": "fft_realpack us per call", "shape": [a.batch, 1, 10, 1600], "variant": k, "median_us": round(statistics.median(v), 2),
                          "min_us": round(min(v), 2), "max_us": round(max(v), 2)}))
    if a.launches:
        launches_of_a_pair(a.batch)


if __name__ == "__main__":
    main()
