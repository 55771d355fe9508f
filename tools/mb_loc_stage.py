"""Microbenchmark of one modality's location-fusion stage (focal_amd/loc_engine.py) at the HAR3LOC step's shapes: N = 2B sequences
of L = 3 location tokens, E = 256, 2 encoder layers + the fusion block, forward + backward with the config's dropout, captured as one
hipGraph and replayed.  Prints one JSON line (ms per replay = one modality's stage in one step).  Under
`rocprofv3 --kernel-trace --stats` every kernel of the trace belongs to the stage: launches per replay = calls / (iters + warm)."""
import argparse
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "focal_amd", "src")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--dtype", default="bf16")
    a = ap.parse_args()
    from models.SW_Transformer import SW_Transformer
    from oracle.config import load_config
    cfg = load_config(os.path.join(ROOT, "focal_amd", "src", "data", "HAR3LOC.yaml"))
    args = argparse.Namespace(model="SW_Transformer", dataset="HAR3LOC", device=torch.device("cuda"), train_mode="contrastive",
                              learn_framework="FOCAL", stage="pretrain", task="activity_classification", tag=None,
                              dataset_config=cfg, compute_dtype=a.dtype)
    net = SW_Transformer(args).cuda().train()
    net.arena()
    stage = net._loc_stages[cfg["modality_names"][0]]
    E = cfg["SW_Transformer"]["loc_out_channels"]
    N = 2 * a.batch
    feats = [torch.randn(N, E, device="cuda") for _ in cfg["location_names"]]
    dy = torch.randn(N, E, device="cuda")

    def body():
        y, sv = stage.forward(feats, 0, True)
        return y, stage.backward(sv, dy)

    warm = 3
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.no_grad(), torch.cuda.stream(side):
        for _ in range(warm):
            body()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        body()
    for _ in range(20):
        graph.replay()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(a.iters):
        graph.replay()
    t1.record()
    torch.cuda.synchronize()
    print(json.dumps({"stage": "location fusion, one modality, fwd + bwd", "N": N, "L": len(cfg["location_names"]), "E": E,
                      "dtype": a.dtype, "ms_per_replay": round(t0.elapsed_time(t1) / a.iters, 4), "replays": a.iters + 20,
                      "eager_warm_runs": warm}))


if __name__ == "__main__":
    main()
