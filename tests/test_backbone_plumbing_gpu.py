"""The launches of one eager training step, stream by stream, against the parent of the backbone-plumbing fold
(tests/golden/plumbing_launches_parent.json, written by gen_plumbing_launches_parent.py on an MI355X in a checkout of that parent).  The
fold is host code only -- one stage node for three, one pass protocol on HipBackbone for two copies, per-pass arguments through
run_stage -- so every workload must enqueue the kernels it enqueued there, with the same grids, in the same order on the same streams."""
import argparse
import collections
import hashlib
import json
import os

import pytest
import torch

from conftest import no_dropout

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLD = os.path.join(ROOT, "tests", "golden", "plumbing_launches_parent.json")
DATA = os.path.join(ROOT, "focal_amd", "src", "data")
B = 8

# name -> (model, dataset, stage setting, FOCAL_DEEPSENSE_TWO_PASSES); between them: the single-tensor node, the list node without and
# with input gradients, both paths of FOCAL.forward, the classifier path with frozen and with trained encoders
WORKLOADS = {
    "swt_mod_pretrain": ("SW_Transformer", "MOD", "pretrain", "0"),
    "swt_har3loc_pretrain": ("SW_Transformer", "HAR3LOC", "pretrain", "0"),
    "deepsense_mod_pretrain": ("DeepSense", "MOD", "pretrain", "0"),
    "deepsense_mod_pretrain_two_passes": ("DeepSense", "MOD", "pretrain", "1"),
    "deepsense_har3loc_pretrain": ("DeepSense", "HAR3LOC", "pretrain", "0"),
    "swt_mod_finetune": ("SW_Transformer", "MOD", "finetune", "0"),
    "deepsense_mod_finetune": ("DeepSense", "MOD", "finetune", "0"),
    "swt_mod_supervised": ("SW_Transformer", "MOD", "supervised", "0"),
    "deepsense_mod_supervised": ("DeepSense", "MOD", "supervised", "0"),
}


def _digest(rows):
    return hashlib.sha256(json.dumps(rows).encode()).hexdigest()


def step_launches(name):
    """The SECOND eager step of the workload (the first builds the arena, the packs and the BatchNorm counter blocks) under the
    library's launch trace -> {"count", "streams": [digest of the ordered (kernel, grid, block) list per stream, streams numbered by first
    appearance], "multiset": digest of the sorted (kernel, grid, block, times) list}.  bf16, dropout off, B = 8, synthetic inputs."""
    from focal_amd import _lib
    from models.FOCALModules import FOCAL
    from models.loss import FOCALLoss
    from oracle.config import load_config
    from oracle.weights import fill_state_dict_, synthetic_freq_input
    model, dataset, stage, two_passes = WORKLOADS[name]
    cfg = no_dropout(load_config(os.path.join(DATA, f"{dataset}.yaml")))
    args = argparse.Namespace(model=model, dataset=dataset, device=torch.device("cuda"), tag=None, dataset_config=cfg, compute_dtype="bf16",
                              train_mode="supervised" if stage == "supervised" else "contrastive",
                              learn_framework="no" if stage == "supervised" else "FOCAL",
                              stage="finetune" if stage == "finetune" else "pretrain",
                              task="vehicle_classification" if dataset == "MOD" else "activity_classification")
    if model == "DeepSense":
        from models.DeepSense import DeepSense as Net
    else:
        from models.SW_Transformer import SW_Transformer as Net
    net = Net(args)
    fill_state_dict_(net.state_dict())
    net = net.to("cuda").train()
    to = lambda d: {l: {m: v.cuda() for m, v in mm.items()} for l, mm in d.items()}
    x1, x2 = to(synthetic_freq_input(cfg, B, seed=311)), to(synthetic_freq_input(cfg, B, seed=312))
    if stage == "pretrain":
        focal, loss_fn = FOCAL(args, net), FOCALLoss(args)

        def step():
            f1, f2 = focal(x1, x2, proj_head=True)
            loss_fn(f1, f2).backward()
    else:
        labels = (torch.arange(B) % cfg[args.task]["num_classes"]).cuda()

        def step():
            torch.nn.functional.cross_entropy(net(x1), labels).backward()
    lib = _lib.load()
    before = os.environ.get("FOCAL_DEEPSENSE_TWO_PASSES")
    os.environ["FOCAL_DEEPSENSE_TWO_PASSES"] = two_passes
    try:
        for _ in range(2):
            net.arena().zero_grad()
            torch.cuda.synchronize()
            _lib.check(lib.focal_trace_begin(8192, _lib.TRACE_DISPATCH))
            try:
                step()
                torch.cuda.synchronize()
            finally:
                lib.focal_trace_end()
            n = lib.focal_trace_count()
            recs = (_lib.TraceRecord * max(n, 1))()
            _lib.check(lib.focal_trace_read(0, n, recs))
    finally:
        if before is None:
            del os.environ["FOCAL_DEEPSENSE_TWO_PASSES"]
        else:
            os.environ["FOCAL_DEEPSENSE_TWO_PASSES"] = before
    assert 0 < n < 8192, n
    per_stream = collections.OrderedDict()
    for i in range(n):
        r = recs[i]
        per_stream.setdefault(r.stream, []).append([r.kernel.decode(), list(r.grid), list(r.block)])
    counts = collections.Counter(json.dumps(row) for rows in per_stream.values() for row in rows)
    return {"count": n, "streams": [_digest(rows) for rows in per_stream.values()], "n_streams": len(per_stream),
            "multiset": _digest(sorted(counts.items()))}


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLD))


def test_the_recorded_workloads_are_these(golden):
    assert sorted(golden["workloads"]) == sorted(WORKLOADS)
    assert all(w["form"] in ("streams", "multiset") for w in golden["workloads"].values())


@pytest.mark.parametrize("name", list(WORKLOADS))
def test_step_launches_are_the_parents(name, golden):
    want = golden["workloads"][name]
    got = step_launches(name)
    print(name, got["count"], "launches on", got["n_streams"], "streams")
    assert got["count"] == want["count"]
    assert got["multiset"] == want["multiset"] and got["n_streams"] == want["n_streams"]
    if want["form"] == "streams":  # (the parent's two recordings agreed stream by stream: so must this one)
        assert got["streams"] == want["streams"]
