"""The backbones' hot-set rule against the parent of the plumbing fold (tests/golden/arena_layouts_parent.json, written by
gen_arena_layouts_parent.py in a checkout of that parent): every yaml under focal_amd/src/data x both models x {pretrain, finetune,
supervised} (x APE off / on for SW_Transformer) gives the arena layout -- names, order, offsets, sizes, shapes -- it gave there, or raises
what it raised there; the rule says `has_head` exactly where the classifier head is in the arena."""
import argparse
import copy
import glob
import hashlib
import json
import os

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLD = os.path.join(ROOT, "tests", "golden", "arena_layouts_parent.json")
DATA = os.path.join(ROOT, "focal_amd", "src", "data")
# stage setting -> (stage, train_mode, learn_framework)
STAGES = {"pretrain": ("pretrain", "contrastive", "FOCAL"), "finetune": ("finetune", "contrastive", "FOCAL"),
          "supervised": ("pretrain", "supervised", "no")}


def case_ids():
    ids = []
    for path in sorted(glob.glob(os.path.join(DATA, "*.yaml"))):
        dataset = os.path.splitext(os.path.basename(path))[0]
        for stage in STAGES:
            ids.append(f"{dataset}/DeepSense/{stage}")
            ids += [f"{dataset}/SW_Transformer/{stage}/ape_{ape}" for ape in ("off", "on")]
    return ids


def build(case):
    """The backbone of one case, on the CPU (goes through constructor arguments only: the fold leaves those alone)."""
    from oracle.config import load_config
    dataset, model, stage, *ape = case.split("/")
    cfg = copy.deepcopy(load_config(os.path.join(DATA, f"{dataset}.yaml")))
    if ape:
        cfg["SW_Transformer"]["APE"] = ape[0] == "ape_on"
    st, train_mode, framework = STAGES[stage]
    task = "vehicle_classification" if "vehicle_classification" in cfg else "activity_classification"
    args = argparse.Namespace(model=model, dataset=dataset, device=torch.device("cpu"), train_mode=train_mode, learn_framework=framework,
                              stage=st, task=task, tag=None, dataset_config=cfg, compute_dtype="fp32")
    if model == "DeepSense":
        from models.DeepSense import DeepSense
        return DeepSense(args)
    from models.SW_Transformer import SW_Transformer
    return SW_Transformer(args)


def record(case):
    from focal_amd.arena import layout
    try:
        net = build(case)
    except NotImplementedError:
        return {"raises": "NotImplementedError"}
    index, total = layout(net, net._hot)
    rows = [[n, off, numel, list(shape)] for n, (off, numel, shape) in index.items()]
    return {"hot": len(rows), "total": total, "sha256": hashlib.sha256(json.dumps(rows).encode()).hexdigest()}


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLD))


def test_the_matrix_is_the_recorded_one(golden):
    assert sorted(golden["cases"]) == sorted(case_ids()) and len(golden["cases"]) == 27
    # the HAR3LOC finetune and supervised cases of both models (SW_Transformer with APE off and on): 2 + 4
    assert sorted(c for c, v in golden["cases"].items() if "raises" in v) == sorted(
        c for c in case_ids() if c.startswith("HAR3LOC/") and c.split("/")[2] != "pretrain")
    assert sum("raises" in v for v in golden["cases"].values()) == 6
    assert golden["cases"]["MOD/SW_Transformer/pretrain/ape_off"]["hot"] == 232
    assert golden["cases"]["MOD/SW_Transformer/pretrain/ape_off"]["total"] == 11446144
    assert golden["cases"]["HAR3LOC/DeepSense/pretrain"]["hot"] == 208
    assert golden["cases"]["HAR3LOC/DeepSense/pretrain"]["total"] == 7434624


@pytest.mark.parametrize("case", case_ids())
def test_arena_layout_is_the_parents(case, golden):
    assert record(case) == golden["cases"][case]


@pytest.mark.parametrize("case", case_ids())
def test_has_head_exactly_where_the_classifier_trains(case, golden):
    if "raises" in golden["cases"][case]:
        with pytest.raises(NotImplementedError):
            build(case)
        return
    net = build(case)
    hot = [n for n, _ in net.named_parameters() if net._hot(n)]
    assert net._hot.has_head == (case.split("/")[2] in ("finetune", "supervised"))
    assert net._hot.has_head == any(n.startswith("class_layer.") for n in hot)
