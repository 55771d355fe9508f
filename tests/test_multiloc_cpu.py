"""Multi-location SW_Transformer (focal_amd/src/data/HAR3LOC.yaml: 3 locations x 2 modalities) on the host: the module tree is the
reference's (tests/golden/manifest_SW_Transformer_3loc.json, written by gen_golden_multiloc.py from the reference itself), a
reference-layout state dict loads, the location fusion is hot in pretraining, and the single-location configs keep their arena."""
import argparse
import json
import os

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLD = os.path.join(ROOT, "tests", "golden")
DATA = os.path.join(ROOT, "focal_amd", "src", "data")

# the hot-set rule of the single-location code (before location fusion existed): everything but these prefixes
SINGLE_LOCATION_DEAD = ("patch_embed.", "class_layer.", "mod_fusion_layers.", "absolute_pos_embed.", "mod_extractors.",
                        "loc_fusion_layers.", "loc_context_layers.", "loc_fusion_layer.")


def _args(dataset, stage="pretrain", train_mode="contrastive"):
    from oracle.config import load_config
    cfg = load_config(os.path.join(DATA, f"{dataset}.yaml"))
    task = "vehicle_classification" if dataset == "MOD" else "activity_classification"
    return argparse.Namespace(model="SW_Transformer", dataset=dataset, device=torch.device("cpu"), train_mode=train_mode,
                              learn_framework="FOCAL", stage=stage, task=task, tag=None, dataset_config=cfg, compute_dtype="fp32")


def _net(dataset, **kw):
    from models.SW_Transformer import SW_Transformer
    return SW_Transformer(_args(dataset, **kw))


def _layout(net, is_hot):
    """(name, offset, numel, shape) of the hot parameters: the layout ParamArena builds (focal_amd/arena.py: layout)."""
    from focal_amd.arena import layout
    index, _ = layout(net, is_hot)
    return [(n, *v) for n, v in index.items()]


def _single_location_layout(net):
    """The single-location code's arena, restated: hot = not a SINGLE_LOCATION_DEAD prefix, module order, segments padded to 8."""
    out, off = [], 0
    for n, p in net.named_parameters():
        if not n.startswith(SINGLE_LOCATION_DEAD):
            out.append((n, off, p.numel(), tuple(p.shape)))
            off += (p.numel() + 7) // 8 * 8
    return out


def test_har3loc_module_tree_matches_the_reference_manifest():
    net = _net("HAR3LOC")
    manifest = json.load(open(os.path.join(GOLD, "manifest_SW_Transformer_3loc.json")))
    got = [[k, list(v.shape)] for k, v in net.state_dict().items()]
    assert got == [[k, shp] for k, shp, _ in manifest]
    names = [k for k, _, _ in manifest]
    for mod in ("acc", "gyr"):
        ctx = [k for k in names if k.startswith(f"loc_context_layers.{mod}.")]
        fus = [k for k in names if k.startswith(f"loc_fusion_layer.{mod}.")]
        assert len(ctx) == 2 * 12 and len(fus) == 6
        n = sum(v.numel() for k, v in net.state_dict().items() if k.startswith((f"loc_context_layers.{mod}.", f"loc_fusion_layer.{mod}.")))
        assert 1.0e6 < n < 1.1e6, n  # ~1.06 M parameters of location fusion per modality at E = 256, 4 heads


def test_har3loc_reference_layout_state_dict_loads():
    from oracle.weights import seeded_values
    net = _net("HAR3LOC")
    manifest = json.load(open(os.path.join(GOLD, "manifest_SW_Transformer_3loc.json")))
    sd = {}
    for k, shp, dt in manifest:
        sd[k] = seeded_values(k, shp) if dt.startswith("float") else torch.zeros(shp, dtype=getattr(torch, dt))
    missing, unexpected = net.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    k = "loc_context_layers.gyr.1.self_attn.in_proj_weight"
    assert torch.equal(net.state_dict()[k], sd[k])
    # ... and a state dict of this build is a reference-layout one (the other direction)
    assert list(net.state_dict().keys()) == [k for k, _, _ in manifest]


def test_har3loc_location_fusion_is_hot_in_pretraining():
    net = _net("HAR3LOC")
    loc = [n for n, _ in net.named_parameters() if n.startswith(("loc_context_layers.", "loc_fusion_layer."))]
    assert len(loc) == 2 * (24 + 6)
    hot = {n for n, *_ in _layout(net, net._hot)}
    assert set(loc) <= hot
    # the rest of the hot set is what the single-location rule selects
    assert hot - set(loc) == {n for n, _ in net.named_parameters() if not n.startswith(SINGLE_LOCATION_DEAD)}
    # the arena keeps the module order: location fusion between mod_in_layers and mod_projectors, as in the state dict
    order = [n for n, *_ in _layout(net, net._hot)]
    first_loc, last_in = order.index(loc[0]), max(i for i, n in enumerate(order) if n.startswith("mod_in_layers."))
    assert last_in < first_loc < min(i for i, n in enumerate(order) if n.startswith("mod_projectors."))


@pytest.mark.parametrize("dataset", ["MOD", "HAR4"])
def test_single_location_hot_set_and_arena_layout_unchanged(dataset):
    net = _net(dataset)
    assert not hasattr(net, "loc_context_layers") and not hasattr(net, "loc_fusion_layer")
    assert _layout(net, net._hot) == _single_location_layout(net)


@pytest.mark.parametrize("kw", [dict(stage="finetune"), dict(train_mode="supervised")])
def test_har3loc_classifier_path_still_raises(kw):
    with pytest.raises(NotImplementedError, match="location fusion in the classifier head"):
        _net("HAR3LOC", **kw)


def test_har3loc_stream_ids_are_distinct():
    """Every (view, modality, layer, site) of the location stage draws its own dropout stream, above the encoders' range."""
    net = _net("HAR3LOC")
    from focal_amd.loc_engine import FUSION_LAYER, LOC_STREAM_BASE
    ids = [st.stream_id(v, layer, site) for st in net._loc_stages.values() for v in (0, 1, 0xFFFF)
           for layer in list(range(st.blocks)) + [FUSION_LAYER] for site in range(4)]
    assert len(ids) == len(set(ids)) and min(ids) >= LOC_STREAM_BASE and max(ids) < 2 ** 32
    # the encoders of the same modality at different locations no longer share their dropout streams
    idx = {k: e.mod_index for k, e in net._encoders.items()}
    assert len(set(idx.values())) == 6 and idx[("wrist", "acc")] == 0 and idx[("wrist", "gyr")] == 1
