"""Multi-location DeepSense (focal_amd/src/data/HAR3LOC.yaml: 3 locations x 2 modalities) on the host: the module tree is the
reference's (tests/golden/manifest_DeepSense_3loc.json, written by gen_golden_deepsense_multiloc.py from the reference itself), a
reference-layout state dict loads, the second ConvBlocks (mod_extractors.*) are hot in pretraining there and nowhere else, the classifier
path and other channel counts are refused, the two new entry points are declared, and no two dropout sites of a step share a stream."""
import argparse
import copy
import hashlib
import json
import os
import re

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLD = os.path.join(ROOT, "tests", "golden")
DATA = os.path.join(ROOT, "focal_amd", "src", "data")

# the hot-set rule of the single-location code: everything but these prefixes
SINGLE_LOCATION_DEAD = ("patch_embed.", "class_layer.", "mod_fusion_layers.", "absolute_pos_embed.", "mod_extractors.",
                        "loc_fusion_layers.", "loc_context_layers.", "loc_fusion_layer.")


def _cfg(dataset):
    from oracle.config import load_config
    return load_config(os.path.join(DATA, f"{dataset}.yaml"))


def _net(dataset, stage="pretrain", train_mode="contrastive", cfg=None):
    from models.DeepSense import DeepSense
    task = "vehicle_classification" if dataset == "MOD" else "activity_classification"
    args = argparse.Namespace(model="DeepSense", dataset=dataset, device=torch.device("cpu"), train_mode=train_mode, learn_framework="FOCAL",
                              stage=stage, task=task, tag=None, dataset_config=cfg or _cfg(dataset), compute_dtype="fp32")
    return DeepSense(args)


def _layout(net, is_hot):
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


@pytest.fixture(scope="module")
def manifest():
    return json.load(open(os.path.join(GOLD, "manifest_DeepSense_3loc.json")))


@pytest.fixture(scope="module")
def net3():
    return _net("HAR3LOC")


def test_har3loc_module_tree_matches_the_reference_manifest(net3, manifest):
    got = [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in net3.state_dict().items()]
    assert got == manifest
    assert len(manifest) == 324 and sum(p.numel() for p in net3.parameters()) == 7442824


def test_har3loc_reference_layout_state_dict_loads(manifest):
    from oracle.weights import seeded_values
    net = _net("HAR3LOC")
    sd = {k: seeded_values(k, shp) if dt.startswith("float") else torch.zeros(shp, dtype=getattr(torch, dt)) for k, shp, dt in manifest}
    missing, unexpected = net.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    k = "mod_extractors.gyr.conv_layers_inter.2.conv.weight"
    assert torch.equal(net.state_dict()[k], sd[k])
    # ... and a state dict of this build is a reference-layout one (the other direction)
    assert list(net.state_dict().keys()) == [k for k, _, _ in manifest]


def test_har3loc_second_conv_blocks_are_hot_in_pretraining(net3):
    second = [n for n, _ in net3.named_parameters() if n.startswith("mod_extractors.")]
    assert len(second) == 36
    order = [n for n, *_ in _layout(net3, net3._hot)]
    hot = set(order)
    assert set(second) <= hot
    # ... and besides them exactly the single-location hot set, restated: the patch embedding, the head and the mean fusion stay out
    pretrain_dead = ("patch_embed.", "class_layer.", "mod_fusion_layers.", "absolute_pos_embed.", "mod_extractors.", "loc_fusion_layers.")
    assert hot - set(second) == {n for n, _ in net3.named_parameters() if not n.startswith(pretrain_dead)}
    assert not any(n.startswith("class_layer.") for n in hot)
    # the arena keeps the module order: the second blocks between the first-level blocks and the GRUs, as in the state dict
    assert order == [n for n, _ in net3.named_parameters() if n in hot]
    first = min(order.index(n) for n in second)
    assert max(i for i, n in enumerate(order) if n.startswith("loc_mod_extractors.")) < first
    assert max(order.index(n) for n in second) < min(i for i, n in enumerate(order) if n.startswith("recurrent_layers."))


def test_mod_keeps_its_hot_set_and_arena_layout():
    net = _net("MOD")
    # the rule is the single-location one: the layout it gives is the restated one, and the parent's recorded one
    assert _layout(net, net._hot) == _single_location_layout(net)
    assert {n for n, _ in net.named_parameters() if net._hot(n)} == {n for n, _ in net.named_parameters() if not n.startswith(SINGLE_LOCATION_DEAD)}
    rows = [[n, off, numel, list(shape)] for n, off, numel, shape in _layout(net, net._hot)]
    parent = json.load(open(os.path.join(GOLD, "arena_layouts_parent.json")))["cases"]["MOD/DeepSense/pretrain"]
    assert hashlib.sha256(json.dumps(rows).encode()).hexdigest() == parent["sha256"] and len(rows) == parent["hot"]
    assert not any(n.startswith("mod_extractors.") for n, *_ in _layout(net, net._hot))


@pytest.mark.parametrize("kw", [dict(stage="finetune"), dict(train_mode="supervised")])
def test_har3loc_classifier_path_raises(kw):
    with pytest.raises(NotImplementedError, match="multi-location"):
        _net("HAR3LOC", **kw)


@pytest.mark.parametrize("key", ["loc_out_channels", "loc_mod_out_channels"])
def test_other_channel_counts_are_refused(key):
    cfg = copy.deepcopy(_cfg("HAR3LOC"))
    cfg["DeepSense"][key] = 256
    with pytest.raises(NotImplementedError, match="128"):
        _net("HAR3LOC", cfg=cfg)


def test_too_many_locations_or_layers_are_refused():
    from focal_amd import deepsense_engine as de
    de.check_stream_ranges(5, 7, 7, 2)
    with pytest.raises(NotImplementedError, match="locations"):
        de.check_stream_ranges(6, 3, 3, 2)
    with pytest.raises(NotImplementedError, match="inter layers"):
        de.check_stream_ranges(3, 8, 3, 2)
    with pytest.raises(NotImplementedError, match="inter layers"):
        de.check_stream_ranges(3, 3, 8, 2)
    cfg = copy.deepcopy(_cfg("HAR3LOC"))
    cfg["DeepSense"]["loc_conv_inter_layers"] = 8
    with pytest.raises(NotImplementedError, match="inter layers"):
        _net("HAR3LOC", cfg=cfg)


def test_mean_fusion_block_is_a_container_that_points_to_the_engine(net3):
    blk = net3.loc_fusion_layers["acc"]
    assert not list(blk.parameters()) and not list(blk.buffers())
    with pytest.raises(NotImplementedError, match="deepsense_engine"):
        blk(torch.zeros(1, 2, 3, 3))


def test_abi_number_and_the_multiloc_entry_points():
    import ctypes as C
    from focal_amd import _lib
    header = open(os.path.join(ROOT, "include", "focal_hip.h")).read()
    assert re.search(r"#define\s+FOCAL_ABI_VERSION\s+14\b", header) and _lib.ABI_VERSION == 14
    for name in ("focal_conv_in_bwd_data", "focal_rows_mean"):
        assert re.search(rf"\bint\s+{name}\s*\(", header), name
        assert name in _lib.PROTOTYPES, name
        assert hasattr(_lib.load(), name)
    assert re.search(r"typedef struct \{ const float\* p\[8\]; \} focal_ptr8;", header) and C.sizeof(_lib.Ptr8) == 64
    # the descriptor the in-conv entry points share is what it was
    assert "typedef struct { int B, cin, I, S_in, S_out, k, stride, pad_left, C; } focal_conv_in_desc;" in header
    assert C.sizeof(_lib.ConvInDesc) == 36
    assert _lib.PROTOTYPES["focal_rows_mean"][1][2] is _lib.Ptr8  # by value, not a pointer to a table


def test_dropout_stream_ids_of_a_step_are_distinct(net3):
    from focal_amd import deepsense_engine as de
    encs = list(net3._encoders.values())
    assert len(encs) == 2 and [e.mod_index for e in encs] == [0, 1]
    uids = encs[0].stream_uids()
    # 3 first-level stacks of 1 + 4 layers, the second-level stack of 1 + 3, one GRU inter-layer site
    assert len(uids) == 3 * 5 + 4 + 1 and len(set(uids)) == len(uids) and max(uids) < 64
    assert encs[0].second.uids() == [0, 1, 2, 3] and encs[0].gru.uids() == [16]
    assert [st.uids()[0] for st in encs[0].first] == [24, 32, 40]
    for views in ((0, 1), (0xFFFE, 0xFFFF)):  # two passes of a step; one pass carries one view number
        ids = [de.dropout_stream_id(v, e.mod_index, uid) for v in views for e in encs for uid in e.stream_uids()]
        assert len(ids) == 2 * 2 * 20 and len(set(ids)) == len(ids)
        assert max(ids) < 2 ** 28  # below the location-fusion range of SW_Transformer (focal_amd/loc_engine.py: LOC_STREAM_BASE)
    # a single-location encoder's ids are what the formula gave before: ((view * 8 + mod_index) * 64 + uid) * 8, uid = layer / 16 + GRU layer
    mod = _net("MOD")
    for (loc, m), e in mod._encoders.items():
        n_inter = e.geo["n_inter"]
        assert e.stream_uids() == list(range(1 + n_inter)) + [16 + layer for layer in range(e.geo["n_rnn"] - 1)]
        for view in (0, 1, 77):
            assert [e.stack._stream(view, layer) for layer in range(1 + n_inter)] == [((view * 8 + e.mod_index) * 64 + layer) * 8
                                                                                      for layer in range(1 + n_inter)]
            assert de.dropout_stream_id(view, e.mod_index, 16) == ((view * 8 + e.mod_index) * 64 + 16) * 8
