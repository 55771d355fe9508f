"""SW_Transformer's `APE` and `in_stride` switches on the host: which parameters join the arena, what stays frozen in finetuning, the
stride-2 module tree against the reference's manifest (tests/golden/manifest_SW_Transformer_stride.json, written by
gen_golden_ape_stride.py from the reference itself), the constructor's refusal of a spectrum the stride does not divide, and the ABI."""
import argparse
import copy
import json
import os
import re

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLD = os.path.join(ROOT, "tests", "golden")
APE = "absolute_pos_embed."


def _net(ape=False, stride=None, stage="pretrain", train_mode="contrastive", spectrum=None):
    from models.SW_Transformer import SW_Transformer
    from oracle.config import load_config
    cfg = copy.deepcopy(load_config())
    cfg["SW_Transformer"]["APE"] = ape
    if stride:
        cfg["SW_Transformer"]["in_stride"] = dict(stride)
    if spectrum:
        cfg["loc_mod_spectrum_len"]["shake"].update(spectrum)
    args = argparse.Namespace(model="SW_Transformer", dataset="MOD", device=torch.device("cpu"), train_mode=train_mode,
                              learn_framework="FOCAL" if train_mode != "supervised" else "no", stage=stage,
                              task="vehicle_classification", tag=None, dataset_config=cfg, compute_dtype="fp32")
    return args, SW_Transformer(args)


def _hot(net):
    from focal_amd.arena import layout
    return list(layout(net, net._hot)[0])


@pytest.mark.parametrize("kw", [dict(), dict(train_mode="supervised")])
def test_ape_joins_the_hot_set_exactly(kw):
    _, off = _net(ape=False, **kw)
    _, on = _net(ape=True, **kw)
    names = [n for n, _ in on.named_parameters() if n.startswith(APE)]
    assert names == [f"{APE}shake.seismic", f"{APE}shake.audio"]
    assert set(_hot(on)) - set(_hot(off)) == set(names) and set(_hot(off)) <= set(_hot(on))
    assert not [n for n in _hot(off) if n.startswith(APE)]
    # module order is kept: the arena of the APE model without its APE segments is the APE-off arena's name list
    assert [n for n in _hot(on) if not n.startswith(APE)] == _hot(off)


def test_har3loc_with_ape_puts_every_location_table_into_the_hot_set():
    """The multi-location pretraining path runs the same encoder code: one table per (location, modality) joins the arena."""
    from models.SW_Transformer import SW_Transformer
    from oracle.config import load_config
    cfg = copy.deepcopy(load_config(os.path.join(ROOT, "focal_amd", "src", "data", "HAR3LOC.yaml")))
    nets = {}
    for ape in (False, True):
        cfg["SW_Transformer"]["APE"] = ape
        args = argparse.Namespace(model="SW_Transformer", dataset="HAR3LOC", device=torch.device("cpu"), train_mode="contrastive",
                                  learn_framework="FOCAL", stage="pretrain", task="activity_classification", tag=None,
                                  dataset_config=copy.deepcopy(cfg), compute_dtype="fp32")
        nets[ape] = SW_Transformer(args)
    added = set(_hot(nets[True])) - set(_hot(nets[False]))
    assert len(added) == 6 and all(n.startswith(APE) for n in added)
    assert [n for n in _hot(nets[True]) if n not in added] == _hot(nets[False])


def test_ape_off_leaves_the_arena_layout_alone():
    """APE off: the pretraining and the supervised arena are what the rules without the switch gave -- restated here as prefix tuples, and
    as the layouts recorded at the commit before the rule became one object (tests/golden/arena_layouts_parent.json)."""
    import hashlib
    from focal_amd.arena import layout
    parent = json.load(open(os.path.join(GOLD, "arena_layouts_parent.json")))["cases"]
    pretrain_dead = ("patch_embed.", "class_layer.", "mod_fusion_layers.", APE, "mod_extractors.", "loc_fusion_layers.")
    supervised_dead = (APE, "mod_extractors.", "loc_fusion_layers.", "loc_context_layers.", "loc_fusion_layer.", "mod_projectors.")
    for kw, dead, case in ((dict(), pretrain_dead, "MOD/SW_Transformer/pretrain/ape_off"),
                           (dict(train_mode="supervised"), supervised_dead, "MOD/SW_Transformer/supervised/ape_off")):
        _, net = _net(ape=False, **kw)
        assert layout(net, net._hot) == layout(net, lambda n: not n.startswith(dead))
        index, total = layout(net, net._hot)
        rows = [[n, off, numel, list(shape)] for n, (off, numel, shape) in index.items()]
        assert (len(rows), total) == (parent[case]["hot"], parent[case]["total"])
        assert hashlib.sha256(json.dumps(rows).encode()).hexdigest() == parent[case]["sha256"]


def test_finetune_keeps_the_position_embedding_frozen():
    from general_utils.weight_utils import set_learnable_params_finetune
    args, net = _net(ape=True, stage="finetune")
    assert not [n for n in _hot(net) if n.startswith(APE)]  # a frozen operand, read where it lives
    set_learnable_params_finetune(args, net)
    learnable = [n for n, p in net.named_parameters() if p.requires_grad]
    assert learnable and not [n for n in learnable if n.startswith(APE)]
    assert all("class_layer" in n or "mod_fusion_layer" in n for n in learnable)


def test_pretraining_freeze_leaves_the_position_embedding_trainable():
    from general_utils.weight_utils import freeze_patch_embedding
    from models.FOCALModules import FOCAL
    args, net = _net(ape=True)
    freeze_patch_embedding(args, FOCAL(args, net))
    p = dict(net.named_parameters())
    assert p[f"{APE}shake.audio"].requires_grad and not p["patch_embed.shake.audio.proj.weight"].requires_grad


def test_stride_two_model_has_the_reference_state_dict():
    _, net = _net(ape=True, stride={"audio": 2, "seismic": 1})
    manifest = json.load(open(os.path.join(GOLD, "manifest_SW_Transformer_stride.json")))
    assert [[k, list(v.shape)] for k, v in net.state_dict().items()] == [[k, shp] for k, shp, _ in manifest]
    sd = net.state_dict()
    assert tuple(sd["patch_embed.shake.audio.proj.weight"].shape) == (64, 4, 1, 40)  # 2 channels x stride 2, 40 taps
    geo = net.geometry["shake"]["audio"]
    assert geo["stride"] == 2 and geo["pad_img"][1] >= 800 and geo["grid"][1] >= 20
    assert tuple(sd[f"{APE}shake.audio"].shape) == (1, geo["grid"][0] * geo["grid"][1], 64)
    # stride 1 stays what it was
    _, one = _net()
    assert one.geometry["shake"]["audio"]["stride"] == 1 and one.geometry["shake"]["audio"]["grid"][1] >= 40


def test_a_stride_that_does_not_divide_the_spectrum_is_refused():
    with pytest.raises(ValueError, match=r"in_stride\[audio\] = 3 .*loc_mod_spectrum_len"):
        _net(stride={"audio": 3, "seismic": 1})
    with pytest.raises(ValueError, match=r"in_stride\[seismic\]"):
        _net(stride={"audio": 1, "seismic": 2}, spectrum={"seismic": 21})


def test_abi_number_and_the_ape_stride_entry_points():
    from focal_amd import _lib
    header = open(os.path.join(ROOT, "include", "focal_hip.h")).read()
    assert re.search(r"#define\s+FOCAL_ABI_VERSION\s+14\b", header) and _lib.ABI_VERSION == 14
    for name in ("focal_pad_patch_embed_ape_ln_fwd", "focal_pad_patch_embed_ape_ln2_fwd", "focal_ape_bwd", "focal_ape_add_fwd"):
        assert re.search(rf"\bint\s+{name}\s*\(", header), name
        assert name in _lib.PROTOTYPES, name
    assert "focal_embed2_desc" in header
    # the descriptors the old entry points take are what they were
    assert "typedef struct { int B, cin, I, S, Hp, Wp, pw, C0; float eps; } focal_embed_desc;" in header
    assert [f[0] for f in _lib.Embed2Desc._fields_] == ["B", "cin", "I", "S", "Hp", "Wp", "pw", "C0", "stride", "eps"]
