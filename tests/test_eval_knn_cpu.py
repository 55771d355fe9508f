"""Host half of eval_knn.py: the checkpoint it resolves, what it refuses before anything is built, the -knn_k flag and the two exports'
declarations."""
import argparse
import importlib.util
import os
import re
import sys

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SRC = os.path.join(ROOT, "focal_amd", "src")


def entry():
    spec = importlib.util.spec_from_file_location("focal_eval_knn_entry", os.path.join(SRC, "eval_knn.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _run(tmp_path, **kw):
    base = dict(dataset="HAR3LOC", model="SW_Transformer", task="activity_classification", learn_framework="FOCAL", stage="pretrain",
                label_ratio=1.0, model_weight=None, weight_folder=str(tmp_path / "weights" / "HAR3LOC_SW_Transformer"), knn_k=5)
    base.update(kw)
    return argparse.Namespace(**base)


def test_resolve_backbone_weight(tmp_path):
    from params.knn_params import resolve_backbone_weight
    folder = str(tmp_path / "weights" / "HAR3LOC_SW_Transformer")
    # the default: what train_utils/pretrain.py writes
    assert resolve_backbone_weight(_run(tmp_path)) == os.path.join(folder, "HAR3LOC_SW_Transformer_pretrain_best.pt")
    other = tmp_path / "elsewhere"
    other.mkdir()
    # -model_weight names a directory: the folder
    got = resolve_backbone_weight(_run(tmp_path, model="DeepSense", dataset="MOD", model_weight=str(other)))
    assert got == os.path.join(str(other), "MOD_DeepSense_pretrain_best.pt")
    # -model_weight names an existing file: that file
    ckpt = other / "anything.pt"
    ckpt.write_bytes(b"")
    assert resolve_backbone_weight(_run(tmp_path, model_weight=str(ckpt))) == str(ckpt)


@pytest.fixture
def nothing_is_built(monkeypatch):
    """A loader, a model or a device selected during a refusal fails the test."""
    import input_utils.multi_modal_dataloader as loaders
    import params.params_util as util
    import train_utils.model_selection as selection

    def forbidden(*a, **k):
        raise AssertionError("built before the refusal")
    monkeypatch.setattr(loaders, "create_dataloader", forbidden)
    monkeypatch.setattr(selection, "init_backbone_model", forbidden)
    monkeypatch.setattr(util, "select_device", forbidden)
    monkeypatch.setattr(torch.cuda, "set_device", forbidden)
    monkeypatch.delenv("WORLD_SIZE", raising=False)


def test_other_frameworks_are_refused(monkeypatch, tmp_path, nothing_is_built):
    from params.knn_params import parse_knn_params
    monkeypatch.setattr(sys, "argv", ["eval_knn.py", "-model=DeepSense", "-dataset=MOD", "-learn_framework=no"])
    with pytest.raises(ValueError, match=r"test\.py -model=DeepSense -dataset=MOD -learn_framework=no"):
        parse_knn_params()
    with pytest.raises(ValueError, match=r"test\.py"):
        entry().evaluate_knn(_run(tmp_path, learn_framework="no", backbone_weight=str(tmp_path / "x.pt")))


def test_data_parallel_is_refused(monkeypatch, tmp_path, nothing_is_built):
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="one process"):
        entry().evaluate_knn(_run(tmp_path, backbone_weight=str(tmp_path / "x.pt")))
    with pytest.raises(SystemExit, match="one process"):
        entry().main_eval_knn()


def test_missing_checkpoint_is_refused(tmp_path, nothing_is_built):
    from params.knn_params import resolve_backbone_weight
    args = _run(tmp_path)
    args.backbone_weight = resolve_backbone_weight(args)
    with pytest.raises(FileNotFoundError, match=r"train\.py -model=SW_Transformer -dataset=HAR3LOC -learn_framework=FOCAL"):
        entry().evaluate_knn(args)
    assert not hasattr(args, "classifier")


@pytest.mark.parametrize("name,flags", [("MOD_DeepSense_vehicle_classification_1.0_finetune_best.pt", "-learn_framework=FOCAL -stage=finetune"),
                                        ("MOD_DeepSense_vehicle_classification_0.1_finetune_latest.pt", "-learn_framework=FOCAL -stage=finetune"),
                                        ("MOD_DeepSense_vehicle_classification_best.pt", "-learn_framework=no")])
def test_classifier_checkpoint_is_refused(tmp_path, nothing_is_built, name, flags):
    path = tmp_path / name
    torch.save({"class_layer.0.weight": torch.zeros(2, 2)}, path)
    args = _run(tmp_path, model="DeepSense", dataset="MOD", task="vehicle_classification", model_weight=str(path), backbone_weight=str(path))
    with pytest.raises(ValueError, match=re.escape(f"test.py -model=DeepSense -dataset=MOD {flags}")):
        entry().evaluate_knn(args)
    assert not hasattr(args, "classifier")


def test_pretraining_checkpoint_with_its_class_layer_is_taken(monkeypatch, tmp_path):
    """What train_utils/pretrain.py saves is the backbone's whole state dict, the untrained class_layer.* included: that file is read and
    the run goes on to build its loaders (where this test stops it)."""
    import input_utils.multi_modal_dataloader as loaders

    class Reached(Exception):
        pass

    def stop(*a, **k):
        raise Reached()
    monkeypatch.setattr(loaders, "create_dataloader", stop)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    path = tmp_path / "MOD_DeepSense_pretrain_best.pt"
    torch.save({"class_layer.0.weight": torch.zeros(2, 2), "mod_projectors.audio.0.bias": torch.zeros(4)}, path)
    args = _run(tmp_path, model="DeepSense", dataset="MOD", task="vehicle_classification", backbone_weight=str(path), batch_size=8, workers=0)
    with pytest.raises(Reached):
        entry().evaluate_knn(args)


def test_knn_k_parses(monkeypatch):
    from params.base_params import parse_base_args
    monkeypatch.setattr(sys, "argv", ["eval_knn.py", "-learn_framework=FOCAL"])
    assert parse_base_args("eval_knn").knn_k == 5
    monkeypatch.setattr(sys, "argv", ["eval_knn.py", "-learn_framework=FOCAL", "-knn_k=9"])
    assert parse_base_args("eval_knn").knn_k == 9


def test_exports_are_declared_at_abi_14():
    from focal_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "focal_hip.h")).read()
    assert re.search(r"#define FOCAL_ABI_VERSION 14\b", hdr) and _lib.ABI_VERSION == 14
    assert re.search(r"typedef struct \{ int nq, nt, D, k, n_classes, slices; \} focal_knn_desc;", hdr)
    assert re.search(r"int focal_knn_search\(const focal_knn_desc\* d, const float\* q, const float\* t, const float\* t_sq, float\* part_d2,\s*"
                     r"int\* part_idx,\s*void\* stream\);", hdr)
    assert re.search(r"int focal_knn_vote\(const focal_knn_desc\* d, const float\* part_d2, const int\* part_idx, const long\* t_labels,\s*"
                     r"const long\* q_labels,\s*long\* preds, int\* nbr_idx, float\* nbr_d2, int\* conf, void\* stream\);", hdr)
    assert len(_lib.PROTOTYPES["focal_knn_search"][1]) == 7 and len(_lib.PROTOTYPES["focal_knn_vote"][1]) == 10
    assert [n for n, _ in _lib.KnnDesc._fields_] == ["nq", "nt", "D", "k", "n_classes", "slices"]
