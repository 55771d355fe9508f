"""Host half of eval_retrieval.py: its flags, what it refuses before anything is built, the metrics on hand-made rank vectors, the
orthogonality cosines against numpy float64, and the export's declarations."""
import argparse
import importlib.util
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SRC = os.path.join(ROOT, "focal_amd", "src")
TWO_MODS = {"modality_names": ["seismic", "audio"], "FOCAL": {"emb_dim": 256}}


def entry():
    spec = importlib.util.spec_from_file_location("focal_eval_retrieval_entry", os.path.join(SRC, "eval_retrieval.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _run(tmp_path, **kw):
    base = dict(dataset="HAR3LOC", model="SW_Transformer", task="activity_classification", learn_framework="FOCAL", stage="pretrain",
                label_ratio=1.0, model_weight=None, weight_folder=str(tmp_path / "weights" / "HAR3LOC_SW_Transformer"),
                retrieval_split="test", retrieval_k="1,5,10", dataset_config=TWO_MODS, backbone_weight=str(tmp_path / "x.pt"))
    base.update(kw)
    return argparse.Namespace(**base)


@pytest.fixture
def nothing_is_built(monkeypatch):
    """A loader, a model or a device selected during a refusal fails the test."""
    import input_utils.multi_modal_dataloader as loaders
    import params.params_util as util
    import params.retrieval_params as rparams
    import train_utils.model_selection as selection

    def forbidden(*a, **k):
        raise AssertionError("built before the refusal")
    monkeypatch.setattr(loaders, "create_dataloader", forbidden)
    monkeypatch.setattr(selection, "init_backbone_model", forbidden)
    monkeypatch.setattr(util, "select_device", forbidden)
    monkeypatch.setattr(rparams, "set_auto_params", forbidden)
    monkeypatch.setattr(torch.cuda, "set_device", forbidden)
    monkeypatch.delenv("WORLD_SIZE", raising=False)


# ------------------------------------------------------------------------------------------ flags
def test_flags_default_and_parse(monkeypatch):
    from params.base_params import parse_base_args
    from params.retrieval_params import parse_retrieval_ks, refuse_retrieval_settings
    monkeypatch.setattr(sys, "argv", ["eval_retrieval.py", "-learn_framework=FOCAL"])
    a = parse_base_args("eval_retrieval")
    assert a.option == "eval_retrieval" and a.retrieval_split == "test" and a.retrieval_k == "1,5,10"
    assert refuse_retrieval_settings(a) == [1, 5, 10]
    monkeypatch.setattr(sys, "argv", ["eval_retrieval.py", "-learn_framework=FOCAL", "-retrieval_split=val", "-retrieval_k=2, 7,100"])
    a = parse_base_args("eval_retrieval")
    assert a.retrieval_split == "val" and refuse_retrieval_settings(a) == [2, 7, 100]
    assert parse_retrieval_ks("3") == [3] and parse_retrieval_ks("1,2,3,4,5,6,7,8") == list(range(1, 9))


# ------------------------------------------------------------------------------------------ refusals
def test_other_frameworks_are_refused(monkeypatch, tmp_path, nothing_is_built):
    from params.retrieval_params import parse_retrieval_params
    monkeypatch.setattr(sys, "argv", ["eval_retrieval.py", "-model=DeepSense", "-dataset=MOD", "-learn_framework=no"])
    with pytest.raises(ValueError, match=r"eval_retrieval\.py.*test\.py -model=DeepSense -dataset=MOD -learn_framework=no"):
        parse_retrieval_params()
    with pytest.raises(ValueError, match=r"eval_retrieval\.py.*test\.py"):
        entry().evaluate_retrieval(_run(tmp_path, learn_framework="no"))


def test_data_parallel_is_refused(monkeypatch, tmp_path, nothing_is_built):
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="one process"):
        entry().evaluate_retrieval(_run(tmp_path))
    with pytest.raises(SystemExit, match="one process"):
        entry().main_eval_retrieval()


def test_missing_checkpoint_is_refused(tmp_path, nothing_is_built):
    from params.knn_params import resolve_backbone_weight
    args = _run(tmp_path)
    args.backbone_weight = resolve_backbone_weight(args)
    with pytest.raises(FileNotFoundError, match=r"train\.py -model=SW_Transformer -dataset=HAR3LOC -learn_framework=FOCAL"):
        entry().evaluate_retrieval(args)
    assert not hasattr(args, "classifier")


@pytest.mark.parametrize("name,flags", [("MOD_DeepSense_vehicle_classification_1.0_finetune_best.pt", "-learn_framework=FOCAL -stage=finetune"),
                                        ("MOD_DeepSense_vehicle_classification_best.pt", "-learn_framework=no")])
def test_classifier_checkpoint_is_refused(tmp_path, nothing_is_built, name, flags):
    path = tmp_path / name
    torch.save({"class_layer.0.weight": torch.zeros(2, 2)}, path)
    args = _run(tmp_path, model="DeepSense", dataset="MOD", task="vehicle_classification", model_weight=str(path), backbone_weight=str(path))
    with pytest.raises(ValueError, match=re.escape(f"test.py -model=DeepSense -dataset=MOD {flags}") + r".*eval_retrieval\.py"):
        entry().evaluate_retrieval(args)
    assert not hasattr(args, "classifier")


@pytest.mark.parametrize("flag,match", [("-retrieval_k=1,,5", "empty entry"), ("-retrieval_k=", "empty entry"), ("-retrieval_k=1,0", ">= 1"),
                                        ("-retrieval_k=-3", ">= 1"), ("-retrieval_k=1,2,3,4,5,6,7,8,9", "at most 8"),
                                        ("-retrieval_k=1,x", "no integer"), ("-retrieval_split=all", "test, val, train")])
def test_settings_are_refused(monkeypatch, tmp_path, nothing_is_built, flag, match):
    from params.retrieval_params import parse_retrieval_params
    monkeypatch.setattr(sys, "argv", ["eval_retrieval.py", "-model=DeepSense", "-dataset=MOD", "-learn_framework=FOCAL", flag])
    with pytest.raises(ValueError, match=r"eval_retrieval\.py.*" + re.escape(match)):
        parse_retrieval_params()
    name, value = flag[1:].split("=", 1)
    with pytest.raises(ValueError, match=re.escape(match)):
        entry().evaluate_retrieval(_run(tmp_path, **{name: value}))


def test_dataset_shape_is_refused(monkeypatch, tmp_path, nothing_is_built):
    from input_utils.yaml_utils import load_yaml
    from params.retrieval_params import parse_retrieval_params
    cfg = load_yaml(os.path.join(SRC, "data", "MOD.yaml"))
    assert len(cfg["modality_names"]) >= 2 and cfg["FOCAL"]["emb_dim"] == 256
    import yaml
    one = dict(cfg, modality_names=cfg["modality_names"][:1])
    odd = dict(cfg, FOCAL=dict(cfg["FOCAL"], emb_dim=36))  # halves of 18 columns
    for name, bad, match in (("one.yaml", one, r"1 modality.*eval_knn\.py -model=DeepSense -dataset=MOD"),
                             ("odd.yaml", odd, r"emb_dim=36.*halves of 18.*multiple of 8")):
        path = tmp_path / name
        path.write_text(yaml.safe_dump(bad))
        monkeypatch.setattr(sys, "argv", ["eval_retrieval.py", "-model=DeepSense", "-dataset=MOD", "-learn_framework=FOCAL", f"-config={path}"])
        with pytest.raises(ValueError, match=match):
            parse_retrieval_params()
        with pytest.raises(ValueError, match=match):
            entry().evaluate_retrieval(_run(tmp_path, model="DeepSense", dataset="MOD", dataset_config=bad))


# ------------------------------------------------------------------------------------------ metrics
def test_retrieval_metrics_on_hand_made_ranks():
    from train_utils.retrieval import retrieval_metrics
    ones = retrieval_metrics(torch.ones(7, dtype=torch.int64), torch.zeros(7, dtype=torch.int64), [1, 5])
    assert ones == {"n": 7, "recall": {1: 1.0, 5: 1.0}, "mrr": 1.0, "median_rank": 1.0, "mean_rank": 1.0, "mean_tied": 0.0}
    perm = torch.tensor([3, 1, 5, 2, 4])  # a permutation of 1 .. 5, odd n
    m = retrieval_metrics(perm, torch.tensor([0, 2, 0, 0, 3]), [1, 2, 5, 9])
    assert m["n"] == 5 and m["recall"] == {1: 0.2, 2: 0.4, 5: 1.0, 9: 1.0}  # (a k larger than n: every query)
    assert m["mrr"] == pytest.approx((1 + 1 / 2 + 1 / 3 + 1 / 4 + 1 / 5) / 5, abs=1e-15)
    assert m["median_rank"] == 3.0 and m["mean_rank"] == 3.0 and m["mean_tied"] == 1.0
    even = retrieval_metrics(torch.tensor([10, 1, 4, 2]), torch.zeros(4, dtype=torch.int64), [1, 3])
    assert even["median_rank"] == 3.0 and even["recall"] == {1: 0.25, 3: 0.5} and even["mean_rank"] == 4.25
    one = retrieval_metrics(torch.tensor([6]), torch.tensor([4]), [5, 10])
    assert one == {"n": 1, "recall": {5: 0.0, 10: 1.0}, "mrr": 1 / 6, "median_rank": 6.0, "mean_rank": 6.0, "mean_tied": 4.0}
    with pytest.raises(ValueError, match="n >= 1"):
        retrieval_metrics(torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), [1])


def test_orthogonality_against_numpy():
    from train_utils.retrieval import orthogonality
    r = np.random.default_rng(5)
    mods = ["seismic", "audio", "acc"]
    proj = {m: r.standard_normal((41, 24)).astype(np.float32) * (1 + 3 * i) for i, m in enumerate(mods)}
    proj["audio"][:, 12:] = 0.5 * proj["audio"][:, :12] + 0.1 * proj["audio"][:, 12:]  # a private half that leaks the shared one
    got = orthogonality({m: torch.from_numpy(v) for m, v in proj.items()}, mods)

    def cos(x, y):
        x, y = x.astype(np.float64), y.astype(np.float64)
        return (x * y).sum(1) / (np.linalg.norm(x, axis=1) * np.linalg.norm(y, axis=1))
    assert list(got["shared_private"]) == mods and list(got["private_private"]) == [("seismic", "audio"), ("seismic", "acc"), ("audio", "acc")]
    for m in mods:
        c = cos(proj[m][:, :12], proj[m][:, 12:])
        assert got["shared_private"][m] == pytest.approx((c.mean(), np.maximum(c, 0).mean()), abs=1e-12)
    for a, b in got["private_private"]:
        c = cos(proj[a][:, 12:], proj[b][:, 12:])
        assert got["private_private"][(a, b)] == pytest.approx((c.mean(), np.maximum(c, 0).mean()), abs=1e-12)
    assert got["shared_private"]["audio"][0] > 0.9  # the leak shows


def test_space_columns():
    cols = entry().space_columns(256)
    assert cols == {"shared": slice(0, 128), "private": slice(128, 256), "full": slice(0, 256)}


# ------------------------------------------------------------------------------------------ declarations
def test_exports_are_declared_at_abi_14():
    from focal_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "focal_hip.h")).read()
    assert re.search(r"#define FOCAL_ABI_VERSION 14\b", hdr) and _lib.ABI_VERSION == 14
    assert re.search(r"typedef struct \{ int nq, nt, D, slices; \} focal_rank_desc;", hdr)
    assert re.search(r"size_t focal_rank_workspace\(const focal_rank_desc\* d\);", hdr)
    assert re.search(r"int focal_rank_positive\(const focal_rank_desc\* d, const float\* q, const float\* t, const float\* t_sq, const int\* pos,\s*"
                     r"int\* before,\s*int\* tied,\s*float\* pos_d2, void\* ws, size_t ws_bytes, void\* stream\);", hdr)
    assert len(_lib.PROTOTYPES["focal_rank_workspace"][1]) == 1 and len(_lib.PROTOTYPES["focal_rank_positive"][1]) == 11
    assert [n for n, _ in _lib.RankDesc._fields_] == ["nq", "nt", "D", "slices"]


def test_rank_source_is_built():
    mk = open(os.path.join(ROOT, "focal_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=\s*(.*)$", mk, re.M).group(1).split()
    assert "rank.hip" in srcs and "knn.hip" in srcs
    assert os.path.isfile(os.path.join(ROOT, "focal_amd", "csrc", "rank.hip"))
