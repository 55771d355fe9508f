"""Host half of evaluation: the metrics taken from a confusion matrix (train_utils/eval_functions.py: metrics_from_confusion) against
the label / prediction form they replace (eval_task_metrics, the CPU reference), and the checkpoint path test.py resolves."""
import argparse
import os

import numpy as np
import pytest


def _args(cfg, task):
    return argparse.Namespace(task=task, dataset_config=cfg)


def _confusion(labels, preds, C):
    conf = np.zeros((C, C), dtype=np.int64)
    np.add.at(conf, (labels, preds), 1)
    return conf


def _vectors(case, C):
    g = np.random.default_rng(4100 + sum(map(ord, case)))
    if case == "all":
        return g.integers(0, C, 50), g.integers(0, C, 50)
    if case == "absent_0_3":
        keep = np.array([c for c in range(C) if c not in (0, 3)])
        return keep[g.integers(0, len(keep), 50)], keep[g.integers(0, len(keep), 50)]
    if case == "predicted_never_label":
        labels, preds = g.integers(0, C - 1, 50), g.integers(0, C - 1, 50)  # class C-1 is never a label ...
        preds[::7] = C - 1                                               # ... and is predicted
        return labels, preds
    if case == "extremes":
        labels, preds = g.integers(0, C, 40), g.integers(0, C, 40)
        labels[:4] = [0, C - 1, 0, C - 1]  # both ends of max(l, C-1-l), hit and missed
        preds[:4] = [0, C - 1, C - 1, 0]
        return labels, preds
    if case == "one":
        return np.array([2]), np.array([1])
    raise AssertionError(case)


@pytest.mark.parametrize("task,case", [("vehicle_classification", "all"), ("vehicle_classification", "absent_0_3"),
                                       ("vehicle_classification", "predicted_never_label"), ("vehicle_classification", "one"),
                                       ("speed_classification", "all"), ("speed_classification", "extremes"),
                                       ("speed_classification", "one")])
def test_metrics_from_confusion_match_the_label_form(cfg, task, case):
    from train_utils.eval_functions import eval_task_metrics, metrics_from_confusion
    C = cfg[task]["num_classes"]
    assert C == (7 if task == "vehicle_classification" else 4)
    labels, preds = _vectors(case, C)
    if case == "absent_0_3":
        assert not ({0, 3} & (set(labels.tolist()) | set(preds.tolist())))
    if case == "predicted_never_label":
        assert C - 1 in preds and C - 1 not in labels
    if case == "extremes":
        assert {0, C - 1} <= set(labels.tolist())
    args = _args(cfg, task)
    acc_ref, f1_ref, conf_ref = eval_task_metrics(args, labels, preds)
    acc, f1, conf = metrics_from_confusion(args, _confusion(labels, preds, C))
    assert abs(acc - acc_ref) <= 1e-12, (acc, acc_ref)
    assert abs(f1 - f1_ref) <= 1e-12, (f1, f1_ref)
    assert conf.shape == conf_ref.shape and np.array_equal(conf, conf_ref)


def _run(tmp_path, **kw):
    base = dict(dataset="MOD", model="DeepSense", task="vehicle_classification", learn_framework="no", stage="pretrain",
                label_ratio=1.0, model_weight=None, weight_folder=str(tmp_path / "weights" / "MOD_DeepSense"))
    base.update(kw)
    return argparse.Namespace(**base)


def test_resolve_classifier_weight(tmp_path):
    from params.test_params import resolve_classifier_weight
    folder = str(tmp_path / "weights" / "MOD_DeepSense")
    # supervised: what train_utils/supervised_train.py writes (the stage flag plays no part without a framework)
    assert resolve_classifier_weight(_run(tmp_path)) == os.path.join(folder, "MOD_DeepSense_vehicle_classification_best.pt")
    # finetune: what train_utils/finetune.py writes, label ratio included
    got = resolve_classifier_weight(_run(tmp_path, model="SW_Transformer", learn_framework="FOCAL", stage="finetune", label_ratio=0.1))
    assert got == os.path.join(folder, "MOD_SW_Transformer_vehicle_classification_0.1_finetune_best.pt")
    # -model_weight names a directory: the folder
    other = tmp_path / "elsewhere"
    other.mkdir()
    got = resolve_classifier_weight(_run(tmp_path, learn_framework="FOCAL", stage="finetune", model_weight=str(other)))
    assert got == os.path.join(str(other), "MOD_DeepSense_vehicle_classification_1.0_finetune_best.pt")
    # -model_weight names an existing file: that file
    ckpt = other / "anything.pt"
    ckpt.write_bytes(b"")
    assert resolve_classifier_weight(_run(tmp_path, model_weight=str(ckpt))) == str(ckpt)


def test_pretrain_stage_is_refused(tmp_path):
    from params.test_params import resolve_classifier_weight
    with pytest.raises(ValueError, match="-stage=finetune"):
        resolve_classifier_weight(_run(tmp_path, learn_framework="FOCAL", stage="pretrain"))
