"""Entry point [build extension]: `python eval_linear.py -model=SW_Transformer -dataset=HAR3LOC -learn_framework=FOCAL [-model_weight=PATH]
[-probe_l2=1e-4,1e-3,1e-2,1e-1] [-probe_max_iter=200] [-probe_tol=1e-5] [-label_ratio=1.0]`: the linear-probe accuracy of a pretrained
backbone's un-projected features -- softmax regression fitted on the frozen features of the training split (train_utils/linear_probe.py:
GpuLinearProbe, every L2 strength in one pass per evaluation), every strength scored on the validation split, the one with the highest
validation accuracy (ties: the larger strength) reported on the test split.  The features are extracted once, so the paper's label-ratio
sweep is a matter of seconds per point; the backbone is built as pretraining builds it, so multi-location datasets -- which finetuning
refuses -- are covered.  The checkpoint and the refusals are eval_knn.py's; two runs on one checkpoint print the same numbers."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from params.knn_params import pretraining_command, refuse_classifier_checkpoint, refuse_other_frameworks  # noqa: E402
from params.linear_params import SCORE, TOOL, parse_linear_params, refuse_probe_settings  # noqa: E402


def refuse_data_parallel():
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit(f"{TOOL} scores on one device: launch it as one process (ranks of such a job would each score the same "
                         f"checkpoint on the same splits); `python {TOOL} ...` without torchrun")


def load_backbone_weight(args):
    """The checkpoint's state dict, read to host memory.  Refused: no checkpoint (nothing is scored at a random initialisation)."""
    import torch
    path = args.backbone_weight
    if not os.path.isfile(path):
        raise FileNotFoundError(f"no backbone checkpoint at {path}: `{pretraining_command(args)}` writes it (or name the folder or the "
                                "file that holds it with -model_weight)")
    return torch.load(path, map_location="cpu")


def labelled_train_loader(args, create_dataloader):
    """The training split as finetuning reads it -- the task's labelled index, cut to `-label_ratio` by the loader -- while everything else
    is built at stage "pretrain"."""
    stage = args.stage
    args.stage = "finetune"
    try:
        return create_dataloader("train", args, batch_size=args.batch_size, workers=args.workers)
    finally:
        args.stage = stage


def apply_label_ratio(args, loader, x, y):
    """A source whose loader holds no ratio (synthetic windows, packed shards): the first round(n * ratio) rows, the file loader's rule."""
    ratio = float(getattr(args, "label_ratio", 1.0) or 1.0)
    if ratio >= 1 or hasattr(getattr(loader, "dataset", None), "sample_files"):
        return x, y
    keep = max(1, round(x.shape[0] * ratio))
    return x[:keep].contiguous(), y[:keep].contiguous()


def choose_l2(l2, val_acc):
    """The index of the highest validation accuracy; ties go to the larger strength."""
    return max(range(len(l2)), key=lambda r: (val_acc[r], l2[r]))


def evaluate_linear(args, keep=False):
    """Score `args.backbone_weight`; returns {"l2": the grid, "val": [(accuracy, macro-F1) per strength], "chosen": index, "chosen_l2",
    "test": (accuracy, macro-F1) of the chosen strength}.  keep=True: also, as a second value, {"train": (features, labels), "val" / "test":
    (features, labels, predictions [R, n]), "estimator", "conf": {"val": [matrix per strength], "test": matrix of the chosen one}} -- the
    very tensors that were scored."""
    refuse_data_parallel()
    refuse_other_frameworks(args, TOOL, SCORE)
    l2 = refuse_probe_settings(args)
    refuse_classifier_checkpoint(args, args.backbone_weight, TOOL)
    state_dict = load_backbone_weight(args)
    from data_augmenter.Augmenter import Augmenter
    from eval_knn import split_features
    from input_utils.multi_modal_dataloader import create_dataloader
    from train_utils.eval_functions import metrics_from_confusion
    from train_utils.linear_probe import GpuLinearProbe
    from train_utils.model_selection import init_backbone_model
    from focal_amd import ops
    loaders = {split: create_dataloader(split, args, batch_size=args.batch_size, workers=args.workers) for split in ("val", "test")}
    loaders["train"] = labelled_train_loader(args, create_dataloader)
    augmenter = Augmenter(args)
    args.augmenter = augmenter
    backbone = init_backbone_model(args)
    backbone.load_state_dict(state_dict, strict=True)
    args.classifier = backbone
    backbone.eval()
    n_cls = int(args.dataset_config[args.task]["num_classes"])
    x, y = apply_label_ratio(args, loaders["train"], *split_features(args, backbone, augmenter, loaders["train"]))
    # (the fused form, not fit(fused=False): profiles/linear_probe_fused.txt)
    estimator = GpuLinearProbe(l2=l2, max_iter=int(getattr(args, "probe_max_iter", 200)), tol=float(getattr(args, "probe_tol", 1e-5)))
    estimator.fit(x, y, n_cls)
    R = len(l2)
    kept = {"train": (x, y), "estimator": estimator, "conf": {}}
    states = {}
    for split in ("val", "test"):
        feats, labels = split_features(args, backbone, augmenter, loaders[split])
        preds = estimator.predict(feats)
        states[split] = [ops.EvalState(n_cls, feats.device) for _ in range(R)]
        for r in range(R):
            states[split][r].add(labels, preds=preds[r])
        kept[split] = (feats, labels, preds)
    # the host reads each matrix once
    val = [metrics_from_confusion(args, states["val"][r].read()[2]) for r in range(R)]
    chosen = choose_l2(l2, [v[0] for v in val])
    test = metrics_from_confusion(args, states["test"][chosen].read()[2])
    out = {"l2": l2, "val": [(v[0], v[1]) for v in val], "chosen": chosen, "chosen_l2": l2[chosen], "test": (test[0], test[1])}
    kept["conf"] = {"val": [v[2] for v in val], "test": test[2]}
    for r in range(R):
        print(f"Linear probe (l2={l2[r]:g}) val acc: {val[r][0]: .5f}, val f1: {val[r][1]: .5f}")
    print(f"Linear probe chosen l2={l2[chosen]:g} ({x.shape[0]} training rows, {estimator.n_eval_} evaluations)")
    print(f"Linear probe (l2={l2[chosen]:g}) test acc: {test[0]: .5f}, test f1: {test[1]: .5f}")
    print(f"Val confusion matrix:\n {kept['conf']['val'][chosen]}")
    print(f"Test confusion matrix:\n {kept['conf']['test']}")
    return (out, kept) if keep else out


def main_eval_linear():
    refuse_data_parallel()
    evaluate_linear(parse_linear_params())


if __name__ == "__main__":
    main_eval_linear()
