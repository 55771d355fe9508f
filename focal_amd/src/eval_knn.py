"""Entry point [build extension]: `python eval_knn.py -model=SW_Transformer -dataset=HAR3LOC -learn_framework=FOCAL [-model_weight=PATH]
[-knn_k=5]`: the KNN accuracy of a pretrained backbone's un-projected features -- the label-free quality number of FOCAL pretraining,
which the training loop logs every tenth epoch (train_utils/pretrain.py, reference train_utils/knn.py) -- for a saved checkpoint: the
estimator is fitted on the training split's features, the validation and test splits are scored, accuracy / macro-F1 / confusion
matrix as the loop reports them.  The checkpoint is the `*_pretrain_best.pt` of the matching `train.py` run (params/knn_params.py:
resolve_backbone_weight); the backbone is built as pretraining builds it, so multi-location datasets (which test.py cannot score: no
classifier path) are covered; one process, the first listed device."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from params.knn_params import (parse_knn_params, pretraining_command, refuse_classifier_checkpoint,  # noqa: E402
                               refuse_other_frameworks)


def refuse_data_parallel():
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("eval_knn.py scores on one device: launch it as one process (ranks of such a job would each score the same "
                         "checkpoint on the same splits); `python eval_knn.py ...` without torchrun")


def load_backbone_weight(args):
    """The checkpoint's state dict, read to host memory.  Refused: no checkpoint (nothing is scored at a random initialisation)."""
    import torch
    path = args.backbone_weight
    if not os.path.isfile(path):
        raise FileNotFoundError(f"no backbone checkpoint at {path}: `{pretraining_command(args)}` writes it (or name the folder or the "
                                "file that holds it with -model_weight)")
    return torch.load(path, map_location="cpu")


def split_features(args, backbone, augmenter, loader):
    """Un-projected features [n, M * D] and class indices [n] of one split, on the device."""
    import torch
    from train_utils.knn import extract_sample_features
    feats, labels = [], []
    with torch.no_grad():
        for time_loc_inputs, y in loader:
            freq_loc_inputs, _ = augmenter.forward("no", time_loc_inputs, y)
            feats.append(extract_sample_features(args, backbone, freq_loc_inputs))
            labels.append(y.argmax(dim=1) if y.dim() > 1 else y)
    if not feats:
        raise ValueError("eval_knn: the loader yielded no batch")
    feats = torch.cat(feats)
    return feats, torch.cat(labels).to(feats.device).long()


def evaluate_knn(args, keep=False):
    """Score `args.backbone_weight`; returns {"val": (accuracy, macro-F1), "test": (accuracy, macro-F1)}.  keep=True: also, as a second
    value, {"train": (features, labels), "val" / "test": (features, labels, predictions), "conf": {"val" / "test": matrix}} -- the very
    tensors that were scored."""
    refuse_data_parallel()
    refuse_other_frameworks(args)
    refuse_classifier_checkpoint(args, args.backbone_weight)
    state_dict = load_backbone_weight(args)
    from data_augmenter.Augmenter import Augmenter
    from input_utils.multi_modal_dataloader import create_dataloader
    from train_utils.eval_functions import metrics_from_confusion
    from train_utils.knn import GpuKNNClassifier
    from train_utils.model_selection import init_backbone_model
    from focal_amd import ops
    loaders = {split: create_dataloader(split, args, batch_size=args.batch_size, workers=args.workers) for split in ("train", "val", "test")}
    augmenter = Augmenter(args)
    args.augmenter = augmenter
    backbone = init_backbone_model(args)
    backbone.load_state_dict(state_dict, strict=True)
    args.classifier = backbone
    backbone.eval()
    k = int(getattr(args, "knn_k", 5))
    x, y = split_features(args, backbone, augmenter, loaders["train"])
    estimator = GpuKNNClassifier(n_neighbors=k).fit(x, y)
    n_cls = args.dataset_config[args.task]["num_classes"]
    kept, states = {"train": (x, y), "conf": {}}, {}
    for split in ("val", "test"):
        feats, labels = split_features(args, backbone, augmenter, loaders[split])
        states[split] = ops.EvalState(n_cls, feats.device)
        # (the fused search, not predict(): faster and without the [queries, training rows] matrix -- profiles/knn_fused.txt)
        preds = estimator.predict_fused(feats, labels=labels, state=states[split])
        kept[split] = (feats, labels, preds)
    out = {}
    for split in ("val", "test"):  # the host reads each matrix once
        acc, f1, conf = metrics_from_confusion(args, states[split].read()[2])
        out[split], kept["conf"][split] = (acc, f1), conf
    print(f"KNN (k={k}) val acc: {out['val'][0]: .5f}, val f1: {out['val'][1]: .5f}")
    print(f"KNN (k={k}) test acc: {out['test'][0]: .5f}, test f1: {out['test'][1]: .5f}")
    print(f"Val confusion matrix:\n {kept['conf']['val']}")
    print(f"Test confusion matrix:\n {kept['conf']['test']}")
    return (out, kept) if keep else out


def main_eval_knn():
    refuse_data_parallel()
    evaluate_knn(parse_knn_params())


if __name__ == "__main__":
    main_eval_knn()
