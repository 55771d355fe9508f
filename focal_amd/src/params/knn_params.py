"""Parameters of `eval_knn.py` [build extension]: which backbone checkpoint is scored, and what is refused before anything is built."""
import os
import re

from params.base_params import parse_base_args
from params.params_util import set_auto_params


def refuse_other_frameworks(args, tool="eval_knn.py", score="the KNN accuracy of its features"):
    if args.learn_framework != "FOCAL":
        raise ValueError(f"{tool} scores the backbone of a FOCAL pretraining run by {score}; "
                         f"-learn_framework={args.learn_framework} trains a classifier: evaluate that with "
                         f"`python test.py -model={args.model} -dataset={args.dataset} -learn_framework={args.learn_framework}`")


def pretraining_command(args):
    return f"python train.py -model={args.model} -dataset={args.dataset} -learn_framework=FOCAL"


def resolve_backbone_weight(args):
    """The checkpoint `eval_knn.py` scores: the `{dataset}_{model}_pretrain_best.pt` that pretraining (train_utils/pretrain.py) writes, in
    `args.weight_folder`, or in `-model_weight` when that names a directory (the reference's meaning of the flag); `-model_weight` naming an
    existing file is that file (as for test.py).  Pure path arithmetic: no device, and the file is not opened here."""
    chosen = getattr(args, "model_weight", None)
    if chosen is not None and os.path.isfile(chosen):
        return chosen
    folder = chosen if chosen is not None else args.weight_folder
    return os.path.join(folder, f"{args.dataset}_{args.model}_pretrain_best.pt")


def refuse_classifier_checkpoint(args, path, tool="eval_knn.py"):
    """A finetuned or supervised classifier's checkpoint is scored by test.py, on its own class layer.  It is told by the name its training
    loop gave it (`*_finetune_{best,latest}.pt`, `{dataset}_{model}_{task}_{best,latest}.pt`) -- not by its tensors: a backbone's state dict
    holds `class_layer.*` at every stage, pretraining's checkpoints included, where they are the untouched initialisation."""
    name = os.path.basename(path)
    task = re.escape(str(getattr(args, "task", None) or ""))
    if re.search(r"_finetune_(best|latest)\.pt$", name) or (task and re.fullmatch(rf".*_{task}_(best|latest)\.pt", name)):
        stage = " -learn_framework=FOCAL -stage=finetune" if "_finetune_" in name else " -learn_framework=no"
        raise ValueError(f"{path} is a classifier checkpoint (the name finetuning / supervised training gives one): its class layer is what "
                         f"is scored, by `python test.py -model={args.model} -dataset={args.dataset}{stage} -model_weight={path}`; "
                         f"{tool} scores what `{pretraining_command(args)}` writes")


def parse_knn_params():
    base = parse_base_args("eval_knn")
    refuse_other_frameworks(base)  # before the device is selected
    base.stage = "pretrain"        # the backbone is built as pretraining builds it: multi-location configurations included
    args = set_auto_params(base)
    args.backbone_weight = resolve_backbone_weight(args)
    refuse_classifier_checkpoint(args, args.backbone_weight)
    return args
