"""Parameters of `test.py` (reference: params/test_params.py, params/output_paths.py:165-186)."""
import os

from params.base_params import parse_base_args
from params.params_util import set_auto_params


def refuse_pretrain_stage(args):
    if args.learn_framework == "FOCAL" and args.stage == "pretrain":
        raise ValueError("test.py scores a classifier, and FOCAL pretraining trains none (its class layer stays at its random "
                         "initialisation): finetune first (`train.py -learn_framework=FOCAL -stage=finetune`) and evaluate that "
                         "with `-stage=finetune`, or train and evaluate a supervised model with `-learn_framework=no`")


def resolve_classifier_weight(args):
    """The checkpoint `test.py` evaluates: the `*_best.pt` that supervised training (train_utils/supervised_train.py) or finetuning
    (train_utils/finetune.py) of the same model / dataset / task writes, in `args.weight_folder`, or in `-model_weight` when that
    names a directory (the reference's meaning of the flag).  [build extension] `-model_weight` naming an existing file is that file.
    Pure path arithmetic: no device, and the file is not opened here."""
    refuse_pretrain_stage(args)
    chosen = getattr(args, "model_weight", None)
    if chosen is not None and os.path.isfile(chosen):
        return chosen
    folder = chosen if chosen is not None else args.weight_folder
    if args.learn_framework == "FOCAL":
        return os.path.join(folder, f"{args.dataset}_{args.model}_{args.task}_{args.label_ratio}_finetune_best.pt")
    return os.path.join(folder, f"{args.dataset}_{args.model}_{args.task}_best.pt")


def parse_test_params():
    base = parse_base_args("test")
    refuse_pretrain_stage(base)  # before the device is selected: nothing is built for a run that cannot be scored
    args = set_auto_params(base)
    args.classifier_weight = resolve_classifier_weight(args)
    return args
